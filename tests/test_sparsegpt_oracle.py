"""tests/sparsegpt_oracle.py against independent mathematics (the reference tree has no SparseGPT to diff against).

For the mask the oracle chose, its float64 run must agree with the paper's unoptimised recursion (Frantar & Alistarh 2023,
eq. 3-5): for every column i in turn, Hi = inv(H[i:, i:]) and W[:, i:] -= ((w - q) / Hi[0, 0]) (x) Hi[0, :], one fresh matrix
inverse per column and no Cholesky factor, no blocks, no trailing product. H = 2/T X^T X + 0.01 mean(diag) I from seeded
Gaussian X with per-column scales in [1, 4] (cond(H) measured 26 - 35).

Relative error = max |delta| / max |value| over Wout. MEASURED (numpy with OpenBLAS LAPACK), over the four cases below:
  float64 oracle vs recursion   7.2e-16 - 1.09e-15
  float32 oracle vs recursion   2.3e-7 - 3.4e-7   (masks identical to the float64 run's)
The assertions allow 100 x the largest measured value of each; the margin covers another LAPACK."""
import numpy as np
import pytest

import sparsegpt_oracle as O

CASES = [(8, 256, 1024, 11), (5, 320, 2048, 12)]          # (R, K, T, seed)
MODES = [dict(sparsity=0.5), dict(nm=(2, 4))]
BOUND_F64 = 100 * 1.09e-15
BOUND_F32 = 100 * 3.4e-7


def make_case(R, K, T, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((T, K)) * rng.uniform(1.0, 4.0, size=K)[None, :]
    H = 2.0 / T * (X.T @ X)
    H += 0.01 * np.mean(np.diag(H)) * np.eye(K)
    W = rng.standard_normal((R, K))
    U = np.linalg.cholesky(np.linalg.inv(H)).T          # upper, H^-1 = U^T U
    return W, H, U


def recursion(W, H, mask):
    W = np.array(W, dtype=np.float64, copy=True)
    K = W.shape[1]
    for i in range(K):
        Hi = np.linalg.inv(H[i:, i:])
        w = W[:, i].copy()
        q = np.where(mask[:, i] != 0, 0.0, w)
        W[:, i:] -= ((w - q) / Hi[0, 0])[:, None] * Hi[0, :][None, :]
        W[:, i] = q
    return W


_cache = {}


def case(idx):
    if idx not in _cache:
        _cache[idx] = make_case(*CASES[idx])
    return _cache[idx]


def rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


@pytest.mark.parametrize('mode', range(len(MODES)))
@pytest.mark.parametrize('idx', range(len(CASES)))
def test_oracle_agrees_with_the_unoptimised_recursion(idx, mode):
    W, H, U = case(idx)
    kw = MODES[mode]
    o64 = O.prune(W, U, dtype=np.float64, **kw)
    want = recursion(W, H, o64['mask'])
    o32 = O.prune(W.astype(np.float32), U.astype(np.float32), dtype=np.float32, **kw)
    e64, e32 = rel(o64['Wout'], want), rel(o32['Wout'].astype(np.float64), want)
    print(f'sparsegpt oracle {CASES[idx][:3]} {kw}: cond(H) = {np.linalg.cond(H):.1f} rel err fp64 = {e64:.3e} fp32 = {e32:.3e}')
    assert np.array_equal(o32['mask'], o64['mask'])
    assert 0.3 < o64['mask'].mean() < 0.7          # the case prunes about half: the recursion is exercised
    assert e64 <= BOUND_F64
    assert e32 <= BOUND_F32


def test_nm_edge_cases():
    W, H, U = case(0)
    W32, U32 = W.astype(np.float32), U.astype(np.float32)
    none = O.prune(W32, U32, nm=(0, 4))
    assert np.array_equal(O.bits(none['Wout']), O.bits(W32)) and not none['mask'].any()
    assert np.array_equal(O.bits(none['W']), O.bits(W32)) and not none['losses'].any()
    every = O.prune(W32, U32, nm=(4, 4))
    assert not O.bits(every['Wout']).any() and every['mask'].all()          # all +0
    for n, m in ((2, 4), (1, 4), (4, 8), (1, 2), (8, 16)):
        o = O.prune(W32, U32, nm=(n, m))
        zeros = (o['Wout'] == 0).reshape(W.shape[0], -1, m).sum(axis=2)
        assert (zeros >= n).all() and (o['mask'].reshape(W.shape[0], -1, m).sum(axis=2) == n).all()
        assert np.array_equal(o['Wout'] == 0, o['mask'] != 0)          # a kept Gaussian weight is not zero


@pytest.mark.parametrize('sparsity', [0.0, 0.5, 0.9])
def test_unstructured_mask_is_the_threshold_rule(sparsity):
    W, H, U = case(1)
    R, K = W.shape
    o = O.prune(W.astype(np.float32), U.astype(np.float32), sparsity=sparsity)
    assert len(o['thresh']) == -(-K // 128)
    for b, t in enumerate(o['thresh']):
        i1, i2 = 128 * b, min(128 * b + 128, K)
        s, mk = o['scores'][:, i1:i2], o['mask'][:, i1:i2] != 0
        assert np.array_equal(mk, s <= t)
        kth = int(R * (i2 - i1) * sparsity)
        assert mk.sum() >= kth + 1 and (s < t).sum() <= kth
    if sparsity == 0.0:          # the published code's behaviour: the minimum-score element(s) of each block go
        assert o['mask'].sum() >= len(o['thresh'])
