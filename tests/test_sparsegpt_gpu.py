"""llmc_sparsegpt_prune (csrc/sparsegpt_loop.hip) against tests/sparsegpt_oracle.py, bit for bit as uint32 views: Wout, losses, mask
and the running W. Shapes: one row and one block (no trailing update), a ragged workgroup, a ragged last block of 64, a last
block of 4, several blocks, and many workgroups feeding one histogram over eight blocks."""
import numpy as np
import pytest
import torch

import sparsegpt_oracle as O
from gptq_fp8_oracle import synth_upper

pytestmark = pytest.mark.gpu

SHAPES = [(1, 128), (17, 256), (40, 320), (16, 132), (64, 512), (300, 1024)]
MODES = [dict(sparsity=0.0), dict(sparsity=0.5), dict(sparsity=0.9), dict(nm=(2, 4)), dict(nm=(1, 4)), dict(nm=(4, 8)),
         dict(nm=(1, 2)), dict(nm=(8, 16))]
CASES = [(R, K, i) for (R, K) in SHAPES for i, md in enumerate(MODES) if 'nm' not in md or K % md['nm'][1] == 0]


def ops():
    from llmc_amd.compression.sparsification import sparse_ops
    return sparse_ops


def weights(R, K, seed=0):
    return (np.random.default_rng(1000 * R + K + seed).standard_normal((R, K)) * 0.05).astype(np.float32)


def run_kernel(W, U, want_losses=True, want_mask=True, **kw):
    Wg, Ug = torch.from_numpy(W).cuda(), torch.from_numpy(U).cuda()
    out, losses, mask = ops().sparsegpt_prune(Wg, Ug, want_losses=want_losses, want_mask=want_mask, **kw)
    torch.cuda.synchronize()
    return dict(Wout=out.cpu().numpy(), losses=None if losses is None else losses.cpu().numpy(),
                mask=None if mask is None else mask.cpu().numpy(), W=Wg.cpu().numpy())


def assert_same(got, want, what):
    for k in ('Wout', 'losses', 'W'):
        bad = O.bits(got[k]) != O.bits(want[k])
        assert not bad.any(), (what, k, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    assert got['mask'].dtype == np.uint8 and np.array_equal(got['mask'], want['mask']), (what, 'mask')


_ref = {}


def reference(R, K, mode):
    key = (R, K, mode)
    if key not in _ref:
        W, U = weights(R, K), synth_upper(K, R + K)
        _ref[key] = (W, U, O.prune(W, U, **MODES[mode]))
    return _ref[key]


@pytest.mark.parametrize('R,K,mode', CASES)
def test_kernel_equals_the_oracle_bit_for_bit(R, K, mode):
    W, U, want = reference(R, K, mode)
    assert_same(run_kernel(W, U, **MODES[mode]), want, (R, K, MODES[mode]))


@pytest.mark.parametrize('nm', [(0, 4), (4, 4)])
def test_nm_extremes(nm):
    W, U = weights(17, 256), synth_upper(256, 5)
    got = run_kernel(W, U, nm=nm)
    assert_same(got, O.prune(W, U, nm=nm), nm)
    if nm[0] == 0:
        assert np.array_equal(O.bits(got['Wout']), O.bits(W)) and not got['mask'].any()
    else:
        assert not O.bits(got['Wout']).any() and got['mask'].all()


@pytest.mark.parametrize('mode', [dict(sparsity=0.5), dict(nm=(2, 4))])
def test_a_real_factor(mode):
    """U from chol_inv_upper on the device, copied to the host: the oracle gets the same bits"""
    from llmc_amd.compression.quantization import gptq_ops
    R, K = 64, 512
    g = torch.Generator().manual_seed(7)
    X = torch.randn(2048, K, generator=g) * (1 + 3 * torch.rand(K, generator=g))
    H = (2.0 / 2048 * (X.T @ X)).float()
    H += 0.01 * torch.diagonal(H).mean() * torch.eye(K)
    U = gptq_ops.chol_inv_upper(H.cuda().contiguous()).cpu().numpy()
    W = weights(R, K, seed=3)
    assert_same(run_kernel(W, U, **mode), O.prune(W, U, **mode), mode)


@pytest.mark.parametrize('mode', [dict(sparsity=0.5), dict(nm=(2, 4))])
def test_ties(mode):
    """small integer weights (with -0.0) and a constant diagonal: many equal scores. Unstructured prunes every tie of the
    threshold; n:m breaks ties by the lower column; a pruned -0 becomes +0 and a kept weight keeps its bits."""
    R, K = 40, 320
    rng = np.random.default_rng(9)
    W = rng.integers(-2, 3, size=(R, K)).astype(np.float32)
    W[rng.random((R, K)) < 0.1] = np.float32(-0.0)
    U = synth_upper(K, 3)
    U[np.arange(K), np.arange(K)] = np.float32(0.75)
    want = O.prune(W, U, **mode)
    if 'sparsity' in mode:
        s0 = want['scores'][:, :128]
        assert (s0 == want['thresh'][0]).sum() > 1 and want['mask'][:, :128].sum() > int(R * 128 * 0.5) + 1
    else:
        first = W[:, :4]          # the first group of a row is scored before any update: its ties are the input's
        assert (np.abs(first[:, 0]) == np.abs(first[:, 1])).any()
    assert_same(run_kernel(W, U, **mode), want, mode)


def test_twice_the_same_and_optional_outputs():
    R, K = 300, 1024
    W, U, want = reference(R, K, 1)
    a, b = run_kernel(W, U, sparsity=0.5), run_kernel(W, U, sparsity=0.5)
    assert_same(a, b, 'second run')
    c = run_kernel(W, U, want_losses=False, want_mask=False, sparsity=0.5)
    assert c['losses'] is None and c['mask'] is None
    assert np.array_equal(O.bits(c['Wout']), O.bits(want['Wout'])) and np.array_equal(O.bits(c['W']), O.bits(want['W']))
    d = run_kernel(W, U, want_losses=False, want_mask=False, nm=(2, 4))
    assert np.array_equal(O.bits(d['Wout']), O.bits(reference(R, K, 3)[2]['Wout']))
