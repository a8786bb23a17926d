"""The inputs of tests/test_sparsegpt_widths_gpu.py, importable without a GPU: tests/test_sparsegpt_cases.py proves on the oracle
alone (tests/sparsegpt_oracle.py) that every builder produces the condition it is named for — all scores of a panel in one
first-digit bin of the select, a threshold of exactly +0, subnormal scores, scores that overflow to +inf from finite weights —
and the GPU tests run the same arrays. Every builder returns (W [R, K], U [K, K]) as float32, seeded and read-only. What each
case reaches in llmc_amd/csrc/sparsegpt_loop.hip is stated next to it."""
import functools

import numpy as np

from gptq_fp8_oracle import synth_upper


def mode_kw(mode):
    """a mode is a string, so that it reads in a test id: 's<sparsity>' (unstructured) or 'n:m'. -> the keyword arguments of
    sparse_ops.sparsegpt_prune / sparsegpt_oracle.prune"""
    if mode.startswith('s'):
        return dict(sparsity=float(mode[1:]))
    n, m = mode.split(':')
    return dict(nm=(int(n), int(m)))


# ---- the select's edges (k_sg_hist, k_sg_scan, k_sg_hist_low): (builder, mode) ---------------------------------------------------------
ONE_BIN_SHAPE = (300, 384)       # three blocks; many workgroups feed one histogram
EDGE_SHAPE = (40, 320)           # two blocks and a last one of 64
RANK_SHAPE, RANK_SPARSITY = (17, 256), 0.99999          # int(17 * 128 * 0.99999) == 17 * 128 - 1: the last rank of a panel
SELECT = [('one_bin', 's0.5'),                                     # the second digit decides alone
          ('zero_floor', 's0.5'), ('zero_floor', 's0.59'), ('zero_floor', '2:4'),      # threshold in bin 0: the key of +0
          ('subnormal', 's0.5'), ('subnormal', '2:4'),
          ('overflow', 's0.5'), ('overflow', 's0.985'),            # keys of +inf: bin 0x7f80, and +inf as the threshold
          ('rank_last', 's%r' % RANK_SPARSITY)]

# ---- one ragged block, rows around the 16-row workgroup and the 4-row wave ---------------------------------------------------------------
RAGGED_SHAPES = [
    (1, 4),          # one float4 of U; one column step in the first stripe
    (3, 20),         # a stripe of 16 and one of 4; three rows of one wave
    (5, 100),        # six stripes and 4 columns; a second wave with one row
    (16, 124),       # one group short of a full block; exactly one workgroup
    (33, 136),       # a last block of one 4:8 group; one row in a third workgroup
    (15, 144),       # a last block of one 8:16 group; one row short of a workgroup
    (31, 260),       # two full blocks and 4 columns: a trailing update with N = 4
    (4, 128),        # one full block, no trailing update; exactly one wave
]
RAGGED = [(R, K, mode) for (R, K) in RAGGED_SHAPES
          for mode, m in (('s0.5', 1), ('2:4', 4), ('4:8', 8), ('8:16', 16)) if K % m == 0]

# ---- tall panels and model widths -------------------------------------------------------------------------------------------------------
TALL = [(20000, 132), (4100, 256)]          # 20000 x 128 elements exceed 256 CUs x 8192: k_sg_hist's grid is capped
WIDE = [(64, 4096), (32, 11008)]            # 32 and 86 blocks; the factor is made on the device from real_hessian
BIG_MODES = ['s0.5', '2:4']
LOWER = [(40, 320), (64, 512)]              # the strict lower triangle of the device's U is NaN
# the workspace sequence: (builder, R, K, mode) in order; the first entry is repeated at the end
SEQUENCE = [('general', 300, 1024, 's0.5'), ('general', 17, 256, 's0.9'), ('general', 40, 320, '4:8'),
            ('zero_floor', 40, 320, 's0.5'), ('general', 300, 1024, 's0.5')]


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def weights(R, K, seed=0):
    """0.05 * N(0, 1), the weights of tests/test_sparsegpt_gpu.py"""
    return (np.random.default_rng(1000 * R + K + seed).standard_normal((R, K)) * 0.05).astype(np.float32)


@functools.lru_cache(maxsize=None)
def general(R, K, seed=0):
    return _frozen(weights(R, K, seed), synth_upper(K, R + K + seed))


@functools.lru_cache(maxsize=None)
def one_bin(R, K):
    """W = +-(1 + j 2^-23), j < 2^14, on the identity: every score w w lies in [1, 1 + 2^-8), whose bit patterns share their
    upper 16 bits, in every block (the identity moves nothing between columns)."""
    rng = np.random.default_rng(11 + R + K)
    j = rng.integers(0, 1 << 14, size=(R, K))
    W = (np.float32(1.0) + j.astype(np.float32) * np.float32(2.0 ** -23)).astype(np.float32)
    W = np.where(rng.random((R, K)) < 0.5, -W, W).astype(np.float32)
    return _frozen(W, np.eye(K, dtype=np.float32))


@functools.lru_cache(maxsize=None)
def zero_floor(R, K):
    """exactly 60 % of the entries are zero, a third of those -0.0, and three whole columns besides: at sparsity 0.5 the score
    of the selected rank is +0 in every block, what a half-sparse checkpoint and the columns hessian_prep zeroes produce."""
    rng = np.random.default_rng(23 + R + K)
    W = weights(R, K, seed=1)
    flat = W.reshape(-1)
    zero = rng.permutation(R * K)[:R * K * 6 // 10]
    flat[zero] = 0.0
    flat[zero[::3]] = -0.0
    W[:, rng.choice(K, 3, replace=False)] = 0.0
    return _frozen(W, synth_upper(K, 7))


@functools.lru_cache(maxsize=None)
def subnormal(R, K):
    """3e-20 * N(0, 1): w w is around 1e-39, below 2^-126; a tenth of the entries at 3e-24, whose square is below 2^-149"""
    rng = np.random.default_rng(37 + R + K)
    W = rng.standard_normal((R, K)) * 3e-20
    W[rng.random((R, K)) < 0.1] *= 1e-4
    return _frozen(W.astype(np.float32), synth_upper(K, 9))


@functools.lru_cache(maxsize=None)
def overflow(R, K):
    """general with 2 % of the entries at +3e19 or -2e19: finite weights whose w w is +inf (|w| > 1.85e19)"""
    rng = np.random.default_rng(41 + R + K)
    W, U = general(R, K, seed=2)
    W = W.copy()
    big = rng.permutation(R * K)[:R * K // 50]
    W.reshape(-1)[big] = np.where(rng.random(big.size) < 0.5, np.float32(3e19), np.float32(-2e19))
    return _frozen(W, U)


def build(name, R, K):
    """a builder of SELECT / SEQUENCE by name"""
    if name in ('general', 'rank_last'):
        return general(R, K)
    return {'one_bin': one_bin, 'zero_floor': zero_floor, 'subnormal': subnormal, 'overflow': overflow}[name](R, K)


def select_case(name):
    """(W, U) of one entry of SELECT at its shape"""
    shape = ONE_BIN_SHAPE if name == 'one_bin' else RANK_SHAPE if name == 'rank_last' else EDGE_SHAPE
    return build(name, *shape)


def real_hessian(K, seed):
    """the H of tests/test_sparsegpt_gpu.py's test_a_real_factor at width K: 2048 tokens, column scales in [1, 4], damped by
    1 % of the mean diagonal. A torch CPU tensor."""
    import torch
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(2048, K, generator=g) * (1 + 3 * torch.rand(K, generator=g))
    H = (2.0 / 2048 * (X.T @ X)).float()
    torch.diagonal(H).add_(0.01 * torch.diagonal(H).mean())
    return H


def nan_below(U):
    """a copy of U with NaN in every entry below the diagonal"""
    V = np.array(U, dtype=np.float32, copy=True)
    V[np.tril_indices(V.shape[0], -1)] = np.nan
    return V
