"""The inputs of tests/test_spqr_widths_gpu.py, importable without a GPU: tests/test_spqr_cases.py proves on the oracle alone
(oracle/spqr_ref.py, pinned to the reference by tests/golden/spqr.npz) that every case reaches what it is there for — outliers
are found but stay a minority, groups really hold duplicated extremes when the detection looks at them, a group has every column
flagged — and the GPU tests run the same arrays. Everything is in PROCESSING order: (Wp, U) go to spqr_quantize / the oracle's
weight_transform as they are. What each case reaches in k_spqr_block (llmc_amd/csrc/spqr_loop.hip) is stated next to it."""
import functools
import math

import numpy as np

# ---- A: K that is no multiple of the 128-column block: (R, K, g, relative threshold) ------------------------------------------------
RAGGED = [
    (17, 304, 16, 0.05),     # 2 blocks + 48 columns: three group starts and five skipped ones in the last block
    (33, 160, 32, 0.05),     # 1 block + 32: one group of two registers, then nothing
    (20, 192, 64, 0.05),     # 1 block + 64: the group start at register 4 is skipped
    (3, 400, 16, 0.05),      # 3 blocks + 16: a single stripe; three rows of one wave
    (5, 48, 16, 0.02),       # K < 128: one short block, no trailing update at all
    (16, 16, 16, 0.02),      # one group is the whole matrix; a full workgroup of rows
    (24, 576, 64, 0.05),     # SmolLM-135M's hidden size: 4 blocks + 64
    (24, 960, 32, 0.05),     # SmolLM-360M's hidden size: 7 blocks + 64
]
MODES = ['detect', 'simplified', 'inf']

# ---- B1: weights on a coarse grid, so that a group's min / max is usually held by several columns ------------------------------------
GRID = [(40, 384, 16), (40, 384, 32)]
GRID_U = ['diag', 'general']
GRID_THR = 0.01              # relative threshold of B1: low enough for the flags of tied columns to sit near their margin
PLANT_THR = 0.1              # relative threshold of B2

# ---- C / D / E ------------------------------------------------------------------------------------------------------------------------
EDGE_SHAPE = (40, 256, 16)
EDGE_REL = 0.1               # relative threshold where a case wants an ordinary one (4 bit)
TINY_REL = 1e-6              # "very small": almost every column is an outlier
CUT_BELOW, CUT_ABOVE = 3.0e38, 3.1e38          # the two sides of llmc_spqr_quantize's `finite = !(threshold > 3.0e38f)`
BITS = [2, 3, 8]


def bit_rel(bit):
    """the squared rounding error of a b-bit grid goes with 4^-b: the relative threshold that keeps outliers a small minority at
    4 bit, scaled to b bit (at 8 bit EDGE_REL itself finds nothing, at 2 bit a large share)"""
    return EDGE_REL * 4.0 ** (4 - bit)


SECOND_LEVEL_BITS = [(3, 3), (4, 8), (8, 4)]
ROWS = [1, 15, 16, 17, 63, 65]                 # around the 16-row workgroup and the 4-row wave quarter; K = 256, g = 16

# ---- F: model widths (R, K, g); inputs are made on the GPU ----------------------------------------------------------------------------
MODEL = [(1024, 4096, 16), (1024, 4096, 128), (256, 14336, 16), (512, 1600, 32)]
MODEL_REL = 0.2

# ---- G: q / k / v on one shared factor ------------------------------------------------------------------------------------------------
STACK_K, STACK_ROWS, STACK_DEAD, STACK_REL = 576, (576, 192, 192), 5, 0.2
# ---- B3 ---------------------------------------------------------------------------------------------------------------------------------
DEAD_SHAPE, DEAD_N, DEAD_REL = (40, 384, 32), 40, 0.1


def _S():
    from oracle import spqr_ref
    return spqr_ref


def hessian(K, rs, dead=()):
    """X^T X / 8 of [4K, K] activations with log-normal channel scales, as tests/test_spqr_gpu.py builds it; the channels in
    `dead` are zeroed in X, so their rows, columns and diagonal in H are exact zeros."""
    X = (rs.randn(4 * K, K) * np.exp(0.5 * rs.randn(K))).astype(np.float32)
    X[:, list(dead)] = 0.0
    return (X.T @ X / 8).astype(np.float32)


def weights(R, K, rs):
    """N(0, 0.02) with six heavy columns and isolated outliers of 25x, at least four and one per 400 entries"""
    W = (rs.randn(R, K) * 0.02).astype(np.float32)
    W[:, rs.randint(0, K, 6)] *= 15
    n = max(4, R * K // 400)
    W[rs.randint(0, R, n), rs.randint(0, K, n)] *= 25
    return W


@functools.lru_cache(maxsize=None)
def general(R, K, seed=0):
    """(Wp, U) with a dense upper factor: weights() and hessian() through the oracle's actorder permutation, damping and
    factorisation. Outliers are then planted in the LAST block as well (processing order), so a ragged block has some to find."""
    rs = np.random.RandomState(1000 * K + 10 * R + seed)
    Wp, U, _ = _S().process_hessian_and_weights(weights(R, K, rs), hessian(K, rs), True, 1.0)
    last = (K - 1) // 128 * 128
    n = max(2, R // 8)
    Wp[rs.randint(0, R, n), rs.randint(last, K, n)] *= 25
    Wp = np.ascontiguousarray(Wp)            # the permuted copy is column-major
    Wp.setflags(write=False)
    U.setflags(write=False)
    return Wp, U


@functools.lru_cache(maxsize=None)
def diag_factor(K, seed=0):
    """A diagonal U (d in [0.5, 2)): no column feeds back into another, so every group reaches its group start as written."""
    rs = np.random.RandomState(77 + K + seed)
    U = np.diag(rs.uniform(0.5, 2.0, K).astype(np.float32))
    U.setflags(write=False)
    return U


@functools.lru_cache(maxsize=None)
def rows_input():
    """E: max(ROWS) rows at K = 256 with one threshold; the case of R rows is the first R of them (rows are independent given U
    and the threshold). Row 0 gets two outliers of its own, so that R = 1 has something to find."""
    Wp, U = general(max(ROWS), 256, seed=1)
    Wp = Wp.copy()
    Wp[0, [40, 200]] *= 25
    Wp.setflags(write=False)
    return Wp, U, threshold(Wp, U, EDGE_REL)


def threshold(Wp, U, rel):
    return math.inf if math.isinf(rel) else _S().outlier_threshold(Wp, U, rel)


def mode_args(mode, Wp, U, rel):
    """(threshold, simplified_outliers) of one of MODES"""
    if mode == 'inf':
        return math.inf, False
    return threshold(Wp, U, rel), mode == 'simplified'


@functools.lru_cache(maxsize=None)
def grid(R, K, g, kind):
    """B1: round(3 randn) / 64 — about nine distinct values in a group of 16. kind 'diag': ties survive to the detection of every
    group; 'general': the feedback of earlier columns breaks them everywhere but in the first group of a row."""
    rs = np.random.RandomState(g + R)
    Wp = (np.rint(3.0 * rs.randn(R, K)) / 64.0).astype(np.float32)
    U = diag_factor(K) if kind == 'diag' else general(R, K)[1]
    Wp.setflags(write=False)
    return Wp, U


# B2 plants, one group each (plant() says what the kernel must get right on it)
PLANTS = ['constant', 'two_values', 'min_col0', 'min_col15', 'max_col0', 'max_col15', 'min_reg1', 'max_reg1', 'min_twice',
          'max_twice', 'min_twice_far', 'max_twice_far', 'signed_zeros', 'zeros_and_values']
FAR_D = 64.0                 # d of the two columns that hold the copies in the *_far plants


def plant(name, g, rs):
    """one group of g columns. Body values are distinct by construction (a shuffled arithmetic ladder), so the only duplicated
    extremes are the planted ones."""
    body = ((np.arange(g) - g / 2 + 0.25) * (0.04 / g)).astype(np.float32)
    rs.shuffle(body)
    v = body.copy()
    big = np.float32(0.75)
    if name == 'constant':
        v[:] = 0.013                                        # lo.a == hi.a, multiplicity g on both sides, range clamped to 1e-5
    elif name == 'two_values':
        v[:] = np.where(rs.rand(g) < 0.5, 0.02, -0.01)      # both extremes duplicated: no column's absence changes the grid
        v[0], v[1] = 0.02, -0.01
    elif name in ('min_col0', 'min_col15', 'min_reg1'):
        v[{'min_col0': 0, 'min_col15': 15, 'min_reg1': 16 + 5}[name] % g] = -big       # a unique min: lo.n == 1 picks lo.b
    elif name in ('max_col0', 'max_col15', 'max_reg1'):
        v[{'max_col0': 0, 'max_col15': 15, 'max_reg1': 16 + 5}[name] % g] = big
    elif name in ('min_twice', 'min_twice_far'):
        v[3], v[g - 2] = -big, -big                         # lo.n == 2: leaving one copy out leaves the min where it is
    elif name in ('max_twice', 'max_twice_far'):            # *_far: both copies sit in columns of d = FAR_D and hardly count
        v[3], v[g - 2] = big, big                           # in any sum: only the multiplicity keeps them unflagged, and the
                                                            # group's range with both flagged is the body's
    elif name == 'signed_zeros':
        v[:] = np.where(np.arange(g) % 3 == 0, -0.0, 0.0)   # -0.0 == +0.0 counts towards the multiplicity
    elif name == 'zeros_and_values':
        v[:] = np.abs(body)
        v[1::4], v[2::4] = 0.0, -0.0                        # the min is a zero of either sign, several times
    else:
        raise KeyError(name)
    return v.astype(np.float32)


@functools.lru_cache(maxsize=None)
def planted(g):
    """B2: [4 * len(PLANTS), 384] on a diagonal U; row r holds PLANTS[r % len] in three groups: the first of block 0, one in
    the middle of block 1 and the last of block 2 (other registers, other lanes' stripes). Columns 3 and g - 2 of
    those groups has d = FAR_D, for the *_far plants. Returns (Wp, U, {row: [group, ...]})."""
    R, K = 4 * len(PLANTS), 384
    rs = np.random.RandomState(500 + g)
    Wp = (rs.randn(R, K) * 0.02).astype(np.float32)
    ng = K // g
    where = {}
    d = np.diag(diag_factor(K)).copy()
    for q in (0, ng // 2 - 1, ng // 2, ng - 1):
        d[q * g + 3] = d[(q + 1) * g - 2] = FAR_D
    U = np.diag(d)
    U.setflags(write=False)
    for r in range(R):
        groups = [0, ng // 2 - (r // len(PLANTS)) % 2, ng - 1]
        for q in groups:
            Wp[r, q * g:(q + 1) * g] = plant(PLANTS[r % len(PLANTS)], g, rs)
        where[r] = groups
    Wp.setflags(write=False)
    return Wp, U, where


def dead_inputs(R, K, n_dead, seed=0):
    """B3 / G: (W [R, K] fp32, H [K, K] fp32, dead channel indices). H comes from activations whose dead channels are zero."""
    rs = np.random.RandomState(9000 + K + seed)
    dead = np.sort(rs.choice(K, n_dead, replace=False))
    return weights(R, K, rs), hessian(K, rs, dead), dead


# ---- restatements for the conditions -------------------------------------------------------------------------------------------------

def tie_share(Wp, g):
    """share of groups whose min (max) is held by more than one column: (min share, max share)"""
    G = np.asarray(Wp).reshape(-1, g)
    lo = (G == G.min(1, keepdims=True)).sum(1) > 1
    hi = (G == G.max(1, keepdims=True)).sum(1) > 1
    return float(lo.mean()), float(hi.mean())


def detection_flags(G, d, bit, thr, assume_unique=False):
    """spqr.py:186-203 / 221 on groups G [n, g] that reach their group start as given, d [n, g] their diagonal of U: the
    leave-one-out flags (Base - Loo_j > threshold) in fp32, every sum ascending like oracle/csrc/spqr_canon.c.
    assume_unique: what comes out when a column that holds a copy of the min (max) is always taken for its only holder, so that
    the extreme without it is the next distinct value — the mistake a first / second extreme scheme makes when its multiplicity
    count is wrong. Where the two differ, the input can tell such a kernel from a right one."""
    f = np.float32
    G, d = np.asarray(G, f), np.asarray(d, f)
    n, g = G.shape
    qmax = f(2 ** bit - 1)

    def err2(x, mn, mx, dd):
        rng = np.maximum(mx - mn, f(1e-5)).astype(f)
        s = (rng / qmax).astype(f)
        z = (f(0) - (mn / s).astype(f)).astype(f)
        t = np.clip(np.rint(((x / np.maximum(s, f(1e-9))).astype(f) + z).astype(f)), f(0), qmax)
        e = ((((t - z).astype(f) * s).astype(f) - x).astype(f) / dd).astype(f)
        return (e * e).astype(f)

    def asum(a):
        acc = np.zeros(a.shape[0], f)
        for k in range(a.shape[1]):
            acc = (acc + a[:, k]).astype(f)
        return acc

    mn, mx = G.min(1, keepdims=True), G.max(1, keepdims=True)
    mn2 = np.where(G > mn, G, np.inf).min(1, keepdims=True).astype(f)          # next distinct values (inf: a constant group)
    mx2 = np.where(G < mx, G, -np.inf).max(1, keepdims=True).astype(f)
    base = asum(err2(G, mn, mx, d))
    flags = np.zeros((n, g), bool)
    for j in range(g):
        keep = np.arange(g) != j
        Gj, dj = G[:, keep], d[:, keep]
        lmn, lmx = Gj.min(1, keepdims=True), Gj.max(1, keepdims=True)
        if assume_unique:
            lmn = np.where((G[:, j:j + 1] == mn) & np.isfinite(mn2), mn2, lmn)
            lmx = np.where((G[:, j:j + 1] == mx) & np.isfinite(mx2), mx2, lmx)
        loo = asum(err2(Gj, lmn, lmx, dj))
        flags[:, j] = (base - loo).astype(f) > f(thr)
    return flags


def sample_rows(R, n_random, seed):
    """first 16, last 16 and n_random rows in between (rows of the column loop are independent given U and the threshold)"""
    rs = np.random.RandomState(seed)
    mid = rs.choice(np.arange(16, R - 16), n_random, replace=False) if R > 32 + n_random else np.arange(16, max(16, R - 16))
    return np.unique(np.concatenate([np.arange(min(16, R)), np.arange(max(0, R - 16), R), mid])).astype(np.int64)


def mask_share_ok(mask):
    """the finite-threshold cases must find outliers, and outliers must stay a minority: 1 <= count <= half the entries"""
    n = int(np.asarray(mask).sum())
    return 1 <= n <= np.asarray(mask).size // 2


def model_inputs(R, K, seed, device, tokens=2048):
    """F: (W [R, K] bf16, H [K, K] fp32) made with torch on `device`. H = X^T X of bf16 activations with log-normal channel
    scales and eight channels of 100x (the outlier channels of LLM activations); W as weights(): heavy columns and isolated
    outliers. `tokens` < K is fine: SpQR damps with the whole mean of the diagonal."""
    import torch
    gen = torch.Generator(device=device).manual_seed(seed)
    c = torch.exp(0.5 * torch.randn(K, generator=gen, device=device))
    c[torch.randperm(K, generator=gen, device=device)[:8]] *= 100.0
    X = (torch.randn((tokens, K), generator=gen, device=device) * c).to(torch.bfloat16).float()
    H = (X.T @ X) * (2.0 / tokens)
    W = torch.randn((R, K), generator=gen, device=device) * 0.02
    W[:, torch.randint(0, K, (6,), generator=gen, device=device)] *= 15
    n = R * K // 400
    W[torch.randint(0, R, (n,), generator=gen, device=device), torch.randint(0, K, (n,), generator=gen, device=device)] *= 25
    return W.to(torch.bfloat16), H
