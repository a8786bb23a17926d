"""Numpy oracle of the two token-selection kernels (csrc/token_select.hip, include/llmc_hip.h: llmc_cosine_dist,
llmc_maxmin_select) and of DivPrune's selection as the reference runs it (llmc/compression/token_reduction/divprune.py:13-53).

select(D, k)         the selection rules of the header, on a float matrix: bit for bit what llmc_maxmin_select returns and what the
                     reference's loop returns on the CPU (tools/make_golden_divprune.py asserts the latter on every recorded case).
truth_dist(x)        1 - cos of every pair of rows in fp64.
bound(d, dt)         the derived bound on |D - truth_dist| of llmc_cosine_dist, below.
exact_tokens(N, d, seed)   features on which every distance is exact in fp32, bf16 and f16 whatever the order of summation.

The bound. Write u = 2^-23 for the relative error of one addition of the accumulation and e = 2^-24 for an IEEE fp32 operation
rounded to nearest. u is one ulp and not half of one on purpose: the matrix pipe's adder is not documented to round to nearest,
and a truncating adder commits up to one ulp; the bound holds for either.
  * A product of two bf16 or two f16 values is exact in fp32 (8 + 8 and 11 + 11 significant bits, no underflow for features of
    ordinary size). A product of two fp32 values is rounded once. A sum of d terms in ANY order (any tree: a lane's chain, the
    instruction's internal order, the slices) passes every term through at most d - 1 additions, d with the rounding of an fp32
    product, so with n = d - 1 (16-bit) or n = d (fp32) and g = n u / (1 - n u) (Higham, Accuracy and Stability, lemma 3.1):
        |G^[i][j] - G[i][j]| <= g sum_k |x_ik x_jk| <= g |x_i| |x_j|                 (Cauchy-Schwarz)
    and on the diagonal, where every term is positive, G^[i][i] = |x_i|^2 (1 + t), |t| <= g.
  * sqrtf(G^[i][i]) = |x_i| sqrt(1 + t) (1 + e1) with sqrt(1 + t) inside [1 - g, 1 + g]; the product of the two square roots is
    rounded once more, the division once more. So the computed cosine is (c + a) / r with c the true cosine, |a| <= g, and
    1 / r <= M = 1 / ((1 - g) (1 - e)^4) (and 1 / r >= 2 - M, nearer to 1). With |c| <= 1:
        |c^ - c| <= |c| (M - 1) + g M <= (M - 1) + g M
  * D = fl(1 - c^) adds at most e |1 - c^| <= e (2 + (M - 1) + g M).
    bound = ((M - 1) + g M) (1 + e) + 2 e.
At d = 4096 this is 9.8e-4 for 16-bit features; no constant in it comes from a run. A zero row (0 / 0 = NaN) is outside it."""
import numpy as np

NAN_KEY = np.uint32(0xffffffff)


def keys(D):
    """float32 array -> uint32 keys whose integer order is the order of the header: numbers in their own order, -0 = +0, a NaN
    above every number and equal to every other NaN"""
    D = np.ascontiguousarray(D, dtype=np.float32)
    b = D.view(np.uint32).copy()
    b[b == np.uint32(0x80000000)] = 0
    neg = (b & np.uint32(0x80000000)) != 0
    k = np.where(neg, ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    k[np.isnan(D)] = NAN_KEY
    return k


def select(D, k):
    """D [N, N] (any float dtype numpy holds; bf16 matrices are passed as their exact float32 values) -> int64 [k]."""
    K = keys(D)
    N = K.shape[0]
    if K.ndim != 2 or K.shape[1] != N or N < 2 or k < 0:
        raise ValueError('select takes an N x N matrix with N >= 2 and k >= 0')
    sel = np.empty(k, np.int64)
    score = None
    for i in range(k):
        if i == 0:
            score = np.partition(K, 1, axis=0)[1]                          # the second smallest of every column, NaN last
        elif i == 1:
            score = K[sel[0]].copy()                                       # the chosen rows only: step 1 starts again
        else:
            row = K[sel[i - 1]]
            score = np.where((score == NAN_KEY) | (row == NAN_KEY), NAN_KEY, np.minimum(score, row))
        sel[i] = int(np.argmax(score))                                     # the first of the greatest keys
    return sel


def truth_dist(x):
    x = np.asarray(x, np.float64)
    G = x @ x.T
    n = np.sqrt(np.diag(G))
    with np.errstate(invalid='ignore', divide='ignore'):
        return 1.0 - G / np.outer(n, n)


def bound(d, dt):
    u, e = 2.0 ** -23, 2.0 ** -24
    n = d if dt == 'f32' else d - 1
    g = n * u / (1.0 - n * u)
    M = 1.0 / ((1.0 - g) * (1.0 - e) ** 4)
    return ((M - 1.0) + g * M) * (1.0 + e) + 2.0 * e


def golden_matrix(g, case):
    """the recorded matrix of a group (a) case of tests/golden/divprune.npz as a torch tensor of its dtype"""
    import torch
    dt = str(g[f'{case}/dt'])
    b = g[f'{case}/D_bits']
    if dt == 'f32':
        return torch.from_numpy(b.view(np.int32).copy()).view(torch.float32)
    return torch.from_numpy(b.view(np.int16).copy()).view(torch.bfloat16 if dt == 'bf16' else torch.float16)


EXACT_SHAPES = ((97, 40, 48), (130, 520, 65), (300, 4096, 60))             # (N, d, k) of the exact goldens


def exact_tokens(N, d, seed):
    """float32 [N, d]: every token has 4, 16 or 64 (as many as fit in d) components of +-1 times one power of two 2^-2 .. 2^2, on
    positions drawn from a pool of min(d, 128) columns spread evenly over the row. Every norm is a power of two and every dot
    product a small integer times one, so every cosine is m / 2^p with |m| <= 64 and 2^p <= 64: exact in fp32, bf16 and f16, as
    the features themselves are, in any order of summation. About one token in eight repeats an earlier one (a duplicate)."""
    rng = np.random.RandomState(seed)
    pool = (np.arange(min(d, 128), dtype=np.int64) * d) // min(d, 128)
    counts = [c for c in (4, 16, 64) if c <= len(pool)]
    x = np.zeros((N, d), np.float32)
    for i in range(N):
        if i > 0 and rng.randint(8) == 0:
            x[i] = x[rng.randint(i)]
            continue
        c = counts[rng.randint(len(counts))]
        pos = pool[rng.permutation(len(pool))[:c]]
        x[i, pos] = (rng.randint(2, size=c) * 2 - 1) * 2.0 ** rng.randint(-2, 3)
    return x
