"""llmc_block_influence (csrc/block_influence.hip) restated in numpy in the order include/llmc_hip.h states, bit for bit, beside an
fp64 truth and the bound that separates the two. Values are float32 arrays that are exact in the tensors' dtype.

The stated order. v = 16 / sizeof(dtype) elements make a slot; lane l of 64 folds the slots l, l + 64, ... of a row, the elements
of a slot in index order, onto three fp32 sums from +0 (s = s + x * y, product and add rounded separately); the 64 lane values
are joined by the xor butterfly with the offsets 32, 16, 8, 4, 2, 1. Then sim = dot / (sqrt(sx) * sqrt(sy)), NaN -> 0.5,
+-inf -> +-FLT_MAX, bi = 1 - sim. The total is an fp64 sum: chunks of 4096 rows, thread t of 256 adds the rows t, t + 256, ... of
its chunk from 0, a tree s = 128 .. 1 (v[t] += v[t + s]) joins the 256 values; the chunk values are summed the same way.

The bound on |bi - truth| for one token (`bound`), u = 2^-24, gamma(k) = k u / (1 - k u), no overflow or underflow:
  * a lane folds at most L = v * ceil(ceil(d / v) / 64) elements, so a product goes through at most k = 1 + L + 6 roundings
    before it is part of a row sum: its own, L adds of the lane chain, 6 of the butterfly. Hence
      |dot^ - dot| <= gamma(k) * sum |x y| <= gamma(k) * ||x|| ||y||      (Cauchy-Schwarz: sum |x y| / (||x|| ||y||) <= 1)
      sx^ = sx (1 + t), |t| <= gamma(k), likewise sy (all terms positive).
  * the denominator takes two square roots and one product, three more roundings, and a square root halves a relative error:
      den^ = ||x|| ||y|| (1 + th), |th| <= g = gamma(k + 3).
  * the division rounds once: sim^ = (sim + r) (1 + e) / (1 + th) with |r| <= gamma(k), |e| <= u. With |sim| <= 1 and
    phi = (u + g) / (1 - g):  |sim^ - sim| <= phi + gamma(k) (1 + phi) =: E.
  * bi = fl(1 - sim^) rounds once more, |1 - sim^| <= 2 + E:  |bi - truth| <= E + u (2 + E).
To first order this is (2 L + 20) u. A token whose cosine is NaN (a zero row) is 0.5 on both sides. The truth's own fp64
arithmetic (about d * 2^-53) is three hundred million times smaller and is not counted. A total over N tokens lies within
N * bound of the truth's; its fp64 adds are not counted either."""
import math

import numpy as np

from kvquant_oracle import as_f32, to_bits  # noqa: F401  (the bit-pattern helpers are the same)

VEC = {'bf16': 8, 'f16': 8, 'f32': 4}
CHUNK = 4096
U = 2.0 ** -24
FLT_MAX = np.float32(np.finfo(np.float32).max)


def lane_elements(d, dt):
    """L: the most elements one lane folds"""
    v = VEC[dt]
    return v * math.ceil(math.ceil(d / v) / 64)


def bound(d, dt):
    k = 1 + lane_elements(d, dt) + 6
    gamma = lambda n: n * U / (1 - n * U)      # noqa: E731
    g = gamma(k + 3)
    phi = (U + g) / (1 - g)
    E = phi + gamma(k) * (1 + phi)
    return E + U * (2 + E)


def row_sums(x, y, dt):
    """x, y float32 [N, d] -> (dot, sx, sy) float32 [N] in the kernel's order"""
    x, y = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(y, np.float32)
    N, d = x.shape
    v = VEC[dt]
    nslot = -(-d // v)
    lanes = np.arange(64)
    acc = [np.zeros((N, 64), np.float32) for _ in range(3)]
    for first in range(0, nslot, 64):                     # slot l + first of lane l
        for e in range(v):
            idx = (lanes + first) * v + e
            on = lanes[idx < d]
            if on.size == 0:
                continue
            a, b = x[:, idx[on]], y[:, idx[on]]
            for s, p in zip(acc, (a * b, a * a, b * b)):
                s[:, on] = s[:, on] + p
    out = []
    for s in acc:
        for o in (32, 16, 8, 4, 2, 1):
            s = s + s[:, lanes ^ o]
        out.append(s[:, 0].copy())
    return out


def block_influence(x, y, dt):
    """-> bi float32 [N], the kernel's bits"""
    with np.errstate(all='ignore'):
        dot, sx, sy = row_sums(x, y, dt)
        sim = dot / (np.sqrt(sx) * np.sqrt(sy))
    sim = np.where(np.isnan(sim), np.float32(0.5), sim)
    sim = np.where(np.isposinf(sim), FLT_MAX, np.where(np.isneginf(sim), -FLT_MAX, sim)).astype(np.float32)
    return np.float32(1.0) - sim


def _tree256(v):
    for s in (128, 64, 32, 16, 8, 4, 2, 1):
        v = v[..., :s] + v[..., s:2 * s]
    return v[..., 0]


def _strided_sum(v):
    """v float64 [G, n]: per group, thread t of 256 adds the elements t, t + 256, ... from 0, then the tree. A trailing + 0.0
    leaves an fp64 sum that started at +0 as it is, so the groups are padded with zeros."""
    G, n = v.shape
    rounds = -(-n // 256)
    p = np.zeros((G, rounds * 256), np.float64)
    p[:, :n] = v
    a = np.zeros((G, 256), np.float64)
    for i in range(rounds):
        a = a + p[:, i * 256:(i + 1) * 256]
    return _tree256(a)


def total(bi, running=None):
    """the fp64 sum of bi in the kernel's order; running: the total it is folded into (total = total + batch)"""
    bi = np.asarray(bi, np.float32).astype(np.float64)
    nchunk = -(-bi.size // CHUNK)
    p = np.zeros(nchunk * CHUNK, np.float64)
    p[:bi.size] = bi
    batch = _strided_sum(_strided_sum(p.reshape(nchunk, CHUNK))[None])[0]
    return batch if running is None else np.float64(running) + batch


def truth(x, y):
    """-> bi float64 [N]: the same quantity in fp64, 0.5 where the cosine is NaN"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    with np.errstate(all='ignore'):
        sim = (x * y).sum(-1) / (np.sqrt((x * x).sum(-1)) * np.sqrt((y * y).sum(-1)))
    return 1.0 - np.nan_to_num(sim, nan=0.5)


def golden_case(g, name):
    """-> dt, x, y (float32 [N, d]), ref_bi (float32 [N]: the reference's values, exact), ref_total, ref_dist"""
    dt = str(g[name + '/dt'])
    shape = tuple(int(s) for s in g[name + '/shape'])
    src = str(g[name + '/source'])
    x = as_f32(g[src + '/x_bits'], dt).reshape(-1, shape[-1]).copy()
    y = as_f32(g[src + '/y_bits'], dt).reshape(-1, shape[-1]).copy()
    if int(g[name + '/zero_token']) >= 0:
        x[int(g[name + '/zero_token'])] = 0
    if int(g[name + '/same']):
        y = x.copy()
    return dt, x, y, g[name + '/ref_bi'], float(g[name + '/ref_total']), float(g[name + '/ref_dist'])
