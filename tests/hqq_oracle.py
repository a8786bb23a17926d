"""numpy restatement of HQQ's solver (llmc/compression/quantization/quant.py:588-610, hqq.py:36-60) as llmc_hqq_optimize
computes it: fp32 with one rounding per op, the group mean in ATen's CPU inner-sum order, pow in fp64 by the kernel's
own + - * / sequence (pow_f64), the tensor-wide error summed in fp64 and compared as fp32. Test infrastructure only."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.aten_sum import row_sum  # noqa: E402

f32, f64 = np.float32, np.float64


def inner_sum_fp32(x, V=8):
    """x [G, n] fp32, n a multiple of V: torch.sum(x, -1) on the CPU (SumKernel.cpp vectorized_inner_sum with
    Vectorized<float> of V lanes: row_sum over the vectors, then the lane sums added in order, from +0)."""
    G, n = x.shape
    nv = n // V
    if nv * V != n or nv < 1:
        raise NotImplementedError('inner sums of a multiple of one vector only')
    loads = np.ascontiguousarray(x, dtype=f32).reshape(G, nv, V)
    acc = row_sum(np.moveaxis(loads, 1, 0))                 # [G, V]
    fin = np.zeros(G, f32)
    for lane in range(V):
        fin = (fin + acc[:, lane]).astype(f32)
    return fin


def pow_f64(x, p):
    """llmc_amd/csrc/hqq.hip pow_f64 op for op: x >= 0 finite (fp64 array), p a double."""
    x = np.asarray(x, f64)
    out = np.empty_like(x)
    zero = x == 0
    out[zero] = np.inf if p < 0 else (1.0 if p == 0 else 0.0)
    xs = x[~zero]
    m, e = np.frexp(xs)
    small = m < 0.70710678118654752440
    m = np.where(small, m * 2.0, m)
    e = np.where(small, e - 1, e)
    s = (m - 1.0) / (m + 1.0)
    s2 = s * s
    pl = np.full_like(s, 1.0 / 23.0)
    for k in range(10, -1, -1):
        pl = pl * s2 + 1.0 / float(2 * k + 1)
    ln2 = 0.6931471805599453
    y = p * (e.astype(f64) * ln2 + (2.0 * s) * pl)
    kf = np.rint(y * 1.4426950408889634)
    r = y - kf * ln2
    inv_fact = [1.0, 1.0, 1.0 / 2.0, 1.0 / 6.0, 1.0 / 24.0, 1.0 / 120.0, 1.0 / 720.0, 1.0 / 5040.0, 1.0 / 40320.0,
                1.0 / 362880.0, 1.0 / 3628800.0, 1.0 / 39916800.0, 1.0 / 479001600.0, 1.0 / 6227020800.0]
    pe = np.full_like(r, inv_fact[13])
    for n in range(12, -1, -1):
        pe = pe * r + inv_fact[n]
    out[~zero] = np.ldexp(pe, kf.astype(np.int64))
    return out


def shrink_consts(lp_norm, beta):
    """(c, p1) as ATen meets the reference's Python scalars: 1.0 / beta in double cast to fp32; lp_norm - 1 cast to fp32."""
    return f32(1.0 / beta), f32(lp_norm - 1)


def minmax_qparams(Wg, sym, round_zp, qmin, qmax):
    """get_qparams (quant.py:545-559) on the fp32 groups Wg [G, g] -> (s, z) fp32 [G]."""
    mn, mx = Wg.min(axis=1), Wg.max(axis=1)
    qmin, qmax = f32(qmin), f32(qmax)
    eps = f32(1e-5)
    if sym:
        a = np.maximum(np.maximum(np.abs(mx), np.abs(mn)), eps)
        return (a / qmax).astype(f32), np.zeros(Wg.shape[0], f32)
    s = (np.maximum((mx - mn).astype(f32), eps) / f32(qmax - qmin)).astype(f32)
    r = (mn / s).astype(f32)
    if round_zp:
        z = np.clip((qmin - np.rint(r)).astype(f32), qmin, qmax).astype(f32)
    else:
        z = (qmin - r).astype(f32)
    return s, z


def groups(W, axis, g):
    """the reference's [G, g] view of W.float() (axis 1) or W.float().T (axis 0); a last dim shorter than g stays whole."""
    t = np.asarray(W, f32)
    if axis == 0:
        t = t.T
    n = t.shape[-1]
    gg = g if n >= g else n
    return np.ascontiguousarray(t).reshape(-1, gg)


def solve(Wg, s, z, qmin, qmax, lp_norm, beta, iters, stop_at=None):
    """optimize_weights_proximal from (s, z) on the groups Wg [G, g] -> dict(scales, zeros, T, errs (fp64 means),
    errs32, flagged (groups with an fp64 pow result within 4 fp64 ulps of an fp32 rounding midpoint)).
    stop_at: run exactly to that iteration (T) instead of applying the rule."""
    Wg = np.asarray(Wg, f32)
    G, g = Wg.shape
    N = Wg.size
    c, p1 = shrink_consts(lp_norm, beta)
    qmin, qmax = f32(qmin), f32(qmax)
    inv = (f32(1.0) / np.asarray(s, f32).reshape(G)).astype(f32)
    z = np.asarray(z, f32).reshape(-1)
    if z.size == 1 and G > 1:
        z = np.full(G, z[0], f32)
    best = f32(1e4)
    errs, errs32 = [], []
    T = iters - 1
    flagged = np.zeros(G, bool)
    with np.errstate(divide='ignore', over='ignore', invalid='ignore'):
        for i in range(iters):
            zc = z[:, None]
            xi = (Wg * inv[:, None]).astype(f32)
            q = np.rint((xi + zc).astype(f32))
            q = np.minimum(np.maximum(q, qmin), qmax).astype(f32)
            r = ((q - zc).astype(f32) / inv[:, None]).astype(f32)
            d = (Wg - r).astype(f32)
            ad = np.abs(d)
            if lp_norm == 1:
                rl = np.maximum((ad - c).astype(f32), f32(0))
            else:
                pw64 = pow_f64(ad.astype(f64), float(p1))
                pw = pw64.astype(f32)
                rl = np.maximum((ad - (c * pw).astype(f32)).astype(f32), f32(0))
                # near-midpoint pows (a correctly rounded pow could round the other way), where the shrink is live
                fin = np.isfinite(pw64) & (pw64 > 0) & (rl > 0)
                if fin.any():
                    lo = np.nextafter(pw, f32(0)).astype(f64)
                    hi = np.nextafter(pw, f32(np.inf)).astype(f64)
                    pv = pw.astype(f64)
                    mid_lo, mid_hi = (lo + pv) / 2, (pv + hi) / 2
                    ulp = np.spacing(pw64)
                    near = (np.abs(pw64 - mid_lo) <= 4 * ulp) | (np.abs(pw64 - mid_hi) <= 4 * ulp)
                    flagged |= (near & fin).any(axis=1)
            e = (np.sign(d) * rl).astype(f32)
            t = (q - ((Wg - e).astype(f32) * inv[:, None]).astype(f32)).astype(f32)
            znew = (inner_sum_fp32(t) / f32(g)).astype(f32)
            m = ad.astype(f64).sum() / N
            errs.append(m)
            errs32.append(f32(m))
            z = znew
            if stop_at is not None:
                if i == stop_at:
                    T = i
                    break
                continue
            if f32(m) < best:
                best = f32(m)
            else:
                T = i
                break
    scales = (f32(1.0) / inv).astype(f32)
    return dict(scales=scales, zeros=z, T=T if iters > 0 else -1, errs=np.array(errs, f64),
                errs32=np.array(errs32, f32), flagged=flagged)


def reference_T(errs32):
    """the stop iteration the rule gives on a list of fp32 errors (len(errs32) - 1 when it runs out)"""
    best = f32(1e4)
    for i, e in enumerate(errs32):
        if f32(e) < best:
            best = f32(e)
        else:
            return i
    return len(errs32) - 1
