"""Numpy restatement of FloatQuantizer on the narrow float grids e2m1 (FP4) and e3m2 (FP6): the reference's arithmetic
(quant.py:545-553, 1061-1081 with qmax = tensor(6) / tensor(28)) around two roundings, plus the stored form. Test
infrastructure, beside tests/gptq_fp8_oracle.py; tests/test_fp4_oracle.py pins it to the reference's own output
(tests/golden/fp4.npz).

  'qtorch'  oracle.quant_ref.qtorch_float_quantize(x, E, M), called unchanged: ties away from zero, the top exponent code kept
            for infinity, so the grid ends at 3 (e2m1) / 14 (e3m2); a zero result is +0.
  'ocp'     nearest, ties to the even code, onto the EXPLICIT list of OCP values, saturating at 6 / 28 (infinities too); a NaN
            gives the maximum with the input's sign; the sign survives on a zero result.
Scales: absmax.clamp(1e-5) / qmax rounded to the tensor dtype (the integer 0-dim qmax never promotes), or the OCP MX rule as
e8m0 bytes (then the quotient is exact and is not rounded to the tensor dtype).
"""
import numpy as np

from oracle import quant_ref as Q

F32 = np.float32
FORMATS = {'e2m1': (2, 1, 6.0), 'e3m2': (3, 2, 28.0)}          # (E, M, qmax = the OCP maximum)
QTORCH_MAX = {'e2m1': 3.0, 'e3m2': 14.0}
EMAX = {'e2m1': 2, 'e3m2': 4}


def ocp_values(bit):
    """The non-negative values of the OCP format in code order (index = code without the sign bit)."""
    E, M, _ = FORMATS[bit]
    bias = 2 ** (E - 1) - 1
    out = []
    for e in range(2 ** E):
        for m in range(2 ** M):
            out.append(m * 2.0 ** (1 - bias - M) if e == 0 else (1 + m * 2.0 ** -M) * 2.0 ** (e - bias))
    return np.array(out, dtype=np.float64)


def decode(codes, bit):
    """code -> value (fp32); the sign bit sits on top of the E + M magnitude bits, -0 keeps its sign."""
    E, M, _ = FORMATS[bit]
    codes = np.asarray(codes).astype(np.int64)
    mag = ocp_values(bit)[codes & (2 ** (E + M) - 1)]
    return np.where((codes >> (E + M)) & 1 == 1, -mag, mag).astype(F32)


def encode(v, bit):
    """value ON the OCP grid -> code (uint8)."""
    E, M, _ = FORMATS[bit]
    v = np.asarray(v, dtype=F32)
    vals = ocp_values(bit)
    idx = np.searchsorted(vals, np.abs(v).astype(np.float64))
    assert np.array_equal(vals[np.minimum(idx, len(vals) - 1)], np.abs(v).astype(np.float64)), 'value off the grid'
    return (idx | (np.signbit(v).astype(np.int64) << (E + M))).astype(np.uint8)


def ocp_quantize(t, bit):
    t = np.ascontiguousarray(t, dtype=F32)
    vals = ocp_values(bit)
    a = np.abs(t).astype(np.float64)
    a = np.where(np.isnan(a), np.inf, a)
    hi = np.clip(np.searchsorted(vals, a, side='left'), 1, len(vals) - 1)      # vals[hi - 1] <= a <= vals[hi] inside the range
    lo = hi - 1
    dl, dh = a - vals[lo], vals[hi] - a
    pick = np.where(dl < dh, lo, np.where(dh < dl, hi, np.where(lo % 2 == 0, lo, hi)))       # tie: the even code
    pick = np.where(a >= vals[-1], len(vals) - 1, pick)
    sign = (t.view(np.uint32) >> 31).astype(bool)
    return np.where(sign, -vals[pick], vals[pick]).astype(F32)


def quantize(t, bit, sem):
    if sem == 'qtorch':
        E, M, _ = FORMATS[bit]
        return Q.qtorch_float_quantize(t, E, M)
    assert sem == 'ocp'
    return ocp_quantize(t, bit)


def e8m0_codes(absmax, bit):
    """clamp(floor(log2(absmax)) - emax + 127, 0, 254), 127 for an all-zero row; absmax fp32 (frexp: exact)."""
    absmax = np.asarray(absmax, dtype=F32)
    _, ex = np.frexp(absmax.astype(np.float64))
    code = np.clip(ex - 1 - EMAX[bit] + 127, 0, 254)
    return np.where(absmax == 0, 127, code).astype(np.uint8)


def e8m0_values(codes):
    return np.ldexp(1.0, np.asarray(codes).astype(np.int64) - 127).astype(F32)


def mul_cols(w, cols, dt):
    """awq_ops.mul_cols_: fp32 product, rounded to the tensor dtype."""
    return Q.rnd((np.asarray(w, F32) * np.asarray(cols, F32)[None, :]).astype(F32), dt)


def run(w2d, dt, bit, sem='qtorch', scale_format='dtype', scales=None, sdt=None):
    """One FloatQuantizer step on the [G, g] view (fp32 container of dt values). scales None: dynamic. Else static: fp32
    container [G, 1] of values of dtype sdt, or uint8 e8m0 codes.
    Returns dict: scales_raw (what get_qparams returns), scales (after `scales[scales == 0] = 1`), codes, values, fake."""
    _, _, qmax = FORMATS[bit]
    w2d = np.ascontiguousarray(w2d, dtype=F32)
    G = w2d.shape[0]
    out = {}
    with np.errstate(over='ignore', invalid='ignore', divide='ignore', under='ignore'):
        if scale_format == 'e8m0':
            assert sem == 'ocp'
            codes = e8m0_codes(np.abs(w2d).max(axis=-1, keepdims=True), bit) if scales is None else np.asarray(scales, np.uint8).reshape(G, 1)
            out['scales_raw'] = out['scales'] = codes
            s = e8m0_values(codes)
            t = ((w2d / s).astype(F32) + F32(0.0)).astype(F32)                    # exact: not rounded to dt
        else:
            if scales is None:
                a = np.maximum(np.nanmax(np.abs(w2d), axis=-1, keepdims=True), Q.rnd(F32(1e-5), dt))
                sdt = dt                                                          # bf16 / int64 -> bf16, 0-dim or not
                raw = Q.rnd((a / F32(qmax)).astype(F32), sdt)
            else:
                raw = np.asarray(scales, F32).reshape(G, 1)
            out['scales_raw'] = raw
            s = np.where(raw == 0, F32(1.0), raw).astype(F32)                    # quant.py:1062
            out['scales'] = s
            tdt = dt if G == 1 else Q.promote(dt, sdt)                            # a 0-dim scale does not promote the tensor
            t = Q.rnd(Q.rnd((w2d / s).astype(F32), tdt) + F32(0.0), tdt)
        t = np.where(np.isnan(w2d), w2d, t)                                       # a NaN keeps its sign
        v = quantize(t, bit, sem)
        out['values'] = v
        out['codes'] = encode(v, bit)
        out['fake'] = Q.rnd((v * s).astype(F32), dt)                              # fp32 product, one rounding
    return out


def pack_fp4(codes):
    """[R, K] e2m1 codes -> [R, K / 2]: element 2i in the low nibble, 2i + 1 in the high one."""
    c = np.asarray(codes, dtype=np.uint8)
    return ((c[:, 0::2] & 0xf) | ((c[:, 1::2] & 0xf) << 4)).astype(np.uint8)


def bits16(a, dt):
    """fp32 container of dt values -> their 16-bit patterns."""
    a = np.ascontiguousarray(a, dtype=F32)
    if dt == 'bf16':
        return (a.view(np.uint32) >> 16).astype(np.uint16)
    return a.astype(np.float16).view(np.uint16)


def from_bits16(b, dt):
    b = np.ascontiguousarray(b, dtype=np.uint16)
    if dt == 'bf16':
        return (b.astype(np.uint32) << 16).view(F32)
    return b.view(np.float16).astype(F32)
