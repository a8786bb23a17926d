"""Numpy restatement of the OCP MX path (csrc/mx_gemm.hip): the activation quantizer per 1 x 32 block (e2m1 or e4m3 codes +
e8m0 scale bytes) and the block-scaled product in fp64, with the condition under which that product is exact in fp32 in every
summation order. Test infrastructure beside tests/fp4_oracle.py, whose e2m1 / e8m0 helpers it uses; tests/test_mx_config.py pins
the e4m3 encoder to torch's own cast.

Rules of the activation quantizer (include/llmc_hip.h, llmc_mx_act_quant):
  absmax   fmax over |x| starting from 0: a NaN element is ignored, an infinity gives the exponent field 255
  scale    byte = clamp(exponent_field(absmax) - emax, 0, 254), 127 for an all-zero block; emax = 2 (e2m1), 8 (e4m3)
  t        x * 2^(127 - byte) + 0 in fp32 (exact; the + 0 turns a -0 product into +0), a NaN keeps its bits
  e2m1     fp4_oracle.ocp_quantize: nearest even onto the OCP grid, saturating at 6, NaN -> 6 with the input's sign
  e4m3     nearest even, saturating at 448 (infinities too), NaN -> code 0x7f with the input's sign
"""
import numpy as np

import fp4_oracle as O

F32 = np.float32
BLOCK = 32
EMAX = {'e2m1': 2, 'e4m3': 8}


# ---- e4m3 (OCP e4m3fn) --------------------------------------------------------------------------------------------------------
def e4m3_decode(codes):
    c = np.asarray(codes).astype(np.int64)
    e, m = (c >> 3) & 0xf, c & 7
    mag = np.where(e == 0, m * 2.0 ** -9, (1 + m / 8.0) * 2.0 ** (e - 7.0))
    mag = np.where((c & 0x7f) == 0x7f, np.nan, mag)
    return np.where(c & 0x80, -mag, mag).astype(F32)


def e4m3_encode(t):
    """fp32 -> e4m3fn code: round to nearest even; |t| above 448 (an infinity too) SATURATES to 448 (torch's cast gives NaN
    there); a NaN gives 0x7f; the sign bit is the input's, also on a zero result."""
    t = np.ascontiguousarray(t, dtype=F32)
    b = t.view(np.uint32)
    sign = ((b >> 24) & 0x80).astype(np.uint32)
    ab = b & 0x7fffffff
    nan = ab > 0x7f800000
    ax = np.minimum(np.where(nan, 0, ab).astype(np.uint32).view(F32), F32(448.0))
    sub = np.rint(ax.astype(np.float64) * 512.0).astype(np.uint32)                 # below 2^-6: multiples of 2^-9, ties to even
    a2 = ax.view(np.uint32)
    r = (a2 + 0x7ffff + ((a2 >> 20) & 1)) & 0xfff00000                            # 3 mantissa bits, ties to even, carry into the exponent
    nrm = ((((r >> 23).astype(np.int64) - 120) << 3) | ((r >> 20) & 7)).astype(np.uint32)
    code = np.where(ax < F32(2.0 ** -6), sub, nrm)
    return (np.where(nan, 0x7f, code) | sign).astype(np.uint8)


# ---- the activation quantizer ---------------------------------------------------------------------------------------------------
def block_scales(x, bit):
    """e8m0 bytes [M, K / 32] of x [M, K] (fp32 container)."""
    x = np.ascontiguousarray(x, dtype=F32)
    M, K = x.shape
    am = np.fmax.reduce(np.abs(x.reshape(M, K // BLOCK, BLOCK)), axis=-1, initial=F32(0.0)).astype(F32)      # fmax: NaN ignored
    field = ((am.view(np.uint32) >> 23) & 0xff).astype(np.int64)
    return np.where(am == 0, 127, np.clip(field - EMAX[bit], 0, 254)).astype(np.uint8)


def act_quant(x, bit):
    """x [M, K] fp32 container of bf16 / fp16 values -> (codes, scales): e2m1 codes packed [M, K / 2], e4m3 codes [M, K]."""
    x = np.ascontiguousarray(x, dtype=F32)
    M, K = x.shape
    s = block_scales(x, bit)
    with np.errstate(all='ignore'):
        rs = np.ldexp(1.0, 127 - s.astype(np.int64)).astype(F32)                   # 2^127 .. 2^-127 (an fp32 subnormal)
        t = ((x.reshape(M, K // BLOCK, BLOCK) * rs[..., None]).astype(F32) + F32(0.0)).astype(F32).reshape(M, K)
        t = np.where(np.isnan(x), x, t)
        if bit == 'e2m1':
            return O.pack_fp4(O.encode(O.ocp_quantize(t, 'e2m1'), 'e2m1')), s
        return e4m3_encode(t), s


# ---- the block-scaled product ----------------------------------------------------------------------------------------------------
def unpack_fp4(packed):
    p = np.asarray(packed, dtype=np.uint8)
    out = np.empty((p.shape[0], p.shape[1] * 2), np.uint8)
    out[:, 0::2], out[:, 1::2] = p & 0xf, p >> 4
    return out


def values(codes, bit):
    """codes [R, K] (one per byte) -> fp64 values"""
    return (O.decode(codes, 'e2m1') if bit == 'e2m1' else e4m3_decode(codes)).astype(np.float64)


def scaled(codes, scales, bit):
    """value * 2^(scale - 127) per 32-block, fp64 (exact)"""
    v = values(codes, bit)
    R, K = v.shape
    return (v.reshape(R, K // BLOCK, BLOCK) * np.ldexp(1.0, np.asarray(scales).astype(np.int64) - 127)[..., None]).reshape(R, K)


def gemm(a_codes, a_s, a_bit, b_codes, b_s):
    """(C, S): C[m, n] = sum_kb 2^(a_s + b_s - 254) sum_k a b in fp64, and S = the same sum over |a b| (the error bounds' scale)."""
    A, B = scaled(a_codes, a_s, a_bit), scaled(b_codes, b_s, 'e2m1')
    return A @ B.T, np.abs(A) @ np.abs(B).T


def _granularity(v):
    """the largest power of two that divides every non-zero value of v (fp64 array of format values)"""
    nz = np.abs(v[v != 0])
    if nz.size == 0:
        return 1.0
    m, e = np.frexp(nz)                                  # nz = m 2^e, m in [0.5, 1) with at most 24 significant bits
    mi = np.round(m * 2.0 ** 24).astype(np.int64)
    low = mi & -mi                                       # lowest set bit
    return float(np.min(np.ldexp(low.astype(np.float64), e - 24)))


def exact_in_any_order(a_codes, a_s, a_bit, b_codes, b_s):
    """The condition under which every partial sum of C[m, n], in every order, is an fp32 number: all terms are multiples of the
    quantum q[m, n] = gran(a) gran(b) 2^(min_kb (a_s + b_s) - 254) and sum |terms| < 2^24 q. Returns (holds, worst ratio)."""
    _, S = gemm(a_codes, a_s, a_bit, b_codes, b_s)
    g = _granularity(values(a_codes, a_bit)) * _granularity(values(b_codes, 'e2m1'))
    sa, sb = np.asarray(a_s).astype(np.int64), np.asarray(b_s).astype(np.int64)
    mn = np.full(S.shape, 1 << 30, np.int64)
    for kb in range(sa.shape[1]):
        mn = np.minimum(mn, sa[:, kb, None] + sb[None, :, kb])
    q = g * np.ldexp(1.0, mn - 254)
    ratio = float((S / q).max())
    return ratio < 2.0 ** 24, ratio


def truncating_adder_bound(S, K):
    """|C - C_ref| of an fp32 accumulation of K exact products in ANY order with an adder that rounds or truncates: each of at
    most K additions loses at most one unit roundoff 2^-23 of a partial sum bounded by S."""
    return K * 2.0 ** -23 * S


def half_ulp(x, dt):
    """half a unit in the last place of dtype dt ('bf16', 'f16', 'f32') at magnitude |x| (normal range; the subnormal spacing below it)"""
    p, emin = {'bf16': (8, -126), 'f16': (11, -14), 'f32': (24, -126)}[dt]
    _, e = np.frexp(np.abs(x))
    return 0.5 * np.ldexp(1.0, np.maximum(e - 1, emin) - (p - 1))
