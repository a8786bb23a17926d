// fp8_math.h — OCP e4m3fn conversions shared by fp8_quant.hip, fp4_quant.hip and fp8_block.hip (the quantizer step around them: float_quant_math.h). Rounding is pinned to torch.float8_e4m3fn's
// cast (round to nearest even, no saturation: a value that rounds above 448 becomes NaN).
#pragma once
#include "common.h"

namespace llmc {

// fp32 -> e4m3fn bits with torch's semantics
__device__ __forceinline__ uint8_t f32_to_e4m3fn(float x) {
    const uint32_t b = __float_as_uint(x);
    const uint32_t sign = (b >> 24) & 0x80u;
    const uint32_t ab = b & 0x7fffffffu;
    if (ab > 0x7f800000u) return (uint8_t)(sign | 0x7f);  // NaN
    const float ax = __uint_as_float(ab);
    if (ax < 0.015625f) {  // below 2^-6: subnormal grid 2^-9 (rint = RNE); 8 -> smallest normal
        const uint32_t m = (uint32_t)rintf(ax * 512.0f);
        return (uint8_t)(sign | m);
    }
    // round the fp32 mantissa to 3 bits, RNE, carry propagates into the exponent
    uint32_t r = ab + 0x7ffffu + ((ab >> 20) & 1u);
    r &= 0xfff00000u;
    if (r > 0x43e00000u) return (uint8_t)(sign | 0x7f);  // > 448 after rounding (incl. inf) -> NaN
    const uint32_t e = (r >> 23) - 127 + 7;
    const uint32_t m = (r >> 20) & 7u;
    return (uint8_t)(sign | (e << 3) | m);
}

// Two values at once on v_cvt_pk_fp8_f32 (gfx950: OCP e4m3fn, round to nearest even). Measured against the routine above over
// 4 M bit patterns (tools/probes/fp8_mfma_probe.hip, profiles/r03_fp8_mfma_probe.txt): identical for every finite |x| <= 464
// (= everything that rounds to a finite e4m3 value, subnormals included); NaN and overflow differ (sign of the NaN code), so
// those take the routine above. Result: code of x in bits 0-7, of y in bits 8-15.
__device__ __forceinline__ uint32_t f32x2_to_e4m3fn(float x, float y) {
    if (__builtin_expect(!(fabsf(x) <= 464.0f) || !(fabsf(y) <= 464.0f), 0))
        return (uint32_t)f32_to_e4m3fn(x) | ((uint32_t)f32_to_e4m3fn(y) << 8);
    return (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(x, y, 0, false) & 0xffffu;
}

__device__ __forceinline__ float e4m3fn_to_f32(uint8_t v) {
    const uint32_t e = (v >> 3) & 0xf, m = v & 7;
    float r;
    if ((v & 0x7f) == 0x7f) r = __uint_as_float(0x7fc00000u);
    else if (e == 0) r = (float)m * 0.001953125f;
    else r = __uint_as_float(((e - 7 + 127) << 23) | (m << 20));
    // sign by bit: a negative zero must stay negative ((q - 0) * s = -0.0 in the reference)
    return __uint_as_float(__float_as_uint(r) | ((uint32_t)(v & 0x80) << 24));
}

// ---- e5m2 (torch.float8_e5m2: IEEE-style binary8, round to nearest even, overflow -> inf) ------------------------------
__device__ __forceinline__ uint8_t f32_to_e5m2(float x) {
    const uint32_t b = __float_as_uint(x);
    const uint32_t sign = (b >> 24) & 0x80u;
    const uint32_t ab = b & 0x7fffffffu;
    if (ab > 0x7f800000u) return (uint8_t)(sign | 0x7f);  // NaN
    const float ax = __uint_as_float(ab);
    if (ax < 6.103515625e-05f) {   // below 2^-14: subnormal grid 2^-16 (rint = RNE); 4 -> smallest normal
        const uint32_t m = (uint32_t)rintf(ax * 65536.0f);
        return (uint8_t)(sign | m);
    }
    uint32_t r = ab + 0xfffffu + ((ab >> 21) & 1u);
    r &= 0xffe00000u;
    if (r > 0x47600000u) return (uint8_t)(sign | 0x7c);   // > 57344 after rounding (incl. inf) -> inf
    const uint32_t e = (r >> 23) - 127 + 15;
    const uint32_t m = (r >> 21) & 3u;
    return (uint8_t)(sign | (e << 2) | m);
}
__device__ __forceinline__ float e5m2_to_f32(uint8_t v) {
    const uint32_t e = (v >> 2) & 0x1f, m = v & 3;
    float r;
    if (e == 0x1f) r = m ? __uint_as_float(0x7fc00000u) : __uint_as_float(0x7f800000u);
    else if (e == 0) r = (float)m * 1.52587890625e-05f;
    else r = __uint_as_float(((e - 15 + 127) << 23) | (m << 21));
    return __uint_as_float(__float_as_uint(r) | ((uint32_t)(v & 0x80) << 24));
}

// ---- qtorch.quant.float_quantize(x, E, M, rounding='nearest') (subnormals=True, saturate=True), restated from QPyTorch
// 0.3.0 (quant_cpu.cpp:float_quantize_nearest, bit_helper.cpp) — the arithmetic llmc's FloatQuantizer.quant runs
// (quant.py:1061-1072); oracle/quant_ref.py:qtorch_float_quantize is the same restatement in numpy, with the list of
// differences from torch's own cast. Returns the quantized VALUE (every result is exactly representable in the OCP /
// IEEE 8-bit type of the same widths, so the real-quant cast that follows in the reference is exact).
template <int E, int M> __device__ __forceinline__ float qtorch_quantize(float x) {
    const uint32_t b = __float_as_uint(x);
    const uint32_t sign = b & 0x80000000u;
    const int t_exp = (int)((b & 0x7fffffffu) >> 23) - 127;
    constexpr int min_exp = -((1 << (E - 1)) - 2);
    constexpr uint32_t mask = (1u << (23 - M)) - 1u, half = 1u << (22 - M);
    if (t_exp < min_exp) {                       // the target format's subnormal range: round at 2^min_exp's spacing
        const float shift = __uint_as_float(((uint32_t)(127 + min_exp) << 23) | sign);
        const float val = opaque_f32(x + shift);
        const uint32_t q = (__float_as_uint(val) + half) & ~mask;
        return __uint_as_float(q) - shift;
    }
    uint32_t q = (b + half) & ~mask;             // nearest, ties away from zero
    constexpr uint32_t max_store = (1u << (E - 1)) - 1u + 127u;      // the top exponent code is kept for infinity
    if (q != 0 && ((q & 0x7fffffffu) >> 23) > max_store) q = sign | (max_store << 23) | (((1u << M) - 1u) << (23 - M));
    return __uint_as_float(q);
}

// qtorch_quantize<4, 3> without control flow for a finite, non-NaN x (both ranges evaluated, one selected): the normal range
// as above with the saturation as a clamp to +-240 (256 is the next representable magnitude: nothing lies between); below 2^-6
// the multiples of 2^-9 with ties away, formed exactly like the routine above (|x| + 2^-6 in fp32, rounded on its bits, shifted
// back; a zero result is +0). A NaN takes the routine
// above. tests/test_fp8_fast_gpu.py and the fp8 goldens run both forms on the same data.
__device__ __forceinline__ float qtorch_e4m3_select(float x) {
    const uint32_t u = __float_as_uint(x), a = u & 0x7fffffffu;
    if (__builtin_expect(a > 0x7f800000u, 0)) return qtorch_quantize<4, 3>(x);
    const float n = __builtin_amdgcn_fmed3f(__uint_as_float((u + 0x80000u) & 0xfff00000u), -240.0f, 240.0f);
    // QPyTorch's own two roundings: fl32(|x| + 2^-6) first (spacing 2^-29 there), then ties-away at 2^-9's spacing on
    // the sum's bits — an input within 2^-30 below a (k + 0.5) 2^-9 midpoint is carried over it by the first one
    const float va = opaque_f32(__uint_as_float(a) + 0.015625f);
    const float r = __uint_as_float((__float_as_uint(va) + 0x80000u) & 0xfff00000u) - 0.015625f;
    const float d = __uint_as_float(__float_as_uint(r) | (u & 0x80000000u)) + 0.0f;
    return a < 0x3c800000u ? d : n;
}

// qtorch_quantize<E, M> without control flow for a FINITE x, any (E, M) with 8-bit storage: qtorch_e4m3_select's two ranges with
// the format's constants and no NaN test — the caller proves finiteness (GPTQ's fast in-block step: a quotient of plain operands,
// gptq_loop.hip). Normal range: ties away on the bits, the saturation as a clamp to +-max (the next representable magnitude is
// 2^(max_exp + 1): nothing lies between); below 2^min_exp: fl32(|x| + 2^min_exp), ties away at the subnormal spacing on the sum's
// bits, shifted back, sign restored, a zero result is +0. e4m3: max 240, min_exp -6; e5m2: max 57344, min_exp -14.
template <int E, int M> __device__ __forceinline__ float qtorch_select_finite(float x) {
    constexpr int min_exp = -((1 << (E - 1)) - 2);
    constexpr uint32_t half = 1u << (22 - M), keep = ~((1u << (23 - M)) - 1u);
    constexpr uint32_t lo_bits = (uint32_t)(127 + min_exp) << 23;                                       // 2^min_exp
    constexpr uint32_t max_bits = ((uint32_t)((1 << (E - 1)) - 1 + 127) << 23) | (((1u << M) - 1u) << (23 - M));
    const float lo = __uint_as_float(lo_bits), mx = __uint_as_float(max_bits);
    const uint32_t u = __float_as_uint(x), a = u & 0x7fffffffu;
    const float n = __builtin_amdgcn_fmed3f(__uint_as_float((u + half) & keep), -mx, mx);
    const float va = opaque_f32(__uint_as_float(a) + lo);
    const float r = __uint_as_float((__float_as_uint(va) + half) & keep) - lo;
    const float d = __uint_as_float(__float_as_uint(r) | (u & 0x80000000u)) + 0.0f;
    return a < lo_bits ? d : n;
}

// One element of a FloatQuantizer cast. fmt: 0 = e4m3, 1 = e5m2. sem: 0 = the dtype cast of torch (float8_e4m3fn /
// float8_e5m2: round to nearest even), 1 = qtorch.float_quantize. Returns the code; *val receives the decoded value.
__device__ __forceinline__ uint8_t fp8_encode(float t, int fmt, int sem, float* val) {
    if (sem) {
        const float v = fmt ? qtorch_quantize<5, 2>(t) : qtorch_quantize<4, 3>(t);
        *val = v;
        return fmt ? f32_to_e5m2(v) : f32_to_e4m3fn(v);
    }
    const uint8_t q = fmt ? f32_to_e5m2(t) : f32_to_e4m3fn(t);
    *val = fmt ? e5m2_to_f32(q) : e4m3fn_to_f32(q);
    return q;
}
__device__ __forceinline__ float fp8_format_max(int fmt) { return fmt ? 57344.0f : 448.0f; }

// ---- the narrow OCP formats: e2m1 (FP4: s ee m, bias 1, max 6) and e3m2 (FP6: s eee mm, bias 3, max 28) -----------------
// No infinity, no NaN: all 2^E exponent codes carry numbers. bias = 2^(E-1) - 1, smallest normal 2^(1 - bias), subnormal step
// 2^(1 - bias - M), largest value (2 - 2^-M) 2^(2^E - 1 - bias). qtorch_quantize<E, M> above keeps the top exponent code for
// infinity, so ITS largest value is half of that (3 / 14) — a subset of the OCP grid, with the same subnormals.
template <int E, int M> struct fpx_fmt {
    static constexpr int bias = (1 << (E - 1)) - 1, min_exp = 1 - bias, max_exp = (1 << E) - 1 - bias;
    static constexpr uint32_t lo_bits = (uint32_t)(127 + min_exp) << 23;                                  // smallest normal
    static constexpr uint32_t max_bits = ((uint32_t)(127 + max_exp) << 23) | (((1u << M) - 1u) << (23 - M));
    static constexpr uint32_t sub_up = (uint32_t)(127 + M - min_exp) << 23, sub_dn = (uint32_t)(127 + min_exp - M) << 23;
};

// 'ocp' semantics: round to nearest even onto the OCP grid (subnormals included), saturate at +-max (inf too); a NaN gives
// max with the input's sign (the formats have none; a documented choice); the sign survives on a zero result, like the e4m3
// cast above. No control flow: both ranges are evaluated and one is selected.
template <int E, int M> __device__ __forceinline__ float fpx_ocp_quantize(float x) {
    typedef fpx_fmt<E, M> F;
    constexpr uint32_t keep = ~((1u << (23 - M)) - 1u), half_m1 = (1u << (22 - M)) - 1u;
    const uint32_t u = __float_as_uint(x), a = u & 0x7fffffffu;
    uint32_t n = (a + half_m1 + ((a >> (23 - M)) & 1u)) & keep;            // RNE on the M-bit mantissa; inf / NaN stay above max
    n = n > F::max_bits ? F::max_bits : n;
    const float d = rintf(__uint_as_float(a) * __uint_as_float(F::sub_up)) * __uint_as_float(F::sub_dn);   // exact products
    const uint32_t r = a < F::lo_bits ? __float_as_uint(d) : n;
    return __uint_as_float(r | (u & 0x80000000u));
}

// value ON the OCP grid -> code (sign in bit E + M, the bits above it zero), and back. Exact both ways.
template <int E, int M> __device__ __forceinline__ uint8_t fpx_encode(float v) {
    typedef fpx_fmt<E, M> F;
    const uint32_t u = __float_as_uint(v), a = u & 0x7fffffffu;
    const uint32_t sub = (uint32_t)(__uint_as_float(a) * __uint_as_float(F::sub_up));
    const uint32_t nrm = ((((a >> 23) - (uint32_t)(127 + F::min_exp - 1)) << M) | ((a >> (23 - M)) & ((1u << M) - 1u)));
    return (uint8_t)(((u >> 31) << (E + M)) | (a < F::lo_bits ? sub : nrm));
}
template <int E, int M> __device__ __forceinline__ float fpx_decode(uint32_t c) {
    typedef fpx_fmt<E, M> F;
    const uint32_t e = (c >> M) & ((1u << E) - 1u), m = c & ((1u << M) - 1u);
    const float sub = (float)m * __uint_as_float(F::sub_dn);
    const float nrm = __uint_as_float(((e + (uint32_t)(127 + F::min_exp - 1)) << 23) | (m << (23 - M)));
    return __uint_as_float(__float_as_uint(e ? nrm : sub) | (((c >> (E + M)) & 1u) << 31));
}

// One element of a narrow-format FloatQuantizer step. fmt: 2 = e2m1, 3 = e3m2 (0 / 1 are the 8-bit formats above); ocp: 0 =
// qtorch.float_quantize (any input: the general template), 1 = the OCP rounding above. Returns the value on the grid.
__device__ __forceinline__ float fpx_quantize(float t, int fmt, int ocp) {
    if (fmt == 2) return ocp ? fpx_ocp_quantize<2, 1>(t) : qtorch_quantize<2, 1>(t);
    return ocp ? fpx_ocp_quantize<3, 2>(t) : qtorch_quantize<3, 2>(t);
}
__device__ __forceinline__ uint8_t fpx_code(float v, int fmt) { return fmt == 2 ? fpx_encode<2, 1>(v) : fpx_encode<3, 2>(v); }
__device__ __forceinline__ float fpx_value(uint32_t c, int fmt) { return fmt == 2 ? fpx_decode<2, 1>(c) : fpx_decode<3, 2>(c); }
__device__ __forceinline__ float fpx_format_max(int fmt) { return fmt == 2 ? 6.0f : 28.0f; }

}  // namespace llmc
