// float_quant_math.h — the scalar arithmetic of llmc's FloatQuantizer (e4m3 / e5m2 / e2m1 / e3m2), stated once for every kernel:
// what quant_math.h is to the IntegerQuantizer. Mirrors llmc/compression/quantization/quant.py:545-553 (get_qparams, sym) and
// :1061-1081 (quant / dequant): scale = absmax.clamp(1e-5) / qmax, scales[scales == 0] = 1, q = float_quantize(x / scale + 0),
// q * scale. The formats themselves (the rounding onto each grid, the codes) are fp8_math.h's.
// Users: k_fp8_cast (fp8_quant.hip), k_fpx_seg / k_fpx_row / k_fpx_flat (fp4_quant.hip), the FP8 arm of k_osplus_act_step
// (smooth_osplus.hip), k_mx_act_quant (mx_gemm.hip).
#pragma once
#include "common.h"

namespace llmc {

// ---- the bits of the flag word that mean the same in llmc_fp8_quant and llmc_fpx_quant (include/llmc_hip.h) --------------------
// bit 0: write dequantized values instead of codes; bits 4-5: the format (0 e4m3, 1 e5m2, 2 e2m1, 3 e3m2); bit 11: dynamic
// scales are written back as get_qparams leaves them (an underflowed one stays 0). Bits 8-10 belong to each entry point.
static constexpr int FQ_FAKE = 1, FQ_FMT_SHIFT = 4, FQ_RAW_SCALES = 0x800;

// ---- OCP MX block scales: an e8m0 byte c is 2^(c - 127), 0 the smallest (2^-127) ---------------------------------------------
__device__ __forceinline__ float e8m0_value(uint32_t c) { return __uint_as_float(c ? c << 23 : 0x00400000u); }
__device__ __forceinline__ float e8m0_recip(uint32_t c) { return e8m0_value(254u - c); }
// the OCP MX rule: floor(log2(absmax)) - emax + 127, clamped to [0, 254]; an all-zero row takes 127 (scale 1). emax: the
// exponent of the element format's largest value.
__device__ __forceinline__ uint32_t e8m0_code(float absmax, int emax) {
    const int e = (int)((__float_as_uint(absmax) >> 23) & 0xffu) - emax;
    return absmax == 0.0f ? 127u : (uint32_t)min(max(e, 0), 254);
}

// ---- the scale of one row -------------------------------------------------------------------------------------------------------
// s: the divisor (never 0); rs: fl(1 / s); fast: rs may replace the division (the reciprocal is an ordinary number).
struct FloatScale {
    float s, rs;
    bool fast;
};
__device__ __forceinline__ FloatScale float_scale_from(float s) {
    FloatScale r;
    r.s = s;
    r.rs = 1.0f / s;
    r.fast = s > 1e-30f && s < 1e30f;
    return r;
}
__device__ __forceinline__ FloatScale float_scale_e8m0(uint32_t c) {
    FloatScale r;
    r.s = e8m0_value(c);
    r.rs = e8m0_recip(c);
    r.fast = true;
    return r;
}

// Dynamic scale from the row's absmax, a value of the tensor dtype DT; `clamped`: a pre-pass has applied clamp(1e-5) in DT
// already (llmc_minmax_qparams with qmax = 1). scale = absmax / qmax in the scales' dtype sdt: ATen promotes the 0-dim
// per-tensor absmax / 0-dim fp32 qmax of the 8-bit formats to fp32, but keeps the tensor dtype for the per-channel [R, 1]
// absmax and for the integer qmax of the narrow formats. The `first` lane of the row writes the scale back:
// scales[scales == 0] = 1 IN PLACE (quant.py:1062) reaches the returned scale too, unless the caller asked for get_qparams' own
// value (FQ_RAW_SCALES in `mode`, the only bit looked at: get_tensor_qparams alone never reaches quant()). mx: an e8m0 byte from the PLAIN absmax instead
// (mx_emax: the element format's emax; sdt and qmax are not looked at).
template <int DT>
__device__ __forceinline__ FloatScale float_dynamic_scale(float absmax, bool clamped, float qmax, int sdt, int mode, bool mx, int mx_emax,
                                                          void* scales, int64_t row, bool first) {
    if (mx) {
        const uint32_t c = e8m0_code(absmax, mx_emax);
        if (first) ((uint8_t*)scales)[row] = (uint8_t)c;
        return float_scale_e8m0(c);
    }
    const float am = clamped ? absmax : fmaxf(absmax, rndc<DT>(1e-5f));
    float s = rnd(am / qmax, sdt);
    if (first) store_from_f32(scales, row, sdt, (s == 0.0f && !(mode & FQ_RAW_SCALES)) ? 1.0f : s);
    if (s == 0.0f) s = 1.0f;
    return float_scale_from(s);
}
// Static scale: the caller's tensor is read and left alone; a zero divides as 1. e8m0: bytes as above.
__device__ __forceinline__ FloatScale float_static_scale(const void* scales, int sdt, bool e8m0, int64_t row) {
    if (e8m0) return float_scale_e8m0(((const uint8_t*)scales)[row]);
    float s = load_as_f32(scales, row, sdt);
    if (s == 0.0f) s = 1.0f;
    return float_scale_from(s);
}

// ---- one element, exactly as the reference forms it -----------------------------------------------------------------------------
// tensor / scales + zeros: ATen divides in fp32 and rounds to tdt, the dtype the quotient lives in (the tensor dtype, promoted by
// a dimensioned scale tensor of a wider one; fp32 for an e8m0 scale: exact); the `+ zeros` turns -0 into +0. keep_nan: a NaN
// input keeps the bits it came with. The narrow formats have no NaN and their 'ocp' rounding gives the maximum with the INPUT's
// sign, so they ask for it; the 8-bit encoders take the quotient's NaN (sign and payload of the division).
__device__ __forceinline__ float float_scaled_exact(float w, float s, int tdt, bool keep_nan) {
    const float t = rnd(rnd(w / s, tdt) + 0.0f, tdt);
    return (keep_nan && w != w) ? w : t;
}
// dequant: value * scale as an fp32 product, one rounding to the tensor dtype
template <typename T> __device__ __forceinline__ T float_emit(float v, float s) { return from_f32<T>(opaque_f32(v * s)); }

// ---- eight 16-bit elements without the division ---------------------------------------------------------------------------------
// t = rnd_dt(fl32(w / s)) is what `tensor / scales` leaves. q = w * fl32(1 / s) is within 3 fp32 ulps of fl32(w / s), so both
// round to the same dt value unless q lies within 4 ulps of a dt rounding boundary (9 of 65536 bf16 patterns, 9 of 8192 fp16
// patterns). A vector with such a lane, an f16 result outside the normal range, or a |t| the caller's fast form cannot take goes through
// the division (float_scaled_exact) and the general encoder instead. The guards are running minima / maxima (one v_min3 /
// v_max3 per pair instead of a compare + or per element):
//   special  an all-ones exponent in either half of an input dword (inf / NaN), for callers whose fast form has no place for them
//   tie      min of ((q bits & low mask) - (midpoint - 4)) as unsigned: <= 8 means within 4 ulps of a rounding boundary
//   tiny     f16: min of (|q| bits - 1) as unsigned: a nonzero quotient below the fp16 normal range
//   big      max of |t| bits
template <int DT> struct DivFreeGuard {
    static_assert(DT == LLMC_BF16 || DT == LLMC_F16, "the division-free form is for 16-bit tensors");
    static constexpr uint32_t LOW = DT == LLMC_BF16 ? 0xffffu : 0x1fffu;           // fp32 mantissa bits below the dt mantissa
    static constexpr uint32_t EDGE = DT == LLMC_BF16 ? 0x7ffcu : 0x0ffcu;          // the midpoint of LOW, minus 4 ulps
    static constexpr uint32_t SPAN = 8;                                            // 4 ulps either side
    static constexpr uint32_t F16_TINY = 0x387fffffu, F16_BIG = 0x477fe000u;       // 2^-14 (less one), the top of the fp16 range
    // limits for reaches(): |t| patterns from which a caller's fast form has no place for the vector
    static constexpr uint32_t T_NONFINITE = 0x7f800000u;     // inf / NaN quotients
    static constexpr uint32_t T_ABOVE_464 = 0x43e80001u;     // the e4m3 dtype cast: 464 is the last value v_cvt_pk_fp8_f32 agrees on

    uint32_t special = 0, tie = 0xffffffffu, tiny = 0xffffffffu, big = 0;

    __device__ __forceinline__ void input_pair(uint32_t word) {
        constexpr uint32_t EXPM = DT == LLMC_BF16 ? 0x7f807f80u : 0x7c007c00u, EXPL = DT == LLMC_BF16 ? 0x00800080u : 0x04000400u;
        special |= ((word & EXPM) + EXPL) & 0x80008000u;
    }
    __device__ __forceinline__ void quotient(float q) {
        const uint32_t b = __float_as_uint(q);
        tie = min(tie, (b & LOW) - EDGE);
        if constexpr (DT == LLMC_F16) tiny = min(tiny, (b & 0x7fffffffu) - 1u);
    }
    // |t| of the rounded quotient. A bf16 value has an empty low half; the mask says so on purpose: written as 0x7fffffff the AND
    // merges with the encoders' own |t| and all eight stay live up to the maximum (k_fpx_row<bf16, ocp>: 58 -> 65 VGPRs, one
    // occupancy step; profiles/float_quant_refactor.txt)
    __device__ __forceinline__ void rounded(float t) {
        big = max(big, __float_as_uint(t) & (DT == LLMC_BF16 ? 0x7fff0000u : 0x7fffffffu));
    }
    __device__ __forceinline__ bool slow() const {
        bool r = special != 0 || tie <= SPAN;
        if constexpr (DT == LLMC_F16) r = r || tiny < F16_TINY || big >= F16_BIG;
        return r;
    }
    __device__ __forceinline__ bool reaches(uint32_t t_limit) const { return big >= t_limit; }
};

// ---- absmax of a group that L neighbouring lanes hold (k_fpx_seg of fp4_quant.hip, k_mx_act_quant of mx_gemm.hip) -------------
// max over the L lanes of a group (L a power of two, whole groups active or idle together). Inside a 16-lane row the partner's
// value arrives by DPP: quad_perm [1,0,3,2] and [2,3,0,1], then row_half_mirror and row_mirror (every lane ends with the max of
// its quad / half / row); 32 and 64 lanes add the cross-row exchanges.
__device__ __forceinline__ float fpx_seg_max(float m, int L) {
    auto dpp = [](float x, auto ctrl) {
        const int y = __builtin_amdgcn_update_dpp(0, __float_as_int(x), decltype(ctrl)::value, 0xf, 0xf, true);
        return fmaxf(x, __int_as_float(y));
    };
    if (L > 1) m = dpp(m, std::integral_constant<int, 0xB1>{});
    if (L > 2) m = dpp(m, std::integral_constant<int, 0x4E>{});
    if (L > 4) m = dpp(m, std::integral_constant<int, 0x141>{});
    if (L > 8) m = dpp(m, std::integral_constant<int, 0x140>{});
    if (L > 16) m = fmaxf(m, __shfl_xor(m, 16, 64));
    if (L > 32) m = fmaxf(m, __shfl_xor(m, 32, 64));
    return m;
}

// ---- the row of vector i (vpr vectors per row, nv in all): a 32-bit division where the index fits -----------------------------
__device__ __forceinline__ int64_t row_of_vector(int64_t i, int64_t nv, int64_t vpr) {
    return nv < (int64_t)0xffffffffll ? (int64_t)((uint32_t)i / (uint32_t)vpr) : i / vpr;
}

}  // namespace llmc
