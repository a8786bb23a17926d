// fp8_quant.hip — K11: FloatQuantizer on the 8-bit grids e4m3 (OCP e4m3fn) and e5m2.
//   llmc_fp8_quant      FloatQuantizer sym e4m3 / e5m2: scale = absmax.clamp(1e-5) / finfo.max, q = float_quantize(x / scale)
//                       (quant.py:545-553, 983-1003, 1061-1072, 1195-1221) with qtorch's arithmetic restated (fp8_math.h:
//                       qtorch_quantize; the library is a third-party dependency absent from the reference tree), or
//                       torch's own dtype cast (float8_e4m3fn / float8_e5m2, RNE) for the callers that end in one.
// The quantizer step itself (scale rule, exact element, division-free guard, emit) is float_quant_math.h's.
#include <stdlib.h>
#include "common.h"
#include "float_quant_math.h"
#include "fp8_math.h"

namespace llmc {

static constexpr int FB = 256;

// amax[row] = clamp(absmax, 1e-5) in dt (from llmc_minmax_qparams with qmax = 1); the scale rule is float_dynamic_scale's.
// mode: the shared bits of float_quant_math.h, bit 8 semantics (0 torch's dtype cast, 1 qtorch.float_quantize: fp8_math.h)
static constexpr int FP8_QTORCH = 0x100;
static constexpr int FP8_EXACT_DIV = 0x200;      // A/B: every element through the IEEE division and the general encoder (tests/test_fp8_fast_gpu.py)
static constexpr int FP8_NO_PACKED16 = 0x400;    // A/B: the float form of the division-free path (round 4) instead of the packed 16-bit one
static constexpr int FP8_LAB_BITS = FP8_EXACT_DIV | FP8_NO_PACKED16 | FQ_RAW_SCALES;     // not the encoders' business

template <typename T>
__device__ __forceinline__ void fp8_one(float w, float s, int tdt, int mode, T* of, uint8_t* ob) {
    const float t = float_scaled_exact(w, s, tdt, false);
    float v;
    const uint8_t q = fp8_encode(t, (mode >> FQ_FMT_SHIFT) & 3, mode & FP8_QTORCH, &v);
    if (mode & FQ_FAKE) *of = float_emit<T>(v, s);
    else *ob = q;
}
// two elements: one hardware conversion (fp8_math.h) on the e4m3 cast path
template <typename T>
__device__ __forceinline__ void fp8_two(float w0, float w1, float s, int tdt, int mode, T* of, uint8_t* ob) {
    const int fake = mode & FQ_FAKE;
    if ((mode & ~FQ_FAKE) == FP8_QTORCH) {       // e4m3 with qtorch's rounding: the quantized values are exact e4m3fn numbers,
        const float v0 = qtorch_quantize<4, 3>(float_scaled_exact(w0, s, tdt, false));     // so the hardware conversion is exact
        const float v1 = qtorch_quantize<4, 3>(float_scaled_exact(w1, s, tdt, false));
        if (fake) {
            of[0] = float_emit<T>(v0, s);
            of[1] = float_emit<T>(v1, s);
        } else {
            const uint32_t c = f32x2_to_e4m3fn(v0, v1);
            ob[0] = (uint8_t)c;
            ob[1] = (uint8_t)(c >> 8);
        }
        return;
    }
    if (mode & ~FQ_FAKE) {
        fp8_one<T>(w0, s, tdt, mode, &of[0], &ob[0]);
        fp8_one<T>(w1, s, tdt, mode, &of[1], &ob[1]);
        return;
    }
    const uint32_t c = f32x2_to_e4m3fn(float_scaled_exact(w0, s, tdt, false), float_scaled_exact(w1, s, tdt, false));
    const uint8_t q0 = (uint8_t)c, q1 = (uint8_t)(c >> 8);
    if (fake) {
        of[0] = float_emit<T>(e4m3fn_to_f32(q0), s);
        of[1] = float_emit<T>(e4m3fn_to_f32(q1), s);
    } else {
        ob[0] = q0;
        ob[1] = q1;
    }
}

// ---- eight 16-bit elements at once, without the division ---------------------------------------------------------------
// The division-free form and its guard are float_quant_math.h's (DivFreeGuard); non-finite inputs and, for the dtype cast,
// |t| > 464 leave with the guarded lanes. e4m3 only; qtorch semantics on the fast path = (bits + 0x80000) & ~0xfffff, saturated
// to 240 from 256 upwards (fp8_math.h:qtorch_quantize), then the exact hardware conversion of the on-grid values.
//
// Round 6: eight bf16 elements -> eight e4m3 CODES with qtorch's rounding on 16-bit lanes (two elements per packed
// instruction), about 15 VALU instructions per element instead of 21 (the cast is VALU-bound: 42 us against 21 us of HBM time
// for a 14336 x 4096 weight). t = bf16(w * fl(1 / s)) as above (same tie guard, on the quotients' low halves packed into one
// dword). On t's bf16 pattern m (sign cleared):
//   |t| >= 2^-6: ties-away on the 3-bit mantissa is (m + 8) >> 4 = 8 * exponent + mantissa, the e4m3 code is that minus
//                8 * 120, saturated at 0x77 (240: qtorch keeps the top exponent code for infinity, 248 and above land there);
//   |t| <  2^-6: the format's subnormal range — spacing 2^-9, and the code of k * 2^-9 IS k: floor(|t| * 512 + 0.5), exact for
//                an 8-bit significand (the same formula as the float form below);
// a per-half mask picks one, the sign goes to bit 7 unless the code is 0 (qtorch's x - x = +0). Inf / NaN patterns of t and
// quotients within 4 ulps of a rounding boundary leave through the general encoder like before. Bit-identical to the float
// form and to the division form (tests/test_fp8_fast_gpu.py, fp8 goldens).
__device__ __forceinline__ bool fp8_codes8_bf16_qtorch(const uint4 raw, float rs, uint2* ob) {
    typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
    typedef short i16x2 __attribute__((ext_vector_type(2)));
    typedef float f2 __attribute__((ext_vector_type(2)));
    typedef __bf16 bf2 __attribute__((ext_vector_type(2)));
    typedef DivFreeGuard<LLMC_BF16> Guard;                  // its constants, on 16-bit lanes
    constexpr unsigned short EDGE = (unsigned short)Guard::EDGE, NONFINITE = (unsigned short)(Guard::T_NONFINITE >> 16);
    const uint32_t word[4] = {raw.x, raw.y, raw.z, raw.w};
    u16x2 tie = {0xffff, 0xffff}, big = {0, 0};
    uint32_t cw[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const f2 w = {__uint_as_float(word[p] << 16), __uint_as_float(word[p] & 0xffff0000u)};
        const f2 q = __builtin_elementwise_fma(w, (f2){rs, rs}, (f2){0.0f, 0.0f});      // w * (1 / s) + 0: -0 becomes +0
        const uint32_t lows = __builtin_amdgcn_perm(__float_as_uint(q[1]), __float_as_uint(q[0]), 0x05040100u);
        tie = __builtin_elementwise_min(tie, (u16x2)(__builtin_bit_cast(u16x2, lows) - (u16x2){EDGE, EDGE}));
        const uint32_t pk = __builtin_bit_cast(uint32_t, __builtin_convertvector(q, bf2));     // v_cvt_pk_bf16_f32: RNE
        const uint32_t m = pk & 0x7fff7fffu;
        const u16x2 mv = __builtin_bit_cast(u16x2, m);
        big = __builtin_elementwise_max(big, mv);
        u16x2 r = (u16x2)((u16x2)(mv + (u16x2){8, 8}) >> (u16x2){4, 4});
        r = (u16x2)(__builtin_elementwise_min(r, (u16x2){1079, 1079}) - (u16x2){960, 960});
        const uint32_t k0 = (uint32_t)__builtin_fmaf(__builtin_fabsf(__uint_as_float(pk << 16)), 512.0f, 0.5f);
        const uint32_t k1 = (uint32_t)__builtin_fmaf(__builtin_fabsf(__uint_as_float(pk & 0xffff0000u)), 512.0f, 0.5f);
        const uint32_t kk = __builtin_amdgcn_perm(k1, k0, 0x05040100u);      // the low halves (a large |t| * 512 does not fit 16 bits: its half is not selected)
        const uint32_t sub = __builtin_bit_cast(uint32_t, (i16x2)(__builtin_bit_cast(i16x2, (u16x2)(mv - (u16x2){0x3c80, 0x3c80})) >> (i16x2){15, 15}));
        uint32_t c = (sub & kk) | (~sub & __builtin_bit_cast(uint32_t, r));
        const uint32_t nz = __builtin_bit_cast(uint32_t, (u16x2)(__builtin_bit_cast(u16x2, c) + (u16x2){0x7f, 0x7f}));   // bit 7: code != 0
        c |= (pk >> 8) & nz & 0x00800080u;
        cw[p] = c;
    }
    if (tie[0] <= Guard::SPAN || tie[1] <= Guard::SPAN || big[0] >= NONFINITE || big[1] >= NONFINITE) return false;
    ob->x = __builtin_amdgcn_perm(cw[1], cw[0], 0x06040200u);
    ob->y = __builtin_amdgcn_perm(cw[3], cw[2], 0x06040200u);
    return true;
}

template <typename T>
__device__ __forceinline__ bool fp8_fast8(const uint4 raw, float s, float rs, int mode, T (&of)[8], uint2* ob) {
    constexpr int DT = dt_of<T>::value;
    const bool qt = mode & FP8_QTORCH;
    if constexpr (DT == LLMC_BF16) {
        if (qt && !(mode & FQ_FAKE) && !(mode & FP8_NO_PACKED16)) return fp8_codes8_bf16_qtorch(raw, rs, ob);
    }
    const uint32_t word[4] = {raw.x, raw.y, raw.z, raw.w};
    DivFreeGuard<DT> guard;
    float v[8];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        guard.input_pair(word[p]);                                        // inf / nan: the general path keeps their special cases
        float q0, q1;                                                  // w * (1 / s) + 0: the `+ zeros` of the reference turns -0 into +0
        if constexpr (DT == LLMC_BF16) {
            q0 = __builtin_fmaf(__uint_as_float(word[p] << 16), rs, 0.0f);
            q1 = __builtin_fmaf(__uint_as_float(word[p] & 0xffff0000u), rs, 0.0f);
        } else {
            typedef _Float16 h2 __attribute__((ext_vector_type(2)));
            const h2 hv = __builtin_bit_cast(h2, word[p]);
            q0 = __builtin_fmaf((float)hv[0], rs, 0.0f);
            q1 = __builtin_fmaf((float)hv[1], rs, 0.0f);
        }
        guard.quotient(q0);
        guard.quotient(q1);
        float t0, t1;
        if constexpr (DT == LLMC_BF16) {
            typedef __bf16 bf2 __attribute__((ext_vector_type(2)));
            typedef float f2 __attribute__((ext_vector_type(2)));
            const f2 qq = {q0, q1};
            const uint32_t pk = __builtin_bit_cast(uint32_t, __builtin_convertvector(qq, bf2));     // v_cvt_pk_bf16_f32: RNE
            t0 = __uint_as_float(pk << 16);
            t1 = __uint_as_float(pk & 0xffff0000u);
        } else {
            t0 = (float)(_Float16)q0;
            t1 = (float)(_Float16)q1;
        }
        guard.rounded(t0);
        guard.rounded(t1);
        const uint32_t u0 = __float_as_uint(t0), u1 = __float_as_uint(t1);
        const uint32_t a0 = u0 & 0x7fffffffu, a1 = u1 & 0x7fffffffu;
        if (qt) {
            // nearest with ties away on the 3-bit mantissa, then 256 and above -> 240 (nothing lies between)
            const float n0 = __builtin_amdgcn_fmed3f(__uint_as_float((u0 + 0x80000u) & 0xfff00000u), -240.0f, 240.0f);
            const float n1 = __builtin_amdgcn_fmed3f(__uint_as_float((u1 + 0x80000u) & 0xfff00000u), -240.0f, 240.0f);
            // below 2^-6 (the format's subnormal range) qtorch rounds x + sign * 2^-6 and subtracts the shift again: the
            // multiples of 2^-9, ties away, and a result of zero is +0 (x - x). Per-tensor scales put a good share of a weight
            // with outlier channels here, so this is evaluated for every element and selected, not branched to
            const float d0 = __uint_as_float(__float_as_uint(__builtin_floorf(__builtin_fmaf(__uint_as_float(a0), 512.0f, 0.5f)) * 0.001953125f) |
                                             (u0 & 0x80000000u)) + 0.0f;
            const float d1 = __uint_as_float(__float_as_uint(__builtin_floorf(__builtin_fmaf(__uint_as_float(a1), 512.0f, 0.5f)) * 0.001953125f) |
                                             (u1 & 0x80000000u)) + 0.0f;
            v[2 * p] = a0 < 0x3c800000u ? d0 : n0;
            v[2 * p + 1] = a1 < 0x3c800000u ? d1 : n1;
        } else if constexpr (DT == LLMC_BF16) {
            // the reference adds its zero AFTER the rounding to dt: a negative quotient below half of bf16's smallest subnormal
            // rounds to -0 and leaves as +0 (code 0x00, not 0x80). The zero inside the fma above came too early for it. (f16
            // sends nonzero quotients below its normal range to the division; qtorch returns +0 for every zero result.)
            v[2 * p] = t0 + 0.0f;
            v[2 * p + 1] = t1 + 0.0f;
        } else {
            v[2 * p] = t0;
            v[2 * p + 1] = t1;
        }
    }
    if (guard.slow() || (!qt && guard.reaches(guard.T_ABOVE_464))) return false;
    // four codes per dword straight from the converter (word select: low / high half of the destination)
    uint32_t lo = 0, hi = 0;
    lo = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(v[0], v[1], (int)lo, false);
    lo = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(v[2], v[3], (int)lo, true);
    hi = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(v[4], v[5], (int)hi, false);
    hi = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(v[6], v[7], (int)hi, true);
    if (mode & FQ_FAKE) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint8_t c = (uint8_t)((k < 4 ? lo : hi) >> (8 * (k & 3)));
            of[k] = float_emit<T>(qt ? v[k] : e4m3fn_to_f32(c), s);
        }
    } else {
        *ob = make_uint2(lo, hi);
    }
    return true;
}

// One 16-byte vector per thread and turn, a workgroup on 256 consecutive vectors. Measured on a 14336 x 4096 weight
// (profiles/r04_fp8_cast_ab.txt): ONE vector per thread is the fastest — the kernel is bound by its VALU work, not by loads in
// flight (two equal; four / eight, a thread's vectors a whole grid apart and a smaller grid slower).
template <typename T>
__global__ __launch_bounds__(FB) void k_fp8_cast(const T* __restrict__ W, const T* __restrict__ amax, int sdt,
                                                 void* __restrict__ scales, int static_scales, int64_t G, int64_t g,
                                                 int mode, void* __restrict__ out) {
    const int fake = mode & FQ_FAKE;
    const float fmax = fp8_format_max((mode >> FQ_FMT_SHIFT) & 3);
    constexpr int DT = dt_of<T>::value;
    constexpr int V = 16 / sizeof(T);
    const int pdt = promote(DT, sdt);
    const int tdt = (G == 1) ? DT : pdt;   // a 0-dim fp32 scale does not promote the [R,K] tensor, a [R,1] one does
    const bool vec = (g % V == 0) && (((uintptr_t)W & 15) == 0) && (((uintptr_t)out & 15) == 0);
    // the division-free form: 16-bit tensors whose quotient is rounded in their own dtype, e4m3, a scale whose reciprocal is an
    // ordinary number (per row: FloatScale::fast)
    const bool fast_kind = (V == 8) && tdt == DT && ((mode >> FQ_FMT_SHIFT) & 3) == 0 && !(mode & FP8_EXACT_DIV);
    const int64_t total = G * g;
    auto scale_of = [&](int64_t row, bool first) {
        if (static_scales) return float_static_scale(scales, sdt, false, row);
        return float_dynamic_scale<DT>(to_f32<T>(amax[row]), true, fmax, sdt, mode, false, 0, scales, row, first);
    };
    if (vec) {
        const int64_t nv = total / V, vpr = g / V;                   // a per_tensor call (G == 1) has no row arithmetic at all
        for (int64_t i = (int64_t)blockIdx.x * FB + threadIdx.x; i < nv; i += (int64_t)gridDim.x * FB) {
            const uint4 raw = *reinterpret_cast<const uint4*>(W + i * V);
            const int64_t row = (G == 1) ? 0 : row_of_vector(i, nv, vpr);
            const FloatScale sc = scale_of(row, i == row * vpr);
            if constexpr (V == 8) {
                if (fast_kind && sc.fast) {
                    T of[V];
                    uint2 ob;
                    if (fp8_fast8<T>(raw, sc.s, sc.rs, mode, of, &ob)) {
                        if (fake) {
                            uint4 o;
                            __builtin_memcpy(&o, of, 16);
                            *reinterpret_cast<uint4*>((T*)out + i * V) = o;
                        } else {
                            *reinterpret_cast<uint2*>((uint8_t*)out + i * V) = ob;
                        }
                        continue;
                    }
                }
            }
            // one copy of the general encoder, rolled over pairs (inlined per element it made the kernel 10.6 k instructions long)
#pragma unroll 1
            for (int pr = 0; pr < V / 2; ++pr) {
                float w0, w1;
                if constexpr (V == 8) {
                    uint32_t word = raw.x;
                    if (pr == 1) word = raw.y;
                    if (pr == 2) word = raw.z;
                    if (pr == 3) word = raw.w;
                    T a, b;
                    a.u = (uint16_t)(word & 0xffffu);
                    b.u = (uint16_t)(word >> 16);
                    w0 = to_f32<T>(a);
                    w1 = to_f32<T>(b);
                } else {
                    w0 = __uint_as_float(pr ? raw.z : raw.x);
                    w1 = __uint_as_float(pr ? raw.w : raw.y);
                }
                T of[2];
                uint8_t ob[2];
                fp8_two<T>(w0, w1, sc.s, tdt, mode & ~FP8_LAB_BITS, of, ob);
                const int64_t e = i * V + 2 * pr;
                if (fake) {
                    ((T*)out)[e] = of[0];
                    ((T*)out)[e + 1] = of[1];
                } else {
                    ((uint8_t*)out)[e] = ob[0];
                    ((uint8_t*)out)[e + 1] = ob[1];
                }
            }
        }
        return;
    }
    for (int64_t i = (int64_t)blockIdx.x * FB + threadIdx.x; i < total; i += (int64_t)gridDim.x * FB) {
        const int64_t row = i / g;
        const FloatScale sc = scale_of(row, i == row * g);
        T of;
        uint8_t ob;
        fp8_one<T>(to_f32<T>(W[i]), sc.s, tdt, mode & ~FP8_LAB_BITS, &of, &ob);
        if (fake) ((T*)out)[i] = of; else ((uint8_t*)out)[i] = ob;
    }
}

}  // namespace llmc

using namespace llmc;

extern "C" size_t llmc_fp8_quant_ws_bytes(int64_t G, int64_t g) {
    if (G <= 0 || g <= 0) return 0;
    return (((size_t)G * 4 + 255) & ~(size_t)255) + llmc_minmax_qparams_ws_bytes(G, g);
}

extern "C" int llmc_fp8_quant(const void* W, int dt, int64_t G, int64_t g, int fake, void* out, void* scales,
                              int sdt, int static_scales, void* ws, llmc_stream_t stream) {
    LLMC_REQUIRE(dtype_ok(dt) && dtype_ok(sdt) && W && out && scales && G > 0 && g > 0, "fp8_quant: bad argument");
    LLMC_REQUIRE(static_scales || ws, "fp8_quant: workspace required for dynamic scales");
    if (((fake >> FQ_FMT_SHIFT) & 3) > 1) {
        set_last_error_msg("fp8_quant: format is 0 (e4m3) or 1 (e5m2); e2m1 / e3m2 are llmc_fpx_quant's");
        return LLMC_ENOTSUP;
    }
    void* amax = ws;
    if (!static_scales) {
        void* ws2 = (char*)ws + (((size_t)G * 4 + 255) & ~(size_t)255);
        // clamp(absmax, 1e-5) in dt: the symmetric qparams with qmax = 1
        int rc = llmc_minmax_qparams(W, dt, G, g, /*sym*/ 1, 1, -1.0f, 1.0f, amax, nullptr, ws2, stream);
        if (rc) return rc;
    }
    if (opt(OPT_FP8_EXACT_DIV)) fake |= FP8_EXACT_DIV;      // A/B switch, same results (include/llmc_hip.h)
    if (opt(OPT_FP8_NO_PACKED16)) fake |= FP8_NO_PACKED16;
    hipStream_t st = (hipStream_t)stream;
    const int V = 16 / dtype_size(dt);
    const int grid = capped_grid(G * g / V + 1, FB, 8192);
    DISPATCH_DT(dt, hipLaunchKernelGGL((k_fp8_cast<T>), dim3(grid), dim3(FB), 0, st, (const T*)W, (const T*)amax, sdt, scales,
                                       static_scales, G, g, fake, out));
    LLMC_LAUNCH_CHECK();
    return LLMC_OK;
}
