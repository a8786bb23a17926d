// fp4_quant.hip — FloatQuantizer on the narrow float grids e2m1 (FP4) and e3m2 (FP6): quant.py:963-1003, 1061-1081 with
// qmax = 6 / 28, in ONE pass over the tensor, plus the nibble packer and the dequantizer of the stored form.
//   llmc_fpx_quant    per row of the [G, g] view: absmax -> scale -> t = rnd_dt(w / s) + 0 -> round onto the grid -> q * s
//                     (fake) or one code per byte. Rounding: qtorch.float_quantize restated (fp8_math.h: qtorch_quantize<2, 1> /
//                     <3, 2>, largest value 3 / 14: the reference's arithmetic) or the OCP grid with round-to-nearest-even and
//                     saturation at 6 / 28 (fpx_ocp_quantize). Scales: absmax.clamp(1e-5) / qmax in the scale dtype, or the OCP
//                     MX power of two as an e8m0 byte. An optional column multiplier (AWQ's candidate scales) is applied on the
//                     way in: rnd_dt(w * cols[k]), what llmc_mul_cols would have left in memory.
//   llmc_fp4_pack     two e2m1 codes per byte, element 2i in the low nibble.
//   llmc_fpx_dequant  codes (packed or one per byte) x scales (dtype or e8m0) -> the fake-quant value, bit for bit.
// Three kernels, chosen by the row geometry (V = elements of a 16-byte vector):
//   k_fpx_seg   dynamic scales, g = V * L with L a power of two <= 64: one vector per lane, L lanes own a group (g = 128 on
//               16-bit data: 16 lanes, four groups per wave and load), absmax by DPP inside the 16-lane row. One HBM read.
//   k_fpx_row   dynamic scales, any other g <= 16384 that is a multiple of V: one workgroup per row, the row (after the column
//               multiplier) waits in LDS between the reduction and the rounding. One HBM read.
//   k_fpx_flat  static scales, and dynamic ones on everything else (longer rows, g not a multiple of V, misaligned pointers):
//               absmax from llmc_minmax_qparams first (a second read), then a flat grid-stride pass, vectors or scalars.
// The quantizer step (scale rule, exact element, the division-free form of 16-bit tensors with its guard, emit) is
// float_quant_math.h's, shared with k_fp8_cast (fp8_quant.hip).
#include <type_traits>

#include "common.h"
#include "float_quant_math.h"
#include "fp8_math.h"

namespace llmc {
namespace {

constexpr int XB = 256;
constexpr int FPX_OCP = 0x100, FPX_E8M0 = 0x200;        // beside the shared bits of float_quant_math.h
constexpr int64_t FPX_RESIDENT = 16384;      // elements of a row k_fpx_row keeps in LDS

struct FpxArgs {
    const void* W;
    const void* cols;        // [K] in the tensor dtype or null
    const void* amax;        // k_fpx_flat, dynamic: clamp(absmax, 1e-5) per row in the tensor dtype
    void* scales;            // [G] in sdt, or e8m0 bytes
    void* out;
    int64_t G, g, K;
    int sdt, static_scales, mode;
};

// KIND = 2 * (format - 2) + ocp
template <int KIND> __device__ __forceinline__ float fpx_q_finite(float t) {
    if constexpr (KIND == 0) return qtorch_select_finite<2, 1>(t);
    else if constexpr (KIND == 1) return fpx_ocp_quantize<2, 1>(t);
    else if constexpr (KIND == 2) return qtorch_select_finite<3, 2>(t);
    else return fpx_ocp_quantize<3, 2>(t);
}
template <int KIND> __device__ __forceinline__ float fpx_q_any(float t) { return fpx_quantize(t, 2 + (KIND >> 1), KIND & 1); }
template <int KIND> __device__ __forceinline__ uint8_t fpx_enc(float v) { return fpx_code(v, 2 + (KIND >> 1)); }
template <int KIND> __device__ __forceinline__ float fpx_qmax() { return fpx_format_max(2 + (KIND >> 1)); }

// the exponent of the format's largest value: what the OCP MX scale rule subtracts
template <int KIND> constexpr int fpx_emax() { return fpx_fmt<(KIND >> 1) ? 3 : 2, (KIND >> 1) ? 2 : 1>::max_exp; }

// dynamic scale from the row's absmax (a value of the tensor dtype); `first` lanes write it back
template <typename T, int KIND>
__device__ __forceinline__ FloatScale fpx_dynamic_scale(float absmax, bool clamped, const FpxArgs& a, int64_t row, bool first) {
    return float_dynamic_scale<dt_of<T>::value>(absmax, clamped, fpx_qmax<KIND>(), a.sdt, a.mode,
                                                a.mode & FPX_E8M0, fpx_emax<KIND>(), a.scales, row, first);
}
template <typename T, int KIND>
__device__ __forceinline__ void fpx_emit(float v, float s, int fake, T* of, uint8_t* ob) {
    if (fake) *of = float_emit<T>(v, s);
    else *ob = fpx_enc<KIND>(v);
}

// one 16-byte vector of (already column-scaled) elements
template <typename T, int KIND>
__device__ __forceinline__ void fpx_vec(const T (&w)[16 / sizeof(T)], const FloatScale sc, int tdt, int mode, T* of, uint8_t* ob) {
    constexpr int DT = dt_of<T>::value;
    constexpr int V = 16 / sizeof(T);
    const int fake = mode & FQ_FAKE;
    float v[V];
    bool done = false;
    if (mode & FPX_E8M0) {                                    // a power-of-two scale: the product with its reciprocal IS the quotient
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const float x = to_f32<T>(w[k]);
            const float t = __builtin_fmaf(x, sc.rs, 0.0f);
            v[k] = fpx_q_any<KIND>(x != x ? x : t);
        }
        done = true;
    } else if constexpr (V == 8) {
        if (sc.fast && tdt == DT) {
            DivFreeGuard<DT> guard;
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const float q = __builtin_fmaf(to_f32<T>(w[k]), sc.rs, 0.0f);
                guard.quotient(q);
                const float t = rndc<DT>(q);
                guard.rounded(t);
                v[k] = fpx_q_finite<KIND>(t);
            }
            done = !(guard.slow() || guard.reaches(guard.T_NONFINITE));
        }
    }
    if (!done) {
#pragma unroll
        for (int k = 0; k < V; ++k) v[k] = fpx_q_any<KIND>(float_scaled_exact(to_f32<T>(w[k]), sc.s, tdt, true));
    }
#pragma unroll
    for (int k = 0; k < V; ++k) fpx_emit<T, KIND>(v[k], sc.s, fake, &of[k], &ob[k]);
}

template <typename T>
__device__ __forceinline__ void fpx_store_vec(const FpxArgs& a, int64_t i, const T* of, const uint8_t* ob) {
    constexpr int V = 16 / sizeof(T);
    if (a.mode & FQ_FAKE) {
        uint4 o;
        __builtin_memcpy(&o, of, 16);
        *reinterpret_cast<uint4*>((T*)a.out + i * V) = o;
    } else if constexpr (V == 8) {
        uint2 o;
        __builtin_memcpy(&o, ob, 8);
        *reinterpret_cast<uint2*>((uint8_t*)a.out + i * V) = o;
    } else {
        uint32_t o;
        __builtin_memcpy(&o, ob, 4);
        *reinterpret_cast<uint32_t*>((uint8_t*)a.out + i * V) = o;
    }
}

// load vector i of W, apply the column multiplier, return the largest magnitude
template <typename T>
__device__ __forceinline__ float fpx_load_vec(const FpxArgs& a, int64_t i, T (&w)[16 / sizeof(T)]) {
    constexpr int DT = dt_of<T>::value;
    constexpr int V = 16 / sizeof(T);
    const uint4 raw = *reinterpret_cast<const uint4*>((const T*)a.W + i * V);
    __builtin_memcpy(w, &raw, 16);
    float m = 0.0f;
    if (a.cols) {
        const int64_t e = i * V;
        const int64_t col = (e >> 32) ? e % a.K : (int64_t)((uint32_t)e % (uint32_t)a.K);
        const uint4 rc = *reinterpret_cast<const uint4*>((const T*)a.cols + col);
        T c[V];
        __builtin_memcpy(c, &rc, 16);
#pragma unroll
        for (int k = 0; k < V; ++k) w[k] = from_f32<T>(rndc<DT>(to_f32<T>(w[k]) * to_f32<T>(c[k])));     // llmc_mul_cols' arithmetic
    }
#pragma unroll
    for (int k = 0; k < V; ++k) m = fmaxf(m, fabsf(to_f32<T>(w[k])));
    return m;
}

// fpx_seg_max (the max over the L lanes of a group, by DPP inside a 16-lane row): float_quant_math.h

template <typename T, int KIND>
__global__ __launch_bounds__(XB) void k_fpx_seg(const FpxArgs a, int L, int lshift) {
    constexpr int DT = dt_of<T>::value;
    constexpr int V = 16 / sizeof(T);
    const int64_t nv = a.G << lshift;
    const int tdt = (a.mode & FPX_E8M0) ? LLMC_F32 : (a.G == 1 ? DT : promote(DT, a.sdt));
    for (int64_t base = (int64_t)blockIdx.x * XB; base < nv; base += (int64_t)gridDim.x * XB) {     // uniform per workgroup
        const int64_t i = base + threadIdx.x;
        const bool active = i < nv;                            // nv is a multiple of L: a group is active as a whole
        T w[V];
        float m = 0.0f;
        if (active) m = fpx_load_vec<T>(a, i, w);
        m = fpx_seg_max(m, L);
        if (active) {
            const int64_t row = i >> lshift;
            const FloatScale sc = fpx_dynamic_scale<T, KIND>(m, false, a, row, (i & (L - 1)) == 0);
            T of[V];
            uint8_t ob[V];
            fpx_vec<T, KIND>(w, sc, tdt, a.mode, of, ob);
            fpx_store_vec<T>(a, i, of, ob);
        }
    }
}

template <typename T, int KIND>
__global__ __launch_bounds__(XB) void k_fpx_row(const FpxArgs a) {
    constexpr int DT = dt_of<T>::value;
    constexpr int V = 16 / sizeof(T);
    extern __shared__ uint4 fpx_lds[];             // the row, g * sizeof(T) bytes
    __shared__ float red[XB / 64];
    const int64_t vpr = a.g / V;
    const int tdt = (a.mode & FPX_E8M0) ? LLMC_F32 : (a.G == 1 ? DT : promote(DT, a.sdt));
    for (int64_t row = blockIdx.x; row < a.G; row += gridDim.x) {
        float m = 0.0f;
        for (int64_t j = threadIdx.x; j < vpr; j += XB) {
            T w[V];
            m = fmaxf(m, fpx_load_vec<T>(a, row * vpr + j, w));
            uint4 keep;
            __builtin_memcpy(&keep, w, 16);
            fpx_lds[j] = keep;                      // read back by the same thread only
        }
        m = wave_max(m, 64);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
        __syncthreads();
        m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
        __syncthreads();                            // red is written again for the next row
        const FloatScale sc = fpx_dynamic_scale<T, KIND>(m, false, a, row, threadIdx.x == 0);
        for (int64_t j = threadIdx.x; j < vpr; j += XB) {
            T w[V], of[V];
            uint8_t ob[V];
            const uint4 keep = fpx_lds[j];
            __builtin_memcpy(w, &keep, 16);
            fpx_vec<T, KIND>(w, sc, tdt, a.mode, of, ob);
            fpx_store_vec<T>(a, row * vpr + j, of, ob);
        }
    }
}

template <typename T, int KIND>
__global__ __launch_bounds__(XB) void k_fpx_flat(const FpxArgs a, int vec) {
    constexpr int DT = dt_of<T>::value;
    constexpr int V = 16 / sizeof(T);
    const int tdt = (a.mode & FPX_E8M0) ? LLMC_F32 : (a.G == 1 ? DT : promote(DT, a.sdt));
    const int64_t total = a.G * a.g;
    auto scale_of = [&](int64_t row, bool first) {
        if (a.static_scales) return float_static_scale(a.scales, a.sdt, a.mode & FPX_E8M0, row);
        return fpx_dynamic_scale<T, KIND>(to_f32<T>(((const T*)a.amax)[row]), true, a, row, first);      // the pre-pass clamped it
    };
    if (vec) {
        const int64_t nv = total / V, vpr = a.g / V;
        for (int64_t i = (int64_t)blockIdx.x * XB + threadIdx.x; i < nv; i += (int64_t)gridDim.x * XB) {
            const int64_t row = a.G == 1 ? 0 : row_of_vector(i, nv, vpr);
            T w[V], of[V];
            uint8_t ob[V];
            fpx_load_vec<T>(a, i, w);
            const FloatScale sc = scale_of(row, i == row * vpr);
            fpx_vec<T, KIND>(w, sc, tdt, a.mode, of, ob);
            fpx_store_vec<T>(a, i, of, ob);
        }
        return;
    }
    for (int64_t i = (int64_t)blockIdx.x * XB + threadIdx.x; i < total; i += (int64_t)gridDim.x * XB) {
        const int64_t row = i / a.g;
        const FloatScale sc = scale_of(row, i == row * a.g);
        float x = to_f32<T>(((const T*)a.W)[i]);
        if (a.cols) x = rndc<DT>(x * to_f32<T>(((const T*)a.cols)[i % a.K]));
        const float t = (a.mode & FPX_E8M0) ? (x != x ? x : __builtin_fmaf(x, sc.rs, 0.0f)) : float_scaled_exact(x, sc.s, tdt, true);
        T of;
        uint8_t ob;
        fpx_emit<T, KIND>(fpx_q_any<KIND>(t), sc.s, a.mode & FQ_FAKE, &of, &ob);
        if (a.mode & FQ_FAKE) ((T*)a.out)[i] = of; else ((uint8_t*)a.out)[i] = ob;
    }
}

// ---- stored form ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(XB) void k_fp4_pack(const uint8_t* __restrict__ codes, int64_t n2, uint8_t* __restrict__ packed) {
    for (int64_t i = (int64_t)blockIdx.x * XB + threadIdx.x; i < n2; i += (int64_t)gridDim.x * XB) {
        const uint32_t lo = codes[2 * i], hi = codes[2 * i + 1];
        packed[i] = (uint8_t)((lo & 0xfu) | ((hi & 0xfu) << 4));
    }
}

template <typename T>
__global__ __launch_bounds__(XB) void k_fpx_dequant(const uint8_t* __restrict__ codes, int packed, int fmt,
                                                    const void* __restrict__ scales, int sdt, int64_t total, int64_t g,
                                                    T* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * XB + threadIdx.x; i < total; i += (int64_t)gridDim.x * XB) {
        const uint32_t c = packed ? (codes[i >> 1] >> (4 * (i & 1))) & 0xfu : codes[i];
        const int64_t row = i / g;
        const float s = sdt < 0 ? e8m0_value(((const uint8_t*)scales)[row]) : load_as_f32(scales, row, sdt);
        out[i] = from_f32<T>(opaque_f32(fpx_value(c, fmt) * s));
    }
}

template <typename T, int KIND>
int fpx_launch(const FpxArgs& a, void* ws, hipStream_t st) {
    constexpr int V = 16 / sizeof(T);
    const bool aligned = (((uintptr_t)a.W | (uintptr_t)a.out | (uintptr_t)a.cols) & 15) == 0;
    const bool vec = aligned && a.g % V == 0 && (!a.cols || a.K % V == 0);
    if (!a.static_scales && vec && a.g <= FPX_RESIDENT) {
        const int64_t L = a.g / V;
        if (L <= 64 && (L & (L - 1)) == 0) {
            int lshift = 0;
            while ((1 << lshift) < L) ++lshift;
            hipLaunchKernelGGL((k_fpx_seg<T, KIND>), dim3(capped_grid(a.G * L, XB, 8192)), dim3(XB), 0, st, a, (int)L, lshift);
        } else {
            const int lds = (int)(a.g * sizeof(T));
            if (int rc = ensure_dynamic_lds((const void*)k_fpx_row<T, KIND>, (int)(FPX_RESIDENT * sizeof(T)))) return rc;
            hipLaunchKernelGGL((k_fpx_row<T, KIND>), dim3((unsigned)(a.G > 8192 ? 8192 : a.G)), dim3(XB), lds, st, a);
        }
        LLMC_LAUNCH_CHECK();
        return LLMC_OK;
    }
    FpxArgs b = a;
    if (!a.static_scales) {
        if (a.cols) {
            set_last_error_msg("fpx_quant: a column multiplier with dynamic scales needs 16-B aligned rows of at most 16384 elements");
            return LLMC_ENOTSUP;
        }
        if (a.mode & FPX_E8M0) {      // the MX rule takes the plain absmax; the pre-pass below returns the clamped one
            set_last_error_msg("fpx_quant: dynamic e8m0 scales need 16-B aligned groups of at most 16384 elements, a multiple of the vector");
            return LLMC_ENOTSUP;
        }
        LLMC_REQUIRE(ws, "fpx_quant: workspace required for dynamic scales on this geometry");
        // clamp(absmax, 1e-5) in dt: the symmetric qparams with qmax = 1, as llmc_fp8_quant takes them (same workspace layout)
        void* ws2 = (char*)ws + (((size_t)a.G * 4 + 255) & ~(size_t)255);
        if (int rc = llmc_minmax_qparams(a.W, dt_of<T>::value, a.G, a.g, /*sym*/ 1, 1, -1.0f, 1.0f, ws, nullptr, ws2, (llmc_stream_t)st)) return rc;
        b.amax = ws;
    }
    hipLaunchKernelGGL((k_fpx_flat<T, KIND>), dim3(capped_grid(a.G * a.g / (vec ? V : 1) + 1, XB, 8192)), dim3(XB), 0, st, b, (int)vec);
    LLMC_LAUNCH_CHECK();
    return LLMC_OK;
}

template <typename T>
int fpx_launch_kind(int kind, const FpxArgs& a, void* ws, hipStream_t st) {
    switch (kind) {
        case 0: return fpx_launch<T, 0>(a, ws, st);
        case 1: return fpx_launch<T, 1>(a, ws, st);
        case 2: return fpx_launch<T, 2>(a, ws, st);
        default: return fpx_launch<T, 3>(a, ws, st);
    }
}

}  // namespace
}  // namespace llmc

using namespace llmc;

extern "C" size_t llmc_fpx_quant_ws_bytes(int64_t G, int64_t g) { return llmc_fp8_quant_ws_bytes(G, g); }

extern "C" int llmc_fpx_quant(const void* W, int dt, int64_t G, int64_t g, const void* cols, int64_t K, int mode, void* out,
                              void* scales, int sdt, int static_scales, void* ws, llmc_stream_t stream) {
    LLMC_REQUIRE(dtype_ok(dt) && W && out && scales && G > 0 && g > 0, "fpx_quant: bad argument");
    const int fmt = (mode >> FQ_FMT_SHIFT) & 3;
    if (fmt != 2 && fmt != 3) {
        set_last_error_msg("fpx_quant: format must be 2 (e2m1) or 3 (e3m2); e4m3 / e5m2 are llmc_fp8_quant's");
        return LLMC_ENOTSUP;
    }
    if (mode & ~(FQ_FAKE | (3 << FQ_FMT_SHIFT) | FPX_OCP | FPX_E8M0 | FQ_RAW_SCALES)) {
        set_last_error_msg("fpx_quant: unknown semantics bits in mode");
        return LLMC_ENOTSUP;
    }
    if ((mode & FPX_E8M0) && !(mode & FPX_OCP)) {
        set_last_error_msg("fpx_quant: e8m0 scales go with the ocp semantics only");
        return LLMC_ENOTSUP;
    }
    LLMC_REQUIRE((mode & FPX_E8M0) || dtype_ok(sdt), "fpx_quant: bad scale dtype");
    LLMC_REQUIRE(!cols || (K > 0 && K % g == 0), "fpx_quant: cols needs the row length K, a multiple of g");
    FpxArgs a;
    a.W = W, a.cols = cols, a.amax = nullptr, a.scales = scales, a.out = out;
    a.G = G, a.g = g, a.K = cols ? K : 1;
    a.sdt = (mode & FPX_E8M0) ? LLMC_F32 : sdt, a.static_scales = static_scales, a.mode = mode;
    const int kind = 2 * (fmt - 2) + ((mode & FPX_OCP) ? 1 : 0);
    hipStream_t st = (hipStream_t)stream;
    DISPATCH_DT(dt, return fpx_launch_kind<T>(kind, a, ws, st));
}

extern "C" int llmc_fp4_pack(const void* codes, int64_t R, int64_t K, void* packed, llmc_stream_t stream) {
    LLMC_REQUIRE(codes && packed && R > 0 && K > 0 && K % 2 == 0, "fp4_pack: needs codes [R, K] with K even");
    hipLaunchKernelGGL(k_fp4_pack, dim3(capped_grid(R * K / 2, XB, 8192)), dim3(XB), 0, (hipStream_t)stream, (const uint8_t*)codes, R * K / 2,
                       (uint8_t*)packed);
    LLMC_LAUNCH_CHECK();
    return LLMC_OK;
}

extern "C" int llmc_fpx_dequant(const void* codes, int fmt, int packed, const void* scales, int sdt, int64_t G, int64_t g,
                                void* out, int odt, llmc_stream_t stream) {
    LLMC_REQUIRE(codes && scales && out && G > 0 && g > 0 && dtype_ok(odt), "fpx_dequant: bad argument");
    LLMC_REQUIRE(sdt == -1 || dtype_ok(sdt), "fpx_dequant: scale dtype must be a float dtype or -1 (e8m0 bytes)");
    if ((fmt != 2 && fmt != 3) || (packed && fmt != 2)) {
        set_last_error_msg("fpx_dequant: format must be 2 (e2m1, packed or not) or 3 (e3m2, one code per byte)");
        return LLMC_ENOTSUP;
    }
    LLMC_REQUIRE(!packed || (G * g) % 2 == 0, "fpx_dequant: packed codes need an even element count");
    hipStream_t st = (hipStream_t)stream;
    const int64_t total = G * g;
    DISPATCH_DT(odt, hipLaunchKernelGGL((k_fpx_dequant<T>), dim3(capped_grid(total, XB, 8192)), dim3(XB), 0, st, (const uint8_t*)codes,
                                        packed, fmt, scales, sdt, total, g, (T*)out));
    LLMC_LAUNCH_CHECK();
    return LLMC_OK;
}
