// smooth_osplus.hip — the device side of SmoothQuant (smoothquant.py:39-59) and OS+ (osplus.py:61-170).
//   llmc_col_stats         per-column max / min / max|x| of [N, K], folded into running fp32 [3, K] buffers; two stages, no
//                          atomics: max and min do not depend on the order, so the result is bit-exact by construction.
//   llmc_smooth_scales     (x_max^a / w_max^(1-a)).clamp(1e-5), every op rounded to the weight dtype.
//   llmc_osplus_scale      cur_scale of one threshold of the OS+ grid, from a device array of thresholds.
//   llmc_osplus_act_step   fake_quant_act_dynamic(x / cur_scale) per token in one pass: the row's quotients stay in
//                          registers between the range reduction and the quantize. Same bits as llmc_div_cols followed by
//                          llmc_quant_dynamic (integer) or llmc_fp8_quant (FP8, dynamic per-row scales).
// All three data passes are HBM-bound; DESIGN.md holds the byte counts they are measured against.
#include "col_reduce.h"
#include "common.h"
#include "float_quant_math.h"
#include "fp8_math.h"
#include "quant_group.h"
#include "quant_math.h"
#include "vec_powf.h"

namespace llmc {

static constexpr int SB = 256;            // threads per workgroup, every kernel of this file
static constexpr int CS_ROWS = 16;        // rows one workgroup of k_col_stats_partial folds per turn (4 per wave)
static constexpr int CS_MAX_BLOCKS = 2048;

__device__ __forceinline__ float nan_max(float a, float b) { return (a != a || b != b) ? NAN : fmaxf(a, b); }
__device__ __forceinline__ float nan_min(float a, float b) { return (a != a || b != b) ? NAN : fminf(a, b); }

// ---- column statistics: col_reduce.h's two stages over max, min and max|x|. torch.amax / amin / max propagate NaN; fmaxf drops it
struct Extremes {
    static constexpr int NS = 3;
    static __device__ __forceinline__ float identity(int s) { return s == 0 ? -INFINITY : (s == 1 ? INFINITY : 0.0f); }
    static __device__ __forceinline__ void step(float (&a)[3], float f) {
        a[0] = nan_max(a[0], f);
        a[1] = nan_min(a[1], f);
        a[2] = nan_max(a[2], fabsf(f));
    }
    static __device__ __forceinline__ float join(int s, float a, float b) { return s == 1 ? nan_min(a, b) : nan_max(a, b); }
};

template <typename T, int VEC>
__global__ __launch_bounds__(SB) void k_col_stats_partial(const T* __restrict__ X, int64_t N, int64_t K, int64_t rows_per_chunk,
                                                          float* __restrict__ part) {
    col_reduce_partial<Extremes, T, VEC, SB>(X, N, K, rows_per_chunk, part);
}

__global__ __launch_bounds__(SB) void k_col_stats_fold(const float* __restrict__ part, int64_t nchunk, int64_t K, int init,
                                                       float* __restrict__ run) {
    const int64_t k = (int64_t)blockIdx.x * SB + threadIdx.x;
    if (k >= K) return;
    float a[3];
    col_reduce_fold<Extremes>(part, nchunk, K, k, init, run, a);
}

// stage 3 (optional): glob[0] = max(0, max_k run_max), glob[1] = min(0, min_k run_min) — osplus.py:97-102
__global__ __launch_bounds__(1024) void k_col_stats_global(const float* __restrict__ run, int64_t K, float* __restrict__ glob) {
    __shared__ float sa[16], sb[16];
    __shared__ int snan[2];
    if (threadIdx.x < 2) snan[threadIdx.x] = 0;
    __syncthreads();
    float a = -INFINITY, b = INFINITY;
    int na = 0, nb = 0;
    for (int64_t k = threadIdx.x; k < K; k += 1024) {
        const float x = run[k], y = run[K + k];
        na |= (x != x);
        nb |= (y != y);
        a = fmaxf(a, x);
        b = fminf(b, y);
    }
    a = wave_max(a, 64);
    b = wave_min(b, 64);
    if (na) snan[0] = 1;
    if (nb) snan[1] = 1;
    if ((threadIdx.x & 63) == 0) {
        sa[threadIdx.x >> 6] = a;
        sb[threadIdx.x >> 6] = b;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < 16; ++i) {
            a = fmaxf(a, sa[i]);
            b = fminf(b, sb[i]);
        }
        // Python's max(x.max(), 0) / min(x.min(), 0): `0 > nan` is False, so a NaN extreme stays
        glob[0] = snan[0] ? NAN : fmaxf(a, 0.0f);
        glob[1] = snan[1] ? NAN : fminf(b, 0.0f);
    }
}

// ---- SmoothQuant.search_scale_subset (smoothquant.py:54-59) -----------------------------------------------------------------
// ATen's Tensor.pow(python_float) casts the exponent to the tensor dtype and evaluates 0.5 as sqrt; any other exponent goes to
// its vectorised pow, which computes in fp32 for every dtype (vec_powf.h) and rounds to the tensor dtype.
template <int DT> __device__ __forceinline__ float pow_dt(float x, float e) {
    if (e == 0.5f) return rndc<DT>(sqrtf(x));
    if (e == 1.0f) return x;
    if (e == 0.0f) return 1.0f;
    if (x > 0.0f && x < INFINITY) return rndc<DT>(sf_powf_pos(x, e));
    return rndc<DT>((float)pow((double)x, (double)e));      // 0, inf, NaN
}
template <typename T>
__global__ __launch_bounds__(SB) void k_smooth_scales(const float* __restrict__ xmax, const float* __restrict__ wmax, int64_t K,
                                                      float alpha, float one_minus_alpha, T* __restrict__ out) {
    constexpr int DT = dt_of<T>::value;
    const int64_t k = (int64_t)blockIdx.x * SB + threadIdx.x;
    if (k >= K) return;
    const float lo = rndc<DT>(1e-5f);
    const float ea = rndc<DT>(alpha), ew = rndc<DT>(one_minus_alpha);
    const float x = rndc<DT>(xmax[k]);                 // x_max.to(dtype=w_max.dtype)
    const float w = nan_max(wmax[k], lo);              // .clamp(min=1e-5) of get_weight_scale
    const float s = rndc<DT>(pow_dt<DT>(x, ea) / pow_dt<DT>(w, ew));
    out[k] = from_f32<T>(nan_max(s, lo));
}

// ---- OS+ cur_scale (osplus.py:118-131): thresholds already rounded to the activation dtype -----------------------------------
template <typename T>
__global__ __launch_bounds__(SB) void k_osplus_scale(const float* __restrict__ cmx, const float* __restrict__ cmn,
                                                     const T* __restrict__ thr, int64_t K, T* __restrict__ out) {
    constexpr int DT = dt_of<T>::value;
    const int64_t k = (int64_t)blockIdx.x * SB + threadIdx.x;
    if (k >= K) return;
    const float st = to_f32<T>(thr[0]);
    const float a = cmx[k], b = cmn[k];
    const float ms = a > st ? rndc<DT>(a / st) : 1.0f;
    const float ns = b < -st ? rndc<DT>(b / -st) : 1.0f;
    out[k] = from_f32<T>(nan_max(ms, ns));
}

// ---- the fused activation step ---------------------------------------------------------------------------------------------
// One workgroup per token row; thread t owns the 16-byte vectors t, t + 256, ... of the row (MAXV of them at most). The
// quotients rnd(x / s) stay packed in registers; min / max go through a wave shuffle and 4 LDS words.
static constexpr int ACT_INT = 0, ACT_FP8 = 1;

template <typename T, int MAXV, int KIND>
__global__ __launch_bounds__(SB) void k_osplus_act_step(const T* __restrict__ X, const T* __restrict__ s, int64_t N, int K,
                                                        int sym, float qmin, float qmax, int mode, T* __restrict__ out) {
    constexpr int DT = dt_of<T>::value;
    constexpr int V = 16 / sizeof(T);
    __shared__ float red[2 * (SB / 64)];
    const int nv = K / V;
    for (int64_t row = blockIdx.x; row < N; row += gridDim.x) {
        const T* xp = X + row * K;
        uint4 q[MAXV];            // the quotients wait as packed 16-byte words: the FP8 arm selects among them by value
        float mn = INFINITY, mx = -INFINITY;
#pragma unroll
        for (int j = 0; j < MAXV; ++j) {
            const int vi = j * SB + threadIdx.x;
            if (vi < nv) {
                const Vec<T, V> xv = load_vec<T, V>(xp + vi * V), sv = load_vec<T, V>(s + vi * V);
                Vec<T, V> ov;
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    const float f = rndc<DT>(to_f32<T>(xv.v[k]) / to_f32<T>(sv.v[k]));     // llmc_div_cols
                    ov.v[k] = from_f32<T>(f);
                    mn = fminf(mn, f);
                    mx = fmaxf(mx, f);
                }
                __builtin_memcpy(&q[j], &ov, 16);
            }
        }
        block_minmax<SB>(red, mn, mx);
        T* op = out + row * K;
        if constexpr (KIND == ACT_INT) {
            // fake_quant_act_dynamic is round_zp = 1 only: no fractional-zero-point arm (GroupQuant<false>)
            const GroupQuant<> gq = GroupQuant<>::from_minmax(mn, mx, DT, sym, 1, qmin, qmax);
#pragma unroll
            for (int j = 0; j < MAXV; ++j) {
                const int vi = j * SB + threadIdx.x;
                if (vi < nv) {
                    Vec<T, V> v, o;
                    __builtin_memcpy(&v, &q[j], 16);
                    quant_vec<LLMC_OUT_FAKE>(o, v, gq, qmin, qmax);
                    store_vec<T, V>(op + vi * V, o);
                }
            }
        } else {
            // llmc_fp8_quant with dynamic per-row scales (float_quant_math.h); the scale is not returned
            const int fmt = (mode >> FQ_FMT_SHIFT) & 3, sem = mode & 0x100;
            const float amax = qparams_from_minmax(mn, mx, DT, 1, 1, -1.0f, 1.0f).s;      // clamp(absmax, 1e-5) in dt
            const float sc = float_dynamic_scale<DT>(amax, true, fp8_format_max(fmt), DT, 0, false, 0, nullptr, row, false).s;
#pragma unroll 1
            for (int j = 0; j < MAXV; ++j) {
                const int vi = j * SB + threadIdx.x;
                if (vi < nv) {
                    uint4 rq = q[0];
#pragma unroll
                    for (int jj = 1; jj < MAXV; ++jj)
                        if (jj == j) rq = q[jj];
                    Vec<T, V> v, o;
                    __builtin_memcpy(&v, &rq, 16);
#pragma unroll
                    for (int k = 0; k < V; ++k) {
                        float val;
                        (void)fp8_encode(float_scaled_exact(to_f32<T>(v.v[k]), sc, DT, false), fmt, sem, &val);
                        o.v[k] = float_emit<T>(val, sc);
                    }
                    store_vec<T, V>(op + vi * V, o);
                }
            }
        }
    }
}

// vectors per thread the row needs: 0 = the kernel does not take the width
static inline int act_step_tier(int dt, int64_t K) {
    const int V = 16 / dtype_size(dt);
    if (K <= 0 || K % V != 0) return 0;
    const int64_t per = ceil_div64(K / V, SB);
    if (per <= 2) return 2;
    if (per <= 4) return 4;
    if (per <= 8) return 8;
    if (per <= 14) return 14;
    return 0;
}

}  // namespace llmc

using namespace llmc;

static inline int64_t cs_chunks(int64_t N, int64_t K, int vec) { return col_chunks(N, K, vec, CS_ROWS, CS_MAX_BLOCKS); }

extern "C" size_t llmc_col_stats_ws_bytes(int64_t N, int64_t K) {
    if (N <= 0 || K <= 0) return 0;
    // sized for the scalar form (the most column blocks leave the fewest chunks; the vector forms never need more per chunk)
    int64_t n = cs_chunks(N, K, 8), n1 = cs_chunks(N, K, 1), n4 = cs_chunks(N, K, 4);
    if (n1 > n) n = n1;
    if (n4 > n) n = n4;
    return (size_t)n * 3 * (size_t)K * sizeof(float);
}

extern "C" int llmc_col_stats(const void* X, int dt, int64_t N, int64_t K, int init, float* run, float* glob, void* ws,
                              llmc_stream_t stream) {
    LLMC_REQUIRE(dtype_ok(dt), "col_stats: bad dtype");
    LLMC_REQUIRE(X && run && ws && N > 0 && K > 0, "col_stats: null/empty argument");
    LLMC_REQUIRE(N < (1ll << 31) + 1 && K < (1ll << 31), "col_stats: N up to 2^31 rows, K below 2^31");
    hipStream_t st = (hipStream_t)stream;
    const int v = col_vec(X, dt, K);
    const int64_t nchunk = cs_chunks(N, K, v);          // the form's vector width: max and min do not depend on the order
    float* part = (float*)ws;
    col_reduce_launch(dt, v, N, K, nchunk, [&](auto t, auto vec, dim3 grid, int64_t rpc) {
        using T = decltype(t);
        hipLaunchKernelGGL((k_col_stats_partial<T, decltype(vec)::value>), grid, dim3(SB), 0, st, (const T*)X, N, K, rpc, part);
    });
    LLMC_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_col_stats_fold, dim3((unsigned)ceil_div64(K, SB)), dim3(SB), 0, st, (const float*)part, nchunk, K,
                       init, run);
    LLMC_LAUNCH_CHECK();
    if (glob) {
        hipLaunchKernelGGL(k_col_stats_global, dim3(1), dim3(1024), 0, st, (const float*)run, K, glob);
        LLMC_LAUNCH_CHECK();
    }
    return LLMC_OK;
}

extern "C" int llmc_smooth_scales(const float* x_absmax, const float* w_absmax, int dt, int64_t K, double alpha,
                                  double one_minus_alpha, void* out, llmc_stream_t stream) {
    LLMC_REQUIRE(dtype_ok(dt), "smooth_scales: bad dtype");
    LLMC_REQUIRE(x_absmax && w_absmax && out && K > 0, "smooth_scales: null/empty argument");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)ceil_div64(K, SB));
    DISPATCH_DT(dt, hipLaunchKernelGGL((k_smooth_scales<T>), grid, dim3(SB), 0, st, x_absmax, w_absmax, K, (float)alpha,
                                       (float)one_minus_alpha, (T*)out));
    LLMC_LAUNCH_CHECK();
    return LLMC_OK;
}

extern "C" int llmc_osplus_scale(const float* cmx, const float* cmn, const void* thresholds, int64_t index, int dt, int64_t K,
                                 void* out, llmc_stream_t stream) {
    LLMC_REQUIRE(dtype_ok(dt), "osplus_scale: bad dtype");
    LLMC_REQUIRE(cmx && cmn && thresholds && out && K > 0 && index >= 0, "osplus_scale: null/empty argument");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)ceil_div64(K, SB));
    const char* thr = (const char*)thresholds + (size_t)index * dtype_size(dt);
    DISPATCH_DT(dt, hipLaunchKernelGGL((k_osplus_scale<T>), grid, dim3(SB), 0, st, cmx, cmn, (const T*)thr, K, (T*)out));
    LLMC_LAUNCH_CHECK();
    return LLMC_OK;
}

extern "C" int llmc_osplus_act_step_tier(int dt, int64_t K) {
    if (!dtype_ok(dt)) return 0;
    return act_step_tier(dt, K);
}

template <typename T, int KIND>
static int act_step_launch(int tier, const void* X, const void* s, int64_t N, int64_t K, int sym, float qmin, float qmax,
                           int mode, void* out, hipStream_t st) {
    const int64_t cap = (int64_t)device_cu_count() * 8;
    const dim3 grid((unsigned)(N < cap ? N : cap));
#define LLMC_ACT_STEP(M)                                                                                              \
    hipLaunchKernelGGL((k_osplus_act_step<T, M, KIND>), grid, dim3(SB), 0, st, (const T*)X, (const T*)s, N, (int)K, sym, \
                       qmin, qmax, mode, (T*)out)
    switch (tier) {
        case 2: LLMC_ACT_STEP(2); break;
        case 4: LLMC_ACT_STEP(4); break;
        case 8: LLMC_ACT_STEP(8); break;
        default: LLMC_ACT_STEP(14); break;
    }
#undef LLMC_ACT_STEP
    LLMC_LAUNCH_CHECK();
    return LLMC_OK;
}

extern "C" int llmc_osplus_act_step(const void* X, const void* s, int dt, int64_t N, int64_t K, int kind, int sym, float qmin,
                                    float qmax, int fp8_mode, void* out, llmc_stream_t stream) {
    LLMC_REQUIRE(dtype_ok(dt), "osplus_act_step: bad dtype");
    LLMC_REQUIRE(X && s && out && N > 0 && K > 0, "osplus_act_step: null/empty argument");
    LLMC_REQUIRE(kind == ACT_INT || kind == ACT_FP8, "osplus_act_step: kind is 0 (integer) or 1 (FP8)");
    LLMC_REQUIRE(kind == ACT_INT || ((fp8_mode >> 4) & 3) <= 1, "osplus_act_step: FP8 format is e4m3 or e5m2");
    const int tier = act_step_tier(dt, K);
    if (tier == 0 || ((uintptr_t)X & 15) || ((uintptr_t)s & 15) || ((uintptr_t)out & 15)) {
        set_last_error_msg("osplus_act_step: rows of whole 16-byte vectors, at most 14 per thread of a 256-thread workgroup "
                           "(K <= 28672 16-bit, 14336 fp32), 16-byte aligned buffers");
        return LLMC_ENOTSUP;
    }
    hipStream_t st = (hipStream_t)stream;
    const int mode = fp8_mode & 0x130;
    if (kind == ACT_INT) {
        DISPATCH_DT(dt, return act_step_launch<T, ACT_INT>(tier, X, s, N, K, sym, qmin, qmax, mode, out, st));
    }
    DISPATCH_DT(dt, return act_step_launch<T, ACT_FP8>(tier, X, s, N, K, sym, qmin, qmax, mode, out, st));
}
