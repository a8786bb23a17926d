// awq_kernels.hip — HBM-bound pieces of AWQ's scale search (awq.py:48-108) and of apply_scale /
// scaling_input (base_blockwise_quantization.py:597-611, 877-897). All arithmetic in the tensor dtype with
// ATen's per-op rounding; reductions accumulate in fp32 in a fixed order (deterministic).
#include "common.h"
#include "vec16.h"

namespace llmc {

static constexpr int AB = 256;
static constexpr int TOK_CHUNK = 512;  // tokens per partial sum of the column mean

// ---- column mean of |x| over tokens: stage 1 partial sums [nchunk][K] fp32, stage 2 ordered sum / N -> dt
template <typename T>
__global__ __launch_bounds__(AB) void k_abs_colsum_partial(const T* __restrict__ X, int64_t N, int64_t K,
                                                           float* __restrict__ part) {
    constexpr int V = 16 / sizeof(T);
    const int64_t c0 = ((int64_t)blockIdx.x * AB + threadIdx.x) * V;
    if (c0 >= K) return;
    const int64_t t0 = (int64_t)blockIdx.y * TOK_CHUNK;
    const int64_t t1 = t0 + TOK_CHUNK < N ? t0 + TOK_CHUNK : N;
    float acc[V];
#pragma unroll
    for (int i = 0; i < V; ++i) acc[i] = 0.0f;
    for (int64_t t = t0; t < t1; ++t) {          // llmc_awq_act_mean takes rows of whole vectors only: c0 + V <= K
        const Vec<T, V> v = load_vec<T, V>(X + t * K + c0);
#pragma unroll
        for (int i = 0; i < V; ++i) acc[i] += fabsf(to_f32<T>(v.v[i]));
    }
#pragma unroll
    for (int i = 0; i < V; ++i) part[(int64_t)blockIdx.y * K + c0 + i] = acc[i];
}
template <typename T>
__global__ __launch_bounds__(AB) void k_colsum_final(const float* __restrict__ part, int64_t nchunk, int64_t K,
                                                     float denom, T* __restrict__ out) {
    constexpr int DT = dt_of<T>::value;
    const int64_t c = (int64_t)blockIdx.x * AB + threadIdx.x;
    if (c >= K) return;
    float s = 0.0f;
    for (int64_t i = 0; i < nchunk; ++i) s += part[i * K + c];
    out[c] = from_f32<T>(rndc<DT>(s / denom));
}

// ---- Awq.get_weight_scale for one layer: mean over rows of |w| / groupmax(|w|)   (awq.py:59-66)
// one workgroup per slab of rows; thread owns 16-B column chunks; group max via the LPR-lane shuffle
template <typename T>
__global__ __launch_bounds__(AB) void k_wscale_partial(const T* __restrict__ W, int64_t R, int64_t K, int g,
                                                       int rows_per_block, float* __restrict__ part) {
    constexpr int DT = dt_of<T>::value;
    constexpr int V = 16 / sizeof(T);
    const int lpr = g / V;  // lanes per group (power of two <= 64 enforced by the host)
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
    const int64_t r1 = r0 + rows_per_block < R ? r0 + rows_per_block : R;
    for (int64_t c0 = (int64_t)threadIdx.x * V; c0 < K; c0 += (int64_t)AB * V) {
        float acc[V];
#pragma unroll
        for (int i = 0; i < V; ++i) acc[i] = 0.0f;
        for (int64_t r = r0; r < r1; ++r) {
            const Vec<T, V> v = load_vec<T, V>(W + r * K + c0);
            float a[V], m = 0.0f;
#pragma unroll
            for (int i = 0; i < V; ++i) {
                a[i] = fabsf(to_f32<T>(v.v[i]));
                m = fmaxf(m, a[i]);
            }
            m = wave_max(m, lpr);
#pragma unroll
            for (int i = 0; i < V; ++i) acc[i] += rndc<DT>(a[i] / m);
        }
#pragma unroll
        for (int i = 0; i < V; ++i) part[(int64_t)blockIdx.x * K + c0 + i] = acc[i];
    }
}

// Same partial sums for any group width (K % g == 0; per-channel g = K up to whole rows). One workgroup per slab of
// WS_ROWS rows; the columns are walked in tiles of whole groups: first the tile's group maxima of the slab's rows into LDS
// (LPR lanes per group, each lane looping over its part of the group, as the quantizer kernels do), then the per-column
// sums over the slab's rows in row order: the summation order of k_wscale_partial, so both give the same bits.
static constexpr int WS_ROWS = 16;
static constexpr int WS_TILE_GROUPS = 256;   // groups per column tile: LDS of WS_ROWS x 256 floats

template <typename T, int VEC>
__device__ __forceinline__ void load_abs(const T* p, float (&a)[VEC]) {
    const Vec<T, VEC> v = load_vec<T, VEC>(p);
#pragma unroll
    for (int i = 0; i < VEC; ++i) a[i] = fabsf(to_f32<T>(v.v[i]));
}

template <typename T, int VEC>  // VEC > 1 needs g % VEC == 0 and 16-B aligned rows: a vector never straddles two groups
__global__ __launch_bounds__(AB) void k_wscale_partial_any(const T* __restrict__ W, int64_t R, int64_t K, int64_t g,
                                                           int lpr, float* __restrict__ part) {
    constexpr int DT = dt_of<T>::value;
    __shared__ float gmax[WS_ROWS * WS_TILE_GROUPS];
    const int64_t r0 = (int64_t)blockIdx.x * WS_ROWS;
    const int nr = (int)(R - r0 < WS_ROWS ? R - r0 : WS_ROWS);
    const int64_t ngr = K / g;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int gpw = 64 / lpr, sub = lane / lpr, sl = lane % lpr;   // groups per wave pass, this lane's group and slot
    for (int64_t j0 = 0; j0 < ngr; j0 += WS_TILE_GROUPS) {
        const int nj = (int)(ngr - j0 < WS_TILE_GROUPS ? ngr - j0 : WS_TILE_GROUPS);
        const int items = nr * nj;                                  // (row, group) pairs of the tile, row-major
        for (int base = wave * gpw; base < items; base += (AB / 64) * gpw) {
            const int item = base + sub;
            const int it = item < items ? item : items - 1;         // idle lanes repeat the last pair: the shuffle needs all
            const T* p = W + (r0 + it / nj) * K + (j0 + it % nj) * g;
            float m = 0.0f;
            for (int64_t c = (int64_t)sl * VEC; c < g; c += (int64_t)lpr * VEC) {
                float a[VEC];
                load_abs<T, VEC>(p + c, a);
#pragma unroll
                for (int i = 0; i < VEC; ++i) m = fmaxf(m, a[i]);
            }
            m = wave_max(m, lpr);
            if (item < items && sl == 0) gmax[item] = m;
        }
        __syncthreads();
        const int64_t c0t = j0 * g, c1t = (j0 + nj) * g;
        for (int64_t c = c0t + (int64_t)threadIdx.x * VEC; c < c1t; c += (int64_t)AB * VEC) {
            const int j = (int)((c - c0t) / g);
            float acc[VEC];
#pragma unroll
            for (int i = 0; i < VEC; ++i) acc[i] = 0.0f;
            for (int r = 0; r < nr; ++r) {
                float a[VEC];
                load_abs<T, VEC>(W + (r0 + r) * K + c, a);
                const float m = gmax[r * nj + j];
#pragma unroll
                for (int i = 0; i < VEC; ++i) acc[i] += rndc<DT>(a[i] / m);
            }
#pragma unroll
            for (int i = 0; i < VEC; ++i) part[(int64_t)blockIdx.x * K + c + i] = acc[i];
        }
        __syncthreads();   // the next tile overwrites gmax
    }
}

// ---- Awq.get_scales (awq.py:98-108), single workgroup
template <typename T>
__global__ __launch_bounds__(1024) void k_awq_scales(const T* __restrict__ xm, const T* __restrict__ wm, int64_t K,
                                                     float ratio, float one_minus_ratio, int version,
                                                     T* __restrict__ out) {
    constexpr int DT = dt_of<T>::value;
    __shared__ float smx[16], smn[16];
    const float lo = rndc<DT>(1e-4f);
    // Tensor.pow(python_float) casts the exponent to the tensor dtype first (ATen CPU scalar handling)
    const float er = rndc<DT>(ratio), ew = rndc<DT>(one_minus_ratio);
    float mx = -INFINITY, mn = INFINITY;
    for (int64_t k = threadIdx.x; k < K; k += 1024) {
        float s;
        const float x = to_f32<T>(xm[k]);
        if (version == 1) {
            const float a = rndc<DT>(powf(x, er));
            const float b = rndc<DT>(powf(to_f32<T>(wm[k]), ew));
            s = rndc<DT>(a / b);
        } else {
            s = rndc<DT>(powf(x, er));
        }
        s = fmaxf(s, lo);
        out[k] = from_f32<T>(s);
        mx = fmaxf(mx, s);
        mn = fminf(mn, s);
    }
    mx = wave_max(mx, 64);
    mn = wave_min(mn, 64);
    if ((threadIdx.x & 63) == 0) {
        smx[threadIdx.x >> 6] = mx;
        smn[threadIdx.x >> 6] = mn;
    }
    __syncthreads();
    mx = smx[0];
    mn = smn[0];
    for (int i = 1; i < 16; ++i) {
        mx = fmaxf(mx, smx[i]);
        mn = fminf(mn, smn[i]);
    }
    const float den = rndc<DT>(sqrtf(rndc<DT>(mx * mn)));
    for (int64_t k = threadIdx.x; k < K; k += 1024) out[k] = from_f32<T>(rndc<DT>(to_f32<T>(out[k]) / den));
}

// ---- x / s[col], w * s[col], clamp per (row, group)
template <typename T, int OP>  // OP 0: out = x / s ; 1: out = x * s
__global__ __launch_bounds__(AB) void k_cols_op(const T* __restrict__ X, const T* __restrict__ s, int64_t N,
                                                int64_t K, T* __restrict__ out) {
    constexpr int DT = dt_of<T>::value;
    constexpr int V = 16 / sizeof(T);
    const int64_t nv = K / V;
    const int64_t total = N * nv;
    for (int64_t i = (int64_t)blockIdx.x * AB + threadIdx.x; i < total; i += (int64_t)gridDim.x * AB) {
        const int64_t r = i / nv, c = (i - r * nv) * V;
        const Vec<T, V> xv = load_vec<T, V>(X + r * K + c), sv = load_vec<T, V>(s + c);
        Vec<T, V> ov;
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const float a = to_f32<T>(xv.v[k]), b = to_f32<T>(sv.v[k]);
            ov.v[k] = from_f32<T>(rndc<DT>(OP == 0 ? a / b : a * b));
        }
        store_vec<T, V>(out + r * K + c, ov);
    }
}
// x / s[col] written K-TILED (T[K/32][rows][32], linear_eval.hip): block = 64 rows x two 32-k slices, thread = one 16-B
// chunk of each; whole 128-B lines in, KiB runs out. 16-bit T only.
template <typename T>
__global__ __launch_bounds__(256) void k_div_cols_kt(const T* __restrict__ X, const T* __restrict__ s, int64_t N,
                                                     int64_t K, T* __restrict__ out) {
    constexpr int DT = dt_of<T>::value;
    const int r = threadIdx.x >> 2, c = threadIdx.x & 3;
    const int64_t row = (int64_t)blockIdx.x * 64 + r;
    if (row >= N) return;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int64_t kt = (int64_t)blockIdx.y * 2 + j;
        if (kt * 32 >= K) break;
        const int64_t col = kt * 32 + c * 8;
        const Vec<T, 8> xv = load_vec<T, 8>(X + row * K + col), sv = load_vec<T, 8>(s + col);
        Vec<T, 8> ov;
#pragma unroll
        for (int k = 0; k < 8; ++k) ov.v[k] = from_f32<T>(rndc<DT>(to_f32<T>(xv.v[k]) / to_f32<T>(sv.v[k])));
        store_vec<T, 8>(out + (kt * N + row) * 32 + c * 8, ov);
    }
}
template <typename T>
__global__ __launch_bounds__(AB) void k_clamp_groups(T* __restrict__ W, int64_t R, int64_t K, int64_t g,
                                                     const T* __restrict__ mn, const T* __restrict__ mx) {
    const int64_t total = R * K;
    const int64_t gpr = K / g;
    for (int64_t i = (int64_t)blockIdx.x * AB + threadIdx.x; i < total; i += (int64_t)gridDim.x * AB) {
        const int64_t r = i / K, c = i - r * K;
        const int64_t gi = r * gpr + c / g;
        float v = to_f32<T>(W[i]);
        v = fminf(fmaxf(v, to_f32<T>(mn[gi])), to_f32<T>(mx[gi]));
        W[i] = from_f32<T>(v);
    }
}

}  // namespace llmc

using namespace llmc;

extern "C" size_t llmc_awq_act_mean_ws_bytes(int64_t N, int64_t K) {
    if (N <= 0 || K <= 0) return 0;
    return (size_t)ceil_div64(N, TOK_CHUNK) * K * sizeof(float);
}

extern "C" int llmc_awq_act_mean(const void* X, int dt, int64_t N, int64_t K, void* out, void* ws,
                                 llmc_stream_t stream) {
    LLMC_REQUIRE(dtype_ok(dt), "awq_act_mean: bad dtype");
    LLMC_REQUIRE(X && out && ws && N > 0 && K > 0, "awq_act_mean: null/empty argument");
    LLMC_REQUIRE(((uintptr_t)X & 15) == 0 && (K * dtype_size(dt)) % 16 == 0, "awq_act_mean: rows must be 16-B aligned");
    hipStream_t st = (hipStream_t)stream;
    const int64_t nchunk = ceil_div64(N, TOK_CHUNK);
    const int V = 16 / dtype_size(dt);
    dim3 grid((unsigned)ceil_div64(K, (int64_t)AB * V), (unsigned)nchunk);
    DISPATCH_DT(dt, hipLaunchKernelGGL((k_abs_colsum_partial<T>), grid, dim3(AB), 0, st, (const T*)X, N, K, (float*)ws));
    LLMC_LAUNCH_CHECK();
    DISPATCH_DT(dt, hipLaunchKernelGGL((k_colsum_final<T>), dim3((unsigned)ceil_div64(K, AB)), dim3(AB), 0, st,
                                       (const float*)ws, nchunk, K, (float)N, (T*)out));
    LLMC_LAUNCH_CHECK();
    return LLMC_OK;
}

extern "C" size_t llmc_awq_weight_mean_ws_bytes(int64_t R, int64_t K) {
    if (R <= 0 || K <= 0) return 0;
    return (size_t)ceil_div64(R, 16) * K * sizeof(float);
}

extern "C" int llmc_awq_weight_mean(const void* W, int dt, int64_t R, int64_t K, int64_t g, void* out_dt, void* ws,
                                    llmc_stream_t stream) {
    LLMC_REQUIRE(dtype_ok(dt), "awq_weight_mean: bad dtype");
    LLMC_REQUIRE(W && out_dt && ws && R > 0 && K > 0, "awq_weight_mean: null/empty argument");
    if (g <= 0) g = K;
    LLMC_REQUIRE(K % g == 0, "awq_weight_mean: K must be a multiple of the group size");
    hipStream_t st = (hipStream_t)stream;
    const int V = 16 / dtype_size(dt);
    const int64_t nblk = ceil_div64(R, WS_ROWS);
    const bool vec = g % V == 0 && ((uintptr_t)W & 15) == 0;   // K % g == 0: whole rows of 16-B chunks too
    const int64_t lpr = g / V;
    if (vec && lpr <= 64 && (lpr & (lpr - 1)) == 0) {
        // a group is a power of two <= 64 of 16-B chunks: one shuffle over the group's lanes per row, one pass over W
        DISPATCH_DT(dt, hipLaunchKernelGGL((k_wscale_partial<T>), dim3((unsigned)nblk), dim3(AB), 0, st, (const T*)W, R,
                                           K, (int)g, WS_ROWS, (float*)ws));
    } else if (vec) {
        const int l = pow2_ceil(lpr < 64 ? lpr : 64);
        DISPATCH_DT(dt, hipLaunchKernelGGL((k_wscale_partial_any<T, 16 / sizeof(T)>), dim3((unsigned)nblk), dim3(AB), 0,
                                           st, (const T*)W, R, K, g, l, (float*)ws));
    } else {
        const int l = pow2_ceil(g < 64 ? g : 64);
        DISPATCH_DT(dt, hipLaunchKernelGGL((k_wscale_partial_any<T, 1>), dim3((unsigned)nblk), dim3(AB), 0, st,
                                           (const T*)W, R, K, g, l, (float*)ws));
    }
    LLMC_LAUNCH_CHECK();
    DISPATCH_DT(dt, hipLaunchKernelGGL((k_colsum_final<T>), dim3((unsigned)ceil_div64(K, AB)), dim3(AB), 0, st,
                                       (const float*)ws, nblk, K, (float)R, (T*)out_dt));
    LLMC_LAUNCH_CHECK();
    return LLMC_OK;
}

extern "C" int llmc_awq_scales(const void* x_mean, const void* w_mean, int dt, int64_t K, double ratio_d,
                               int version, void* out, llmc_stream_t stream) {
    const float ratio = (float)ratio_d;
    LLMC_REQUIRE(dtype_ok(dt), "awq_scales: bad dtype");
    LLMC_REQUIRE(x_mean && out && K > 0, "awq_scales: null/empty argument");
    LLMC_REQUIRE(version == 2 || (version == 1 && w_mean), "awq_scales: v1 needs w_mean");
    hipStream_t st = (hipStream_t)stream;
    DISPATCH_DT(dt, hipLaunchKernelGGL((k_awq_scales<T>), dim3(1), dim3(1024), 0, st, (const T*)x_mean,
                                       (const T*)w_mean, K, ratio, (float)(1.0 - (double)ratio_d), version, (T*)out));
    LLMC_LAUNCH_CHECK();
    return LLMC_OK;
}

extern "C" int llmc_div_cols(const void* X, const void* s, int dt, int64_t N, int64_t K, void* out,
                             llmc_stream_t stream) {
    LLMC_REQUIRE(dtype_ok(dt) && X && s && out && N > 0 && K > 0, "div_cols: bad argument");
    LLMC_REQUIRE((K * dtype_size(dt)) % 16 == 0 && ((uintptr_t)X & 15) == 0 && ((uintptr_t)out & 15) == 0 &&
                     ((uintptr_t)s & 15) == 0, "div_cols: rows must be 16-B aligned");
    hipStream_t st = (hipStream_t)stream;
    const int V = 16 / dtype_size(dt);
    DISPATCH_DT(dt, hipLaunchKernelGGL((k_cols_op<T, 0>), dim3(capped_grid(N * (K / V), AB, 8192)), dim3(AB), 0, st, (const T*)X,
                                       (const T*)s, N, K, (T*)out));
    LLMC_LAUNCH_CHECK();
    return LLMC_OK;
}

extern "C" int llmc_div_cols_kt(const void* X, const void* s, int dt, int64_t N, int64_t K, void* out,
                                llmc_stream_t stream) {
    LLMC_REQUIRE((dt == LLMC_F16 || dt == LLMC_BF16) && X && s && out && X != out && N > 0 && K > 0,
                 "div_cols_kt: bad argument (16-bit dtypes, out of place)");
    LLMC_REQUIRE(K % 32 == 0 && K / 64 < 65535 && ((uintptr_t)X & 15) == 0 && ((uintptr_t)out & 15) == 0 &&
                     ((uintptr_t)s & 15) == 0, "div_cols_kt: needs K % 32 == 0 and 16-B aligned buffers");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)ceil_div64(N, 64), (unsigned)ceil_div64(K, 64));
    DISPATCH_DT(dt, if constexpr (sizeof(T) == 2) hipLaunchKernelGGL((k_div_cols_kt<T>), grid, dim3(256), 0, st, (const T*)X,
                                                                     (const T*)s, N, K, (T*)out));
    LLMC_LAUNCH_CHECK();
    return LLMC_OK;
}

extern "C" int llmc_mul_cols(void* W, const void* s, int dt, int64_t R, int64_t K, llmc_stream_t stream) {
    LLMC_REQUIRE(dtype_ok(dt) && W && s && R > 0 && K > 0, "mul_cols: bad argument");
    LLMC_REQUIRE((K * dtype_size(dt)) % 16 == 0 && ((uintptr_t)W & 15) == 0 && ((uintptr_t)s & 15) == 0,
                 "mul_cols: rows must be 16-B aligned");
    hipStream_t st = (hipStream_t)stream;
    const int V = 16 / dtype_size(dt);
    DISPATCH_DT(dt, hipLaunchKernelGGL((k_cols_op<T, 1>), dim3(capped_grid(R * (K / V), AB, 8192)), dim3(AB), 0, st, (const T*)W,
                                       (const T*)s, R, K, (T*)W));
    LLMC_LAUNCH_CHECK();
    return LLMC_OK;
}

extern "C" int llmc_clamp_groups(void* W, int dt, int64_t R, int64_t K, int64_t g, const void* min_val,
                                 const void* max_val, llmc_stream_t stream) {
    LLMC_REQUIRE(dtype_ok(dt) && W && min_val && max_val && R > 0 && K > 0, "clamp_groups: bad argument");
    if (g <= 0) g = K;
    LLMC_REQUIRE(K % g == 0, "clamp_groups: K must be a multiple of the group size");
    hipStream_t st = (hipStream_t)stream;
    DISPATCH_DT(dt, hipLaunchKernelGGL((k_clamp_groups<T>), dim3(capped_grid(R * K, AB, 8192)), dim3(AB), 0, st, (T*)W, R, K, g,
                                       (const T*)min_val, (const T*)max_val));
    LLMC_LAUNCH_CHECK();
    return LLMC_OK;
}
