// quant_cols.hip — the min/max quantizer along COLUMNS of a row-major weight (fake_quant_weight_dynamic with dim = 'ic',
// quant.py:833-869; AdaDim re-quantizes every `ic` layer on every forward). A group is g consecutive rows of one column of
// W [R, K]; group index k * (R / g) + r / g, the order of reshape_tensor(W.T). The composition this replaces is a contiguous
// transposed copy -> llmc_quant_dynamic -> a transposed view the GEMM makes contiguous again: three reads and three writes of W.
// Layout: lanes walk columns. A lane owns VEC = 16 B of consecutive columns; 16 lanes cover a 256-B row segment, so one load
// instruction of a wave reads four such segments (four consecutive rows of the strip) and a workgroup of four waves sixteen rows.
// Min / max are kept per lane per column and never cross columns: two shuffle steps fold the wave's four rows, LDS folds the waves.
// No transposed copy, no LDS transpose, no atomics. The group step is quant_group.h's GroupQuant, the one k_quant_static runs.
//   tile   (g <= kTileMaxG) one workgroup per (group row, strip): min/max down the g rows, then the tile again (L2) for the store
//   slab   (g >  kTileMaxG) rows cut into slabs of kSlab: k_cols_partial -> ws, k_cols_fold per column, k_cols_apply quantizes
// Both exist with VEC = 1 for operands that do not allow 16-byte vectors.
#include "common.h"
#include "quant_group.h"
#include "quant_math.h"

namespace llmc {

static constexpr int kBlock = 256;
static constexpr int kWaves = kBlock / 64;
static constexpr int kSeg = 16;                          // lanes per row segment
static constexpr int kRowsPerLoad = 64 / kSeg;           // rows one load instruction of a wave covers
static constexpr int kRowsPerPass = kWaves * kRowsPerLoad;
static constexpr int kUnr = 4;                           // loads in flight per lane
static constexpr int kTileMaxG = 256;                    // tile path: g rows x 256 B <= 64 KiB per workgroup, re-read from L2
static constexpr int kSlab = 64;                         // rows per slab of the slab path
static constexpr int kMaxGrid = 256 * 32;

__host__ __device__ static inline int64_t cols_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

enum { PATH_TILE = 0, PATH_SLAB = 1, PATH_SCALAR = 2, PATH_COUNT = 3 };

// where a thread stands in the strip: its wave, the row of the wave's load it reads, its first column
struct Lane {
    int wave, sub, sl;
};
__device__ __forceinline__ Lane lane_of() {
    Lane l;
    l.wave = threadIdx.x >> 6;
    l.sub = (threadIdx.x & 63) / kSeg;
    l.sl = threadIdx.x & (kSeg - 1);
    return l;
}

// min / max of rows [r0, r1) of this lane's VEC columns at column c, over the rows this lane reads (every kRowsPerPass-th)
template <typename T, int VEC>
__device__ __forceinline__ void lane_minmax(const T* __restrict__ W, int64_t ld, int64_t r0, int64_t r1, int64_t c, bool col_ok,
                                            const Lane& l, float (&mn)[VEC], float (&mx)[VEC]) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        mn[k] = INFINITY;
        mx[k] = -INFINITY;
    }
    if (!col_ok) return;
    for (int64_t r = r0 + l.wave * kRowsPerLoad + l.sub; r < r1; r += (int64_t)kRowsPerPass * kUnr) {
        Vec<T, VEC> v[kUnr];
        bool ok[kUnr];
#pragma unroll
        for (int u = 0; u < kUnr; ++u) {
            const int64_t rr = r + (int64_t)u * kRowsPerPass;
            ok[u] = rr < r1;
            if (ok[u]) v[u] = load_vec<T, VEC>(W + rr * ld + c);
        }
#pragma unroll
        for (int u = 0; u < kUnr; ++u) {
            if (!ok[u]) continue;
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const float f = to_f32<T>(v[u].v[k]);
                mn[k] = fminf(mn[k], f);
                mx[k] = fmaxf(mx[k], f);
            }
        }
    }
}

// fold the per-lane min / max of a workgroup per column: the wave's four rows by shuffles, the four waves through LDS.
// Every thread leaves with the strip's min / max of its own VEC columns. Two barriers; every thread of the block calls it.
template <int VEC>
__device__ __forceinline__ void block_fold(float (&mn)[VEC], float (&mx)[VEC], const Lane& l, float* smn, float* smx) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
#pragma unroll
        for (int o = kSeg; o < 64; o <<= 1) {
            mn[k] = fminf(mn[k], __shfl_xor(mn[k], o, 64));
            mx[k] = fmaxf(mx[k], __shfl_xor(mx[k], o, 64));
        }
    }
    __syncthreads();          // the previous tile's readers are done with smn / smx
    if (l.sub == 0) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            smn[(l.wave * kSeg + l.sl) * VEC + k] = mn[k];
            smx[(l.wave * kSeg + l.sl) * VEC + k] = mx[k];
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        mn[k] = smn[l.sl * VEC + k];
        mx[k] = smx[l.sl * VEC + k];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) {
            mn[k] = fminf(mn[k], smn[(w * kSeg + l.sl) * VEC + k]);
            mx[k] = fmaxf(mx[k], smx[(w * kSeg + l.sl) * VEC + k]);
        }
    }
}

// quantize rows [r0, r1) of this lane's VEC columns from their groups' min / max and store fake values or codes. A group takes
// either branch of round_zp at run time (GroupQuant<true>): round_zp = 0 is quant_static's LLMC_FRACTIONAL_ZP arithmetic.
template <typename T, int VEC, int KIND>
__device__ __forceinline__ void lane_quant(const T* __restrict__ W, int64_t ld, int64_t K, int64_t r0, int64_t r1, int64_t c,
                                           const Lane& l, const float (&mn)[VEC], const float (&mx)[VEC], int sym, int round_zp,
                                           float qmin, float qmax, void* __restrict__ out) {
    using O = typename out_elem<KIND, T>::type;
    GroupQuant<true> q[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k)
        q[k] = GroupQuant<true>::from_minmax(mn[k], mx[k], dt_of<T>::value, sym, round_zp, qmin, qmax);
    for (int64_t r = r0 + l.wave * kRowsPerLoad + l.sub; r < r1; r += (int64_t)kRowsPerPass * kUnr) {
        Vec<T, VEC> v[kUnr];
        bool ok[kUnr];
#pragma unroll
        for (int u = 0; u < kUnr; ++u) {
            const int64_t rr = r + (int64_t)u * kRowsPerPass;
            ok[u] = rr < r1;
            if (ok[u]) v[u] = load_vec<T, VEC>(W + rr * ld + c);
        }
#pragma unroll
        for (int u = 0; u < kUnr; ++u) {
            if (!ok[u]) continue;
            const int64_t rr = r + (int64_t)u * kRowsPerPass;
            Vec<O, VEC> o;
#pragma unroll
            for (int k = 0; k < VEC; ++k) {        // one group per column: quant_vec's step with a quantizer per element
                const float x = to_f32<T>(v[u].v[k]);
                if constexpr (KIND == LLMC_OUT_FAKE) o.v[k] = from_f32<T>(q[k].fake(x, qmin, qmax));
                else o.v[k] = (O)q[k].code(x, qmin, qmax);
            }
            store_vec_wide<O, VEC>((O*)out + rr * K + c, o);     // llmc_quant_dynamic_cols requires a 16-B aligned `out`
        }
    }
}

// scales / zeros of this lane's VEC columns for group row gb, in group order
template <typename T, int VEC>
__device__ __forceinline__ void store_qparams(const float (&mn)[VEC], const float (&mx)[VEC], int64_t c, int64_t gb, int64_t ngr,
                                              int sym, int round_zp, float qmin, float qmax, T* __restrict__ scales,
                                              T* __restrict__ zeros) {
    constexpr int DT = dt_of<T>::value;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        const QParams q = qparams_from_minmax(mn[k], mx[k], DT, sym, round_zp, qmin, qmax);
        if (scales) scales[(c + k) * ngr + gb] = from_f32<T>(q.s);
        if (zeros) zeros[(c + k) * ngr + gb] = from_f32<T>(q.z);
    }
}

// tile path: one workgroup per (group row gb, strip). Consecutive blocks take neighbouring strips of one group row.
template <typename T, int VEC, int KIND>
__global__ __launch_bounds__(kBlock) void k_cols_tile(const T* __restrict__ W, int64_t R, int64_t K, int64_t ld, int64_t g,
                                                      int sym, int round_zp, float qmin, float qmax, void* __restrict__ out,
                                                      T* __restrict__ scales, T* __restrict__ zeros) {
    __shared__ float smn[kWaves * kSeg * VEC], smx[kWaves * kSeg * VEC];
    const Lane l = lane_of();
    const int64_t nstrip = cols_cdiv(K, kSeg * VEC), ngr = R / g;
    for (int64_t t = blockIdx.x; t < nstrip * ngr; t += gridDim.x) {
        const int64_t gb = t / nstrip, c = (t - gb * nstrip) * (kSeg * VEC) + l.sl * VEC;
        const bool col_ok = c < K;            // K % VEC == 0: a lane's columns are all inside or all outside
        float mn[VEC], mx[VEC];
        lane_minmax<T, VEC>(W, ld, gb * g, gb * g + g, c, col_ok, l, mn, mx);
        block_fold<VEC>(mn, mx, l, smn, smx);
        if (!col_ok) continue;
        if (l.wave == 0 && l.sub == 0 && (scales || zeros))
            store_qparams<T, VEC>(mn, mx, c, gb, ngr, sym, round_zp, qmin, qmax, scales, zeros);
        lane_quant<T, VEC, KIND>(W, ld, K, gb * g, gb * g + g, c, l, mn, mx, sym, round_zp, qmin, qmax, out);
    }
}

// slab path, launch 1: per-slab min / max of every column -> pmn / pmx [nslab_total, K]. Slab s covers rows
// gb * g + j * kSlab .. of group row gb = s / spg, j = s % spg (spg slabs per group, the last one of a group may be short).
template <typename T, int VEC>
__global__ __launch_bounds__(kBlock) void k_cols_partial(const T* __restrict__ W, int64_t R, int64_t K, int64_t ld, int64_t g,
                                                         int64_t spg, float* __restrict__ pmn, float* __restrict__ pmx) {
    __shared__ float smn[kWaves * kSeg * VEC], smx[kWaves * kSeg * VEC];
    const Lane l = lane_of();
    const int64_t nstrip = cols_cdiv(K, kSeg * VEC), nslab = (R / g) * spg;
    for (int64_t t = blockIdx.x; t < nstrip * nslab; t += gridDim.x) {
        const int64_t s = t / nstrip, c = (t - s * nstrip) * (kSeg * VEC) + l.sl * VEC;
        const int64_t gb = s / spg, r0 = gb * g + (s - gb * spg) * kSlab;
        const int64_t r1 = r0 + kSlab < gb * g + g ? r0 + kSlab : gb * g + g;
        const bool col_ok = c < K;
        float mn[VEC], mx[VEC];
        lane_minmax<T, VEC>(W, ld, r0, r1, c, col_ok, l, mn, mx);
        block_fold<VEC>(mn, mx, l, smn, smx);
        if (col_ok && l.wave == 0 && l.sub == 0) {
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                pmn[s * K + c + k] = mn[k];
                pmx[s * K + c + k] = mx[k];
            }
        }
    }
}
// launch 2: one thread per (group row, column) folds the spg partials -> fmn / fmx [R / g, K], and the qparams where asked for
template <typename T>
__global__ __launch_bounds__(kBlock) void k_cols_fold(const float* __restrict__ pmn, const float* __restrict__ pmx, int64_t ngr,
                                                      int64_t K, int64_t spg, int sym, int round_zp, float qmin, float qmax,
                                                      float* __restrict__ fmn, float* __restrict__ fmx, T* __restrict__ scales,
                                                      T* __restrict__ zeros) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < ngr * K; i += (int64_t)gridDim.x * kBlock) {
        const int64_t gb = i / K, c = i - gb * K;
        float mn[1] = {INFINITY}, mx[1] = {-INFINITY};
        for (int64_t j = 0; j < spg; ++j) {
            mn[0] = fminf(mn[0], pmn[(gb * spg + j) * K + c]);
            mx[0] = fmaxf(mx[0], pmx[(gb * spg + j) * K + c]);
        }
        fmn[i] = mn[0];
        fmx[i] = mx[0];
        if (scales || zeros) store_qparams<T, 1>(mn, mx, c, gb, ngr, sym, round_zp, qmin, qmax, scales, zeros);
    }
}
// launch 3: quantize slab by slab from the folded min / max
template <typename T, int VEC, int KIND>
__global__ __launch_bounds__(kBlock) void k_cols_apply(const T* __restrict__ W, int64_t R, int64_t K, int64_t ld, int64_t g,
                                                       int64_t spg, const float* __restrict__ fmn, const float* __restrict__ fmx,
                                                       int sym, int round_zp, float qmin, float qmax, void* __restrict__ out) {
    const Lane l = lane_of();
    const int64_t nstrip = cols_cdiv(K, kSeg * VEC), nslab = (R / g) * spg;
    for (int64_t t = blockIdx.x; t < nstrip * nslab; t += gridDim.x) {
        const int64_t s = t / nstrip, c = (t - s * nstrip) * (kSeg * VEC) + l.sl * VEC;
        const int64_t gb = s / spg, r0 = gb * g + (s - gb * spg) * kSlab;
        const int64_t r1 = r0 + kSlab < gb * g + g ? r0 + kSlab : gb * g + g;
        if (c >= K) continue;
        float mn[VEC], mx[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            mn[k] = fmn[gb * K + c + k];
            mx[k] = fmx[gb * K + c + k];
        }
        lane_quant<T, VEC, KIND>(W, ld, K, r0, r1, c, l, mn, mx, sym, round_zp, qmin, qmax, out);
    }
}

static inline bool cols_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static inline int64_t slabs_per_group(int64_t g) { return cols_cdiv(g, kSlab); }

// argument checks + the launch path; everything llmc_quant_dynamic_cols refuses for W's own sake is refused here
static int cols_path(const void* W, int dt, int64_t R, int64_t K, int64_t ld, int64_t g) {
    LLMC_REQUIRE(dtype_ok(dt), "quant_dynamic_cols: bad dtype");
    LLMC_REQUIRE(W != nullptr, "quant_dynamic_cols: null W");
    LLMC_REQUIRE(R > 0 && K > 0 && g > 0, "quant_dynamic_cols: R, K and g must be positive");
    LLMC_REQUIRE(R % g == 0, "quant_dynamic_cols: g must divide R (groups run down a column)");
    LLMC_REQUIRE(ld >= K, "quant_dynamic_cols: ld < K");
    const int vec = 16 / dtype_size(dt);
    if (!(cols_aligned16(W) && ld % vec == 0 && K % vec == 0)) return PATH_SCALAR;
    return g <= kTileMaxG ? PATH_TILE : PATH_SLAB;
}

template <typename T, int VEC, int KIND>
static int cols_launch(const void* W, int64_t R, int64_t K, int64_t ld, int64_t g, int sym, int round_zp, float qmin, float qmax,
                       void* out, void* scales, void* zeros, void* ws, hipStream_t st) {
    const int64_t nstrip = cols_cdiv(K, kSeg * VEC), ngr = R / g;
    if (g <= kTileMaxG) {
        const int grid = capped_grid(nstrip * ngr, 1, kMaxGrid);
        hipLaunchKernelGGL((k_cols_tile<T, VEC, KIND>), dim3(grid), dim3(kBlock), 0, st, (const T*)W, R, K, ld, g, sym, round_zp,
                           qmin, qmax, out, (T*)scales, (T*)zeros);
        LLMC_LAUNCH_CHECK();
        return LLMC_OK;
    }
    const int64_t spg = slabs_per_group(g), nslab = ngr * spg;
    float* pmn = (float*)ws;
    float* pmx = pmn + nslab * K;
    float* fmn = pmx + nslab * K;
    float* fmx = fmn + ngr * K;
    const int grid = capped_grid(nstrip * nslab, 1, kMaxGrid);
    hipLaunchKernelGGL((k_cols_partial<T, VEC>), dim3(grid), dim3(kBlock), 0, st, (const T*)W, R, K, ld, g, spg, pmn, pmx);
    LLMC_LAUNCH_CHECK();
    hipLaunchKernelGGL((k_cols_fold<T>), dim3(capped_grid(ngr * K, kBlock, kMaxGrid)), dim3(kBlock), 0, st, pmn, pmx, ngr, K, spg,
                       sym, round_zp, qmin, qmax, fmn, fmx, (T*)scales, (T*)zeros);
    LLMC_LAUNCH_CHECK();
    hipLaunchKernelGGL((k_cols_apply<T, VEC, KIND>), dim3(grid), dim3(kBlock), 0, st, (const T*)W, R, K, ld, g, spg, fmn, fmx, sym,
                       round_zp, qmin, qmax, out);
    LLMC_LAUNCH_CHECK();
    return LLMC_OK;
}

template <typename T, int KIND>
static int cols_tk(bool vec, const void* W, int64_t R, int64_t K, int64_t ld, int64_t g, int sym, int round_zp, float qmin,
                   float qmax, void* out, void* scales, void* zeros, void* ws, hipStream_t st) {
    constexpr int V16 = 16 / sizeof(T);
    if (vec) return cols_launch<T, V16, KIND>(W, R, K, ld, g, sym, round_zp, qmin, qmax, out, scales, zeros, ws, st);
    return cols_launch<T, 1, KIND>(W, R, K, ld, g, sym, round_zp, qmin, qmax, out, scales, zeros, ws, st);
}

template <typename T>
static int cols_t(bool vec, int kind, const void* W, int64_t R, int64_t K, int64_t ld, int64_t g, int sym, int round_zp,
                  float qmin, float qmax, void* out, void* scales, void* zeros, void* ws, hipStream_t st) {
    DISPATCH_OUT_KIND(kind, return cols_tk<T, KIND>(vec, W, R, K, ld, g, sym, round_zp, qmin, qmax, out, scales, zeros, ws, st));
    set_last_error_msg("quant_dynamic_cols: bad out_kind");
    return LLMC_EINVAL;
}

}  // namespace llmc

using namespace llmc;

extern "C" size_t llmc_quant_dynamic_cols_ws_bytes(int64_t R, int64_t K, int64_t g) {
    if (R <= 0 || K <= 0 || g <= 0 || R % g || g <= kTileMaxG) return 0;
    return (size_t)((R / g) * (slabs_per_group(g) + 1) * K) * 2 * sizeof(float);
}

extern "C" int llmc_quant_dynamic_cols_paths(void) { return PATH_COUNT; }

extern "C" int llmc_quant_dynamic_cols_path(const void* W, int dt, int64_t R, int64_t K, int64_t ld, int64_t g) {
    return cols_path(W, dt, R, K, ld, g);
}

extern "C" int llmc_quant_dynamic_cols(const void* W, int dt, int64_t R, int64_t K, int64_t ld, int64_t g, int sym, int round_zp,
                                       float qmin, float qmax, int out_kind, void* out, void* scales_out, void* zeros_out,
                                       void* ws, llmc_stream_t stream) {
    const int path = cols_path(W, dt, R, K, ld, g);
    if (path < 0) return path;
    LLMC_REQUIRE(out != nullptr, "quant_dynamic_cols: null out");
    LLMC_REQUIRE(out_kind == LLMC_OUT_FAKE || out_kind == LLMC_OUT_I32 || out_kind == LLMC_OUT_I8 || out_kind == LLMC_OUT_U8,
                 "quant_dynamic_cols: bad out_kind");
    LLMC_REQUIRE(cols_aligned16(out), "quant_dynamic_cols: out must be 16-byte aligned");
    const size_t osize = out_kind == LLMC_OUT_FAKE ? dtype_size(dt) : (out_kind == LLMC_OUT_I32 ? 4 : 1);
    const char* w0 = (const char*)W;
    const char* w1 = w0 + ((size_t)(R - 1) * ld + K) * dtype_size(dt);
    const char* o0 = (const char*)out;
    const char* o1 = o0 + (size_t)R * K * osize;
    LLMC_REQUIRE(o1 <= w0 || w1 <= o0, "quant_dynamic_cols: out must not overlap W");
    LLMC_REQUIRE(g <= kTileMaxG || ws != nullptr, "quant_dynamic_cols: workspace required for groups longer than 256 rows");
    hipStream_t st = (hipStream_t)stream;
    DISPATCH_DT(dt, return cols_t<T>(path != PATH_SCALAR, out_kind, W, R, K, ld, g, sym, round_zp, qmin, qmax, out, scales_out,
                                     zeros_out, ws, st));
}
