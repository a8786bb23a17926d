// block_influence.hip — ShortGPT's Block Influence (ShortGPT.compute_bi, shortgpt.py:40-55 of the reference): one cosine per token
// between a block's input X and its output Y, [N, d] each. The reference forms X @ Y.T, an N x N product, and keeps its diagonal;
// here each element of X and Y is read once. One wave owns a row: three fp32 sums (x.y, x.x, y.y) per lane over the row's 16-byte
// slots, a fixed butterfly over the 64 lanes, then the handful of scalar operations of the reference's dot / (norm * norm).
// The sum of the per-token values, the block's score, is folded on the device in fp64 in an order that depends on N alone
// (k_bi_chunk_sums, k_bi_total): no atomics, nothing read on the host. include/llmc_hip.h states the order; tests/shortgpt_oracle.py
// repeats it in numpy bit for bit. Pure streaming: no LDS in the row kernel, U independent 16-byte loads per tensor in flight per
// lane (a row of 4096 bf16 is 8 slots per lane per tensor: two rounds of the unrolled loop).
#include <float.h>

#include "common.h"
#include "vec16.h"

namespace llmc {

static constexpr int kBiBlock = 256, kBiWaves = kBiBlock / 64;
static constexpr int kBiUnroll = 4;                   // slots per tensor a lane loads before it folds them
static constexpr int kBiMaxGrid = 256 * 8;            // blocks of the row kernel: 8 per CU, the rest by the grid-stride loop
static constexpr int kBiChunk = 4096;                 // rows of one chunk of the fp64 total (llmc_hip.h promises this number)

// slot j of a row: its V = 16 / sizeof(T) elements in one load, or element by element with +0 behind the row's end. s + (+0)
// leaves every s of these chains as it is (they start at +0 and never become -0), so the padding is outside the stated order.
template <typename T, bool VECLOAD>
__device__ __forceinline__ Vec<T, 16 / (int)sizeof(T)> load_slot(const T* __restrict__ row, int j, int d) {
    constexpr int V = 16 / (int)sizeof(T);
    const int64_t at = (int64_t)j * V;
    if constexpr (VECLOAD) {
        return load_vec<T, V>(row + at);
    } else {
        Vec<T, V> r;
#pragma unroll
        for (int e = 0; e < V; ++e) r.v[e] = at + e < d ? load_vec<T, 1>(row + at + e).v[0] : zero_of<T>();
        return r;
    }
}

// the elements of one slot onto the lane's three sums, in index order; every product and every add rounded on its own
template <typename T, int V>
__device__ __forceinline__ void fold_slot(const Vec<T, V>& x, const Vec<T, V>& y, float& dot, float& sx, float& sy) {
#pragma unroll
    for (int e = 0; e < V; ++e) {
        const float a = to_f32<T>(x.v[e]), b = to_f32<T>(y.v[e]);
        dot = __fadd_rn(dot, __fmul_rn(a, b));
        sx = __fadd_rn(sx, __fmul_rn(a, a));
        sy = __fadd_rn(sy, __fmul_rn(b, b));
    }
}

// grid-stride over the rows, one wave per row; lane l owns the slots l, l + 64, ...
template <typename T, bool VECLOAD>
__global__ __launch_bounds__(kBiBlock) void k_block_influence(const T* __restrict__ X, const T* __restrict__ Y, int64_t N, int d,
                                                              int nslot, int64_t ldx, int64_t ldy, float* __restrict__ bi) {
    constexpr int V = 16 / (int)sizeof(T), U = kBiUnroll;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t stride = (int64_t)gridDim.x * kBiWaves;
    for (int64_t row = (int64_t)blockIdx.x * kBiWaves + wv; row < N; row += stride) {
        const T* x = X + row * ldx;
        const T* y = Y + row * ldy;
        float dot = 0.0f, sx = 0.0f, sy = 0.0f;
        int j = lane;
        for (; j < nslot - 64 * (U - 1); j += 64 * U) {
            Vec<T, V> xv[U], yv[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                xv[u] = load_slot<T, VECLOAD>(x, j + 64 * u, d);
                yv[u] = load_slot<T, VECLOAD>(y, j + 64 * u, d);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) fold_slot<T, V>(xv[u], yv[u], dot, sx, sy);
        }
        for (; j < nslot; j += 64) fold_slot<T, V>(load_slot<T, VECLOAD>(x, j, d), load_slot<T, VECLOAD>(y, j, d), dot, sx, sy);
        // the xor butterfly 32, 16, 8, 4, 2, 1: every lane ends with the same bits (a + b is commutative)
        dot = wave_sum(dot, 64);
        sx = wave_sum(sx, 64);
        sy = wave_sum(sy, 64);
        if (lane == 0) {
            float sim = dot / (sqrtf(sx) * sqrtf(sy));          // the reference's dot / (norm_in * norm_out); IEEE sqrt and division
            if (__builtin_isnan(sim)) sim = 0.5f;               // nan_to_num(nan=0.5): a zero row, a NaN, inf / inf
            else if (__builtin_isinf(sim)) sim = sim > 0.0f ? FLT_MAX : -FLT_MAX;
            bi[row] = __fsub_rn(1.0f, sim);
        }
    }
}

// 256 fp64 values joined by the tree s = 128, 64, ..., 1: v[t] = v[t] + v[t + s]
__device__ __forceinline__ double bi_tree_sum(double a, double* sm) {
    const int t = threadIdx.x;
    sm[t] = a;
    __syncthreads();
#pragma unroll
    for (int s = kBiBlock / 2; s > 0; s >>= 1) {
        if (t < s) sm[t] = sm[t] + sm[t + s];
        __syncthreads();
    }
    return sm[0];
}

// one workgroup per chunk of kBiChunk rows: thread t adds bi[r0 + t], bi[r0 + t + 256], ... in fp64 from 0
__global__ __launch_bounds__(kBiBlock) void k_bi_chunk_sums(const float* __restrict__ bi, int64_t N, double* __restrict__ part) {
    __shared__ double sm[kBiBlock];
    const int64_t r0 = (int64_t)blockIdx.x * kBiChunk;
    const int64_t r1 = r0 + kBiChunk < N ? r0 + kBiChunk : N;
    double a = 0.0;
#pragma unroll 4
    for (int64_t r = r0 + threadIdx.x; r < r1; r += kBiBlock) a = a + (double)bi[r];
    a = bi_tree_sum(a, sm);
    if (threadIdx.x == 0) part[blockIdx.x] = a;
}

// one workgroup: the chunk values in the same order; init: total is written, else total = total + batch
__global__ __launch_bounds__(kBiBlock) void k_bi_total(const double* __restrict__ part, int64_t nchunk, int init,
                                                       double* __restrict__ total) {
    __shared__ double sm[kBiBlock];
    double a = 0.0;
    for (int64_t c = threadIdx.x; c < nchunk; c += kBiBlock) a = a + part[c];
    a = bi_tree_sum(a, sm);
    if (threadIdx.x == 0) *total = init ? a : *total + a;
}

static inline bool bi_rows_aligned16(const void* p, int64_t ld, int dt) {
    return ((uintptr_t)p & 15) == 0 && (ld * dtype_size(dt)) % 16 == 0;
}

}  // namespace llmc

using namespace llmc;

extern "C" size_t llmc_block_influence_ws_bytes(int64_t N) {
    if (N < 1 || N > (1ll << 31)) return 0;
    return (size_t)ceil_div64(N, kBiChunk) * sizeof(double);
}

extern "C" int llmc_block_influence(const void* X, const void* Y, int dt, int64_t N, int64_t d, int64_t ldx, int64_t ldy, int init,
                                    float* bi, double* total, void* ws, llmc_stream_t stream) {
    LLMC_REQUIRE(dtype_ok(dt), "block_influence: bad dtype");
    LLMC_REQUIRE(X && Y && bi && total && ws, "block_influence: null argument");
    LLMC_REQUIRE(N >= 1 && N <= (1ll << 31) && d >= 1, "block_influence: N in [1, 2^31] rows of d >= 1 elements");
    LLMC_REQUIRE(ldx >= d && ldy >= d, "block_influence: a row stride below d");
    if (d >= (1ll << 31)) {
        set_last_error_msg("block_influence: d >= 2^31 (the slot index of a row is a 32-bit integer)");
        return LLMC_ENOTSUP;
    }
    const int v = 16 / dtype_size(dt);
    const int nslot = (int)ceil_div64(d, v);
    const bool vecload = d % v == 0 && bi_rows_aligned16(X, ldx, dt) && bi_rows_aligned16(Y, ldy, dt);
    const int cap = opt(OPT_BLOCK_INFLUENCE_MAX_GRID) > 0 ? opt(OPT_BLOCK_INFLUENCE_MAX_GRID) : kBiMaxGrid;
    const dim3 grid(capped_grid(N, kBiWaves, cap));
    hipStream_t st = (hipStream_t)stream;
    DISPATCH_DT(dt, if (vecload) hipLaunchKernelGGL((k_block_influence<T, true>), grid, dim3(kBiBlock), 0, st, (const T*)X,
                                                    (const T*)Y, N, (int)d, nslot, ldx, ldy, bi);
                else hipLaunchKernelGGL((k_block_influence<T, false>), grid, dim3(kBiBlock), 0, st, (const T*)X, (const T*)Y, N,
                                        (int)d, nslot, ldx, ldy, bi));
    LLMC_LAUNCH_CHECK();
    const int64_t nchunk = ceil_div64(N, kBiChunk);
    hipLaunchKernelGGL(k_bi_chunk_sums, dim3((unsigned)nchunk), dim3(kBiBlock), 0, st, (const float*)bi, N, (double*)ws);
    LLMC_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_bi_total, dim3(1), dim3(kBiBlock), 0, st, (const double*)ws, nchunk, init, total);
    LLMC_LAUNCH_CHECK();
    return LLMC_OK;
}
