// col_reduce.h — the two-stage reduction of [N, K] over its rows into per-column statistics, stated once: no atomics, and an order
// of joins that is a function of the geometry alone. Users: k_col_sqsum_partial / k_col_sqsum_fold (prune.hip, one sum of squares
// whose order include/llmc_hip.h promises) and k_col_stats_partial / k_col_stats_fold (smooth_osplus.hip, three NaN-propagating
// extremes). What is accumulated is the caller's policy P:
//   P::NS                     statistics per column (part and the running buffers are [NS][K])
//   P::identity(s)            the value statistic s starts from
//   P::step(float (&a)[NS], f)  one element folded into a column's statistics
//   P::join(s, a, b)          two partial values of statistic s; stage 1 and stage 2 call it with the earlier one first
// The caller also keeps what decides the geometry: the rows worth a chunk, the block cap and the vector width the chunk count
// is computed for.
#pragma once
#include "common.h"
#include "vec16.h"

namespace llmc {

// stage 1: grid (column blocks, row chunks), NT threads; a wave reads 64 consecutive vectors of one row; wave w of a workgroup owns
// the rows r0 + w, r0 + w + NT / 64, ... of the chunk and folds them in that order from the identity; waves 1.. hand their values
// over in LDS and wave 0 joins them in wave order onto its own and writes part[chunk][s][K].
template <typename P, typename T, int VEC, int NT>
__device__ __forceinline__ void col_reduce_partial(const T* __restrict__ X, int64_t N, int64_t K, int64_t rows_per_chunk,
                                                   float* __restrict__ part) {
    constexpr int NS = P::NS, NW = NT / 64;
    __shared__ float sm[NS][NW - 1][64 * VEC];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t c = ((int64_t)blockIdx.x * 64 + lane) * VEC;
    const int64_t r0 = (int64_t)blockIdx.y * rows_per_chunk;
    const int64_t r1 = r0 + rows_per_chunk < N ? r0 + rows_per_chunk : N;
    float acc[VEC][NS];
#pragma unroll
    for (int i = 0; i < VEC; ++i)
#pragma unroll
        for (int s = 0; s < NS; ++s) acc[i][s] = P::identity(s);
    if (c < K) {
#pragma unroll 4
        for (int64_t r = r0 + wv; r < r1; r += NW) {
            const Vec<T, VEC> v = load_vec<T, VEC>(X + r * K + c);
#pragma unroll
            for (int i = 0; i < VEC; ++i) P::step(acc[i], to_f32<T>(v.v[i]));
        }
    }
    if (wv > 0) {
#pragma unroll
        for (int i = 0; i < VEC; ++i)
#pragma unroll
            for (int s = 0; s < NS; ++s) sm[s][wv - 1][lane * VEC + i] = acc[i][s];
    }
    __syncthreads();
    if (wv == 0 && c < K) {
        float* p = part + (int64_t)blockIdx.y * NS * K;
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                float a = acc[i][s];
#pragma unroll
                for (int w = 0; w < NW - 1; ++w) a = P::join(s, a, sm[s][w][lane * VEC + i]);
                p[s * K + c + i] = a;
            }
        }
    }
}

// stage 2, one thread per column k < K: the chunks of the column joined in chunk order from the first one; init: the running
// buffers are written, not read; else run = join(run, batch). a: what was written.
template <typename P>
__device__ __forceinline__ void col_reduce_fold(const float* __restrict__ part, int64_t nchunk, int64_t K, int64_t k, int init,
                                                float* __restrict__ run, float (&a)[P::NS]) {
    constexpr int NS = P::NS;
#pragma unroll
    for (int s = 0; s < NS; ++s) a[s] = part[s * K + k];
    for (int64_t ch = 1; ch < nchunk; ++ch) {
        const float* p = part + ch * NS * K;
#pragma unroll
        for (int s = 0; s < NS; ++s) a[s] = P::join(s, a[s], p[s * K + k]);
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        if (!init) a[s] = P::join(s, run[s * K + k], a[s]);
        run[s * K + k] = a[s];
    }
}

// row chunks of stage 1: one per `rows` rows, as many as keep the grid at `max_blocks` workgroups when a column block is 64
// vectors of v elements; at least one
static inline int64_t col_chunks(int64_t N, int64_t K, int v, int rows, int max_blocks) {
    int64_t cap = max_blocks / ceil_div64(K, 64 * (int64_t)v);
    if (cap < 1) cap = 1;
    int64_t n = ceil_div64(N, rows);
    if (n > cap) n = cap;
    return n < 1 ? 1 : n;
}

// elements per load of stage 1: the 16-byte vector of dt where every row of X starts on one, else 1
static inline int col_vec(const void* X, int dt, int64_t K) {
    const int V = 16 / dtype_size(dt);
    return K % V == 0 && ((uintptr_t)X & 15) == 0 ? V : 1;
}

// stage 1's launch: launch(T{}, std::integral_constant<int, VEC>{}, grid, rows per chunk) is called once, with the storage type of
// dt and VEC = v as a constant (v from col_vec), for the caller's own __global__ kernel
template <typename F> static inline void col_reduce_launch(int dt, int v, int64_t N, int64_t K, int64_t nchunk, F&& launch) {
    const dim3 grid((unsigned)ceil_div64(K, 64 * (int64_t)v), (unsigned)nchunk);
    const int64_t rpc = ceil_div64(N, nchunk);
    DISPATCH_DT(dt, if (v > 1) launch(T{}, std::integral_constant<int, 16 / (int)sizeof(T)>{}, grid, rpc);
                else launch(T{}, std::integral_constant<int, 1>{}, grid, rpc));
}

}  // namespace llmc
