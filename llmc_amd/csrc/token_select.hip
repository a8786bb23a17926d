// token_select.hip — the two kernels of visual-token reduction by diversity (DivPrune, llmc/compression/token_reduction/divprune.py
// of the reference): the pairwise cosine distance of [N, d] token features, and the greedy max-min selection on an N x N matrix.
//
// llmc_cosine_dist: D = 1 - X X^T / (|x_i| |x_j|). The Gram matrix runs on the matrix pipe straight from X: both MFMA operands are
// rows of X, 8 consecutive k per lane (16 bytes), so there is no transposed and no normalised copy. Only the 128 x 128 tiles on or
// above the diagonal are multiplied, d is cut into slices so that tiles x slices fill the chip, and a second kernel sums a tile's
// slices in slice order, divides by the two norms it reads from the diagonal tiles' own sums and writes the tile and its mirror,
// one workgroup per 32 x 32 block so that a matrix of a few tiles still spreads over the chip.
//
// llmc_maxmin_select: one pass over the matrix for the step-0 statistic (the second smallest of every column), then ONE workgroup
// of 1024 threads runs all k steps: each thread keeps the running minimum of its columns in registers, a step reads one row of the
// matrix, and the argmax is a reduction over (value, index) keys. Values are only compared, so they are mapped once to unsigned
// keys whose integer order is the order the header states (NaN greatest, -0 = +0).
#include "common.h"
#include "mfma_common.h"

namespace llmc {

// ---------------------------------------------------------------------------------------------------------------------------------
// cosine distance

static constexpr int kCdTile = 128;                   // rows and columns of a workgroup's tile: 2 x 2 waves of 64 x 64 each
static constexpr int kCdBlock = 256;
static constexpr int kCdTileElems = kCdTile * kCdTile;
static constexpr int kCdTargetGroups = 512;           // tiles x slices aimed at: two workgroups per CU of a 256-CU chip
static constexpr int kCdMinSlice = 256;               // a slice is never thinner than this many k (the last one excepted)
static constexpr int64_t kCdMaxN = 46340;             // N * N < 2^31

// the k-slicing of a call: a function of (N, d) alone
struct CdPlan {
    int nt;          // tiles along one side
    int64_t tiles;   // tiles on or above the diagonal
    int ks;          // k per slice, a multiple of 32
    int S;           // slices
};
static inline CdPlan cd_plan(int64_t N, int64_t d) {
    CdPlan p;
    p.nt = (int)ceil_div64(N, kCdTile);
    p.tiles = (int64_t)p.nt * (p.nt + 1) / 2;
    int64_t want = ceil_div64(kCdTargetGroups, p.tiles);
    const int64_t cap = ceil_div64(d, kCdMinSlice);
    if (want > cap) want = cap;
    if (want < 1) want = 1;
    p.ks = (int)(ceil_div64(ceil_div64(d, want), 32) * 32);
    p.S = (int)ceil_div64(d, p.ks);
    return p;
}

// tile t of the upper triangle, rows first: (0,0) (0,1) ... (0,nt-1) (1,1) ...
__device__ __forceinline__ void cd_tile_of(int t, int nt, int& ti, int& tj) {
    ti = 0;
    while (t >= nt - ti) {
        t -= nt - ti;
        ++ti;
    }
    tj = ti + t;
}
__device__ __forceinline__ int64_t cd_tile_index(int ti, int tj, int nt) {
    return (int64_t)ti * nt - (int64_t)ti * (ti - 1) / 2 + (tj - ti);
}

// One MFMA step of a dtype: KSTEP consecutive k, lane half h = lane >> 5 holding KSTEP / 2 of them for its row.
//   16-bit: v_mfma_f32_32x32x16: lane (r, h) holds k0 + 8 h + 0..7 of row r, one instruction.
//   fp32:   four v_mfma_f32_32x32x2f32 on k0 + 4 h + e, e = 0..3 (instruction e sums k0 + e and k0 + 4 + e).
template <typename T> struct CdStep;
template <> struct CdStep<bf16_t> {
    static constexpr int KSTEP = 16, PER_LANE = 8;
    typedef s16x8 frag;
    static __device__ __forceinline__ f32x16 run(frag a, frag b, f32x16 c) { return Mfma<LLMC_BF16>::run(a, b, c); }
};
template <> struct CdStep<f16_t> {
    static constexpr int KSTEP = 16, PER_LANE = 8;
    typedef s16x8 frag;
    static __device__ __forceinline__ f32x16 run(frag a, frag b, f32x16 c) { return Mfma<LLMC_F16>::run(a, b, c); }
};
template <> struct CdStep<float> {
    static constexpr int KSTEP = 8, PER_LANE = 4;
    typedef f32x4 frag;
    static __device__ __forceinline__ f32x16 run(frag a, frag b, f32x16 c) {
#pragma unroll
        for (int e = 0; e < 4; ++e) c = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], b[e], c, 0, 0, 0);
        return c;
    }
};

// the PER_LANE elements of row `row` from k on: one 16-byte load where VEC allows it and the row has them all, else element loads
// with +0 behind the row's end; a row at or past N is all +0 (nothing is read)
template <typename T, bool VEC>
__device__ __forceinline__ typename CdStep<T>::frag cd_load(const T* __restrict__ X, int64_t ldx, int64_t N, int64_t row, int k, int d) {
    constexpr int P = CdStep<T>::PER_LANE;
    typename CdStep<T>::frag f = {};
    if (row >= N || k >= d) return f;
    const T* p = X + row * ldx + k;
    if (VEC && k + P <= d) {
        const uint4 raw = *reinterpret_cast<const uint4*>(p);
        __builtin_memcpy(&f, &raw, 16);
    } else {
        T e[P];
#pragma unroll
        for (int q = 0; q < P; ++q) e[q] = k + q < d ? p[q] : T{};
        __builtin_memcpy(&f, e, sizeof(f));
    }
    return f;
}

// grid (tiles, S): the fp32 partial Gram tile of k slice blockIdx.y, row-major [128][128], to part[(slice * tiles + tile)]
template <typename T, bool VEC>
__global__ __launch_bounds__(kCdBlock) void k_cd_gram(const T* __restrict__ X, int64_t N, int d, int64_t ldx, int nt, int ks,
                                                      float* __restrict__ part) {
    typedef CdStep<T> St;
    int ti, tj;
    cd_tile_of((int)blockIdx.x, nt, ti, tj);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int wr = wv >> 1, wc = wv & 1;
    const int64_t rowA = (int64_t)ti * kCdTile + 64 * wr + r;          // + 32 a
    const int64_t rowB = (int64_t)tj * kCdTile + 64 * wc + r;          // + 32 b
    const int kbeg = (int)blockIdx.y * ks;
    const int kend = kbeg + ks < d ? kbeg + ks : d;
    f32x16 acc[2][2] = {};
#pragma unroll 2
    for (int k0 = kbeg; k0 < kend; k0 += St::KSTEP) {
        const int k = k0 + St::PER_LANE * h;
        typename St::frag fa[2], fb[2];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            fa[a] = cd_load<T, VEC>(X, ldx, N, rowA + 32 * a, k, kend);
            fb[a] = cd_load<T, VEC>(X, ldx, N, rowB + 32 * a, k, kend);
        }
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) acc[a][b] = St::run(fa[a], fb[b], acc[a][b]);
    }
    float* out = part + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * kCdTileElems;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                const int row = 64 * wr + 32 * a + (g & 3) + 8 * (g >> 2) + 4 * h;      // the 32x32 accumulator's map
                out[row * kCdTile + 64 * wc + 32 * b + r] = acc[a][b][g];
            }
}

// element e of a tile: its S partial values added in slice order
__device__ __forceinline__ float cd_slice_sum(const float* __restrict__ part, int64_t tile, int64_t tiles, int S, int e) {
    const float* p = part + tile * kCdTileElems + e;
    float g = p[0];
    for (int s = 1; s < S; ++s) g = __fadd_rn(g, p[(int64_t)s * tiles * kCdTileElems]);
    return g;
}

// grid (tiles, 16): D over one 32 x 32 block of the tile (blockIdx.y = 4 * block row + block column) and over its mirror image
__global__ __launch_bounds__(kCdBlock) void k_cd_finish(const float* __restrict__ part, int64_t N, int nt, int S,
                                                        float* __restrict__ D) {
    __shared__ float norm_i[32], norm_j[32];
    __shared__ float sub[32][33];
    int ti, tj;
    cd_tile_of((int)blockIdx.x, nt, ti, tj);
    const int sr = (int)blockIdx.y >> 2, sc = (int)blockIdx.y & 3;
    const bool diag_tile = ti == tj;
    const int64_t i0 = (int64_t)ti * kCdTile + 32 * sr, j0 = (int64_t)tj * kCdTile + 32 * sc;
    if ((diag_tile && sr > sc) || i0 >= N || j0 >= N) return;          // the mirror of a block above; a block past the edge
    const bool diag_sub = diag_tile && sr == sc;
    const int64_t tiles = gridDim.x;
    const int t = threadIdx.x;
    if (t < 64) {
        // sqrt(G[i][i]) of the block's rows and columns, from the diagonal tiles' own sums
        const int q = t < 32 ? 32 * sr + t : 32 * sc + (t - 32);
        const int td = t < 32 ? ti : tj;
        const float g = cd_slice_sum(part, cd_tile_index(td, td, nt), tiles, S, q * kCdTile + q);
        (t < 32 ? norm_i : norm_j)[t & 31] = sqrtf(g);
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int e = t + kCdBlock * q, r = e >> 5, c = e & 31;
        // on the diagonal both halves take the element above it: the matrix is symmetric by construction
        const bool flip = diag_sub && r > c;
        const int rr = flip ? c : r, cc = flip ? r : c;
        const float g = cd_slice_sum(part, blockIdx.x, tiles, S, (32 * sr + rr) * kCdTile + 32 * sc + cc);
        const float v = __fsub_rn(1.0f, g / __fmul_rn(norm_i[rr], norm_j[cc]));
        sub[r][c] = v;
        const int64_t i = i0 + r, j = j0 + c;
        if (i < N && j < N) D[i * N + j] = v;
    }
    if (diag_sub) return;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int e = t + kCdBlock * q, r = e >> 5, c = e & 31;
        const int64_t j = j0 + r, i = i0 + c;
        if (i < N && j < N) D[j * N + i] = sub[c][r];
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// max-min selection

static constexpr int kMmBlock = 1024;
static constexpr int kMmPerThread = 16;
static constexpr int64_t kMmMaxN = (int64_t)kMmBlock * kMmPerThread;       // 16384: the running minimum stays in registers
static constexpr int kMmStatCols = 64, kMmStatRows = 16;                   // column statistic: 64 columns x 16 row groups a block
static constexpr uint32_t kMmNan = 0xffffffffu;

// the order of the header as an unsigned key: NaN above every number, -0 = +0, numbers in their own order
__device__ __forceinline__ uint32_t mm_key(float v) {
    if (__builtin_isnan(v)) return kMmNan;
    uint32_t b = __float_as_uint(v);
    if (b == 0x80000000u) b = 0;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
// torch.min: a NaN in either operand gives NaN
__device__ __forceinline__ uint32_t mm_min(uint32_t a, uint32_t b) {
    return (a == kMmNan || b == kMmNan) ? kMmNan : (a < b ? a : b);
}
// the two smallest keys (k1 <= k2) with one more
__device__ __forceinline__ void mm_two(uint32_t& k1, uint32_t& k2, uint32_t v) {
    if (v < k1) {
        k2 = k1;
        k1 = v;
    } else if (v < k2) {
        k2 = v;
    }
}

// grid ceil(N / 64): the key of the second smallest element of every column (NaN sorts last) to stat[N]
template <typename T>
__global__ __launch_bounds__(kMmStatCols * kMmStatRows) void k_mm_col_stat(const T* __restrict__ D, int64_t N, int64_t ldd,
                                                                           uint32_t* __restrict__ stat) {
    __shared__ uint32_t s1[kMmStatRows][kMmStatCols], s2[kMmStatRows][kMmStatCols];
    const int c = threadIdx.x & (kMmStatCols - 1), g = threadIdx.x / kMmStatCols;
    const int64_t col = (int64_t)blockIdx.x * kMmStatCols + c;
    // two NaN keys to start from: a column of N >= 2 elements replaces both unless it holds NaNs itself
    uint32_t k1 = kMmNan, k2 = kMmNan;
    if (col < N)
        for (int64_t row = g; row < N; row += kMmStatRows) mm_two(k1, k2, mm_key(to_f32<T>(D[row * ldd + col])));
    s1[g][c] = k1;
    s2[g][c] = k2;
    __syncthreads();
    if (g == 0 && col < N) {
        for (int q = 1; q < kMmStatRows; ++q) {
            mm_two(k1, k2, s1[q][c]);
            mm_two(k1, k2, s2[q][c]);
        }
        stat[col] = k2;
    }
}

// (key, index) of the greatest key, the lowest index among equal keys: the maximum of key << 32 | ~index
__device__ __forceinline__ uint64_t mm_wave_max(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)v, o, 64), hi = __shfl_xor((uint32_t)(v >> 32), o, 64);
        const uint64_t w = ((uint64_t)hi << 32) | lo;
        v = w > v ? w : v;
    }
    return v;
}

// one workgroup: all k steps. Thread t owns the columns t, t + 1024, ...
template <typename T>
__global__ __launch_bounds__(kMmBlock) void k_mm_select(const T* __restrict__ D, int N, int64_t ldd, int64_t k,
                                                        const uint32_t* __restrict__ stat, int64_t* __restrict__ sel) {
    __shared__ uint64_t wave_best[2][kMmBlock / 64];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    uint32_t score[kMmPerThread];
#pragma unroll
    for (int q = 0; q < kMmPerThread; ++q) {
        const int c = t + kMmBlock * q;
        score[q] = c < N ? stat[c] : 0u;
    }
    int chosen = 0;
    for (int64_t step = 0; step < k; ++step) {
        uint64_t best = 0;
        if (step > 0) {
            const T* row = D + (int64_t)chosen * ldd;
#pragma unroll
            for (int q = 0; q < kMmPerThread; ++q) {
                const int c = t + kMmBlock * q;
                if (c < N) {
                    const uint32_t v = mm_key(to_f32<T>(row[c]));
                    score[q] = step == 1 ? v : mm_min(score[q], v);          // step 1 starts again from the row of sel[0]
                }
            }
        }
#pragma unroll
        for (int q = 0; q < kMmPerThread; ++q) {
            const int c = t + kMmBlock * q;
            if (c < N) {
                const uint64_t key = ((uint64_t)score[q] << 32) | (uint32_t)~(uint32_t)c;
                best = key > best ? key : best;
            }
        }
        best = mm_wave_max(best);
        uint64_t* slot = wave_best[step & 1];          // two buffers: one barrier a step
        if (lane == 0) slot[wv] = best;
        __syncthreads();
        best = slot[lane & (kMmBlock / 64 - 1)];
        best = mm_wave_max(best);
        chosen = (int)~(uint32_t)best;
        if (t == 0) sel[step] = chosen;
    }
}

static inline bool cd_rows_aligned16(const void* p, int64_t ld, int dt) {
    return ((uintptr_t)p & 15) == 0 && (ld * dtype_size(dt)) % 16 == 0;
}

}  // namespace llmc

using namespace llmc;

extern "C" size_t llmc_cosine_dist_ws_bytes(int64_t N, int64_t d) {
    if (N < 1 || N > kCdMaxN || d < 1 || d > (1ll << 31) - 64) return 0;
    const CdPlan p = cd_plan(N, d);
    return (size_t)p.S * (size_t)p.tiles * kCdTileElems * sizeof(float);
}

extern "C" int llmc_cosine_dist(const void* X, int dt, int64_t N, int64_t d, int64_t ldx, float* D, void* ws,
                                llmc_stream_t stream) {
    LLMC_REQUIRE(dtype_ok(dt), "cosine_dist: bad dtype");
    LLMC_REQUIRE(X && D && ws, "cosine_dist: null argument");
    LLMC_REQUIRE(N >= 1 && d >= 1, "cosine_dist: N >= 1 rows of d >= 1 elements");
    LLMC_REQUIRE(ldx >= d, "cosine_dist: a row stride below d");
    if (N > kCdMaxN || d > (1ll << 31) - 64) {
        set_last_error_msg("cosine_dist: N > 46340 or d > 2^31 - 64 (an element index of D or of a row leaves 32 bits)");
        return LLMC_ENOTSUP;
    }
    const CdPlan p = cd_plan(N, d);
    const bool vec = cd_rows_aligned16(X, ldx, dt);
    const dim3 grid((unsigned)p.tiles, (unsigned)p.S);
    hipStream_t st = (hipStream_t)stream;
    DISPATCH_DT(dt, if (vec) hipLaunchKernelGGL((k_cd_gram<T, true>), grid, dim3(kCdBlock), 0, st, (const T*)X, N, (int)d, ldx, p.nt,
                                                p.ks, (float*)ws);
                else hipLaunchKernelGGL((k_cd_gram<T, false>), grid, dim3(kCdBlock), 0, st, (const T*)X, N, (int)d, ldx, p.nt, p.ks,
                                        (float*)ws));
    LLMC_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_cd_finish, dim3((unsigned)p.tiles, 16), dim3(kCdBlock), 0, st, (const float*)ws, N, p.nt, p.S, D);
    LLMC_LAUNCH_CHECK();
    return LLMC_OK;
}

extern "C" int llmc_maxmin_select_max_n(void) { return (int)kMmMaxN; }

extern "C" size_t llmc_maxmin_select_ws_bytes(int64_t N) {
    if (N < 2 || N > kMmMaxN) return 0;
    return (size_t)N * sizeof(uint32_t);
}

extern "C" int llmc_maxmin_select(const void* D, int dt, int64_t N, int64_t ldd, int64_t k, int64_t* sel, void* ws,
                                  llmc_stream_t stream) {
    LLMC_REQUIRE(dtype_ok(dt), "maxmin_select: bad dtype");
    LLMC_REQUIRE(N >= 2, "maxmin_select: N < 2 (the second smallest of a column needs two rows)");
    LLMC_REQUIRE(k >= 0, "maxmin_select: k < 0");
    LLMC_REQUIRE(ldd >= N, "maxmin_select: a row stride below N");
    if (k == 0) return LLMC_OK;
    LLMC_REQUIRE(D && sel && ws, "maxmin_select: null argument");
    if (N > kMmMaxN) {
        set_last_error_msg("maxmin_select: N > 16384 (the running minimum of 16 columns per thread of one workgroup)");
        return LLMC_ENOTSUP;
    }
    hipStream_t st = (hipStream_t)stream;
    const dim3 sgrid((unsigned)ceil_div64(N, kMmStatCols));
    DISPATCH_DT(dt, hipLaunchKernelGGL((k_mm_col_stat<T>), sgrid, dim3(kMmStatCols * kMmStatRows), 0, st, (const T*)D, N, ldd,
                                       (uint32_t*)ws));
    LLMC_LAUNCH_CHECK();
    DISPATCH_DT(dt, hipLaunchKernelGGL((k_mm_select<T>), dim3(1), dim3(kMmBlock), 0, st, (const T*)D, (int)N, ldd, k,
                                       (const uint32_t*)ws, sel));
    LLMC_LAUNCH_CHECK();
    return LLMC_OK;
}
