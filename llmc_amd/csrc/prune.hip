// prune.hip — the device side of weight sparsification (llmc/compression/sparsification/wanda.py, magnitude.py).
//   llmc_col_sqsum         per-column sum of squares of [N, K], folded into a running fp32 [K] buffer (Wanda's scaler_row,
//                          wanda.py:27-31); two stages, no float atomics, a fixed order of summation.
//   llmc_prune_rows        in every group of m consecutive columns of a row the n_prune elements of smallest
//                          |w| * sqrt(scaler_row) become +0 (wanda.py:46-56 for m == K; n:m for m in {2, 4, 8, 16}). A row waits in
//                          registers between its load and its store; the k-th order statistic comes from a most-significant-
//                          digit radix select over LDS histograms, ties by a prefix count in column order.
//   llmc_magnitude_prune   global |w| threshold of rank kth and w[|w| <= thresh] = 0 (magnitude.py:26-31): a 32768-bin histogram
//                          of the sign-cleared bit patterns, a one-workgroup scan (radix_select.h), a masking pass.
// All data passes are HBM-bound; DESIGN.md holds the byte counts they are measured against.
#include "col_reduce.h"
#include "common.h"
#include "radix_select.h"
#include "vec16.h"

namespace llmc {
namespace {

// ================================================================================================================================
// column sums of squares
// ================================================================================================================================
constexpr int SQ_B = 256;             // threads per workgroup
constexpr int SQ_ROWS = 64;           // fewest rows worth a chunk of their own
constexpr int SQ_MAX_BLOCKS = 2048;

// The number of row chunks depends on (N, K, dt) only, never on the alignment of X (the dtype's vector width, whatever the loads):
// with col_reduce.h's walk the order of summation is a function of the shape, the one include/llmc_hip.h promises.
inline int64_t sq_chunks(int64_t N, int64_t K, int dt) { return col_chunks(N, K, 16 / dtype_size(dt), SQ_ROWS, SQ_MAX_BLOCKS); }

struct SqSum {
    static constexpr int NS = 1;
    static __device__ __forceinline__ float identity(int) { return 0.0f; }
    static __device__ __forceinline__ void step(float (&a)[1], float f) { a[0] = a[0] + f * f; }          // two roundings: the build turns contraction off
    static __device__ __forceinline__ float join(int, float a, float b) { return a + b; }
};

template <typename T, int VEC>
__global__ __launch_bounds__(SQ_B) void k_col_sqsum_partial(const T* __restrict__ X, int64_t N, int64_t K, int64_t rows_per_chunk,
                                                            float* __restrict__ part) {
    col_reduce_partial<SqSum, T, VEC, SQ_B>(X, N, K, rows_per_chunk, part);
}

__global__ __launch_bounds__(SQ_B) void k_col_sqsum_fold(const float* __restrict__ part, int64_t nchunk, int64_t K, int init,
                                                         float* __restrict__ acc, float* __restrict__ out, float nsamples) {
    const int64_t k = (int64_t)blockIdx.x * SQ_B + threadIdx.x;
    if (k >= K) return;
    float a[1];
    col_reduce_fold<SqSum>(part, nchunk, K, k, init, acc, a);
    if (out) out[k] = a[0] / nsamples;
}

// ================================================================================================================================
// row pruning
// ================================================================================================================================
// The sort key of an element: the bit pattern of its metric fp32(|w|) * sqrtf(scaler_row[k]). The metric is never negative, so
// its bits order like an unsigned integer; -0 (from a -0 scaler) is +0; NaN, whatever its sign or payload, takes the largest
// 31-bit key, after +inf, as torch.sort orders it.
__device__ __forceinline__ uint32_t metric_key(float w, float sq, bool has_s) {
    float m = fabsf(w);
    if (has_s) m = m * sq;
    const uint32_t b = __float_as_uint(m);
    return (m != m) ? 0x7FFFFFFFu : (b & 0x7FFFFFFFu);
}

constexpr int PR_BINS = 2048;                              // 11-bit digits
constexpr int PR_HIST = PR_BINS + PR_BINS / 32 * 4;        // every 32 bins are followed by 4 words of padding: the scan's lanes, which own
                                                           // 32 consecutive bins each, then start 36 words apart and read their 16-byte
                                                           // groups from distinct banks
__device__ __forceinline__ uint32_t hist_slot(uint32_t bin) { return bin + ((bin >> 5) << 2); }

enum PrunePath : int { PATH_WAVE = 0, PATH_BLOCK256, PATH_BLOCK1024, PATH_SCALAR, PATH_NM, PATH_NM_SCALAR, PATH_COUNT };

// One row per TPR threads (a wave, 256 threads or 1024 threads); a workgroup of max(TPR, 256) threads holds 256 / TPR rows
// when TPR == 64. Thread t of a row owns the vectors t, t + TPR, ... (NV of them, VEC elements each; VEC == 1 is the
// one-element-per-lane form for operands that do not allow 16-byte vectors).
template <typename T, int VEC, int NV, int TPR>
__global__ __launch_bounds__(TPR < 256 ? 256 : TPR) void k_prune_rows(T* __restrict__ W, int64_t R, int K, int64_t ld,
                                                                      const float* __restrict__ srow, int s_vec, int n_prune,
                                                                      uint8_t* __restrict__ mask, int mask_vec) {
    constexpr int NT = TPR < 256 ? 256 : TPR;
    constexpr int RPW = NT / TPR;          // rows per workgroup
    constexpr int NW = TPR / 64;           // waves per row
    __shared__ __align__(16) uint32_t s_hist[RPW][PR_HIST];          // read back 16 bytes at a time
    __shared__ uint32_t s_tot[RPW][NV * NW];
    __shared__ uint32_t s_sel[RPW][4];
    const int g = threadIdx.x / TPR, t = threadIdx.x % TPR, lane = threadIdx.x & 63, wv = t >> 6;
    const int64_t row = (int64_t)blockIdx.x * RPW + g;
    const bool active = row < R;
    const int nvec = K / VEC;
    const bool has_s = srow != nullptr;
    T* wrow = W + (active ? row : 0) * ld;

    Vec<T, VEC> raw[VEC > 1 ? NV : 1];
    uint32_t key[NV][VEC];
#pragma unroll
    for (int ii = 0; ii < NV; ++ii) {
        const int i = VEC > 1 ? ii : 0;          // raw slot
        const int v = ii * TPR + t;
        if (active && v < nvec) {
            float sq[VEC];
            if constexpr (VEC > 1) {
                raw[i] = load_vec<T, VEC>(wrow + (int64_t)v * VEC);
                if (has_s) {
                    if (s_vec) {          // fp32 scaler entries, four per load: written out (with load_vec the streams moved)
#pragma unroll
                        for (int j = 0; j < VEC; j += 4) {
                            const float4 s4 = *reinterpret_cast<const float4*>(srow + (int64_t)v * VEC + j);
                            sq[j] = s4.x, sq[j + 1] = s4.y, sq[j + 2] = s4.z, sq[j + 3] = s4.w;
                        }
                    } else {
#pragma unroll
                        for (int j = 0; j < VEC; ++j) sq[j] = srow[(int64_t)v * VEC + j];
                    }
                }
            } else {
                raw[i].v[0] = wrow[v];          // the one-element form keeps the key only: it stores nothing but the zeros
                if (has_s) sq[0] = srow[v];
            }
#pragma unroll
            for (int j = 0; j < VEC; ++j) key[ii][j] = metric_key(to_f32<T>(raw[i].v[j]), has_s ? sqrtf(sq[j]) : 1.0f, has_s);
        } else {
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                raw[i].v[j] = zero_of<T>();
                key[ii][j] = 0xFFFFFFFFu;
            }
        }
    }

    // ---- radix select: the key of 0-based rank n_prune - 1, and how many keys lie below it ---------------------------------
    // Keys have 31 bits; the digits are bits 30..20, 19..9 and 8..0. The first one holds the exponent and three mantissa bits, so
    // the few exponents a row's metrics share are spread over eight bins each.
    uint32_t prefix = 0, below = 0, cnt_eq = 0;
    uint32_t rr = (uint32_t)(n_prune - 1);          // rank still to find among the keys that share the prefix
    if (t < 4) s_sel[g][t] = 0;
#pragma unroll 1
    for (int pass = 0; pass < 3; ++pass) {
        const int shift = pass == 0 ? 20 : (pass == 1 ? 9 : 0);
        const int above = pass == 1 ? 20 : 9;          // passes 1, 2: the bits above the digit must equal the prefix
        const uint32_t dmask = pass == 2 ? 511u : 2047u;
        for (int i = t; i < PR_HIST; i += TPR) s_hist[g][i] = 0;
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const bool valid = active && i * TPR + t < nvec;
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                const uint32_t k = key[i][j];
                const bool in = pass == 0 || ((k ^ prefix) >> above) == 0;
                if (valid && in) atomicAdd(&s_hist[g][hist_slot((k >> shift) & dmask)], 1u);
            }
        }
        __syncthreads();
        if (wv == 0) {
            // lane l of the row's first wave owns bins 32 l .. 32 l + 31: eight 16-byte groups of LDS counters (no vector of
            // elements: with load_vec here the one-element forms compiled to another instruction stream)
            const uint4* p = reinterpret_cast<const uint4*>(&s_hist[g][hist_slot(32u * lane)]);
            uint32_t s8[8], sum = 0;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const uint4 a = p[q];
                s8[q] = a.x + a.y + a.z + a.w;
                sum += s8[q];
            }
            uint32_t incl = sum;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t n = __shfl_up(incl, o, 64);
                if (lane >= o) incl += n;
            }
            uint32_t excl = incl - sum;
            if (excl <= rr && rr < incl) {
                int q = 0;
                uint32_t sq = s8[0];
#pragma unroll
                for (int b = 1; b < 8; ++b) {
                    if (q == b - 1 && excl + sq <= rr) {
                        excl += sq;
                        q = b;
                        sq = s8[b];
                    }
                }
                const uint4 a = p[q];
                const uint32_t c[4] = {a.x, a.y, a.z, a.w};
                int d = 0;
                uint32_t cd = c[0];
#pragma unroll
                for (int b = 1; b < 4; ++b) {
                    if (d == b - 1 && excl + cd <= rr) {
                        excl += cd;
                        d = b;
                        cd = c[b];
                    }
                }
                s_sel[g][0] = (uint32_t)(32 * lane + 4 * q + d);
                s_sel[g][1] = excl;
                s_sel[g][2] = cd;
            }
        }
        __syncthreads();
        prefix |= s_sel[g][0] << shift;
        below += s_sel[g][1];
        rr -= s_sel[g][1];
        cnt_eq = s_sel[g][2];
    }
    const uint32_t thr = prefix;
    uint32_t need_eq = (uint32_t)n_prune - below;       // of the keys equal to the threshold, the first need_eq by column go

    // ---- ties: the position of each thread's equal keys among the row's equal keys, in column order ------------------------
    // (the one-element form keeps no ranks: it recomputes a slot's ballot when it writes the slot)
    uint32_t eq_rank[VEC > 1 ? NV : 1];
#pragma unroll
    for (int i = 0; i < (VEC > 1 ? NV : 1); ++i) eq_rank[i] = 0;
    const bool ties = need_eq < cnt_eq;                  // uniform over the row
    if (ties) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const bool valid = active && i * TPR + t < nvec;
            if constexpr (VEC > 1) {
                uint32_t n = 0;
#pragma unroll
                for (int j = 0; j < VEC; ++j) n += (valid && key[i][j] == thr) ? 1u : 0u;
                uint32_t incl = n;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const uint32_t m = __shfl_up(incl, o, 64);
                    if (lane >= o) incl += m;
                }
                eq_rank[i] = incl - n;
                if (lane == 63) s_tot[g][i * NW + wv] = incl;
            } else {
                const unsigned long long b = __ballot(valid && key[i][0] == thr);
                if (lane == 0) s_tot[g][i * NW + wv] = (uint32_t)__popcll(b);
            }
        }
    } else {
        need_eq = 0xFFFFFFFFu;
    }
    __syncthreads();
    if constexpr (VEC > 1) {
        if (ties) {
            uint32_t run = 0;
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                for (int w = 0; w < NW; ++w) {
                    if (w == wv) eq_rank[i] += run;
                    run += s_tot[g][i * NW + w];
                }
            }
        }
    }

    // ---- write the row -------------------------------------------------------------------------------------------------------
    uint32_t tie_run = 0;          // one-element form: the equal keys of the slots already written
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int v = i * TPR + t;
        uint32_t e = 0;
        if constexpr (VEC > 1) {
            e = eq_rank[i];
        } else if (ties) {          // uniform over the wave: every lane takes part in the ballot
            const unsigned long long b = __ballot(active && v < nvec && key[i][0] == thr);
            e = tie_run + (uint32_t)__popcll(b & ((1ull << lane) - 1));
            for (int w = 0; w < NW; ++w) {
                if (w < wv) e += s_tot[g][i * NW + w];
                tie_run += s_tot[g][i * NW + w];
            }
        }
        if (!(active && v < nvec)) continue;
        Vec<uint8_t, VEC> mk;
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const uint32_t k = key[i][j];
            bool cut = k < thr;
            if (k == thr) {
                cut = e < need_eq;
                ++e;
            }
            if constexpr (VEC > 1) {
                if (cut) raw[i].v[j] = zero_of<T>();
            }
            mk.v[j] = cut ? 1 : 0;
        }
        if constexpr (VEC > 1) {
            store_vec<T, VEC>(wrow + (int64_t)v * VEC, raw[i]);
        } else {
            if (mk.v[0]) wrow[v] = zero_of<T>();
        }
        if (mask) store_bytes<VEC == 8 ? 8 : VEC>(mask + row * K + (int64_t)v * VEC, mk, mask_vec);          // one store of the vector's mask
    }
}

// n:m. A thread owns E consecutive columns of one row, whole groups of M: E = max(M, elements of a 16-byte vector) in the vector
// form, E = M in the one-element-per-lane form. The rank of an element in its group is the count of the elements that sort
// before it (smaller key, or the same key at a lower column); no LDS.
// Its 16-byte accesses and its mask store stay written out here: with vec16.h's Vec / load_vec / store_vec / store_bytes every
// instantiation compiled to another instruction stream (<float, 16, true> 68 -> 81 VGPRs) and two rows measured slower than the
// parent commit's, above its spread (bf16 4096 x 4096 2:4 with a mask +1.9 %, fp32 8:16 +1.1 %; profiles/stream_refactor.txt).
template <typename T, int M, bool VECM>
__global__ __launch_bounds__(256) void k_prune_nm(T* __restrict__ W, int64_t R, int64_t K, int64_t ld, const float* __restrict__ srow,
                                                  int s_vec, int n_prune, uint8_t* __restrict__ mask, int mask_vec) {
    constexpr int VN = 16 / (int)sizeof(T);
    constexpr int E = VECM ? (M > VN ? M : VN) : M;
    const int64_t cpr = K / E;
    const int64_t total = R * cpr;
    const bool has_s = srow != nullptr;
    for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < total; c += (int64_t)gridDim.x * 256) {
        const int64_t r = c / cpr, k0 = (c - r * cpr) * E;
        T* wp = W + r * ld + k0;
        T raw[E];
        float sq[E];
        uint32_t key[E];
        if constexpr (VECM) {
#pragma unroll
            for (int j = 0; j < E; j += VN) {
                const uint4 q = *reinterpret_cast<const uint4*>(wp + j);
                __builtin_memcpy(&raw[j], &q, 16);
            }
        } else {
#pragma unroll
            for (int j = 0; j < E; ++j) raw[j] = wp[j];
        }
        if (has_s) {
            if (VECM && s_vec) {
#pragma unroll
                for (int j = 0; j < E; j += 4) {
                    const float4 s4 = *reinterpret_cast<const float4*>(srow + k0 + j);
                    sq[j] = s4.x, sq[j + 1] = s4.y, sq[j + 2] = s4.z, sq[j + 3] = s4.w;
                }
            } else {
#pragma unroll
                for (int j = 0; j < E; ++j) sq[j] = srow[k0 + j];
            }
        }
#pragma unroll
        for (int j = 0; j < E; ++j) key[j] = metric_key(to_f32<T>(raw[j]), has_s ? sqrtf(sq[j]) : 1.0f, has_s);
        uint8_t mk[E];
#pragma unroll
        for (int g0 = 0; g0 < E; g0 += M) {
#pragma unroll
            for (int i = 0; i < M; ++i) {
                int rank = 0;
#pragma unroll
                for (int j = 0; j < M; ++j) {
                    if (j == i) continue;
                    const uint32_t a = key[g0 + j], b = key[g0 + i];
                    rank += (a < b || (a == b && j < i)) ? 1 : 0;
                }
                mk[g0 + i] = rank < n_prune ? 1 : 0;
            }
        }
#pragma unroll
        for (int j = 0; j < E; ++j)
            if (mk[j]) raw[j] = zero_of<T>();
        if constexpr (VECM) {
#pragma unroll
            for (int j = 0; j < E; j += VN) {
                uint4 q;
                __builtin_memcpy(&q, &raw[j], 16);
                *reinterpret_cast<uint4*>(wp + j) = q;
            }
        } else {
#pragma unroll
            for (int j = 0; j < E; ++j) wp[j] = raw[j];
        }
        if (mask) {
            uint8_t* mp = mask + r * K + k0;
            if (VECM && mask_vec) {
#pragma unroll
                for (int j = 0; j < E; j += 4) {
                    uint32_t q;
                    __builtin_memcpy(&q, &mk[j], 4);
                    *reinterpret_cast<uint32_t*>(mp + j) = q;
                }
            } else {
#pragma unroll
                for (int j = 0; j < E; ++j) mp[j] = mk[j];
            }
        }
    }
}

constexpr int64_t PR_MAX_K = 32768;          // the widest row the register tiers of k_prune_rows hold (1024 threads x 32 elements)

inline bool vec_ok(int dt, int64_t K, int64_t ld, const void* W) {
    const int V = 16 / dtype_size(dt);
    return K % V == 0 && ld % V == 0 && ((uintptr_t)W & 15) == 0;
}

// the launch path of a checked call, or LLMC_ENOTSUP for a row too long to stay resident
inline int prune_path(int dt, int64_t K, int64_t ld, int64_t m, const void* W) {
    const bool vec = vec_ok(dt, K, ld, W);
    if (m != K) return vec ? PATH_NM : PATH_NM_SCALAR;
    if (K > PR_MAX_K) return LLMC_ENOTSUP;
    if (!vec) return PATH_SCALAR;
    const int64_t nvec = K / (16 / dtype_size(dt));
    if (nvec <= 64 * 4) return PATH_WAVE;
    if (nvec <= 256 * 4) return PATH_BLOCK256;
    return PATH_BLOCK1024;
}

inline int prune_check(int dt, int64_t R, int64_t K, int64_t ld, int64_t m, const void* W) {
    LLMC_REQUIRE(dtype_ok(dt), "prune_rows: bad dtype");
    LLMC_REQUIRE(W != nullptr, "prune_rows: null W");
    LLMC_REQUIRE(R > 0 && K > 0 && R < (1ll << 31) && K < (1ll << 31), "prune_rows: R and K in [1, 2^31)");
    LLMC_REQUIRE(ld >= K, "prune_rows: ld < K");
    if (m != K && m != 2 && m != 4 && m != 8 && m != 16) {
        set_last_error_msg("prune_rows: m is K (per row) or 2, 4, 8, 16 (n:m)");
        return LLMC_ENOTSUP;
    }
    LLMC_REQUIRE(K % m == 0, "prune_rows: m does not divide K");
    return LLMC_OK;
}

template <typename T, int VEC, int NV, int TPR>
void launch_rows(void* W, int64_t R, int64_t K, int64_t ld, const float* srow, int n_prune, uint8_t* mask, hipStream_t st) {
    constexpr int RPW = TPR < 256 ? 256 / TPR : 1;
    const int s_vec = ((uintptr_t)srow & 15) == 0, mask_vec = ((uintptr_t)mask & 7) == 0;
    hipLaunchKernelGGL((k_prune_rows<T, VEC, NV, TPR>), dim3((unsigned)ceil_div64(R, RPW)), dim3(TPR < 256 ? 256 : TPR), 0, st, (T*)W, R,
                       (int)K, ld, srow, s_vec, n_prune, mask, mask_vec);
}

template <typename T>
void launch_rows_dt(int path, void* W, int64_t R, int64_t K, int64_t ld, const float* srow, int n_prune, uint8_t* mask,
                    hipStream_t st) {
    constexpr int V = 16 / (int)sizeof(T);
    const int64_t nvec = K / V;
    switch (path) {
        case PATH_WAVE:
            if (nvec <= 64) launch_rows<T, V, 1, 64>(W, R, K, ld, srow, n_prune, mask, st);
            else launch_rows<T, V, 4, 64>(W, R, K, ld, srow, n_prune, mask, st);
            break;
        case PATH_BLOCK256:
            if (nvec <= 512) launch_rows<T, V, 2, 256>(W, R, K, ld, srow, n_prune, mask, st);
            else launch_rows<T, V, 4, 256>(W, R, K, ld, srow, n_prune, mask, st);
            break;
        case PATH_BLOCK1024:
            if (nvec <= 2048) launch_rows<T, V, 2, 1024>(W, R, K, ld, srow, n_prune, mask, st);
            else if (nvec <= 4096) launch_rows<T, V, 4, 1024>(W, R, K, ld, srow, n_prune, mask, st);
            else if constexpr (sizeof(T) == 4) launch_rows<T, V, 8, 1024>(W, R, K, ld, srow, n_prune, mask, st);          // fp32 alone has rows of more than 4096 vectors
            break;
        default:          // PATH_SCALAR
            if (K <= 512) launch_rows<T, 1, 8, 64>(W, R, K, ld, srow, n_prune, mask, st);
            else if (K <= 4096) launch_rows<T, 1, 16, 256>(W, R, K, ld, srow, n_prune, mask, st);
            else launch_rows<T, 1, 32, 1024>(W, R, K, ld, srow, n_prune, mask, st);
            break;
    }
}

template <typename T, bool VECM>
void launch_nm(void* W, int64_t R, int64_t K, int64_t ld, int m, const float* srow, int n_prune, uint8_t* mask, hipStream_t st) {
    constexpr int VN = 16 / (int)sizeof(T);
    const int E = VECM ? (m > VN ? m : VN) : m;
    const int s_vec = ((uintptr_t)srow & 15) == 0, mask_vec = ((uintptr_t)mask & 3) == 0;
    const dim3 grid((unsigned)capped_grid(R * (K / E), 256, (int64_t)device_cu_count() * 32));
#define LLMC_NM(M_) \
    hipLaunchKernelGGL((k_prune_nm<T, M_, VECM>), grid, dim3(256), 0, st, (T*)W, R, K, ld, srow, s_vec, n_prune, mask, mask_vec)
    switch (m) {
        case 2: LLMC_NM(2); break;
        case 4: LLMC_NM(4); break;
        case 8: LLMC_NM(8); break;
        default: LLMC_NM(16); break;
    }
#undef LLMC_NM
}

// ================================================================================================================================
// global magnitude pruning
// ================================================================================================================================
// The select and its workspace are radix_select.h's; the workspace is fresh memory, zeroed here.
__global__ __launch_bounds__(RS_T) void k_mag_zero(uint32_t* __restrict__ ws) {
    for (int i = blockIdx.x * RS_T + threadIdx.x; i < RS_WORDS; i += gridDim.x * RS_T) ws[i] = 0;
}

// the select key: the sign-cleared bit pattern
template <typename T> __device__ __forceinline__ uint32_t abs_bits(T v);
template <> __device__ __forceinline__ uint32_t abs_bits<f16_t>(f16_t v) { return v.u & 0x7FFFu; }
template <> __device__ __forceinline__ uint32_t abs_bits<bf16_t>(bf16_t v) { return v.u & 0x7FFFu; }
template <> __device__ __forceinline__ uint32_t abs_bits<float>(float v) { return __float_as_uint(v) & 0x7FFFFFFFu; }

// element walk shared by the three passes: f(r, k, T&) -> true when the element was changed. VEC == 1: one element per lane.
template <typename T, int VEC, bool WRITE, typename F>
__device__ __forceinline__ void mag_walk(T* __restrict__ W, int64_t R, int64_t K, int64_t ld, uint8_t* __restrict__ mask, int mask_vec,
                                         F&& f) {
    const int64_t vpr = K / VEC, total = R * vpr;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / vpr, k0 = (i - r * vpr) * VEC;
        T* p = W + r * ld + k0;
        Vec<T, VEC> v = load_vec<T, VEC>(p);
        Vec<uint8_t, VEC> mk;
#pragma unroll
        for (int j = 0; j < VEC; ++j) mk.v[j] = f(v.v[j]) ? 1 : 0;
        if constexpr (WRITE) {
            store_vec<T, VEC>(p, v);
            if (mask) store_bytes<(VEC > 1 ? 4 : 1)>(mask + r * K + k0, mk, mask_vec);
        }
    }
}

// first digit (the whole key of a 16-bit dtype)
template <typename T, int VEC>
__global__ __launch_bounds__(RS_T) void k_mag_hist(T* __restrict__ W, int64_t R, int64_t K, int64_t ld, uint32_t* __restrict__ ws) {
    extern __shared__ uint32_t s_bins[];
    rs_clear_bins(s_bins);
    __syncthreads();
    const auto count = rs_count<sizeof(T) != 4>(s_bins);
    mag_walk<T, VEC, false>(W, R, K, ld, nullptr, 0, [&](T& v) {
        count(abs_bits<T>(v));
        return false;
    });
    rs_merge_bins(s_bins, ws);
}

// fp32, second digit
template <int VEC>
__global__ __launch_bounds__(256) void k_mag_hist_low(float* __restrict__ W, int64_t R, int64_t K, int64_t ld,
                                                      uint32_t* __restrict__ ws) {
    const auto count = rs_count_low(ws);
    mag_walk<float, VEC, false>(W, R, K, ld, nullptr, 0, [&](float& v) {
        count(abs_bits<float>(v));
        return false;
    });
}

// a 16-bit dtype is finished after the first digit: its bin is the threshold. The histograms are not cleared: a call zeroes them.
__global__ __launch_bounds__(RS_T) void k_mag_scan(uint32_t* __restrict__ ws, uint32_t kth, int second, int dt,
                                                   void* __restrict__ thresh_out) {
    rs_scan<false>(ws, kth, second, [&](int digit, uint32_t v) {
        if (digit == 1) {
            if (thresh_out) *(uint32_t*)thresh_out = v;
        } else if (dt != LLMC_F32) {
            ws[RS_STATE + 2] = v;
            if (thresh_out) *(uint16_t*)thresh_out = (uint16_t)v;
        }
    });
}

template <typename T, int VEC>
__global__ __launch_bounds__(256) void k_mag_mask(T* __restrict__ W, int64_t R, int64_t K, int64_t ld, const uint32_t* __restrict__ ws,
                                                  uint8_t* __restrict__ mask, int mask_vec) {
    const uint32_t thr = ws[RS_STATE + 2];
    mag_walk<T, VEC, true>(W, R, K, ld, mask, mask_vec, [&](T& v) {
        const bool cut = abs_bits<T>(v) <= thr;
        if (cut) v = zero_of<T>();
        return cut;
    });
}

template <typename T, int VEC>
int magnitude_launch(void* W, int dt, int64_t R, int64_t K, int64_t ld, uint32_t kth, void* thresh_out, uint8_t* mask, uint32_t* ws,
                     hipStream_t st) {
    const int64_t vecs = R * (K / VEC);
    const int cus = device_cu_count();
    const int mask_vec = ((uintptr_t)mask & 3) == 0;
    const dim3 stream_grid((unsigned)capped_grid(vecs, 256, (int64_t)cus * 16));
    hipLaunchKernelGGL(k_mag_zero, dim3(16), dim3(RS_T), 0, st, ws);
    LLMC_LAUNCH_CHECK();
    if (int rc = ensure_dynamic_lds((const void*)k_mag_hist<T, VEC>, RS_BINS * 4)) return rc;
    // a workgroup merges up to RS_BINS counters into ws: no more workgroups than have 4 elements per bin to count, one per CU at most
    hipLaunchKernelGGL((k_mag_hist<T, VEC>), dim3((unsigned)capped_grid(vecs * VEC, (int64_t)RS_BINS * 4, cus)), dim3(RS_T),
                       RS_BINS * 4, st, (T*)W, R, K, ld, ws);
    LLMC_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mag_scan, dim3(1), dim3(RS_T), 0, st, ws, kth, 0, dt, thresh_out);
    LLMC_LAUNCH_CHECK();
    if constexpr (sizeof(T) == 4) {
        hipLaunchKernelGGL((k_mag_hist_low<VEC>), stream_grid, dim3(256), 0, st, (float*)W, R, K, ld, ws);
        LLMC_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_mag_scan, dim3(1), dim3(RS_T), 0, st, ws, kth, 1, dt, thresh_out);
        LLMC_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL((k_mag_mask<T, VEC>), stream_grid, dim3(256), 0, st, (T*)W, R, K, ld, (const uint32_t*)ws, mask, mask_vec);
    LLMC_LAUNCH_CHECK();
    return LLMC_OK;
}

}  // namespace
}  // namespace llmc

using namespace llmc;

extern "C" size_t llmc_col_sqsum_ws_bytes(int64_t N, int64_t K, int dt) {
    if (N <= 0 || K <= 0 || !dtype_ok(dt)) return 0;
    return (size_t)sq_chunks(N, K, dt) * (size_t)K * sizeof(float);
}

extern "C" int llmc_col_sqsum(const void* X, int dt, int64_t N, int64_t K, int init, float* acc, float* out, int64_t nsamples,
                              void* ws, llmc_stream_t stream) {
    LLMC_REQUIRE(dtype_ok(dt), "col_sqsum: bad dtype");
    LLMC_REQUIRE(X && acc && N > 0 && K > 0, "col_sqsum: null/empty argument");
    LLMC_REQUIRE(ws != nullptr, "col_sqsum: missing workspace");
    LLMC_REQUIRE(N < (1ll << 31) + 1 && K < (1ll << 31), "col_sqsum: N up to 2^31 rows, K below 2^31");
    LLMC_REQUIRE(!out || nsamples > 0, "col_sqsum: nsamples must be positive when out is given");
    hipStream_t st = (hipStream_t)stream;
    const int64_t nchunk = sq_chunks(N, K, dt);
    float* part = (float*)ws;
    col_reduce_launch(dt, col_vec(X, dt, K), N, K, nchunk, [&](auto t, auto vec, dim3 grid, int64_t rpc) {
        using T = decltype(t);
        hipLaunchKernelGGL((k_col_sqsum_partial<T, decltype(vec)::value>), grid, dim3(SQ_B), 0, st, (const T*)X, N, K, rpc, part);
    });
    LLMC_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_col_sqsum_fold, dim3((unsigned)ceil_div64(K, SQ_B)), dim3(SQ_B), 0, st, (const float*)part, nchunk, K, init,
                       acc, out, (float)nsamples);
    LLMC_LAUNCH_CHECK();
    return LLMC_OK;
}

extern "C" int llmc_prune_rows_paths(void) { return PATH_COUNT; }

extern "C" int llmc_prune_rows_path(int dt, int64_t R, int64_t K, int64_t ld, int64_t m, const void* W) {
    if (int rc = prune_check(dt, R, K, ld, m, W)) return rc;
    const int p = prune_path(dt, K, ld, m, W);
    if (p == LLMC_ENOTSUP) set_last_error_msg("prune_rows: a row of more than 32768 columns does not stay resident");
    return p;
}

extern "C" int llmc_prune_rows(void* W, int dt, int64_t R, int64_t K, int64_t ld, const float* scaler_row, int64_t n_prune,
                               int64_t m, uint8_t* mask_out, llmc_stream_t stream) {
    if (int rc = prune_check(dt, R, K, ld, m, W)) return rc;
    LLMC_REQUIRE(n_prune >= 0 && n_prune <= m, "prune_rows: n_prune outside [0, m]");
    const int path = prune_path(dt, K, ld, m, W);
    if (path < 0) {
        set_last_error_msg("prune_rows: a row of more than 32768 columns does not stay resident");
        return path;
    }
    hipStream_t st = (hipStream_t)stream;
    if (n_prune == 0) {
        if (mask_out) LLMC_HIP_CHECK(hipMemsetAsync(mask_out, 0, (size_t)R * (size_t)K, st));
        return LLMC_OK;
    }
    if (path == PATH_NM) {
        DISPATCH_DT(dt, launch_nm<T, true>(W, R, K, ld, (int)m, scaler_row, (int)n_prune, mask_out, st));
    } else if (path == PATH_NM_SCALAR) {
        DISPATCH_DT(dt, launch_nm<T, false>(W, R, K, ld, (int)m, scaler_row, (int)n_prune, mask_out, st));
    } else {
        DISPATCH_DT(dt, launch_rows_dt<T>(path, W, R, K, ld, scaler_row, (int)n_prune, mask_out, st));
    }
    LLMC_LAUNCH_CHECK();
    return LLMC_OK;
}

extern "C" size_t llmc_magnitude_prune_ws_bytes(int dt, int64_t R, int64_t K) {
    if (!dtype_ok(dt) || R <= 0 || K <= 0) return 0;
    return (size_t)RS_WORDS * sizeof(uint32_t);
}

extern "C" int llmc_magnitude_prune(void* W, int dt, int64_t R, int64_t K, int64_t ld, int64_t kth, void* thresh_out,
                                    uint8_t* mask_out, void* ws, llmc_stream_t stream) {
    LLMC_REQUIRE(dtype_ok(dt), "magnitude_prune: bad dtype");
    LLMC_REQUIRE(W != nullptr, "magnitude_prune: null W");
    LLMC_REQUIRE(R > 0 && K > 0 && R < (1ll << 31) && K < (1ll << 31) && R * K < (1ll << 32),
                 "magnitude_prune: R, K >= 1 and R * K below 2^32");
    LLMC_REQUIRE(ld >= K, "magnitude_prune: ld < K");
    LLMC_REQUIRE(kth >= 0 && kth < R * K, "magnitude_prune: kth outside [0, R * K)");
    LLMC_REQUIRE(ws != nullptr && ((uintptr_t)ws & 3) == 0, "magnitude_prune: missing workspace");
    hipStream_t st = (hipStream_t)stream;
    const bool vec = vec_ok(dt, K, ld, W);
    if (vec) {
        DISPATCH_DT(dt, return magnitude_launch<T, 16 / (int)sizeof(T)>(W, dt, R, K, ld, (uint32_t)kth, thresh_out, mask_out, (uint32_t*)ws, st));
    }
    DISPATCH_DT(dt, return magnitude_launch<T, 1>(W, dt, R, K, ld, (uint32_t)kth, thresh_out, mask_out, (uint32_t*)ws, st));
}
