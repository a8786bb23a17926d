// sparsegpt_loop.hip — SparseGPT's `fasterprune` (Frantar & Alistarh 2023) in fp32 at blocksize 128: GPTQ's blocked column loop
// with the quantizer replaced by a mask. The reference tree has no counterpart; include/llmc_hip.h states the arithmetic and
// tests/sparsegpt_oracle.py restates it in numpy, which the kernel matches bit for bit.
//
// Blocks, ownership and the trailing update are col_block.h's. Per block:
//   unstructured  the score s = fl(fl(w w) / fl(d d)) of every element of the [R, count] panel as the block finds it; the score
//                 of 0-based rank kth = int(R count sparsity) by radix_select.h's two-digit select over the score's bit pattern
//                 (never negative: it orders like an unsigned integer) — k_sg_hist, k_sg_scan, k_sg_hist_low, k_sg_scan. The
//                 threshold stays in the workspace; the block kernel reads it there and masks every s <= thresh.
//   n:m           no select. Since m divides 16 and a group starts at a column i with i % m == 0, its m columns sit in m
//                 adjacent lanes of the row at one register index: at the group's first column every lane scores its RUNNING
//                 weight and ranks it among the m lanes (lower score first, equal scores by lower column) by m cross-lane reads.
//   per column    q = masked ? +0 : w, err = fl(fl(w - q) / d), loss = fl(fl(diff diff) / fl(d d)),
//                 w_j = fl(w_j - fl(err U[c][j])) for the later columns of the block: one rounding per op, no fma.
#include "col_block.h"
#include "radix_select.h"

namespace llmc {
namespace {

// the select key of a weight: the bits of its score. dd = fl(d d). The sign bit is cleared so that a NaN score of either sign
// still names a bin inside the histogram (non-finite weights are outside the contract; they must not index out of bounds).
__device__ __forceinline__ uint32_t sg_key(float w, float dd) {
    const float s = (w * w) / dd;
    return __float_as_uint(s) & 0x7FFFFFFFu;
}

// walk of the [R, count] panel W[:, i1 : i1 + count] shared by the two histogram kernels; s_dd[j] = fl(d_j d_j)
template <typename F>
__device__ __forceinline__ void sg_walk(const float* __restrict__ W, const float* __restrict__ U, int64_t R, int K, int i1, int count,
                                        float* s_dd, F&& f) {
    for (int j = threadIdx.x; j < count; j += blockDim.x) {
        const float d = U[(int64_t)(i1 + j) * K + i1 + j];
        s_dd[j] = d * d;
    }
    __syncthreads();
    const int64_t total = R * count;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / count;
        const int j = (int)(i - r * count);
        f(sg_key(W[r * K + i1 + j], s_dd[j]));
    }
}

__global__ __launch_bounds__(RS_T) void k_sg_hist(const float* __restrict__ W, const float* __restrict__ U, int64_t R, int K, int i1,
                                                  int count, uint32_t* __restrict__ ws) {
    extern __shared__ uint32_t s_bins[];
    __shared__ float s_dd[CB_BS];
    rs_clear_bins(s_bins);
    sg_walk(W, U, R, K, i1, count, s_dd, rs_count<false>(s_bins));          // the barrier behind s_dd covers the clearing
    rs_merge_bins(s_bins, ws);
}

__global__ __launch_bounds__(256) void k_sg_hist_low(const float* __restrict__ W, const float* __restrict__ U, int64_t R, int K, int i1,
                                                     int count, uint32_t* __restrict__ ws) {
    __shared__ float s_dd[CB_BS];
    sg_walk(W, U, R, K, i1, count, s_dd, rs_count_low(ws));
}

// the select's words lie behind Err and are zeroed once per call: every scan clears the histogram it has read, so the next block
// finds it empty. The threshold stays in state[2], where the block kernel reads it.
__global__ __launch_bounds__(RS_T) void k_sg_scan(uint32_t* __restrict__ ws, uint32_t kth, int second) {
    rs_scan<true>(ws, kth, second, [](int, uint32_t) {});
}

struct SgBlockArgs {
    const float* W;          // [R, K] running weights
    const float* U;          // [K, K] upper factor
    float* Wout;             // [R, K]
    float* losses;           // [R, K] or null
    uint8_t* mask;           // [R, K] or null
    float* Err;              // [R, 128] err of this block
    const uint32_t* state;   // select state (unstructured): state[2] = threshold key
    int64_t R;
    int K, i1, count, prune_n;
};

// M = 0: unstructured (mask from the block-start scores and the selected threshold); M in {2, 4, 8, 16}: prune_n of every M
template <int M>
__global__ __launch_bounds__(CB_NT) void k_sparsegpt_block(SgBlockArgs a) {
#include "col_block_stage.h"

    float w[8], wf[8];                     // running weights; the weight as its own column step found it
    unsigned mk = 0;                       // bit e: column p + 16 e is pruned
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int c = p + 16 * e;
        w[e] = (active && c < a.count) ? a.W[row * a.K + a.i1 + c] : 0.0f;
        wf[e] = 0.0f;
    }
    if constexpr (M == 0) {
        const uint32_t thr = a.state[2];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int c = p + 16 * e;
            const float d = dg[c];
            if (c < a.count && sg_key(w[e], d * d) <= thr) mk |= 1u << e;
        }
    }
    const float* us = Us + p * 8;

    static_for<0, 8>([&](auto ec) {
        constexpr int E = decltype(ec)::value;
        if (16 * E < a.count) {
            const float dE = dg[16 * E + p];          // this lane's column of the stripe
            const int steps = a.count - 16 * E < 16 ? a.count - 16 * E : 16;
#pragma unroll 1
            for (int po = 0; po < steps; ++po) {
                if constexpr (M > 0) {
                    if ((po & (M - 1)) == 0) {
                        // ---- group start: columns 16E + po .. + M - 1 = register E of the lanes po .. po + M - 1
                        const uint32_t key = sg_key(w[E], dE * dE);
                        const int gb = p & ~(M - 1), tm = p & (M - 1);
                        int rank = 0;
#pragma unroll
                        for (int t = 0; t < M; ++t) {
                            const uint32_t kt = __float_as_uint(row_lane(__uint_as_float(key), gb + t));
                            rank += (kt < key || (kt == key && t < tm)) ? 1 : 0;
                        }
                        if (gb == po && rank < a.prune_n) mk |= 1u << E;
                    }
                }
                const int i = 16 * E + po;
                const float wo = w[E];
                const float q = ((mk >> E) & 1u) ? 0.0f : wo;
                const float diff = wo - q;
                const float e1 = row_lane(diff / dE, po);
                if (p == po) wf[E] = wo;
                col_rank1(w, e1, us, i);
            }
        }
    });

    if (!active) return;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int c = p + 16 * e;
        float err = 0.0f;
        if (c < a.count) {
            const bool cut = (mk >> e) & 1u;
            const float d = dg[c];
            const float q = cut ? 0.0f : wf[e];
            const float diff = wf[e] - q;
            err = diff / d;          // the division of the column's own step, again
            const int64_t o = row * a.K + a.i1 + c;
            a.Wout[o] = q;
            if (a.losses) a.losses[o] = (diff * diff) / (d * d);
            if (a.mask) a.mask[o] = cut ? 1 : 0;
        }
        a.Err[row * CB_BS + c] = err;
    }
}

}  // namespace
}  // namespace llmc

using namespace llmc;

extern "C" size_t llmc_sparsegpt_prune_ws_bytes(int64_t R, int64_t K) {
    if (R <= 0 || K <= 0) return 0;
    return (size_t)R * CB_BS * sizeof(float) + (size_t)RS_WORDS * sizeof(uint32_t);
}

extern "C" int llmc_sparsegpt_prune(float* W, const float* Hinv, int64_t R, int64_t K, double sparsity, int64_t prune_n,
                                    int64_t prune_m, float* Wout, float* losses, uint8_t* mask, int blocksize, void* ws,
                                    llmc_stream_t stream) {
    LLMC_REQUIRE(W && Hinv && Wout && ws && R > 0 && K > 0, "sparsegpt_prune: null/empty argument");
    LLMC_REQUIRE(R < (1ll << 24) && K < (1ll << 30), "sparsegpt_prune: R below 2^24, K below 2^30");
    LLMC_REQUIRE(blocksize == CB_BS, "sparsegpt_prune: blocksize must be 128");
    const bool nm = prune_m != 0;
    if (!nm) {
        LLMC_REQUIRE(sparsity >= 0.0 && sparsity < 1.0, "sparsegpt_prune: sparsity outside [0, 1)");
    } else if (prune_m == 2 || prune_m == 4 || prune_m == 8 || prune_m == 16) {
        LLMC_REQUIRE(prune_n >= 0 && prune_n <= prune_m, "sparsegpt_prune: prune_n outside [0, m]");
    }
    if (K % 4 != 0) {
        set_last_error_msg("sparsegpt_prune: K must be a multiple of 4");
        return LLMC_ENOTSUP;
    }
    if (nm && !(prune_m == 2 || prune_m == 4 || prune_m == 8 || prune_m == 16)) {
        set_last_error_msg("sparsegpt_prune: m must be 2, 4, 8 or 16 (0 = unstructured)");
        return LLMC_ENOTSUP;
    }
    if (nm && K % prune_m != 0) {
        set_last_error_msg("sparsegpt_prune: m does not divide K");
        return LLMC_ENOTSUP;
    }
    hipStream_t st = (hipStream_t)stream;
    float* Err = (float*)ws;
    uint32_t* sel = (uint32_t*)(Err + R * CB_BS);
    const int cus = device_cu_count();
    if (!nm) {
        if (int rc = ensure_dynamic_lds((const void*)k_sg_hist, RS_BINS * 4)) return rc;
        LLMC_HIP_CHECK(hipMemsetAsync(sel, 0, (size_t)RS_WORDS * sizeof(uint32_t), st));
    }
    return col_blocks(W, Hinv, Err, R, K, st, [&](int i1, int count) {
        if (!nm) {
            const int64_t numel = R * count;
            const uint32_t kth = (uint32_t)(int64_t)((double)numel * sparsity);
            // 8 elements per thread: the walk is a chain of dependent loads, so the panel is spread over many workgroups (one per CU
            // at most); a workgroup merges only the bins it filled, and the scores of a panel share a few exponents
            hipLaunchKernelGGL(k_sg_hist, dim3((unsigned)capped_grid(numel, (int64_t)RS_T * 8, cus)), dim3(RS_T), RS_BINS * 4, st,
                               (const float*)W, Hinv, R, (int)K, i1, count, sel);
            LLMC_LAUNCH_CHECK();
            hipLaunchKernelGGL(k_sg_scan, dim3(1), dim3(RS_T), 0, st, sel, kth, 0);
            LLMC_LAUNCH_CHECK();
            hipLaunchKernelGGL(k_sg_hist_low, dim3((unsigned)capped_grid(numel, 256 * 8, (int64_t)cus * 8)), dim3(256), 0, st,
                               (const float*)W, Hinv, R, (int)K, i1, count, sel);
            LLMC_LAUNCH_CHECK();
            hipLaunchKernelGGL(k_sg_scan, dim3(1), dim3(RS_T), 0, st, sel, kth, 1);
            LLMC_LAUNCH_CHECK();
        }
        SgBlockArgs a;
        a.W = W; a.U = Hinv; a.Wout = Wout; a.losses = losses; a.mask = mask; a.Err = Err; a.state = sel + RS_STATE;
        a.R = R; a.K = (int)K; a.i1 = i1; a.count = count; a.prune_n = (int)prune_n;
        const dim3 grid((unsigned)ceil_div64(R, CB_NT / 16));
        switch ((int)prune_m) {
            case 0: hipLaunchKernelGGL((k_sparsegpt_block<0>), grid, dim3(CB_NT), 0, st, a); break;
            case 2: hipLaunchKernelGGL((k_sparsegpt_block<2>), grid, dim3(CB_NT), 0, st, a); break;
            case 4: hipLaunchKernelGGL((k_sparsegpt_block<4>), grid, dim3(CB_NT), 0, st, a); break;
            case 8: hipLaunchKernelGGL((k_sparsegpt_block<8>), grid, dim3(CB_NT), 0, st, a); break;
            default: hipLaunchKernelGGL((k_sparsegpt_block<16>), grid, dim3(CB_NT), 0, st, a); break;
        }
        LLMC_LAUNCH_CHECK();
        return (int)LLMC_OK;
    });
}
