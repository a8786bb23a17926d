// radix_select.h — the global rank select of prune.hip (magnitude pruning) and sparsegpt_loop.hip (a block's score threshold): the
// key of 0-based rank kth among the keys a caller's walk visits, by a two-digit radix select. Keys are bit patterns that order
// like unsigned integers: 31 bits (a sign-cleared fp32 pattern; digits: bits 30..16, then bits 15..0 of the keys inside the first
// digit's bin) or 15 bits (a sign-cleared 16-bit pattern: the first digit is the key). The callers keep their walks, their keys,
// their kernels and their grids: a histogram kernel calls its own walk with the counting functor made here. (The histograms as
// one function around a walk passed in compiled SparseGPT's two kernels to another stream: profiles/col_block_refactor.txt.)
#pragma once
#include "common.h"

namespace llmc {

constexpr int RS_BINS = 32768;             // first digit
constexpr int RS_LOW_BINS = 65536;         // second digit
constexpr int RS_T = 1024;                 // threads of the first histogram's workgroups and of the scan's one workgroup
// workspace, in uint32 words: [0, RS_BINS) first histogram, [RS_BINS, RS_BINS + RS_LOW_BINS) second histogram, then
// state[0] = bin of the first digit, state[1] = rank left inside it, state[2] = threshold key. Zeroed once per call, before the
// first histogram.
constexpr int RS_STATE = RS_BINS + RS_LOW_BINS;
constexpr int RS_WORDS = RS_STATE + 4;

// first digit: a histogram per workgroup of RS_T threads in LDS (s_bins: RS_BINS words, 128 KiB) — rs_clear_bins, a barrier (the
// caller's: its walk may have one already), the caller's walk with rs_count<KEY15>(s_bins), rs_merge_bins. The merge into ws is by
// integer atomics — exact, so deterministic; a workgroup merges only the bins it filled. KEY15: the key is the digit.
__device__ __forceinline__ void rs_clear_bins(uint32_t* s_bins) {
    for (int i = threadIdx.x; i < RS_BINS; i += RS_T) s_bins[i] = 0;
}
template <bool KEY15>
__device__ __forceinline__ auto rs_count(uint32_t* s_bins) {
    return [=](uint32_t key) { atomicAdd(&s_bins[KEY15 ? key : (key >> 16)], 1u); };
}
__device__ __forceinline__ void rs_merge_bins(const uint32_t* s_bins, uint32_t* __restrict__ ws) {
    __syncthreads();
    for (int i = threadIdx.x; i < RS_BINS; i += RS_T) {
        const uint32_t n = s_bins[i];
        if (n) atomicAdd(&ws[i], n);
    }
}

// second digit, the functor of the caller's walk: only the keys whose upper half is the first digit's bin count
__device__ __forceinline__ auto rs_count_low(uint32_t* __restrict__ ws) {
    const uint32_t hi = ws[RS_STATE];
    return [=](uint32_t key) {
        if ((key >> 16) == hi) atomicAdd(&ws[RS_BINS + (key & 0xFFFFu)], 1u);
    };
}

// one workgroup of RS_T threads: the bin that holds the rank. second == 0: rank `kth` in the first histogram -> state[0],
// state[1], then found(0, bin). second == 1: rank state[1] in the second -> state[2] = state[0] << 16 | bin, then found(1,
// state[2]). found runs in the one thread whose bins hold the rank. CLEAR: the histogram is zeroed once it has been read, so
// that the next select on this workspace finds it empty.
template <bool CLEAR, typename Found>
__device__ __forceinline__ void rs_scan(uint32_t* __restrict__ ws, uint32_t kth, int second, Found&& found) {
    __shared__ uint32_t s_w[RS_T / 64];
    uint32_t* hist = ws + (second ? RS_BINS : 0);
    const int per = (second ? RS_LOW_BINS : RS_BINS) / RS_T;
    const uint32_t rank = second ? ws[RS_STATE + 1] : kth;
    const uint32_t hi = second ? ws[RS_STATE] : 0u;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int b0 = threadIdx.x * per;
    uint32_t sum = 0;
    for (int i = 0; i < per; ++i) sum += hist[b0 + i];
    uint32_t incl = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t n = __shfl_up(incl, o, 64);
        if (lane >= o) incl += n;
    }
    if (lane == 63) s_w[wv] = incl;
    __syncthreads();
    uint32_t base = 0;
    for (int w = 0; w < wv; ++w) base += s_w[w];
    uint32_t excl = base + incl - sum;
    if (excl <= rank && rank < excl + sum) {          // one thread: the bins are its own, and the walk never leaves them
        int b = b0;
        for (; b < b0 + per - 1; ++b) {
            const uint32_t n = hist[b];
            if (rank < excl + n) break;
            excl += n;
        }
        if (!second) {
            ws[RS_STATE] = (uint32_t)b;
            ws[RS_STATE + 1] = rank - excl;
            found(0, (uint32_t)b);
        } else {
            const uint32_t thr = (hi << 16) | (uint32_t)b;
            ws[RS_STATE + 2] = thr;
            found(1, thr);
        }
    }
    if constexpr (CLEAR) {
        for (int i = 0; i < per; ++i) hist[b0 + i] = 0;
    }
}

}  // namespace llmc
