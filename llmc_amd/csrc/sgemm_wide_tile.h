// sgemm_wide_tile.h — one tile of K4's phased far update as a device function: the body of k_sgemm_wide (sgemm_wide.hip, where
// the design is described) for the kernels that run it — k_sgemm_wide itself and the rider role of k_gptq_block_riders
// (gptq_loop.hip). 256 threads work on one tile; `tid` is the thread's index among them and `smem` their Wide<MB>::LDS bytes.
// The function synchronises with workgroup barriers: every wave of a workgroup that calls it must call it, with the same `nst`.
#pragma once
#include "mfma_common.h"
#include "sgemm.h"

namespace llmc {
namespace wide {

constexpr int W_BN = 128, W_K = 16, W_SLOTS = 4;
constexpr int W_ROW = 1152;                    // LDS pitch of a 1-KiB piece: 1024 + 128, so that the piece holding k + 1 starts in the other half of the banks
constexpr int W_BB = (W_K / 2) * W_ROW;        // a 128-wide operand's part of a stage: 8 pieces = rows (4q + e, 4q + e + 2), q = 0..3, e = 0..1
constexpr int W_PHASE = 128 / W_K;             // stages per phase
// MB = 32-row blocks per wave along M: 4 -> 256 x 128 workgroup tile, 407 registers, one workgroup per CU, an XCD's 32 tiles = 4 x 8;
//                                      2 -> 128 x 128, two workgroups per CU (one covers the other's first and last microseconds), 64 tiles = 8 x 8
template <int MB> struct Wide {
    static constexpr int BM = 64 * MB;
    static constexpr int AB = MB == 4 ? W_K * W_ROW : W_BB;      // 256 wide: one k-row per piece; 128 wide: as B
    static constexpr int SLOT = AB + W_BB;
    static constexpr int LDS = W_SLOTS * SLOT;                   // 110592 / 73728
    static constexpr int PER_XCD = MB == 4 ? 32 : 64;            // tiles an XCD runs at a time = one block of 2^sm x 2^sn tiles (host's choice)
    static constexpr int D = MB + 2;                             // DMA instructions per wave and stage
    static constexpr int NBLK = 2 * MB;                          // accumulator blocks per wave
};

struct WideArgs {
    const float* A;
    const float* B;
    float* C;
    int64_t ldc;
    uint32_t rowA, rowB, rowC;          // bytes between k-rows of A, of B, between rows of C
    uint32_t bytesA, bytesB, bytesC;    // buffer extents from a tile's first element
    int nst;                            // Kd / 16
    int tm, tn, sbm, nsb;               // tiles along M, N; tile blocks along M; tile blocks
    int sm_log, sn_log;                 // a tile block = 2^sm_log x 2^sn_log tiles
};

// the operand part of WideArgs for the product `a` (host)
template <int MB> static inline void wide_operands(const SgemmArgs& a, WideArgs& w) {
    using W = Wide<MB>;
    w.A = a.A; w.B = a.B; w.C = a.C; w.ldc = a.ldc;
    w.rowA = (uint32_t)(a.lda * 4); w.rowB = (uint32_t)(a.ldb * 4); w.rowC = (uint32_t)(a.ldc * 4);
    w.bytesA = (uint32_t)(((int64_t)(a.Kd - 1) * a.lda + W::BM) * 4);
    w.bytesB = (uint32_t)(((int64_t)(a.Kd - 1) * a.ldb + W_BN) * 4);
    w.bytesC = (uint32_t)(((int64_t)(W::BM - 1) * a.ldc + W_BN) * 4);
    w.nst = a.Kd / W_K;
    w.tm = a.M / W::BM; w.tn = a.N / W_BN;
}

template <int MB>
__device__ __forceinline__ void wide_tile(const WideArgs& a, const int ti, const int tj, char* smem, const int tid) {
    using W = Wide<MB>;
    const int lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wv >> 1, wn = wv & 1;
    const auto dA = uniform_rsrc(a.A + (int64_t)ti * W::BM, a.bytesA);
    const auto dB = uniform_rsrc(a.B + (int64_t)tj * W_BN, a.bytesB);
    const auto dC = uniform_rsrc(a.C + (int64_t)ti * W::BM * a.ldc + (int64_t)tj * W_BN, a.bytesC);
    LDS_AS char* lds = (LDS_AS char*)smem;
    const uint32_t lds0 = (uint32_t)(uintptr_t)lds;
    const int nst = a.nst;

    // ---- LDS-DMA. A 128-wide operand: piece (q, e) = k-rows 4q + e (lanes 0-31) and 4q + e + 2 (lanes 32-63), 512 B each, at
    // (2q + e) * W_ROW; wave wv brings k-quad q = wv. The 256-wide A: one k-row (1 KiB) per piece at k * W_ROW, wave wv brings rows 4 wv ..
    const uint32_t voA = MB == 4 ? (uint32_t)lane * 16u : (uint32_t)(lane >> 5) * 2u * a.rowA + (uint32_t)(lane & 31) * 16u;
    const uint32_t voB = (uint32_t)(lane >> 5) * 2u * a.rowB + (uint32_t)(lane & 31) * 16u;
    auto issue = [&](int j) {
        const uint32_t slot = lds0 + (uint32_t)(j & (W_SLOTS - 1)) * W::SLOT;
        const uint32_t k = (uint32_t)(j * W_K + 4 * wv);
        if constexpr (MB == 4) {
#pragma unroll
            for (int i = 0; i < 4; ++i) dma16_to(dA, voA, (k + i) * a.rowA, slot + (uint32_t)(4 * wv + i) * W_ROW);
        } else {
#pragma unroll
            for (int e = 0; e < 2; ++e) dma16_to(dA, voA, (k + e) * a.rowA, slot + (uint32_t)(2 * wv + e) * W_ROW);
        }
#pragma unroll
        for (int e = 0; e < 2; ++e) dma16_to(dB, voB, (k + e) * a.rowB, slot + W::AB + (uint32_t)(2 * wv + e) * W_ROW);
    };

    // ---- operand reads: pair kp of a stage = k-rows 2 kp (lanes 0-31) and 2 kp + 1 (lanes 32-63); two base registers per operand
    // (slots 0-1 / 2-3: the ds_read offset field has 16 bits)
    LDS_AS char* pA[2];
    LDS_AS char* pB[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        pA[h] = lds + h * 2 * W::SLOT + (lane >> 5) * W_ROW + (wm * 32 * MB + (lane & 31)) * 4;
        pB[h] = lds + h * 2 * W::SLOT + W::AB + (lane >> 5) * W_ROW + (wn * 64 + (lane & 31)) * 4;
    }
    float fa[2][MB], fb[2][2];
    auto rd = [&](auto cc, auto slc, auto kpc, auto ic) {
        constexpr int c = decltype(cc)::value, SL = decltype(slc)::value, kp = decltype(kpc)::value, i = decltype(ic)::value;
        constexpr int narrow = (SL & 1) * W::SLOT + (kp >> 1) * 2 * W_ROW + (kp & 1) * 512;
        if constexpr (i < MB) {
            if constexpr (MB == 4) fa[c][i] = *(LDS_AS const float*)(pA[SL >> 1] + (SL & 1) * W::SLOT + kp * 2 * W_ROW + i * 128);
            else fa[c][i] = *(LDS_AS const float*)(pA[SL >> 1] + narrow + i * 128);
        } else {
            fb[c][i - MB] = *(LDS_AS const float*)(pB[SL >> 1] + narrow + (i - MB) * 128);
        }
    };

    // ---- the C tile of this wave: block (m, n) element r of lane l = row wm*32*MB + m*32 + (r & 3) + 8 (r >> 2) + 4 (l >> 5),
    // column wn*64 + n*32 + (l & 31)
    const uint32_t voC = (uint32_t)(wm * 32 * MB + 4 * (lane >> 5)) * a.rowC + (uint32_t)(wn * 64 + (lane & 31)) * 4u;
    auto soC = [&](uint32_t rowC, int m, int n, int r) { return (uint32_t)(m * 32 + (r & 3) + 8 * (r >> 2)) * rowC + (uint32_t)n * 128u; };
    f32x16 cv[MB][2], acc[MB][2];
    const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

    // prologue: three stages requested (nst >= 8), the first one published
    issue(0);
    issue(1);
    issue(2);
    vm_wait<2 * W::D>();
    __builtin_amdgcn_s_barrier();
    static_for<0, MB + 2>([&](auto ic) { rd(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{}, ic); });
    __builtin_amdgcn_sched_barrier(0);

    // One phase = 8 stages of 8 pairs of 2 MB MFMAs. Behind MFMA i of pair p: i < MB + 2 -> operand i of the next pair (pair 7: the
    // next stage's first pair; the barrier in pair 5 has published that stage). Pair 5, last MFMA: this wave's pieces of stage j + 1
    // have landed, barrier (every wave is past its last read of stage j - 1). Pair 6, last MFMA: stage j + 3 requested into the slot
    // of stage j - 1. First phase, pair 7 of stages s < 2 MB: the C values of block s requested, i.e. issue order
    // D0 D1 D2 | D3 C0 | D4 C1 | ..: when stage j waits for D(j+1) the younger requests are C(j-2) D(j+2) C(j-1).
    constexpr int LASTI = 2 * MB - 1, CPER = 16 / (2 * MB);
    auto phase = [&](auto firstc, int j0) {
        constexpr bool FIRST = decltype(firstc)::value;
        static_for<0, W_PHASE>([&](auto sc) {
            constexpr int s = decltype(sc)::value, SL = s & (W_SLOTS - 1), SN = (s + 1) & (W_SLOTS - 1);
            const int j = j0 + s;
            static_for<0, 8>([&](auto pc) {
                constexpr int p = decltype(pc)::value, c = p & 1;
                static_for<0, 2 * MB>([&](auto ic) {
                    constexpr int i = decltype(ic)::value, m = i >> 1, n = (m & 1) ? 1 - (i & 1) : (i & 1);
                    if constexpr (s == 0 && p == 0) {
                        // a phase's first product starts from +0 (inline constant: no zeroing); the previous phase's block is
                        // subtracted from C just before its accumulator is overwritten, under the MFMA issued before it
                        if constexpr (!FIRST) cv[m][n] = cv[m][n] - acc[m][n];
                        acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[c][m], fb[c][n], zero, 0, 0, 0);
                    } else {
                        acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[c][m], fb[c][n], acc[m][n], 0, 0, 0);
                    }
                    if constexpr (i < MB + 2) {
                        if constexpr (p < 7) rd(std::integral_constant<int, c ^ 1>{}, std::integral_constant<int, SL>{}, std::integral_constant<int, (p + 1) & 7>{}, ic);
                        else rd(std::integral_constant<int, c ^ 1>{}, std::integral_constant<int, SN>{}, std::integral_constant<int, 0>{}, ic);
                    }
                    if constexpr (p == 5 && i == LASTI) {
                        if (j + 2 < nst) {
                            constexpr int younger_c = FIRST ? 16 * ((s >= 2 && s - 2 < W::NBLK) + (s >= 1 && s - 1 < W::NBLK)) : 0;
                            vm_wait<W::D + younger_c>();
                        } else {
                            vm_wait<0>();
                        }
                        __builtin_amdgcn_s_barrier();
                    }
                    if constexpr (p == 6 && i == LASTI) {
                        if (j + 3 < nst) issue(j + 3);
                    }
                    if constexpr (FIRST && p == 7 && s < W::NBLK) {
#pragma unroll
                        for (int e = 0; e < CPER; ++e) {
                            constexpr int bm = s >> 1, bn = s & 1;
                            cv[bm][bn][CPER * i + e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(dC, voC, soC(a.rowC, bm, bn, CPER * i + e), 0));
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);
                });
            });
        });
        if constexpr (FIRST) vm_wait<0>();      // the C values are here (and every request older than them)
        __builtin_amdgcn_sched_barrier(0);
    };
    phase(std::true_type{}, 0);
    for (int j0 = W_PHASE; j0 < nst; j0 += W_PHASE) phase(std::false_type{}, j0);
#pragma unroll
    for (int m = 0; m < MB; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) cv[m][n] = cv[m][n] - acc[m][n];

    uint32_t rowC2 = a.rowC;      // opaque copy: the row offsets are recomputed here, not kept in SGPRs from the first phase on
    asm volatile("" : "+s"(rowC2));
#pragma unroll
    for (int m = 0; m < MB; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float v = cv[m][n][r];      // (a bit_cast applied to the vector element itself reads element 0: hipcc 7.2)
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), dC, voC, soC(rowC2, m, n, r), 0);
            }
}

}  // namespace wide
}  // namespace llmc
