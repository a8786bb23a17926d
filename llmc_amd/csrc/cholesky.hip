// cholesky.hip — K2/K3 of the GPTQ path (gptq.py:139-174):
//   llmc_hessian_prep     dead-column fix, actorder gather of H and W, damping
//   llmc_chol_inv_upper   U upper with H^-1 = U^T U, the factor the reference obtains from
//                         cholesky -> cholesky_inverse -> cholesky(upper)
//
// Math (fp32 throughout, like the reference): with J the index reversal, U = J * inv(chol_lower(J H J)) * J.
// In upper/row-major form: A' = antitranspose(H); A' = U'^T U' (blocked right-looking, 128-wide panels:
// one workgroup factors + inverts the diagonal block, the panel solve and the symmetric trailing update
// are fp32-MFMA GEMMs); V = U'^-1 by recursive doubling over the already inverted diagonal blocks
// ([[A,C],[0,B]]^-1 = [[A^-1, -A^-1 C B^-1],[0, B^-1]]); U = antitranspose(V).  2K^3/3 flops instead of
// the reference's 4K^3/3.
#include <stdlib.h>
#include "common.h"
#include "mfma_common.h"
#include "sgemm.h"
#include "pipe_lanes.h"

namespace llmc {

static constexpr int NB = 128;

// ---------------------------------------------------------------------------------------------
// out[i][j] = in[n-1-j][n-1-i]  (reflection across the anti-diagonal), 32x32 LDS tiles, coalesced both
// ways. upper_only: write 0 for j < i.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_antitranspose(const float* __restrict__ in, float* __restrict__ out,
                                                       int n, int upper_only) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
    const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;    // input tile
    for (int y = ty; y < 32; y += 8) {
        int r = r0 + y, c = c0 + tx;
        tile[y][tx] = (r < n && c < n) ? in[(int64_t)r * n + c] : 0.0f;
    }
    __syncthreads();
    // in[r][c] -> out[n-1-c][n-1-r]; output row = n-1-(c0+y'), output col = n-1-(r0+x')
    for (int y = ty; y < 32; y += 8) {
        int c = c0 + y, r = r0 + tx;
        if (r < n && c < n) {
            int orow = n - 1 - c, ocol = n - 1 - r;
            float v = tile[tx][y];
            if (upper_only && ocol < orow) v = 0.0f;
            out[(int64_t)orow * n + ocol] = v;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Diagonal block (<= 128 x 128): U = chol_upper(D), V = U^-1, one workgroup of 4 waves, everything in LDS.
// Blocked over 32 x 32 sub-blocks:
//   - a sub-block is factored / inverted by ONE wave with lane j owning column j in 32 registers; pivots
//     and multipliers travel by v_readlane (uniform lane index), no LDS, no barriers inside;
//   - panel solves, trailing updates and the doubling steps of the inverse are 32x32x32 block products on
//     the f32 MFMA pipe, spread over the 4 waves.
// Replaces a 128-step barrier-synchronised kernel (396 us on MI355X, profiles/r01_a) on the critical path
// of the blocked factorisation. Partial blocks are padded with the identity.
// ---------------------------------------------------------------------------------------------
static constexpr int PLD = 132;  // LDS leading dimension (floats)

__device__ __forceinline__ float rdlane(float v, int l) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}

// wave-level: factor the 32x32 block at S (upper Cholesky, in place, strict lower zeroed) and write its inverse to V.
// An identity carried next to the block receives the SAME row operations (scale row i by 1/u_ii, subtract u_ik * row i
// from row k): the operations that turn A into U turn I into U^-T, so the inverse needs no back-substitution pass.
// 1/sqrt(d) is the hardware rsq (1 ulp) + one Newton step instead of the correctly rounded sqrt and divide (about 30
// dependent instructions on the pivot chain); nothing downstream needs those last bits. (Earlier variants kept the
// block in 32 registers per lane with v_readlane / LDS-broadcast multipliers; see the git history.)
//
// On the matrix pipe: the 32x32 block and the identity live in two MFMA accumulators
// (C layout: register r of lane l holds row (r&3) + 8*(r>>2) + 4*(l>>5), column l&31), and the rank-1 update of pivot i,
// rows k > i of [A | I] -= u_ik * (scaled row i), is ONE v_mfma_f32_32x32x2_f32 per accumulator: the scaled row sits in
// the 32 lanes of one half-wave, which is exactly where the MFMA takes both its row-indexed multipliers (A operand,
// masked to rows > i) and its column-indexed row vector (B operand) for k-slot `half`; the other k-slot is fed zeros.
// No cross-lane traffic besides the pivot's v_readlane; 2 x 64 matrix-pipe cycles per pivot instead of ~2 x 31
// readlane + fma pairs.
__device__ __forceinline__ void wave_potrf32_inv(float* __restrict__ S, float* __restrict__ V,
                                                 float* __restrict__ rowbuf, int lane, int kglobal,
                                                 int* __restrict__ info) {
#pragma clang fp contract(fast)
    (void)rowbuf;
    const int j = lane & 31, h = lane >> 5;
    f32x16 A, E;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
        A[r] = S[row * PLD + j];
        E[r] = row == j ? 1.0f : 0.0f;
    }
    bool bad = false;
    // Round 4: pivots in PANELS of four. Rows 4q .. 4q+3 sit in the four registers 4(q>>1) .. +3 of ONE half-wave
    // (q & 1), so a panel is factored on the VALU alone — pivot, rsq + Newton, scale the row, and update the (at most
    // three) later rows of the panel with one v_readlane + one fma each, the same fma(-u, row_i, row_k) the matrix pipe
    // would do — while the matrix pipe applies the PREVIOUS panel's pivots to the identity half (E). The rows below the
    // panel then get the panel's four pivots as two rank-2 updates per accumulator (both k-slots of v_mfma_f32_32x32x2:
    // the second pivot's row is moved to the other half-wave by v_permlane32_swap). Before (round 3) every pivot waited
    // for its own two dependent MFMAs (2 x 64 pipe cycles + the accumulator read-back): 269 cycles per pivot measured
    // (profiles/r04_potrf_stamps.txt); now the matrix pipe carries 4 MFMAs per panel and the pivot chain is VALU-only.
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int rb = 4 * (q >> 1), hq = q & 1;
        const bool mine = h == hq;
        float row[4], va[4], rinv[4], m[4][4];
#pragma unroll
        for (int t = 0; t < 4; ++t) row[t] = A[rb + t];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int i = 4 * q + t;
            const float d = rdlane(row[t], hq * 32 + i);
            if (!(d > 0.0f)) bad = true;
            float ri = __builtin_amdgcn_rsqf(d);
            ri = ri * (1.5f - 0.5f * d * ri * ri);
            rinv[t] = ri;
            va[t] = (mine && j >= i) ? row[t] * ri : 0.0f;          // scaled row i (upper part); the other half-wave holds 0
#pragma unroll
            for (int s2 = t + 1; s2 < 4; ++s2) {
                m[t][s2] = rdlane(va[t], hq * 32 + 4 * q + s2);     // u_{i, 4q+s2}
                row[s2] = __builtin_fmaf(-m[t][s2], va[t], row[s2]);
            }
        }
        // the identity half of the panel, with the multipliers found above
        float er[4], ve[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) er[t] = E[rb + t];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            ve[t] = mine ? er[t] * rinv[t] : 0.0f;
#pragma unroll
            for (int s2 = t + 1; s2 < 4; ++s2) er[s2] = __builtin_fmaf(-m[t][s2], ve[t], er[s2]);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            A[rb + t] = mine ? va[t] : A[rb + t];
            E[rb + t] = mine ? ve[t] : E[rb + t];
        }
        if (q < 7) {
            // rows >= 4q+4: two rank-2 updates per accumulator. Operand lanes 0..31 = k-slot 0, 32..63 = k-slot 1.
#pragma unroll
            for (int pr = 0; pr < 2; ++pr) {
                const float b0 = va[2 * pr], b1 = va[2 * pr + 1];
                const float e0 = ve[2 * pr], e1 = ve[2 * pr + 1];
                const float a0 = (mine && j >= 4 * q + 4) ? -b0 : 0.0f;      // -u_{i,k} as the multiplier of row k = j
                const float a1 = (mine && j >= 4 * q + 4) ? -b1 : 0.0f;
                float opa, opb, ope;
                if (hq == 0) {       // data in lanes 0..31: x = [p0 | 0], y = [p1 | 0] -> [p0 | p1]
                    opa = __int_as_float(__builtin_amdgcn_permlane32_swap(__float_as_int(a0), __float_as_int(a1), false, false)[0]);
                    opb = __int_as_float(__builtin_amdgcn_permlane32_swap(__float_as_int(b0), __float_as_int(b1), false, false)[0]);
                    ope = __int_as_float(__builtin_amdgcn_permlane32_swap(__float_as_int(e0), __float_as_int(e1), false, false)[0]);
                } else {             // data in lanes 32..63: swap(y, x) leaves [p1 | p0] in the second result
                    opa = __int_as_float(__builtin_amdgcn_permlane32_swap(__float_as_int(a1), __float_as_int(a0), false, false)[1]);
                    opb = __int_as_float(__builtin_amdgcn_permlane32_swap(__float_as_int(b1), __float_as_int(b0), false, false)[1]);
                    ope = __int_as_float(__builtin_amdgcn_permlane32_swap(__float_as_int(e1), __float_as_int(e0), false, false)[1]);
                }
                A = __builtin_amdgcn_mfma_f32_32x32x2f32(opa, opb, A, 0, 0, 0);
                E = __builtin_amdgcn_mfma_f32_32x32x2f32(opa, ope, E, 0, 0, 0);
            }
        }
    }
    if (bad && lane == 0) atomicCAS(info, 0, kglobal + 1);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
        S[row * PLD + j] = j >= row ? A[r] : 0.0f;
    }
    // E = U^-T: E[row][j] = V[j][row]; four consecutive rows per register quad -> one 16-B store
#pragma unroll
    for (int q = 0; q < 4; ++q)
        *reinterpret_cast<float4*>(V + j * PLD + 8 * q + 4 * h) = make_float4(E[4 * q], E[4 * q + 1], E[4 * q + 2], E[4 * q + 3]);
}

// 32x32x32 block product on the f32 MFMA: acc += op(A) * B, op(A)[i][k] = TA ? A[k][i] : A[i][k]
template <bool TA>
__device__ __forceinline__ f32x16 blk_mm(const float* __restrict__ A, const float* __restrict__ B, f32x16 acc,
                                          int lane) {
    const int c = lane & 31, h = lane >> 5;
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
        const int k = 2 * kk + h;
        const float av = TA ? A[k * PLD + c] : A[c * PLD + k];
        const float bv = B[k * PLD + c];
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
    }
    return acc;
}
__device__ __forceinline__ void blk_store(float* __restrict__ C, const f32x16& acc, int lane, float sign) {
    const int c = lane & 31, h = lane >> 5;
#pragma unroll
    for (int r = 0; r < 16; ++r) C[((r & 3) + 8 * (r >> 2) + 4 * h) * PLD + c] = sign * acc[r];
}
__device__ __forceinline__ void blk_sub(float* __restrict__ C, const f32x16& acc, int lane) {
    const int c = lane & 31, h = lane >> 5;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        float* p = C + ((r & 3) + 8 * (r >> 2) + 4 * h) * PLD + c;
        *p = *p - acc[r];
    }
}
#define PBLK(M, bi, bj) ((M) + (bi) * 32 * PLD + (bj) * 32)
// Blocks of the inverse V live in the part of S the factor does not use: V(a,b), a < b, in S's block (b,a) below the
// diagonal; the four diagonal blocks V(a,a) side by side in a 32-row strip Vd. That keeps the kernel at 85 KB of
// LDS (S 66 KB + strip 16.5 KB) instead of 2 x 66 KB, so it can be co-resident with workgroups of the far-update
// GEMM running on the helper stream instead of waiting for a CU to drain.
#define VBLK(a, b) ((a) == (b) ? (Vd + (a) * 32) : PBLK(S, b, a))

// phase stamps for tools/probes/probe_potrf.hip (compiled out of the product build)
#ifdef LLMC_PROBE_STAMPS
__device__ long long g_potrf_stamps[32];
#define LLMC_STAMP(i) do { if (threadIdx.x == 0) g_potrf_stamps[i] = clock64(); } while (0)
#else
#define LLMC_STAMP(i) do { } while (0)
#endif

__global__ __launch_bounds__(256, 2) void k_potrf_inv(float* __restrict__ W, int64_t ld, int k0, int nb,
                                                   float* __restrict__ Vout, int* __restrict__ info) {
    extern __shared__ __attribute__((aligned(16))) float plds[];
    float* S = plds;
    float* Vd = plds + NB * PLD;
    float* rowbuf = plds + NB * PLD + 32 * PLD;   // 64 floats of wave-private scratch for the 32x32 factor
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    LLMC_STAMP(0);
    // load the block with 16 independent 16-B loads per thread in flight (a scalar loop here serialises 64
    // dependent global-load latencies and was most of this kernel's time)
    {
        float4 ld4[16];
        const bool full = nb == NB && (ld % 4 == 0) && (k0 % 4 == 0);
        // the whole-block path has NO control flow between its 16 loads: with the edge path merged into the same loop the
        // compiler waited for every load before issuing the next (16 serialised round trips, 22.6k of the kernel's 93.7k
        // cycles: profiles/r04_potrf_stamps.txt)
        if (full) {
            const float* base = W + (int64_t)(k0 + (tid >> 5)) * ld + k0 + (tid & 31) * 4;
#pragma unroll
            for (int q = 0; q < 16; ++q) ld4[q] = *reinterpret_cast<const float4*>(base + (int64_t)(8 * q) * ld);
        } else {
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int e4 = tid + 256 * q;            // float4 index: row = e4 >> 5, col4 = e4 & 31
                const int i = e4 >> 5, j = (e4 & 31) * 4;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (i < nb) {
                    const float* p = W + (int64_t)(k0 + i) * ld + k0 + j;
                    if (j < nb) v.x = p[0];
                    if (j + 1 < nb) v.y = p[1];
                    if (j + 2 < nb) v.z = p[2];
                    if (j + 3 < nb) v.w = p[3];
                }
                ld4[q] = v;
            }
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int e4 = tid + 256 * q;
            const int i = e4 >> 5, j = (e4 & 31) * 4;
            float vv[4] = {ld4[q].x, ld4[q].y, ld4[q].z, ld4[q].w};
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int jj = j + t;
                float x = (i == jj) ? 1.0f : 0.0f;                 // identity padding
                if (i < nb && jj < nb) x = (jj >= i) ? vv[t] : 0.0f;
                vv[t] = x;
            }
            *reinterpret_cast<float4*>(S + i * PLD + j) = make_float4(vv[0], vv[1], vv[2], vv[3]);
        }
        // V needs no initialisation: every block of its upper part is written before it is read
    }
    __syncthreads();
    LLMC_STAMP(1);
    // ---- blocked upper Cholesky over 4 block rows
    for (int kb = 0; kb < 4; ++kb) {
        if (wv == 0) wave_potrf32_inv(PBLK(S, kb, kb), VBLK(kb, kb), rowbuf, lane, k0 + kb * 32, info);
        __syncthreads();
        LLMC_STAMP(2 + 2 * kb);
        {   // panel: S(kb, jb) = V_kk^T * S(kb, jb)
            const int jb = kb + 1 + wv;
            if (jb < 4) {
                f32x16 acc = blk_mm<true>(VBLK(kb, kb), PBLK(S, kb, jb), zero, lane);
                blk_store(PBLK(S, kb, jb), acc, lane, 1.0f);
            }
        }
        __syncthreads();
        {   // trailing: S(ib, jb) -= S(kb, ib)^T * S(kb, jb), kb < ib <= jb
            int idx = 0;
            for (int ib = kb + 1; ib < 4; ++ib)
                for (int jb = ib; jb < 4; ++jb, ++idx)
                    if ((idx & 3) == wv) {
                        f32x16 acc = blk_mm<true>(PBLK(S, kb, ib), PBLK(S, kb, jb), zero, lane);
                        blk_sub(PBLK(S, ib, jb), acc, lane);
                    }
        }
        __syncthreads();
        LLMC_STAMP(3 + 2 * kb);
    }
    // ---- U back to the work matrix (S becomes scratch afterwards)
    if (nb == NB && (ld % 4 == 0) && (k0 % 4 == 0)) {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int e4 = tid + 256 * q;
            const int i = e4 >> 5, j = (e4 & 31) * 4;
            // diagonal blocks hold zeros below the diagonal; blocks below it are about to receive parts of V
            float4 s4 = make_float4(0.f, 0.f, 0.f, 0.f);
            if ((j >> 5) >= (i >> 5)) s4 = *reinterpret_cast<const float4*>(S + i * PLD + j);
            *reinterpret_cast<float4*>(W + (int64_t)(k0 + i) * ld + k0 + j) = s4;
        }
    } else {
        for (int e = tid; e < NB * NB; e += 256) {
            const int i = e >> 7, j = e & 127;
            if (i < nb && j < nb) W[(int64_t)(k0 + i) * ld + k0 + j] = (j >= i) ? S[i * PLD + j] : 0.0f;
        }
    }
    LLMC_STAMP(10);
    // ---- V = U^-1 by doubling. Level 32 -> 64: pairs (0,1) and (2,3)
    if (wv < 2) {
        const int a = 2 * wv, b = a + 1;
        f32x16 x = blk_mm<false>(VBLK(a, a), PBLK(S, a, b), zero, lane);   // X = V_aa * U_ab
        blk_store(VBLK(a, b), x, lane, 1.0f);
        f32x16 y = blk_mm<false>(VBLK(a, b), VBLK(b, b), zero, lane);   // Y = X * V_bb
        blk_store(VBLK(a, b), y, lane, -1.0f);
    }
    __syncthreads();
    // Level 64 -> 128: X = V[0:64,0:64] * U[0:64,64:128] (into V scratch), then -X * V[64:,64:] (into S scratch)
    {
        const int r = wv >> 1, c = 2 + (wv & 1);
        f32x16 x = blk_mm<false>(VBLK(r, r), PBLK(S, r, c), zero, lane);
        if (r == 0) x = blk_mm<false>(VBLK(0, 1), PBLK(S, 1, c), x, lane);
        __syncthreads();  // everyone has read U[0:64,64:128] from S and the level-1 V blocks
        blk_store(VBLK(r, c), x, lane, 1.0f);
    }
    __syncthreads();
    {
        const int r = wv >> 1, c = 2 + (wv & 1);
        f32x16 y = blk_mm<false>(VBLK(r, 2), VBLK(2, c), zero, lane);
        if (c == 3) y = blk_mm<false>(VBLK(r, 3), VBLK(3, 3), y, lane);
        blk_store(PBLK(S, r, c), y, lane, -1.0f);
    }
    __syncthreads();
    LLMC_STAMP(11);
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int e4 = tid + 256 * q;
        const int i = e4 >> 5, j = (e4 & 31) * 4;
        const int bi = i >> 5, bj = j >> 5;
        float4 v4 = make_float4(0.f, 0.f, 0.f, 0.f);
        if (bi == bj) v4 = *reinterpret_cast<const float4*>(Vd + (i & 31) * PLD + j);             // zeros below diag
        else if (bi < 2 && bj >= 2) v4 = *reinterpret_cast<const float4*>(S + i * PLD + j);       // level-2 result
        else if (bi < bj) v4 = *reinterpret_cast<const float4*>(S + (bj * 32 + (i & 31)) * PLD + bi * 32 + (j & 31));
        *reinterpret_cast<float4*>(Vout + i * NB + j) = v4;
    }
    LLMC_STAMP(12);
}
#undef PBLK

// gemm6 skips the zero part of a triangular operand at 256 granularity: the 128 x 128 block below the diagonal inside
// every 256-aligned diagonal tile must really be zero (nothing else reads that part of the work matrix)
__global__ __launch_bounds__(256) void k_zero_subdiag(float* __restrict__ W, int64_t ld, int K) {
    const int r0 = blockIdx.x * 256 + 128, c0 = blockIdx.x * 256;
    for (int e = threadIdx.x; e < 128 * 128; e += 256) {
        const int i = r0 + (e >> 7), j = c0 + (e & 127);
        if (i < K && j < K) W[(int64_t)i * ld + j] = 0.0f;
    }
}

// copy the inverted diagonal blocks into the work matrix (upper), before the doubling levels
__global__ __launch_bounds__(256) void k_place_diag_inv(float* __restrict__ W, int64_t ld, int K,
                                                        const float* __restrict__ Vbuf, int b0) {
    const int b = b0 + blockIdx.x;
    const int k0 = b * NB;
    const int nb = min(NB, K - k0);
    const float* V = Vbuf + (int64_t)b * NB * NB;
    for (int e = threadIdx.x; e < NB * NB; e += 256) {
        int i = e >> 7, j = e & 127;
        if (i < nb && j < nb) W[(int64_t)(k0 + i) * ld + k0 + j] = V[e];
    }
}

// ---------------------------------------------------------------------------------------------
// K2 helpers
// ---------------------------------------------------------------------------------------------
// pass 1: dead fix on the diagonal, dead flags, sum of the fixed diagonal (fixed-order tree: deterministic)
__global__ __launch_bounds__(1024) void k_diag_fix(float* __restrict__ H, int K, uint8_t* __restrict__ dead,
                                                   float* __restrict__ diag_mean) {
    __shared__ double red[1024];
    double s = 0.0;
    for (int i = threadIdx.x; i < K; i += 1024) {
        float d = H[(int64_t)i * K + i];
        uint8_t dd = (d == 0.0f);
        if (dd) {
            d = 1.0f;
            H[(int64_t)i * K + i] = 1.0f;
        }
        dead[i] = dd;
        s += (double)d;
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) *diag_mean = (float)(red[0] / (double)K);
}

// Hout[i][j] = H[perm[i]][perm[j]] + (i == j) * percdamp * mean(diag)
__global__ __launch_bounds__(256) void k_gather_h(const float* __restrict__ H, int K,
                                                  const int64_t* __restrict__ perm, float percdamp,
                                                  const float* __restrict__ diag_mean, float* __restrict__ Hout) {
    const int i = blockIdx.y;
    const int64_t pi = perm ? perm[i] : i;
    const float damp = percdamp * (*diag_mean);
    for (int j = blockIdx.x * 256 + threadIdx.x; j < K; j += gridDim.x * 256) {
        const int64_t pj = perm ? perm[j] : j;
        float v = H[pi * K + pj];
        if (i == j) v += damp;
        Hout[(int64_t)i * K + j] = v;
    }
}

// Wout[r][j] = dead[perm[j]] ? 0 : float(W[r][perm[j]])
template <typename T>
__global__ __launch_bounds__(256) void k_gather_w(const T* __restrict__ W, int64_t R, int K,
                                                  const int64_t* __restrict__ perm,
                                                  const uint8_t* __restrict__ dead, float* __restrict__ Wout) {
    const int64_t r = blockIdx.y;
    for (int j = blockIdx.x * 256 + threadIdx.x; j < K; j += gridDim.x * 256) {
        const int64_t pj = perm ? perm[j] : j;
        float v = dead[pj] ? 0.0f : to_f32<T>(W[r * K + pj]);
        Wout[r * K + j] = v;
    }
}


// LDS-staged gathers (K % 4 == 0, K*4 <= 160 KB, i.e. K <= 40960: a 70B down_proj row, K = 28672, is 112 KB): a workgroup
// reads ONE source row contiguously (16-B loads), keeps it in LDS as fp32, and writes the permuted row contiguously (16-B
// stores) — both HBM streams coalesced; the random access happens in LDS. The element-wise kernels above remain for other
// shapes.
template <typename T> __device__ __forceinline__ float4 load4_f32(const T* p);
template <> __device__ __forceinline__ float4 load4_f32<float>(const float* p) {
    return *reinterpret_cast<const float4*>(p);
}
template <> __device__ __forceinline__ float4 load4_f32<f16_t>(const f16_t* p) {
    const uint2 u = *reinterpret_cast<const uint2*>(p);
    f16_t h[4];
    __builtin_memcpy(h, &u, 8);
    return make_float4(to_f32<f16_t>(h[0]), to_f32<f16_t>(h[1]), to_f32<f16_t>(h[2]), to_f32<f16_t>(h[3]));
}
template <> __device__ __forceinline__ float4 load4_f32<bf16_t>(const bf16_t* p) {
    const uint2 u = *reinterpret_cast<const uint2*>(p);
    bf16_t h[4];
    __builtin_memcpy(h, &u, 8);
    return make_float4(to_f32<bf16_t>(h[0]), to_f32<bf16_t>(h[1]), to_f32<bf16_t>(h[2]), to_f32<bf16_t>(h[3]));
}

// MODE 0: out[r][j] = in[r][idx[j]]                                   (column gather)
// MODE 1: out[r][j] = dead[idx[j]] ? 0 : in[r][idx[j]]                (k_gather_w)
// MODE 2: out[r][j] = in[idx[r]][idx[j]] + (r == j) * damp            (k_gather_h)
// A workgroup handles GATHER_ROWS consecutive output rows and keeps the column indices of its threads in registers across
// them (round 4: with one row per workgroup every row re-read the whole int64 index vector, twice the bytes of the row itself).
static constexpr int GATHER_ROWS = 8;
static constexpr int GATHER_MAXJ = 7;     // 4 * 512 * 7 = 14336 columns per register pass (28 index registers); wider rows take more passes
template <typename T, int MODE>
__global__ __launch_bounds__(512) void k_gather_lds(const T* __restrict__ in, int K, const int64_t* __restrict__ idx,
                                                   const uint8_t* __restrict__ dead, float percdamp,
                                                   const float* __restrict__ diag_mean, float* __restrict__ out, int64_t R) {
    extern __shared__ __attribute__((aligned(16))) float grow[];
    const float damp = MODE == 2 ? percdamp * (*diag_mean) : 0.0f;
    const int64_t r_begin = (int64_t)blockIdx.x * GATHER_ROWS;
    const int64_t r_end = r_begin + GATHER_ROWS < R ? r_begin + GATHER_ROWS : R;
    for (int c_pass = 0; c_pass < K; c_pass += 4 * 512 * GATHER_MAXJ) {
        // this thread's columns of the pass: c = c_pass + 4 * tid + 2048 * j
        int pj[GATHER_MAXJ][4];
        uint32_t deadbits = 0;
#pragma unroll
        for (int j = 0; j < GATHER_MAXJ; ++j) {
            const int c = c_pass + 4 * (int)threadIdx.x + 4 * 512 * j;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                int v = 0;
                if (c < K) {
                    v = idx ? (int)idx[c + t] : c + t;
                    if (MODE == 1 && dead[v]) deadbits |= 1u << (4 * j + t);
                }
                pj[j][t] = v;
            }
        }
        for (int64_t r = r_begin; r < r_end; ++r) {
            const int64_t sr = (MODE == 2 && idx) ? idx[r] : r;
            const T* src = in + sr * K;
            __syncthreads();          // the previous row's gathers are done with the LDS row
            for (int c = 4 * threadIdx.x; c < K; c += 4 * 512) *reinterpret_cast<float4*>(grow + c) = load4_f32<T>(src + c);
            __syncthreads();
#pragma unroll
            for (int j = 0; j < GATHER_MAXJ; ++j) {
                const int c = c_pass + 4 * (int)threadIdx.x + 4 * 512 * j;
                if (c >= K) break;
                float v[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    float x = grow[pj[j][t]];
                    if (MODE == 1 && ((deadbits >> (4 * j + t)) & 1u)) x = 0.0f;
                    if (MODE == 2 && r == c + t) x += damp;
                    v[t] = x;
                }
                *reinterpret_cast<float4*>(out + r * K + c) = make_float4(v[0], v[1], v[2], v[3]);
            }
        }
    }
}

static constexpr int GATHER_LDS_MAX = 160 * 1024;   // the whole LDS of a CU (one workgroup per CU above 80 KB)

template <typename T, int MODE>
static int gather_lds_launch(const T* in, int64_t R, int64_t K, const int64_t* idx, const uint8_t* dead,
                             float percdamp, const float* diag_mean, float* out, hipStream_t st) {
    // rows above 64 KB need the kernel's dynamic-LDS ceiling raised once (per device and instantiation)
    if (K * 4 > 65536)
        if (int rc = ensure_dynamic_lds((const void*)k_gather_lds<T, MODE>, GATHER_LDS_MAX)) return rc;
    hipLaunchKernelGGL((k_gather_lds<T, MODE>), dim3((unsigned)ceil_div64(R, GATHER_ROWS)), dim3(512), (size_t)K * 4, st, in,
                       (int)K, idx, dead, percdamp, diag_mean, out, R);
    LLMC_LAUNCH_CHECK();
    return LLMC_OK;
}
static inline bool gather_lds_ok(int64_t K, const void* in, const void* out, int esz) {
    return K % 4 == 0 && K * 4 <= GATHER_LDS_MAX && ((uintptr_t)in % (4 * esz)) == 0 && ((uintptr_t)out & 15) == 0;
}

}  // namespace llmc

using namespace llmc;

extern "C" int llmc_gather_cols(const float* in, int64_t R, int64_t K, const int64_t* idx, float* out,
                                llmc_stream_t stream) {
    LLMC_REQUIRE(in && idx && out && R > 0 && K > 0, "gather_cols: null/empty argument");
    LLMC_REQUIRE(in != out, "gather_cols: out must not alias in");
    hipStream_t st = (hipStream_t)stream;
    if (gather_lds_ok(K, in, out, 4))
        return gather_lds_launch<float, 0>(in, R, K, idx, nullptr, 0.0f, nullptr, out, st);
    set_last_error_msg("gather_cols: K must be a multiple of 4 with K <= 40960 and 16-byte aligned rows");
    return LLMC_ENOTSUP;
}

extern "C" size_t llmc_hessian_prep_ws_bytes(int64_t K) {
    if (K <= 0) return 0;
    // mean + dead flags, then (16-B aligned) the reversed permutation of llmc_hessian_prep_rev
    return (size_t)(((K + 63) / 64) * 64 + 64) + (size_t)K * 8;
}

namespace llmc {
__global__ __launch_bounds__(256) void k_reverse_perm(const int64_t* __restrict__ perm, int K, int64_t* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < K) out[i] = perm ? perm[K - 1 - i] : (int64_t)(K - 1 - i);
}
}  // namespace llmc

static int hessian_prep_impl(float* H, const void* W, int wdt, int64_t R, int64_t K, const int64_t* perm, float percdamp,
                             float* Hout, float* Wout, void* ws, llmc_stream_t stream, bool rev) {
    LLMC_REQUIRE(H && ws && K > 0, "hessian_prep: null/empty argument");
    LLMC_REQUIRE((W && Wout && R > 0) || (!W && !Wout), "hessian_prep: W and Wout go together");
    LLMC_REQUIRE(dtype_ok(wdt), "hessian_prep: bad dtype");
    LLMC_REQUIRE(Hout != H, "hessian_prep: Hout must not alias H");
    LLMC_REQUIRE(K < (1ll << 31) && R < 65536ll * 32768ll, "hessian_prep: shape too large");
    hipStream_t st = (hipStream_t)stream;
    float* diag_mean = (float*)ws;
    uint8_t* dead = (uint8_t*)ws + 64;
    hipLaunchKernelGGL(k_diag_fix, dim3(1), dim3(1024), 0, st, H, (int)K, dead, diag_mean);
    LLMC_LAUNCH_CHECK();
    int gx = (int)ceil_div64(K, 256 * 4);
    if (Hout) {
        const int64_t* hperm = perm;
        if (rev) {     // the permutation read backwards (identity: K-1 .. 0): Hout comes out reflected across the anti-diagonal
            int64_t* pr = (int64_t*)((char*)ws + (((K + 63) / 64) * 64 + 64));
            hipLaunchKernelGGL(k_reverse_perm, dim3((unsigned)ceil_div64(K, 256)), dim3(256), 0, st, perm, (int)K, pr);
            LLMC_LAUNCH_CHECK();
            hperm = pr;
        }
        if (gather_lds_ok(K, H, Hout, 4)) {
            int rc = gather_lds_launch<float, 2>(H, K, K, hperm, nullptr, percdamp, diag_mean, Hout, st);
            if (rc) return rc;
        } else {
            hipLaunchKernelGGL(k_gather_h, dim3(gx, (unsigned)K), dim3(256), 0, st, (const float*)H, (int)K, hperm,
                               percdamp, (const float*)diag_mean, Hout);
            LLMC_LAUNCH_CHECK();
        }
    }
    if (W && gather_lds_ok(K, W, Wout, wdt == LLMC_F32 ? 4 : 2)) {
        int rc;
        if (wdt == LLMC_F16) rc = gather_lds_launch<f16_t, 1>((const f16_t*)W, R, K, perm, dead, 0.0f, nullptr, Wout, st);
        else if (wdt == LLMC_BF16)
            rc = gather_lds_launch<bf16_t, 1>((const bf16_t*)W, R, K, perm, dead, 0.0f, nullptr, Wout, st);
        else rc = gather_lds_launch<float, 1>((const float*)W, R, K, perm, dead, 0.0f, nullptr, Wout, st);
        return rc;
    }
    // grid.y is limited to 65535: loop over row slabs
    for (int64_t r0 = 0; W && r0 < R; r0 += 32768) {
        int64_t rows = R - r0 < 32768 ? R - r0 : 32768;
        dim3 grid(gx, (unsigned)rows);
        if (wdt == LLMC_F16)
            hipLaunchKernelGGL((k_gather_w<f16_t>), grid, dim3(256), 0, st, (const f16_t*)W + r0 * K, rows, (int)K,
                               perm, (const uint8_t*)dead, Wout + r0 * K);
        else if (wdt == LLMC_BF16)
            hipLaunchKernelGGL((k_gather_w<bf16_t>), grid, dim3(256), 0, st, (const bf16_t*)W + r0 * K, rows, (int)K,
                               perm, (const uint8_t*)dead, Wout + r0 * K);
        else
            hipLaunchKernelGGL((k_gather_w<float>), grid, dim3(256), 0, st, (const float*)W + r0 * K, rows, (int)K,
                               perm, (const uint8_t*)dead, Wout + r0 * K);
        LLMC_LAUNCH_CHECK();
    }
    return LLMC_OK;
}

extern "C" int llmc_hessian_prep(float* H, const void* W, int wdt, int64_t R, int64_t K, const int64_t* perm,
                                 float percdamp, float* Hout, float* Wout, void* ws, llmc_stream_t stream) {
    return hessian_prep_impl(H, W, wdt, R, K, perm, percdamp, Hout, Wout, ws, stream, false);
}

// The same preparation with Hout written index-REVERSED: Hout[i][j] = Hp[K-1-i][K-1-j] (Hp = the permuted, damped matrix
// llmc_hessian_prep writes). For a symmetric H that is Hp reflected across its anti-diagonal — exactly the matrix
// llmc_chol_inv_upper builds first from Hp with a transposing pass over K^2 floats — at no cost: it is the same gather with
// the permutation read backwards. llmc_chol_inv_upper_rev takes it. W is gathered with `perm` as always.
extern "C" int llmc_hessian_prep_rev(float* H, const void* W, int wdt, int64_t R, int64_t K, const int64_t* perm,
                                     float percdamp, float* Hout, float* Wout, void* ws, llmc_stream_t stream) {
    return hessian_prep_impl(H, W, wdt, R, K, perm, percdamp, Hout, Wout, ws, stream, true);
}

static inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// doubling levels of the triangular inverse from this block size on run on the one-wave-per-SIMD GEMM (gemm6_launch)
static constexpr int64_t GEMM6_MIN_H = 4096;
static size_t gemm6_bytes(int64_t K) {
    size_t mx = 0;
    for (int64_t h = NB; h < K; h *= 2)
        if (h >= GEMM6_MIN_H) {
            const size_t b = gemm6_ws_bytes((int)h, (int)h, (int)h);
            if (b > mx) mx = b;
        }
    return align256(mx);
}

// The workspace: the working matrix (unused by the in-place form), the inverted diagonal blocks V, X (the inverse levels' A^-1 C,
// and the bf16 planes of a far update's panel), gemm6's planes. Byte offsets, each 256-B aligned.
struct FactorWs { size_t work, vbuf, xbuf, xbuf_bytes, g6, total; };
static FactorWs factor_ws(int64_t K) {
    FactorWs w{};
    w.vbuf = align256((size_t)K * K * 4);
    w.xbuf = w.vbuf + align256((size_t)ceil_div64(K, NB) * NB * NB * 4);
    w.xbuf_bytes = (size_t)(K / 2 + NB) * (K / 2 + NB) * 4;
    w.g6 = w.xbuf + align256(w.xbuf_bytes);
    w.total = w.g6 + gemm6_bytes(K);
    return w;
}

extern "C" size_t llmc_chol_inv_upper_ws_bytes(int64_t K) { return K <= 0 ? 0 : factor_ws(K).total; }

// The host schedule: DESIGN.md §3 "K3's host schedule". Two-level blocked upper Cholesky Wk = U'^T U' — 128-wide factor steps
// inside 512-wide outer blocks, whose rows beyond the block receive ONE far update with Kd = 512 — then V = U'^-1 by doubling
// levels. Where a step's columns and a far update's rows are cut, and onto which lane, is data (pieces); every kernel computes an
// element the same way whatever the cut, so the factor is bit-identical with or without the helper stream as long as per element
// the updates arrive in step order — which the waits in chol_inv_upper_impl state and tests/test_chol_plan.py replays.
static constexpr int NBO = 4 * NB;
struct Piece { int a0, a1; Lane lane; };      // columns of a factor step, or rows of a far update
// A factor step's columns [c1, K): in one piece on one stream (the split costs two more launches per step and buys nothing there),
// else NEAR (the block's own, which the next step needs) on the chain and FAR (the bulk of a step's work) on the bulk lane.
static int step_pieces(int c1, int oend, int K, bool piped, Piece* p) {
    if (!piped || oend >= K) return p[0] = Piece{c1, K, CHAIN}, 1;
    return p[0] = Piece{c1, oend, CHAIN}, p[1] = Piece{oend, K, BULK}, 2;
}
// An outer block's far update of the rows [oend, K): merged (one stream: one launch less per block, no round of 216 tiles on its
// own), else the NEXT block's rows first, on the chain (its factor steps need them), and the rest on the bulk lane.
static int far_pieces(int oend, int K, bool merged, Piece* p) {
    if (merged || oend + NBO >= K) return p[0] = Piece{oend, K, CHAIN}, 1;
    return p[0] = Piece{oend, oend + NBO, CHAIN}, p[1] = Piece{oend + NBO, K, BULK}, 2;
}

// What every launch's arguments are made from: the buffers, K and the options, read once. The only pointer arithmetic of K3.
struct Level { int64_t h, stride, ldX; int npairs, n2_last; bool x3, g6; };
struct FactorCall {
    float* Wk; float* Vbuf; float* Xbuf; void* G6buf; int K; size_t xbuf_bytes;
    // x3: the large products (far updates, inverse levels >= 512) as split-bf16 products on the 16-bit MFMA pipe (gemm3.hip:
    // fp32-level accuracy, 1.3-1.5x the fp32-MFMA kernel; option k3_fp32). planes: a far update's panel split ONCE into bf16 planes
    bool x3, planes, merge_far, g6;
    float* at(int64_t r, int64_t c) const { return Wk + r * K + c; }
    float* V(int c0) const { return Vbuf + (size_t)(c0 / NB) * NB * NB; }
    static SgemmArgs one(int M, int N, int Kd, int epilogue) {
        SgemmArgs g{};
        g.M = g.M_last = M; g.N = g.N_last = N; g.Kd = g.Kd_last = Kd; g.epilogue = epilogue; g.batch = 1;
        return g;
    }
    // P = V^T P for P = rows [c0, c0 + nb), columns [col0, col1)  (op(A)[i][k] = V[k][i], lower triangular)
    SgemmArgs panel_solve(int c0, int nb, int col0, int col1) const {
        SgemmArgs g = one(nb, col1 - col0, nb, SG_SET);
        g.A = V(c0); g.lda = NB; g.B = g.C = at(c0, col0); g.ldb = g.ldc = K; g.a_lower = 1;
        return g;
    }
    // rows [c0 + nb, oend) of the trailing matrix, columns [col0, col1):  C -= P[:, rows]^T P[:, cols]
    SgemmArgs inblock_update(int c0, int nb, int oend, int col0, int col1) const {
        SgemmArgs u = one(oend - (c0 + nb), col1 - col0, nb, SG_SUB);
        u.A = at(c0, c0 + nb); u.B = at(c0, col0); u.C = at(c0 + nb, col0); u.lda = u.ldb = u.ldc = K;
        u.c_upper_only = col0 == c0 + nb ? 1 : 0;      // the far columns lie right of every row
        return u;
    }
    // rows [r0, r1) of the far update T -= P^T P, P = rows [k0, oend), columns [oend, K): upper triangle, columns [r0, K)
    SgemmArgs far(int k0, int oend, int r0, int r1, bool with_planes) const {
        SgemmArgs u = one(r1 - r0, K - r0, oend - k0, SG_SUB);
        u.A = u.B = at(k0, r0); u.C = at(r0, r0); u.lda = u.ldb = u.ldc = K; u.c_upper_only = 1;
        if (with_planes) {
            u.planesA = u.planesB = (const uint16_t*)Xbuf + (r0 - oend);
            u.ldp = K - oend; u.plane_stride = (int64_t)(oend - k0) * (K - oend);
        }
        return u;
    }
    // the planes of P (in Xbuf, which otherwise only the inverse levels use) are worth it when the last piece would run on them
    bool split_planes(int k0, int oend, int r0) const {
        const int nfar = K - oend;
        return x3 && planes && nfar % 8 == 0 && (size_t)3 * (oend - k0) * nfar * 2 <= xbuf_bytes && gemm3_route(far(k0, oend, r0, K, true), true).planes();
    }
    // level h of V = U'^-1: pairs [[A, C], [0, B]] of h-blocks with a non-empty right block, C = -A^-1 C B^-1 through X = A^-1 C
    Level level(int64_t h) const {
        Level l{h, 2 * h * ((int64_t)K + 1), h, (int)((K - h + 2 * h - 1) / (2 * h)), 0, false, false};
        if (l.npairs <= 0) return l;
        const int64_t rest = K - (int64_t)(l.npairs - 1) * 2 * h - h;
        l.n2_last = (int)(rest < h ? rest : h);
        if (l.npairs == 1) l.ldX = ((l.n2_last + 3) / 4) * 4;      // X is [h x n2]: one pair keeps it within K^2 / 4 floats
        l.x3 = x3 && h >= 512;      // small levels are latency-bound: the fp32 kernels stay
        // large, deep levels: operands split once into stacked bf16 planes, product on the one-wave-per-SIMD GEMM
        l.g6 = l.x3 && g6 && h >= GEMM6_MIN_H && h % 256 == 0 && l.n2_last % 256 == 0;
        return l;
    }
    SgemmArgs level_x(const Level& l) const {      // X = A^-1 C: A^-1 at (o, o), upper, C at (o, o + h)
        SgemmArgs x = one((int)l.h, (int)l.h, (int)l.h, SG_SET);
        x.A = Wk; x.B = Wk + l.h; x.lda = x.ldb = K; x.sA = x.sB = l.stride; x.C = Xbuf; x.ldc = l.ldX; x.sC = l.h * l.h;
        x.N_last = l.n2_last; x.a_upper = 1; x.batch = l.npairs;
        return x;
    }
    SgemmArgs level_c(const Level& l) const {      // C = -X B^-1: B^-1 at (o + h, o + h), upper
        SgemmArgs y = one((int)l.h, (int)l.h, (int)l.h, SG_NEG);
        y.A = Xbuf; y.lda = l.ldX; y.sA = l.h * l.h; y.B = Wk + l.h * ((int64_t)K + 1); y.C = Wk + l.h; y.ldb = y.ldc = K; y.sB = y.sC = l.stride;
        y.N_last = y.Kd_last = l.n2_last; y.b_upper = 1; y.batch = l.npairs;
        return y;
    }
    static SgemmArgs problem(SgemmArgs g, int z) {      // the z-th problem of a batch on its own (gemm6 takes one at a time)
        g.A += z * g.sA; g.B += z * g.sB; g.C += z * g.sC;
        if (z == g.batch - 1) g.M = g.M_last, g.N = g.N_last, g.Kd = g.Kd_last;
        g.batch = 1;
        return g;
    }
};

// One place that either launches or, for a plan, writes down what WOULD be launched: rows of CP_W int32 (include/llmc_hip_test.h),
// every rectangle read back from the pointers and leading dimensions the launch gets.
enum { CP_TRANSPOSE = 0, CP_POTRF = 1, CP_SOLVE = 2, CP_UPDATE = 3, CP_SPLIT = 4, CP_FAR = 7, CP_PLACE = 8, CP_ZERO = 9, CP_INV_X = 10,
       CP_INV_C = 11, CP_W = 22 };
enum { F_KERNEL = 0, F_SGEMM = 1, F_GEMM3 = 2, F_GEMM6 = 3 };
struct Rect { int32_t buf, r0, r1, c0, c1; };      // buf: 0 working matrix, 1 V blocks, 2 X / planes, 3 gemm6 workspace, 4 the caller's other matrix
static const int32_t CP_BLANK[CP_W] = {0, 0, -1, 0, 0, 0, 0, -1, 0, 0, 0, 0, -1, 0, 0, 0, 0, -1, 0, 0, 0, 0};
static constexpr int POTRF_LDS = (NB * PLD + 32 * PLD + 64) * (int)sizeof(float);
static int launched() { LLMC_LAUNCH_CHECK(); return LLMC_OK; }
struct FactorSink {
    const FactorCall& o; const Lanes& ln; PlanRec* rec; const float* other; const char* ws_end; int32_t* info;
    // [rows x cols] floats at p: X and the gemm6 workspace as flat ranges of floats, a wrong leading dimension as buffer -2
    Rect rect(const void* p, int64_t ld, int64_t rows, int64_t cols) const {
        const float* f = (const float*)p;
        if ((const char*)f >= (const char*)o.Xbuf && (const char*)f < ws_end) {
            const bool x = (const void*)f < o.G6buf;
            const int64_t off = f - (x ? o.Xbuf : (const float*)o.G6buf);
            return Rect{x ? 2 : 3, 0, 1, (int32_t)off, (int32_t)(off + (rows - 1) * ld + cols)};
        }
        const bool v = f >= o.Vbuf && f < o.Xbuf, w = f >= o.Wk && f < o.Wk + (size_t)o.K * o.K;
        const int64_t n = v ? NB : o.K, off = f - (v ? o.Vbuf : w ? o.Wk : other);
        return Rect{ld != n ? -2 : v ? 1 : w ? 0 : 4, (int32_t)(off / n), (int32_t)(off / n + rows), (int32_t)(off % n), (int32_t)(off % n + cols)};
    }
    int add(int kind, int form, Lane lane, Rect w, Rect a = Rect{-1}, Rect b = Rect{-1}, Rect w2 = Rect{-1}) const {
        int32_t v[CP_W] = {kind, form};
        memcpy(v + 2, &w, sizeof w), memcpy(v + 7, &a, sizeof a), memcpy(v + 12, &b, sizeof b), memcpy(v + 17, &w2, sizeof w2);
        rec->row(v, ln.lane_of(ln.s[lane]));
        return LLMC_OK;
    }
    int transpose(const float* in, float* out, int upper_only) const {
        if (rec) return add(CP_TRANSPOSE, F_KERNEL, CHAIN, rect(out, o.K, o.K, o.K), rect(in, o.K, o.K, o.K));
        hipLaunchKernelGGL(k_antitranspose, dim3((o.K + 31) / 32, (o.K + 31) / 32), dim3(256), 0, ln.s[CHAIN], in, out, o.K, upper_only);
        return launched();
    }
    int potrf(int c0, int nb) const {      // factors and inverts the diagonal block: rewrites it, writes its V block (and the failure flag)
        float* Vb = o.V(c0);
        if (rec) return add(CP_POTRF, F_KERNEL, CHAIN, rect(o.at(c0, c0), o.K, nb, nb), rect(o.at(c0, c0), o.K, nb, nb), Rect{-1}, rect(Vb, NB, nb, NB));
        hipLaunchKernelGGL(k_potrf_inv, dim3(1), dim3(256), POTRF_LDS, ln.s[CHAIN], o.Wk, (int64_t)o.K, c0, nb, Vb, info);
        return launched();
    }
    // a product: fp32 (sgemm_launch) or split-bf16; the rectangles of a batch are the hull of the first and the last problem
    int product(int kind, const SgemmArgs& g, int form, bool TA, Lane lane) const {
        if (g.M <= 0 || g.N <= 0) return LLMC_OK;
        const hipStream_t st = ln.s[lane];
        if (!rec) return form == F_SGEMM ? sgemm_launch(g, TA, false, st) : gemm3_launch(g, TA, st);
        auto hull = [&](const float* p, int64_t ld, int64_t s, int r, int c, int rl, int cl) {
            const Rect a = rect(p, ld, r, c), b = rect(p + (g.batch - 1) * s, ld, rl, cl);
            return Rect{a.buf, a.r0, b.r1, a.c0, b.c1};
        };
        auto planes = [&](const void* p, int n) { return rect(p, 1, 1, (2 * g.plane_stride + (g.Kd - 1) * g.ldp + n + 1) / 2); };
        const bool pl = form == F_GEMM3 && gemm3_route(g, TA).planes();
        return add(kind, form, lane, hull(g.C, g.ldc, g.sC, g.M, g.N, g.M_last, g.N_last),
                   pl ? planes(g.planesA, g.M) : TA ? hull(g.A, g.lda, g.sA, g.Kd, g.M, g.Kd_last, g.M_last) : hull(g.A, g.lda, g.sA, g.M, g.Kd, g.M_last, g.Kd_last),
                   pl ? planes(g.planesB, g.N) : hull(g.B, g.ldb, g.sB, g.Kd, g.N, g.Kd_last, g.N_last));
    }
    int split(int k0, int oend) const {      // the hi | mid | lo bf16 planes of the far panel P into X
        const int nbo = oend - k0, nfar = o.K - oend;
        if (rec) return add(CP_SPLIT, F_KERNEL, CHAIN, rect(o.Xbuf, 1, 1, ((int64_t)3 * nbo * nfar + 1) / 2), rect(o.at(k0, oend), o.K, nbo, nfar));
        return gemm3_split_planes(o.at(k0, oend), o.K, nbo, nfar, o.Xbuf, nfar, (int64_t)nbo * nfar, ln.s[CHAIN]);
    }
    int gemm6(int kind, const SgemmArgs& g) const {      // one problem: A row-major, B k-major, SG_SET or SG_NEG
        if (rec) return add(kind, F_GEMM6, CHAIN, rect(g.C, g.ldc, g.M, g.N), rect(g.A, g.lda, g.M, g.Kd), rect(g.B, g.ldb, g.Kd, g.N),
                            rect(o.G6buf, 1, 1, (int64_t)(gemm6_ws_bytes(g.M, g.N, g.Kd) / 4)));
        return gemm6_launch(g.A, g.lda, g.B, g.ldb, g.C, g.ldc, g.M, g.N, g.Kd, g.a_upper, g.b_upper, g.epilogue == SG_NEG ? -1.0f : 1.0f,
                            o.G6buf, ln.s[CHAIN]);
    }
    int place_diag() const {      // the inverted diagonal blocks into the working matrix
        const int nblk = (o.K + NB - 1) / NB;
        if (rec) return add(CP_PLACE, F_KERNEL, CHAIN, rect(o.Wk, o.K, o.K, o.K), rect(o.Vbuf, NB, (int64_t)nblk * NB, NB));
        hipLaunchKernelGGL(k_place_diag_inv, dim3(nblk), dim3(256), 0, ln.s[CHAIN], o.Wk, (int64_t)o.K, o.K, (const float*)o.Vbuf, 0);
        return launched();
    }
    int zero_subdiag() const {
        if (rec) return add(CP_ZERO, F_KERNEL, CHAIN, rect(o.Wk, o.K, o.K, o.K));
        hipLaunchKernelGGL(k_zero_subdiag, dim3((o.K + 255) / 256), dim3(256), 0, ln.s[CHAIN], o.Wk, (int64_t)o.K, o.K);
        return launched();
    }
};

static int chol_inv_upper_impl(float* A, float* Uout, int64_t K64, void* ws, int32_t* info_dev, llmc_stream_t stream, PlanRec* rec = nullptr) {
    LLMC_REQUIRE(A && ws && info_dev && K64 > 0, "chol_inv_upper: null/empty argument");
    LLMC_REQUIRE(K64 % 4 == 0 && K64 < (1 << 30), "chol_inv_upper: K must be a multiple of 4");
    LLMC_REQUIRE(((uintptr_t)A & 15) == 0 && ((uintptr_t)ws & 255) == 0, "chol_inv_upper: alignment");
    const int K = (int)K64;
    const bool rev = Uout != nullptr;          // A already holds the reflected matrix: work in it
    const FactorWs l = factor_ws(K);
    char* const w = (char*)ws;
    const FactorCall o{rev ? A : (float*)(w + l.work), (float*)(w + l.vbuf), (float*)(w + l.xbuf), w + l.g6, K, l.xbuf_bytes,
                       !opt(OPT_K3_FP32), !opt(OPT_K3_NO_PLANES), !opt(OPT_K3_SPLIT_FAR), !opt(OPT_K3_NO_GEMM6)};
    Lanes ln((hipStream_t)stream, rec);
    const FactorSink sink{o, ln, rec, rev ? Uout : A, w + l.total, info_dev};
    LLMC_TRY(ln.fork());
    if (!rec) {
        LLMC_HIP_CHECK(hipMemsetAsync(info_dev, 0, 4, ln.s[CHAIN]));
        LLMC_TRY(ensure_dynamic_lds((const void*)k_potrf_inv, POTRF_LDS));
    }
    if (!rev) LLMC_TRY(sink.transpose(A, o.Wk, 0));
    Piece pc[2];
    Ev planes_read{};      // bulk: the far update that read the planes in X is complete (they may be rewritten)
    for (int k0 = 0; k0 < K; k0 += NBO) {
        const int oend = k0 + NBO < K ? k0 + NBO : K;
        for (int c0 = k0; c0 < oend; c0 += NB) {
            const int nb = K - c0 < NB ? K - c0 : NB;
            LLMC_TRY(sink.potrf(c0, nb));
            if (c0 + nb >= K) break;
            // the chain piece's update goes last: the bulk piece is on its way before the chain goes on to the next step
            const int np = step_pieces(c0 + nb, oend, K, ln.piped(), pc);
            LLMC_TRY(sink.product(CP_SOLVE, o.panel_solve(c0, nb, pc[0].a0, pc[0].a1), F_SGEMM, true, CHAIN));
            if (np > 1) {
                LLMC_TRY(ln.order(CHAIN, BULK));      // this step's near panel is complete (the far update of the step reads it)
                LLMC_TRY(sink.product(CP_SOLVE, o.panel_solve(c0, nb, pc[1].a0, pc[1].a1), F_SGEMM, true, BULK));
                LLMC_TRY(sink.product(CP_UPDATE, o.inblock_update(c0, nb, oend, pc[1].a0, pc[1].a1), F_SGEMM, true, BULK));
            }
            LLMC_TRY(sink.product(CP_UPDATE, o.inblock_update(c0, nb, oend, pc[0].a0, pc[0].a1), F_SGEMM, true, CHAIN));
        }
        if (oend >= K) break;
        // the block's far panels are complete (behind them on the in-order bulk lane: the previous block's update of these rows)
        LLMC_TRY(ln.order(BULK, CHAIN));
        const int np = far_pieces(oend, K, !ln.piped() && o.x3 && o.merge_far, pc);
        const bool planes = o.split_planes(k0, oend, pc[np - 1].a0);
        if (planes) {
            // the planes the previous block's update reads are free (implied today by the wait above — stated all the same)
            LLMC_TRY(ln.wait(CHAIN, planes_read));
            LLMC_TRY(sink.split(k0, oend));
        }
        for (int i = 0; i < np; ++i) {
            // the bulk piece goes behind the chain's: the planes are split there, and the rows the next block's steps need go first
            if (pc[i].lane == BULK) LLMC_TRY(ln.order(CHAIN, BULK));
            LLMC_TRY(sink.product(CP_FAR, o.far(k0, oend, pc[i].a0, pc[i].a1, planes), o.x3 ? F_GEMM3 : F_SGEMM, true, pc[i].lane));
            if (pc[i].lane == BULK) LLMC_TRY(ln.record(BULK, &planes_read));
        }
    }
    // ---- V = U'^-1: inverted diagonal blocks, then doubling levels. Nothing is left on the bulk lane: the last block with a far
    // update has no piece there
    LLMC_TRY(sink.place_diag());
    if (o.x3 && o.g6 && K > GEMM6_MIN_H) LLMC_TRY(sink.zero_subdiag());
    for (int64_t h = NB; h < K; h *= 2) {
        const Level lv = o.level(h);
        if (lv.npairs <= 0) break;
        for (int z = 0; lv.g6 && z < lv.npairs; ++z) {
            LLMC_TRY(sink.gemm6(CP_INV_X, o.problem(o.level_x(lv), z)));
            LLMC_TRY(sink.gemm6(CP_INV_C, o.problem(o.level_c(lv), z)));
        }
        if (lv.g6) continue;
        LLMC_TRY(sink.product(CP_INV_X, o.level_x(lv), lv.x3 ? F_GEMM3 : F_SGEMM, false, CHAIN));
        LLMC_TRY(sink.product(CP_INV_C, o.level_c(lv), lv.x3 ? F_GEMM3 : F_SGEMM, false, CHAIN));
    }
    LLMC_TRY(sink.transpose(o.Wk, rev ? Uout : A, 1));
    return ln.join();
}

extern "C" int llmc_chol_inv_upper(float* A, int64_t K64, void* ws, int32_t* info_dev, llmc_stream_t stream) {
    return chol_inv_upper_impl(A, nullptr, K64, ws, info_dev, stream);
}

// The same factor from the index-reversed matrix llmc_hessian_prep_rev writes: Arev is factored IN PLACE (destroyed) and U is
// written to Uout (must not alias Arev): no transposing pass in front of the factorisation. Same workspace size as
// llmc_chol_inv_upper; same kernels in the same order on the same values: U is bit-identical to llmc_chol_inv_upper's on the
// un-reversed matrix whenever that matrix is exactly symmetric (every Hessian of this library is).
extern "C" int llmc_chol_inv_upper_rev(float* Arev, float* Uout, int64_t K64, void* ws, int32_t* info_dev, llmc_stream_t stream) {
    LLMC_REQUIRE(Uout && Uout != Arev && ((uintptr_t)Uout & 15) == 0, "chol_inv_upper_rev: Uout must be a separate 16-B aligned buffer");
    return chol_inv_upper_impl(Arev, Uout, K64, ws, info_dev, stream);
}

// Test hook (include/llmc_hip_test.h): K3's launch plan for this K under the calling thread's options, without a device.
extern "C" int llmc_test_chol_plan(int64_t K, int rev, int with_lanes, int32_t* out, int cap) {
    LLMC_REQUIRE(out && cap >= 0, "chol plan: null output");
    PlanRec rec{out, cap, 0, CP_W, with_lanes != 0, CP_BLANK};
    // addresses that are only ever offset and compared, never read: 256-B aligned like device allocations, far apart
    float* const base = (float*)(uintptr_t)((uint64_t)1 << 40);
    const size_t span = (size_t)1 << 36;
    const int rc = chol_inv_upper_impl(base, rev ? base + span : nullptr, K, base + 2 * span, (int32_t*)(base + 3 * span), nullptr, &rec);
    return rc ? rc : rec.n;
}
