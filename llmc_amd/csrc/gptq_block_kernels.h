// gptq_block_kernels.h — the in-block kernels of GPTQ's column loop (k_gptq_block, k_gptq_block_riders) and their launch, as
// templates over the step's quantizer kind. One translation unit per kind instantiates them — gptq_loop.hip the integer grid,
// gptq_loop_e4m3.hip and gptq_loop_e5m2.hip the FP8 grids — so the 27 unrolled kernels compile side by side and the integer
// ones from exactly the text they always had. The algorithm is described at the top of gptq_loop.hip.
#pragma once
#include <stdlib.h>
#include "common.h"
#include "quant_math.h"
#include "fp8_math.h"
#include "sgemm.h"
#include "sgemm_wide_tile.h"

namespace llmc {

static constexpr int BS = 128;  // GPTQ blocksize

template <int PO> __device__ __forceinline__ float group_bcast(float v) {
    // lane' = (lane & 0x10) | PO inside each 32-lane half: broadcast of lane PO of every 16-lane group
    return __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), 0x10 | (PO << 5)));
}

struct GptqBlockArgs {
    const float* W;       // [R, K] running weights (panel read at cols i1..i1+count)
    const float* U;       // [K, K] upper factor
    float* Wout;          // [R, K] tmp
    float* losses;        // [R, K] or null
    float* Err;           // err of this block, c < 128: Err[row * err_ld + c], or k-major (err_kmajor) Err[c * err_ld + row]
    int err_ld;
    int err_kmajor;
    float* scales;        // [R, ng]
    float* zeros;         // [R, ng] or null (sym static)
    const int32_t* col_group;  // [K] group of processed column (static mode), or null: group (i1 + c) / col_gsz
    int col_gsz;          // static mode without col_group: processing-order groups (per_channel: 1 << 30, group 0)
    int64_t R;
    int K;
    int i1;
    int count;            // columns in this block (<= 128)
    int ng;               // groups per row in scales/zeros
    int gsz;              // dynamic mode: group size (<= 128, divides 128); static mode: unused
    int static_mode;      // 0: qparams from current W at group starts; 1: given, gathered by col_group
    int sym;
    float qmin, qmax;
};

// The quantizer of a column step, a compile-time parameter of the step: the integer grid clamp(rint(w / s) + z, qmin, qmax), or a
// FloatQuantizer grid (quant.py:1061-1081 with use_qtorch, sym, zeros = tensor(0.)): float_quantize(w / s + 0, E, M) * s.
enum QKind { QK_INT = 0, QK_E4M3 = 1, QK_E5M2 = 2 };

// FloatQuantizer.quant_dequant on one element, the reference's ops in order: scales[scales == 0] = 1; w / s; + zeros (0: -0 becomes
// +0); float_quantize; (- zeros) * s.
template <int KIND> __device__ __forceinline__ float float_qdq(float w, float s) {
    const float s1 = (s == 0.0f) ? 1.0f : s;
    float t = w / s1;
    t = t + 0.0f;
    const float v = KIND == QK_E4M3 ? qtorch_quantize<4, 3>(t) : qtorch_quantize<5, 2>(t);
    return (v - 0.0f) * s1;
}

template <int I> struct StepIdx {
    static constexpr int PO = I & 15;
    static constexpr int EO = I >> 4;
};

// one column step, I compile-time
template <int I, int KIND>
__device__ __forceinline__ void gptq_step(float (&w)[8], const float (&w0)[8], float (&er)[8], float (&ls)[8],
                                          float (&sc)[8], float (&zr)[8], const float* __restrict__ us,
                                          float d, int p, float& s_cur, float& z_cur, const GptqBlockArgs& a) {
    constexpr int PO = StepIdx<I>::PO, EO = StepIdx<I>::EO;
    // ---- group start (dynamic mode). The reference takes min/max from W[:, i:i+g] (gptq.py:216), which
    // inside a block still holds the values the block STARTED with (only the clone W1 receives the
    // in-block updates), hence w0 and not w for groups that start mid-block (group_size < 128).
    if (!a.static_mode && (I % 16 == 0)) {
        if ((I % a.gsz) == 0) {
            float mn = INFINITY, mx = -INFINITY;
            const int e1 = (I + a.gsz) >> 4;  // gsz is a multiple of 16
#pragma unroll
            for (int e = EO; e < 8; ++e)
                if (e < e1 && p + 16 * e < a.count) {
                    mn = fminf(mn, w0[e]);
                    mx = fmaxf(mx, w0[e]);
                }
            mn = wave_min(mn, 16);
            mx = wave_max(mx, 16);
            QParams q = qparams_from_minmax(mn, mx, LLMC_F32, a.sym, 1, a.qmin, a.qmax);
            s_cur = q.s;
            z_cur = q.z;
        }
    }
    float wi = group_bcast<PO>(w[EO]);
    float s = s_cur, z = z_cur;
    if (a.static_mode) {
        s = group_bcast<PO>(sc[EO]);
        if (KIND == QK_INT) z = group_bcast<PO>(zr[EO]);
    }
    float q;
    if constexpr (KIND == QK_INT) {
        const float qc = quant_code(wi, s, z, LLMC_F32, LLMC_F32, a.qmin, a.qmax);
        q = dequant_code(qc, s, z, LLMC_F32);
    } else {
        q = float_qdq<KIND>(wi, s);
    }
    const float diff = wi - q;
    const float err = diff / d;
    if (p == PO) {
        er[EO] = err;
        ls[EO] = (diff * diff) / (2.0f * (d * d));
    }
#pragma unroll
    for (int e = EO; e < 8; ++e) {
        const float u = us[I * BS + e];
        const float t = err * u;
        w[e] = w[e] - t;
    }
}

template <int I0, int KIND>
__device__ __forceinline__ void gptq_steps16(float (&w)[8], const float (&w0)[8], float (&er)[8], float (&ls)[8],
                                             float (&sc)[8], float (&zr)[8], const float* __restrict__ us,
                                             const float* __restrict__ dg, int p, float& s_cur, float& z_cur,
                                             const GptqBlockArgs& a) {
#define LLMC_STEP(J)                                                                         \
    if (I0 + J < a.count) gptq_step<I0 + J, KIND>(w, w0, er, ls, sc, zr, us, dg[I0 + J], p, s_cur, z_cur, a);
    LLMC_STEP(0) LLMC_STEP(1) LLMC_STEP(2) LLMC_STEP(3) LLMC_STEP(4) LLMC_STEP(5) LLMC_STEP(6) LLMC_STEP(7)
    LLMC_STEP(8) LLMC_STEP(9) LLMC_STEP(10) LLMC_STEP(11) LLMC_STEP(12) LLMC_STEP(13) LLMC_STEP(14) LLMC_STEP(15)
#undef LLMC_STEP
}


// ---------------------------------------------------------------------------------------------------------
// Fast in-block path (count == 128). The serial chain of a column step is what bounds this kernel (one wave
// per SIMD at R = 4096), so the chain is cut to ~22 dependent VALU ops:
//   * the two IEEE divisions (w / scale and diff / d) divide by values that are fixed for many steps, so
//     the reciprocal refinement  y = rcp(d) * (2 - d * rcp(d))  is hoisted (per column for d, per group for
//     the scale) and each quotient is the remaining 5 ops of the very sequence hipcc emits for `n / d`
//     (mul, fma, fma, fma, div_fmas == fma).  That sequence first passes n and d through v_div_scale_f32,
//     which is the identity when both are "plain" (2^-40 <= |x| < 2^40, see the ISA's scaling rules), and
//     ends in v_div_fixup_f32, which only acts on zero / inf / nan / denormal operands.  Every numerator
//     of the block is still in registers after the loop (w[] holds each column's value at the time it was
//     visited, df[] each diff), so ONE check after the 128 steps proves all operands were plain (+0 counts:
//     the 5-op chain returns +0 for it, like the division); a wave that saw anything else (-0, tiny, huge,
//     inf, nan) discards its work and redoes the block with the generic path below, so results are
//     bit-identical by construction, not by argument.
//   * the broadcast of the current column is a DPP row_newbcast (VALU latency) instead of an LDS swizzle;
//   * the U row, d and 1/d of a step do not depend on the chain and are read from LDS ahead of it; there is
//     no control flow inside the 128 steps, the losses are evaluated after the loop.
template <int PO> __device__ __forceinline__ float row_bcast(float v) {
    // row_newbcast:PO (gfx90a+): every lane of a 16-lane row reads lane PO of its row
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x150 + PO, 0xf, 0xf, false));
}
// plain numerator: 2^-40 <= |x| < 2^40, or +0
__device__ __forceinline__ bool plain_num(float x) {
    const uint32_t b = __float_as_uint(x);
    return ((b & 0x7fffffffu) - 0x2B800000u) < 0x28000000u || b == 0u;
}
// One step. (u, dd) were loaded during the previous step; this step loads (un, ddn) for the next one first.
template <int I, bool STATIC, int KIND>
__device__ __forceinline__ void fast_step(float (&w)[8], float (&er)[8], float (&df)[8], const float (&sc)[8],
                                          const float (&zr)[8], const float (&ys)[8],
                                          const float* __restrict__ us, const float2* __restrict__ dtab, int p,
                                          float s_cur, float z_cur, float y_cur, float qmin, float qmax,
                                          const float (&u)[8], const float2& dd, float (&un)[8],
                                          float2& ddn) {
    constexpr int PO = StepIdx<I>::PO, EO = StepIdx<I>::EO;
    if (I + 1 < BS) {
        constexpr int EN = StepIdx<I + 1>::EO;
#pragma unroll
        for (int e = EN; e < 8; ++e) un[e] = us[(I + 1) * BS + e];
        ddn = dtab[I + 1];
    }
    float s = s_cur, z = z_cur, y = y_cur;
    if (STATIC) {
        s = row_bcast<PO>(sc[EO]);
        if (KIND == QK_INT) z = row_bcast<PO>(zr[EO]);
        y = row_bcast<PO>(ys[EO]);
    }
    const float wi = row_bcast<PO>(w[EO]);
    float t = div_tail(wi, s, y);                   // quant_code(): x / s; plain s > 0, y = rcp_refined(s), wi a plain numerator
    float q;
    if constexpr (KIND == QK_INT) {
        t = rintf(t);
        t = t + z;
        const float qc = fminf(fmaxf(t, qmin), qmax);
        q = (qc - z) * s;                           // dequant_code()
    } else {
        // float_qdq() for a plain s and a plain numerator: s != 0; the quotient is finite and never -0, so "+ zeros" is the
        // identity; the rounding without control flow (fp8_math.h)
        q = (KIND == QK_E4M3 ? qtorch_select_finite<4, 3>(t) : qtorch_select_finite<5, 2>(t)) * s;
    }
    const float diff = wi - q;
    const float err = div_tail(diff, dd.x, dd.y);
    const bool own = p == PO;
    er[EO] = own ? err : er[EO];
    df[EO] = own ? diff : df[EO];
    // pin the two selects here: left alone, the optimiser turns the 16-deep select chains into a private array
    // indexed by p after the loop, which keeps all 256 err / diff values alive (spills)
    asm volatile("" : "+v"(er[EO]), "+v"(df[EO]));
    // w[e] -= fl(err * u[e]) for e >= EO, two columns per packed instruction where a pair is whole
    typedef float v2f __attribute__((ext_vector_type(2)));
    if (EO & 1) {
        const float tt = err * u[EO];
        w[EO] = w[EO] - tt;
    }
#pragma unroll
    for (int e = (EO + 1) & ~1; e < 8; e += 2) {
        const v2f uu = {u[e], u[e + 1]};
        v2f ww = {w[e], w[e + 1]};
        const v2f tt = uu * err;
        ww = ww - tt;
        w[e] = ww.x;
        w[e + 1] = ww.y;
    }
    __builtin_amdgcn_sched_barrier(0);   // keep the scheduler from hoisting later steps' loads (register blow-up)
}

template <int I0, bool STATIC, int KIND>
__device__ __forceinline__ void fast_steps16(float (&w)[8], float (&er)[8], float (&df)[8], const float (&sc)[8],
                                             const float (&zr)[8], const float (&ys)[8],
                                             const float* __restrict__ us, const float2* __restrict__ dtab,
                                             int p, float s_cur, float z_cur, float y_cur, float qmin,
                                             float qmax, float (&ua)[8], float2& da, float (&ub)[8],
                                             float2& db) {
#define LLMC_FSTEP2(J)                                                                                        \
    fast_step<I0 + J, STATIC, KIND>(w, er, df, sc, zr, ys, us, dtab, p, s_cur, z_cur, y_cur, qmin, qmax, ua, da, \
                              ub, db);                                                                        \
    fast_step<I0 + J + 1, STATIC, KIND>(w, er, df, sc, zr, ys, us, dtab, p, s_cur, z_cur, y_cur, qmin, qmax, ub, \
                                  db, ua, da);
    LLMC_FSTEP2(0) LLMC_FSTEP2(2) LLMC_FSTEP2(4) LLMC_FSTEP2(6) LLMC_FSTEP2(8) LLMC_FSTEP2(10) LLMC_FSTEP2(12)
    LLMC_FSTEP2(14)
#undef LLMC_FSTEP2
}

// Whole block for one wave (4 rows); returns false (and stores nothing) if any lane met a non-plain operand.
template <bool STATIC, int GSZ, int KIND>
__device__ __forceinline__ bool block_fast(const GptqBlockArgs& a, const float* __restrict__ Us,
                                           const float2* __restrict__ dtab, int p, int64_t row, bool active) {
    const int64_t rr = active ? row : a.R - 1;
    float w[8], w0[8], er[8], df[8], sc[8], zr[8], ys[8];
    bool bad = false;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int c = p + 16 * e;
        w[e] = a.W[rr * a.K + a.i1 + c];
        w0[e] = w[e];
        er[e] = 0.0f;
        df[e] = 0.0f;
        sc[e] = 1.0f;
        zr[e] = 0.0f;
        ys[e] = 1.0f;
        if (STATIC) {
            const int g = a.col_group ? a.col_group[a.i1 + c] : (a.i1 + c) / a.col_gsz;
            sc[e] = a.scales[rr * a.ng + g];
            zr[e] = a.zeros ? a.zeros[rr * a.ng + g] : 0.0f;
            ys[e] = rcp_refined(sc[e]);
            bad |= !plain_pos(sc[e]);
        }
    }
    float s_cur = 1.0f, z_cur = 0.0f, y_cur = 1.0f;
    float s_grp[8], z_grp[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        s_grp[e] = 0.0f;
        z_grp[e] = 0.0f;
    }
    const float* us = Us + p * 8;
    float ua[8], ub[8];
    float2 da = dtab[0], db = da;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        ua[e] = us[e];
        ub[e] = 0.0f;
    }
#define LLMC_FCHUNK(E)                                                                                 \
    if (!STATIC && ((16 * E) % GSZ) == 0) {                                                            \
        float mn = INFINITY, mx = -INFINITY;                                                           \
        constexpr int e1 = (16 * E + GSZ) >> 4;                                                        \
        _Pragma("unroll") for (int e = E; e < 8; ++e) if (e < e1) {                                    \
            mn = fminf(mn, w0[e]);                                                                     \
            mx = fmaxf(mx, w0[e]);                                                                     \
        }                                                                                              \
        mn = wave_min(mn, 16);                                                                         \
        mx = wave_max(mx, 16);                                                                         \
        const QParams qp = qparams_from_minmax(mn, mx, LLMC_F32, a.sym, 1, a.qmin, a.qmax);            \
        s_cur = qp.s;                                                                                  \
        z_cur = qp.z;                                                                                  \
        y_cur = rcp_refined(s_cur);                                                                    \
        bad |= !plain_pos(s_cur);                                                                      \
    }                                                                                                  \
    fast_steps16<16 * E, STATIC, KIND>(w, er, df, sc, zr, ys, us, dtab, p, s_cur, z_cur, y_cur, a.qmin, a.qmax, \
                                 ua, da, ub, db);                                                      \
    s_grp[E] = s_cur;                                                                                  \
    z_grp[E] = z_cur;
    LLMC_FCHUNK(0) LLMC_FCHUNK(1) LLMC_FCHUNK(2) LLMC_FCHUNK(3) LLMC_FCHUNK(4) LLMC_FCHUNK(5) LLMC_FCHUNK(6)
    LLMC_FCHUNK(7)
#undef LLMC_FCHUNK
#pragma unroll
    for (int e = 0; e < 8; ++e) bad |= !plain_num(w[e]) | !plain_num(df[e]);
    if (__any(bad)) return false;
    if (!active) return true;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int c = p + 16 * e;
        a.Wout[row * a.K + a.i1 + c] = w[e];
        if (a.losses) {
            const float d = dtab[c].x;
            a.losses[row * a.K + a.i1 + c] = (df[e] * df[e]) / (2.0f * (d * d));
        }
        a.Err[a.err_kmajor ? (int64_t)c * a.err_ld + row : (int64_t)row * a.err_ld + c] = er[e];
    }
    if (!STATIC && p == 0) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int i = 16 * e;
            if ((i % GSZ) == 0) {
                const int g = (a.i1 + i) / GSZ;
                a.scales[row * a.ng + g] = s_grp[e];
                if (a.zeros) a.zeros[row * a.ng + g] = z_grp[e];
            }
        }
    }
    return true;
}

static constexpr int GBT = 512;  // threads per workgroup: 8 waves x 4 rows (1024 for tall weights, see launch)

// VARIANT: 0 generic path only; 1 fast path for given qparams (static groups / per-channel); 16/32/64/128 fast
// path for qparams taken at group starts with that group size. The fast variants fall back to the generic code
// per wave. KIND: the step's quantizer (QKind).
template <int VARIANT, int NT, int KIND = QK_INT>
__global__ __launch_bounds__(NT) void k_gptq_block(GptqBlockArgs a) {
    __shared__ __attribute__((aligned(16))) float Us[BS * BS];
    __shared__ float dg[BS];
    __shared__ float2 dtab[BS];
    __shared__ int d_not_plain;
#include "gptq_block_body.h"
}

// ---------------------------------------------------------------------------------------------------------
// The in-block kernel with RIDERS: one grid, two roles chosen by blockIdx, no data shared between them inside a launch.
//   chain role  (blockIdx < nchain): exactly k_gptq_block<VARIANT, 512> on group g + 1's block (its columns, ErrBuf[(g+1) % 3]);
//   rider role  (the rest): ONE queued 128 x 128 tile of group g's far update (columns beyond group g + 1, ErrBuf[g % 3], read-only
//                rows of U), two of its four 128-k phases, on the workgroup's first four waves — exactly k_sgemm_wide<2>'s tile
//                (sgemm_wide_tile.h): one accumulator per element and phase, ascending k from +0 on v_mfma_f32_32x32x2_f32, one
//                rounding C - acc per phase, the C tile in registers over the launch's phases. The other four waves end at once
//                (a barrier counts the surviving waves only).
// A launch is as long as its longest workgroup, and the chain role takes 24-28 us. Measured on down_proj's chain alone (profiles/
// NOTES.md, chain riders): two whole tiles per CU share its MFMA pipes and take 64-70 us (the launch: 69 us); one whole tile 37-39 us
// (launch 39 us); one tile's two phases 26-27 us (launch 27 us) — hence one tile per CU, cut along k into RIDER_PASSES slices of
// whole phases that different launches carry: the C tile goes to memory and comes back in between (fp32: exact), per element the
// same chain. 72 KiB of LDS, the chain role uses the first 66 KiB. The chain workgroups have the lowest indices: they are
// dispatched first, the riders take the CUs the chain leaves free (the host sizes the grid: one tile per free CU). Workgroup b
// runs on XCD b % 8: where the counts allow, an XCD's riders are `per` = tm / 8 consecutive tile rows of every tile column of the
// launch (`per` A panels and the launch's few B panels in that XCD's L2).
struct RiderArgs {
    wide::WideArgs w;     // this launch's slice of the previous group's far update: whole tile columns, whole phases
    int nchain;           // chain-role workgroups
    int per;              // tile rows per XCD (nchain % 8 == 0, tm % 8 == 0), or 0: tiles in column-major order
};
static constexpr int RIDER_LDS = wide::Wide<2>::LDS;     // 73728
static constexpr int RIDER_PASSES = 2;                    // k slices of a rider tile (divides GRP = 4 phases and the 4 carrying launches)

template <int VARIANT, int KIND = QK_INT>
__global__ __launch_bounds__(GBT) void k_gptq_block_riders(GptqBlockArgs a, RiderArgs r) {
    extern __shared__ __attribute__((aligned(16))) char smem_r[];
    if ((int)blockIdx.x < r.nchain) {
        constexpr int NT = GBT;
        float* Us = reinterpret_cast<float*>(smem_r);
        float* dg = Us + BS * BS;
        float2* dtab = reinterpret_cast<float2*>(dg + BS);
        int& d_not_plain = *reinterpret_cast<int*>(dtab + BS);
#include "gptq_block_body.h"
        return;
    }
    if (threadIdx.x >= 256) return;
    const int rw = (int)blockIdx.x - r.nchain;
    int ti = rw % r.w.tm, tj = rw / r.w.tm;
    if (r.per) {
        const int q = rw >> 3;
        ti = (rw & 7) * r.per + q % r.per;
        tj = q / r.per;
    }
    wide::wide_tile<2>(r.w, ti, tj, smem_r, (int)threadIdx.x);
}


// The in-block kernel of block a.i1 for one quantizer kind on stream st: with the rider tiles `ra` if any, else with 1024- or
// 512-thread workgroups. variant: the VARIANT of k_gptq_block.
template <int KIND>
static int launch_in_block(const GptqBlockArgs& a, int variant, int nt, int grid, const RiderArgs* ra, hipStream_t st) {
    switch (variant) {
#define LLMC_GB(V)                                                                                                          \
    case V:                                                                                                                 \
        if (ra) {                                                                                                           \
            if (int rc = ensure_dynamic_lds((const void*)k_gptq_block_riders<V, KIND>, RIDER_LDS)) return rc;               \
            hipLaunchKernelGGL((k_gptq_block_riders<V, KIND>), dim3(grid + ra->w.tm * ra->w.tn), dim3(GBT), RIDER_LDS, st, a, *ra); \
        } else if (nt == 1024) {                                                                                            \
            hipLaunchKernelGGL((k_gptq_block<V, 1024, KIND>), dim3(grid), dim3(1024), 0, st, a);                            \
        } else {                                                                                                            \
            hipLaunchKernelGGL((k_gptq_block<V, GBT, KIND>), dim3(grid), dim3(GBT), 0, st, a);                              \
        }                                                                                                                   \
        break;
        LLMC_GB(0) LLMC_GB(1) LLMC_GB(128)
#undef LLMC_GB
    }
    LLMC_LAUNCH_CHECK();
    return LLMC_OK;
}
// the FP8 kinds' launches, compiled in their own translation units
int gptq_launch_in_block_e4m3(const GptqBlockArgs& a, int variant, int nt, int grid, const RiderArgs* ra, hipStream_t st);
int gptq_launch_in_block_e5m2(const GptqBlockArgs& a, int variant, int nt, int grid, const RiderArgs* ra, hipStream_t st);

}  // namespace llmc
