// quant_group.h — what every kernel of the IntegerQuantizer builds from quant_math.h's scalar ops, stated once: the container of
// an output kind, the step of one quantization group (min / max or given qparams -> hoisted divisor -> code or fake value) and the
// workgroup's min / max. quant_math.h is the arithmetic; this is how a group runs it. The 16-byte vector of a lane is vec16.h's.
// Users: k_quant_static, k_quant_dynamic_small, k_minmax_partial, k_minmax_final (quant_kernels.hip), k_cols_tile, k_cols_apply
// (quant_cols.hip; k_cols_partial takes vec16.h's vector only), k_mixed_mask, k_mixed_idx (mixed_quant.hip; they spell the code /
// fake select themselves), k_osplus_act_step (smooth_osplus.hip). quant_rows (quant_kernels.hip) takes Vec, out_elem and the
// scalar form of quant_vec, not GroupQuant. Each exception is measured: profiles/quant_group_refactor.txt.
#pragma once
#include "common.h"
#include "quant_math.h"
#include "vec16.h"

namespace llmc {

// what a kernel of output kind KIND writes per element: fake values in the tensor dtype, or codes in KIND's container
template <int KIND, typename T> struct out_elem;
template <typename T> struct out_elem<LLMC_OUT_FAKE, T> { using type = T; };
template <typename T> struct out_elem<LLMC_OUT_I32, T> { using type = int32_t; };
template <typename T> struct out_elem<LLMC_OUT_I8, T> { using type = int8_t; };
template <typename T> struct out_elem<LLMC_OUT_U8, T> { using type = uint8_t; };

// ---- the quantizer of one group -------------------------------------------------------------------------------------------------
// s, z: the group's qparams (dequant's); dv: the hoisted divisor of quant; p1 = promote(wdt, sdt), p2 = promote(p1, zdt).
// FZ: the kernel serves the reference's round_zp = False branch too (quant.py:702-707: round(x / s.clamp_min(1e-9) + z), the
// ABI's LLMC_FRACTIONAL_ZP); `fz` then says at run time whether this group takes it: dv is the divisor of the CLAMPED scale and
// the zero point is added before the rounding. A kernel with FZ = false carries no such select and must not be given a
// fractional zero point: its host refuses round_zp = 0 where it quantizes (llmc_quant_dynamic).
template <bool FZ = false> struct GroupQuant {
    float s, z;
    Divisor dv;
    int p1, p2;
    bool fz;

    // the scalar 1e-9 is cast to the scale's dtype `sd`, like every scalar operand
    __device__ __forceinline__ static float clamped_scale(float s, int sd) { return fmaxf(s, rnd(1e-9f, sd)); }

    // the dynamic kernels: get_qparams of the group's min / max, which are values of the tensor dtype dt
    __device__ __forceinline__ static GroupQuant from_minmax(float mn, float mx, int dt, int sym, int round_zp, float qmin,
                                                             float qmax) {
        const QParams q = qparams_from_minmax(mn, mx, dt, sym, round_zp, qmin, qmax);
        GroupQuant g;
        g.s = q.s;
        g.z = q.z;
        g.p1 = g.p2 = dt;
        g.fz = FZ && !round_zp;
        g.dv = make_divisor(!g.fz ? q.s : clamped_scale(q.s, dt), fmaxf(fabsf(mn), fabsf(mx)));
        return g;
    }
    // given qparams (llmc_quant_static): sdt / zdt are the ABI's words, a dtype in the low bits. LLMC_SCALAR_QPARAM: a 0-dim
    // operand keeps its own precision but does not take part in type promotion. absmax: a bound of |x| over the elements that
    // this value of the struct will divide (a thread's own will do).
    __device__ __forceinline__ static GroupQuant from_qparams(float s, float z, bool has_zeros, int wdt, int sdt, int zdt,
                                                              float absmax) {
        GroupQuant g;
        g.s = s;
        g.z = z;
        g.p1 = (sdt & LLMC_SCALAR_QPARAM) ? wdt : promote(wdt, sdt & 3);
        g.p2 = (has_zeros && !(zdt & LLMC_SCALAR_QPARAM)) ? promote(g.p1, zdt & 3) : g.p1;
        g.fz = FZ && (zdt & LLMC_FRACTIONAL_ZP) != 0;
        g.dv = make_divisor(!g.fz ? s : clamped_scale(s, sdt & 3), absmax);
        return g;
    }

    __device__ __forceinline__ float code(float x, float qmin, float qmax) const {
        if constexpr (FZ) return !fz ? quant_code(x, dv, z, p1, p2, qmin, qmax) : quant_code_fz(x, dv, z, p1, p2, qmin, qmax);
        else return quant_code(x, dv, z, p1, p2, qmin, qmax);
    }
    __device__ __forceinline__ float fake(float x, float qmin, float qmax) const {
        return dequant_code(code(x, qmin, qmax), s, z, p2);
    }
};

// one vector of a group: fake values of T (LLMC_OUT_FAKE) or codes in KIND's container.
// First form: the scalar statement, no fractional arm (dv divides by the scale; s, z, p2 are dequant's). quant_rows calls it
// directly, with a Divisor of its own: with a GroupQuant in its row loop two of its instantiations compiled to another
// instruction stream and measured slower than the parent commit's (scalar bf16 rows +2.5 %, scaled f16 rows +0.3 %, both above
// the run-to-run spread; profiles/quant_group_refactor.txt). Every other kernel takes the second form, from the group's quantizer.
template <int KIND, typename T, int N>
__device__ __forceinline__ void quant_vec(Vec<typename out_elem<KIND, T>::type, N>& o, const Vec<T, N>& v, const Divisor& dv,
                                          float s, float z, int p1, int p2, float qmin, float qmax) {
    using O = typename out_elem<KIND, T>::type;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const float q = quant_code(to_f32<T>(v.v[k]), dv, z, p1, p2, qmin, qmax);
        if constexpr (KIND == LLMC_OUT_FAKE) o.v[k] = from_f32<T>(dequant_code(q, s, z, p2));
        else o.v[k] = (O)q;
    }
}
template <int KIND, bool FZ, typename T, int N>
__device__ __forceinline__ void quant_vec(Vec<typename out_elem<KIND, T>::type, N>& o, const Vec<T, N>& v, const GroupQuant<FZ>& g,
                                          float qmin, float qmax) {
    using O = typename out_elem<KIND, T>::type;
    if constexpr (!FZ) {
        quant_vec<KIND>(o, v, g.dv, g.s, g.z, g.p1, g.p2, qmin, qmax);
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k) {
            if constexpr (KIND == LLMC_OUT_FAKE) o.v[k] = from_f32<T>(g.fake(to_f32<T>(v.v[k]), qmin, qmax));
            else o.v[k] = (O)g.code(to_f32<T>(v.v[k]), qmin, qmax);
        }
    }
}

// ---- min / max over a workgroup of NT threads: wave reduction, NT / 64 words of LDS each (red holds 2 * NT / 64 floats), fold.
// Every thread calls it and leaves with the result. Two barriers: the first lets the previous round's readers finish before
// red is written again. fminf / fmaxf drop NaNs whatever the order, and the sign of a zero minimum or maximum does not reach the
// qparams (|.| in the symmetric branch; mx - mn and qmin - round(mn / s) in the other), so the order is free.
// PAIRWISE chooses between the two orders the kernels had before they shared this function, because each measured slower with
// the other's (profiles/quant_group_refactor.txt): false folds the words one after the other onto the thread's own value
// (k_osplus_act_step: pairwise +0.1 - 0.2 %), true folds the words alone in pairs (k_mixed_mask / k_mixed_idx: +0.5 / +1.9 %
// with the sequential one).
template <int N, bool MAX> __device__ __forceinline__ float fold_pairs(const float* r) {
    if constexpr (N == 1) return r[0];
    else if constexpr (MAX) return fmaxf(fold_pairs<N / 2, MAX>(r), fold_pairs<N / 2, MAX>(r + N / 2));
    else return fminf(fold_pairs<N / 2, MAX>(r), fold_pairs<N / 2, MAX>(r + N / 2));
}
template <int NT, bool PAIRWISE = false> __device__ __forceinline__ void block_minmax(float* red, float& mn, float& mx) {
    constexpr int NW = NT / 64;
    static_assert(NW >= 1 && (NW & (NW - 1)) == 0, "block_minmax: a power of two of waves");
    mn = wave_min(mn, 64);
    mx = wave_max(mx, 64);
    __syncthreads();                       // the previous round's readers are done
    if ((threadIdx.x & 63) == 0) {
        red[threadIdx.x >> 6] = mn;
        red[NW + (threadIdx.x >> 6)] = mx;
    }
    __syncthreads();
    if constexpr (PAIRWISE) {
        mn = fold_pairs<NW, false>(red);
        mx = fold_pairs<NW, true>(red + NW);
    } else {
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            mn = fminf(mn, red[i]);
            mx = fmaxf(mx, red[NW + i]);
        }
    }
}

}  // namespace llmc
