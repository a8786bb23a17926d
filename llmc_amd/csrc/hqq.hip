// hqq.hip — HQQ's half-quadratic zero-point solver (llmc/compression/quantization/hqq.py:36-60,
// quant.py:588-610 optimize_weights_proximal) on the weight in place, every iteration on register-resident groups.
//
// One thread owns one group of g in {16, 32, 64, 128} weights for all iterations:
//   axis 1: g consecutive elements of a row (groups of W itself);
//   axis 0: g consecutive rows of one column (groups of W.T, group index k * (R / g) + r / g); lanes walk columns, so
//           the loads are coalesced and no transposed copy is made.
// Per iteration (fp32, one rounding per op, no contraction; inv = 1 / s):
//   q = clamp(rint(x * inv + z), qmin, qmax); r = (q - z) / inv; d = x - r; e = shrink(d)
//   z' = mean_g(q - (x - e) * inv) in ATen's CPU inner-sum order;   err = mean over the whole tensor of |d|
// The stop rule (stop at the first iteration whose fp32 error is not below the best one; that iteration's z is the
// result) couples every group, so the iterations run in chunks of kc: a chunk launch writes the z of each of its
// iterations and one fp64 |d| partial per (wave, iteration); a one-block finalize sums the partials in index order,
// rounds the mean to fp32 and applies the rule on device. Later chunks see the stop flag and return. Nothing
// synchronises with the host, so the whole solve is stream-ordered and graph-capturable.
#include <math.h>

#include "common.h"
#include "quant_math.h"
#include "vec16.h"

namespace llmc {
namespace {

constexpr int kHqqBlock = 256;
constexpr int kHqqChunk = 20;   // iterations per chunk launch: the shipped config (iters 20) is one launch

struct HqqState {
    int stopped;
    int T;        // iteration whose z is returned; -1 -> the initial z (iters == 0)
    float best;   // best fp32 error so far (the reference's best_error = 1e4)
    int pad;
};

struct HqqArgs {
    const void* W;
    int64_t R, K, ld, G;
    int axis, vec;
    int sym, round_zp;
    float qmin, qmax;
    float c, p1, tau;           // shrink: c = fp32(1 / beta), p1 = fp32(lp_norm - 1); |d| < tau -> shrink is 0 (no pow)
    const float* s_in;          // given qparams (group order) or null: min / max of the group
    const float* z_in;
    float* inv;                 // [G] thread order
    float* z0;                  // [G]
    float* zs;                  // [kc][G]
    double* part;               // [kc][nw]
    HqqState* st;
    int64_t nw;
    int kc, iters;
};

// thread t -> reference group index
__device__ __forceinline__ int64_t group_of(const HqqArgs& a, int64_t t, int g) {
    if (a.axis == 0) {
        const int64_t k = t % a.K, rb = t / a.K;
        return k * (a.R / g) + rb;
    }
    return t;
}

template <typename T, int GS>
__device__ __forceinline__ void load_group(const HqqArgs& a, int64_t t, float (&w)[GS]) {
    const T* W = (const T*)a.W;
    if (a.axis == 0) {
        const int64_t k = t % a.K, r0 = (t / a.K) * GS;
#pragma unroll
        for (int j = 0; j < GS; ++j) w[j] = to_f32<T>(W[(r0 + j) * a.ld + k]);
    } else {
        const int64_t per_row = a.K / GS;
        const int64_t base = (t / per_row) * a.ld + (t % per_row) * GS;
        if (a.vec) {
            constexpr int V = 16 / sizeof(T);
#pragma unroll
            for (int j = 0; j < GS / V; ++j) {
                // a plain struct load, which claims the element's alignment only. With load_vec (a 16-byte aligned uint4) here
                // k_hqq_chunk compiled to other register counts, 154 -> 248 VGPRs at <float, 64>: one occupancy step lost
                // (profiles/quant_group_refactor.txt)
                const Vec<T, V> v = *(const Vec<T, V>*)(W + base + j * V);
#pragma unroll
                for (int u = 0; u < V; ++u) w[j * V + u] = to_f32<T>(v.v[u]);
            }
        } else {
#pragma unroll
            for (int j = 0; j < GS; ++j) w[j] = to_f32<T>(W[base + j]);
        }
    }
}

// x^p for finite x >= 0 in fp64 from + - * / and the exact frexp / ldexp only, so that a numpy restatement repeats it
// bit for bit (tests/hqq_oracle.py:pow_f64): ln x = e ln2 + 2 atanh((m - 1) / (m + 1)) with m in [sqrt(1/2), sqrt(2)),
// 12 odd terms; exp(y) = 2^k exp(y - k ln2), 14 Taylor terms. Relative error ~1e-14, far below the fp32 rounding that
// follows. (ocml's fp64 pow is an out-of-line call here: a stack frame in scratch for each of the unrolled elements.)
__device__ __forceinline__ double pow_f64(double x, double p) {
    const bool zero = x == 0.0;                 // selected at the end: no branch per element
    x = zero ? 1.0 : x;
    int e;
    // frexp of a normal double (x comes from an fp32 value): x = m 2^e, m in [0.5, 1)
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    e = (int)((b >> 52) & 0x7ff) - 1022;
    double m = __longlong_as_double((long long)((b & 0x800fffffffffffffull) | 0x3fe0000000000000ull));
    if (m < 0.70710678118654752440) {
        m = m * 2.0;
        e = e - 1;
    }
    const double s = (m - 1.0) / (m + 1.0);
    const double s2 = s * s;
    double pl = 1.0 / 23.0;
    pl = pl * s2 + 1.0 / 21.0;
    pl = pl * s2 + 1.0 / 19.0;
    pl = pl * s2 + 1.0 / 17.0;
    pl = pl * s2 + 1.0 / 15.0;
    pl = pl * s2 + 1.0 / 13.0;
    pl = pl * s2 + 1.0 / 11.0;
    pl = pl * s2 + 1.0 / 9.0;
    pl = pl * s2 + 1.0 / 7.0;
    pl = pl * s2 + 1.0 / 5.0;
    pl = pl * s2 + 1.0 / 3.0;
    pl = pl * s2 + 1.0;
    const double ln2 = 0.6931471805599453;
    const double y = p * ((double)e * ln2 + (2.0 * s) * pl);
    const double kf = rint(y * 1.4426950408889634);
    const double r = y - kf * ln2;
    double pe = 1.0 / 6227020800.0;
    pe = pe * r + 1.0 / 479001600.0;
    pe = pe * r + 1.0 / 39916800.0;
    pe = pe * r + 1.0 / 3628800.0;
    pe = pe * r + 1.0 / 362880.0;
    pe = pe * r + 1.0 / 40320.0;
    pe = pe * r + 1.0 / 5040.0;
    pe = pe * r + 1.0 / 720.0;
    pe = pe * r + 1.0 / 120.0;
    pe = pe * r + 1.0 / 24.0;
    pe = pe * r + 1.0 / 6.0;
    pe = pe * r + 1.0 / 2.0;
    pe = pe * r + 1.0;
    pe = pe * r + 1.0;
    const double v = ldexp(pe, (int)kf);
    return zero ? (p < 0.0 ? __builtin_inf() : (p == 0.0 ? 1.0 : 0.0)) : v;
}

// Shrink modes of one iteration: lp_norm == 1; lp_norm != 1 with every |d| below tau (e = sign(d) * +0, no pow; `need`
// reports an element at or above tau, and the iteration is then recomputed in the third mode); lp_norm != 1 in full.
enum { SH_LP1 = 0, SH_GUARD = 1, SH_POW = 2 };

// One element of one iteration: returns q - (x - e) * inv and adds |d| to es. FAST: the group's numerators q - z are 0
// or in [2^-60, 2^40) and inv is plain, so the 5-op tail from the hoisted reciprocal is the IEEE quotient (the sign of a
// zero quotient may differ; d = x - r then differs at most in the sign of a zero d, which no later op sees).
template <int MODE, bool FAST>
__device__ __forceinline__ float hqq_term(float x, float inv, float y, float z, const HqqArgs& a, double& es,
                                          bool& need) {
    asm volatile("" : "+v"(x));                     // one element at a time (with the barrier on the result below): the
                                                    // unrolled group otherwise interleaves every element's chain and spills
    const float xi = x * inv;
    float q = rintf(xi + z);                        // each op rounds (-ffp-contract=off); torch.round: half to even
    q = fminf(fmaxf(q, a.qmin), a.qmax);
    const float n = q - z;
    const float r = FAST ? div_tail(n, inv, y) : n / inv;
    const float d = x - r;
    const float ad = fabsf(d);
    es += (double)ad;
    // e = sign(d) * relu(.) is written copysign(relu(.), d): the two differ only in the sign of a zero e (d = -0), which
    // changes x - e only in the sign of a zero, and a zero's sign never reaches z (each sum starts from +0)
    float tt;
    if constexpr (MODE == SH_LP1) {
        tt = q - (x - copysignf(fmaxf(ad - a.c, 0.0f), d)) * inv;      // relu(|d| - 1 / beta)
    } else if constexpr (MODE == SH_GUARD) {
        need = need || !(ad < a.tau);               // below tau, c * |d|^p1 > |d| with margin: e = sign(d) * +0
        tt = q - xi;                                // (x - (+-0)) * inv is x * inv up to the sign of a zero
    } else {
        // torch.pow(|d|, p1): evaluated in fp64 and rounded once (pow(0, p1 < 0) = inf -> relu(-inf) = 0)
        const float pw = (float)pow_f64((double)ad, (double)a.p1);
        tt = q - (x - copysignf(fmaxf(ad - a.c * pw, 0.0f), d)) * inv;
    }
    asm volatile("" : "+v"(tt), "+v"(es));
    return tt;
}

// z' = mean over the group in ATen's order for a contiguous fp32 inner reduction (SumKernel.cpp vectorized_inner_sum,
// Vectorized<float> of V = 8 lanes): lane l sums vectors j = l (mod 8) as row_sum (4 interleaved streams when there are
// >= 4 vectors), the 8 lane sums are then added in lane order; every sum starts from +0.
template <int GS, int MODE, bool FAST>
__device__ __forceinline__ float hqq_iter(const float (&w)[GS], float inv, float y, float z, const HqqArgs& a,
                                          double& es, bool& need) {
    constexpr int NV = GS / 8;
    float fin = 0.0f;
#pragma unroll
    for (int l = 0; l < 8; ++l) {
        float P;
        if constexpr (NV < 4) {
            P = 0.0f;
#pragma unroll
            for (int j = 0; j < NV; ++j) P = P + hqq_term<MODE, FAST>(w[j * 8 + l], inv, y, z, a, es, need);
        } else {
            float part[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float s = 0.0f;
#pragma unroll
                for (int m = 0; m < NV / 4; ++m)
                    s = s + hqq_term<MODE, FAST>(w[(4 * m + k) * 8 + l], inv, y, z, a, es, need);
                part[k] = s;
            }
            P = ((part[0] + part[1]) + part[2]) + part[3];
        }
        fin = fin + P;
    }
    return fin / (float)GS;
}

// The same iteration in the general form with pow, for g >= 64: the eight lane slots run as a loop that is not unrolled
// (64 or 128 unrolled fp64 pows are too large to unroll fully, and a partly unrolled loop indexes w at run time: scratch). Slot l is
// read at offset 0 of every 8-element block, and each block is rotated by one after each slot, so after eight slots w
// is back in place.
template <int GS>
__device__ __forceinline__ float hqq_iter_pow(float (&w)[GS], float inv, float y, float z, const HqqArgs& a,
                                              double& es) {
    constexpr int NV = GS / 8;
    bool need = false;
    float fin = 0.0f;
#pragma unroll 1
    for (int l = 0; l < 8; ++l) {
        float P;
        if constexpr (NV < 4) {
            P = 0.0f;
#pragma unroll
            for (int j = 0; j < NV; ++j) P = P + hqq_term<SH_POW, false>(w[j * 8], inv, y, z, a, es, need);
        } else {
            float part[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float s = 0.0f;
#pragma unroll
                for (int m = 0; m < NV / 4; ++m) s = s + hqq_term<SH_POW, false>(w[(4 * m + k) * 8], inv, y, z, a, es, need);
                part[k] = s;
            }
            P = ((part[0] + part[1]) + part[2]) + part[3];
        }
        fin = fin + P;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const float t0 = w[j * 8];
#pragma unroll
            for (int u = 0; u < 7; ++u) w[j * 8 + u] = w[j * 8 + u + 1];
            w[j * 8 + 7] = t0;
        }
    }
    return fin / (float)GS;
}

// one iteration of one group: the next z, |d| summed into es. The common case runs the fast form (hoisted reciprocal,
// shrink known to be 0); a group with a numerator outside the tail's range or a |d| at or above tau runs the iteration
// again in the general form (IEEE division, pow).
template <int GS, bool LP1>
__device__ __forceinline__ float hqq_step(float (&w)[GS], float inv, float y, bool pfast, float z,
                                          const HqqArgs& a, double& es) {
    // q - z is 0 or at least 2^-25 when q != 0 (Sterbenz); with q = 0 it is -z
    const float az = fabsf(z);
    const bool fast = pfast && (az == 0.0f || az >= 0x1p-60f) && az < 0x1p39f;
    bool need = !fast;
    float zn = 0.0f;
    if (fast) zn = hqq_iter<GS, LP1 ? SH_LP1 : SH_GUARD, true>(w, inv, y, z, a, es, need);
    if (need) {
        es = 0.0;
        if constexpr (LP1)
            zn = hqq_iter<GS, SH_LP1, false>(w, inv, y, z, a, es, need);
        else if constexpr (GS <= 32)     // small enough to unroll whole
            zn = hqq_iter<GS, SH_POW, false>(w, inv, y, z, a, es, need);
        else
            zn = hqq_iter_pow<GS>(w, inv, y, z, a, es);
    }
    return zn;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Iterations [it0, it0 + nit) of every group. first: derive (s, z) (min / max or given) and start from them.
template <typename T, int GS, bool LP1>
__global__ __launch_bounds__(kHqqBlock, GS == 128 ? 1 : 2) void k_hqq_chunk(HqqArgs a, int nit, int first) {
    if (!first && a.st->stopped) return;
    const int64_t t = (int64_t)blockIdx.x * kHqqBlock + threadIdx.x;
    const bool live = t < a.G;
    float w[GS];
    if (live) {
        load_group<T, GS>(a, t, w);
    } else {
#pragma unroll
        for (int j = 0; j < GS; ++j) w[j] = 0.0f;
    }
    float inv, z;
    if (first) {
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            a.st->stopped = 0;
            a.st->T = a.iters - 1;   // ran out without a stop (-1: iters == 0, the initial z)
            a.st->best = 1e4f;
            a.st->pad = 0;
        }
        float s;
        z = 0.0f;
        if (a.s_in) {
            const int64_t gi = live ? group_of(a, t, GS) : 0;
            s = live ? a.s_in[gi] : 1.0f;
            if (a.z_in && live) z = a.z_in[gi];
        } else {
            float mn = w[0], mx = w[0];
#pragma unroll
            for (int j = 1; j < GS; ++j) {
                mn = fminf(mn, w[j]);
                mx = fmaxf(mx, w[j]);
            }
            // the reference reduces W.float(): qparams in fp32, bit for bit llmc_minmax_qparams on the fp32 view
            const QParams qp = qparams_from_minmax(mn, mx, LLMC_F32, a.sym, a.round_zp, a.qmin, a.qmax);
            s = qp.s;
            z = a.sym ? 0.0f : qp.z;
        }
        inv = 1.0f / s;                              // 1 / scales: IEEE reciprocal
        if (live) {
            a.inv[t] = inv;
            a.z0[t] = z;
        }
    } else {
        inv = a.inv[t < a.G ? t : 0];
        z = a.zs[(int64_t)(a.kc - 1) * a.G + (live ? t : 0)];
    }
    const float y = rcp_refined(inv);
    const bool pfast = plain_pos(inv);
    const int64_t wave = t >> 6;
    for (int i = 0; i < nit; ++i) {
        double es = 0.0;
        z = hqq_step<GS, LP1>(w, inv, y, pfast, z, a, es);
        if (live) a.zs[(int64_t)i * a.G + t] = z;
        es = wave_sum_f64(live ? es : 0.0);
        if ((threadIdx.x & 63) == 0 && wave < a.nw) a.part[(int64_t)i * a.nw + wave] = es;   // whole dead waves: none
    }
}

// The stop rule on the chunk's iterations [it0, it0 + nit): fixed-order fp64 sums of the wave partials, mean over n,
// rounded to fp32 and compared with the best fp32 error (ties stop). errs (optional): the fp64 means.
__global__ __launch_bounds__(kHqqBlock) void k_hqq_finalize(HqqArgs a, int it0, int nit, double n, double* errs) {
    __shared__ double red[kHqqBlock];
    __shared__ int stop;
    if (threadIdx.x == 0) stop = a.st->stopped;
    __syncthreads();
    for (int i = 0; i < nit && !stop; ++i) {
        double s = 0.0;
        for (int64_t j = threadIdx.x; j < a.nw; j += kHqqBlock) s += a.part[(int64_t)i * a.nw + j];
        red[threadIdx.x] = s;
        __syncthreads();
        for (int o = kHqqBlock / 2; o > 0; o >>= 1) {
            if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            const double m = red[0] / n;
            const float e = (float)m;
            if (errs) errs[it0 + i] = m;
            if (e < a.st->best) {
                a.st->best = e;
            } else {
                a.st->stopped = 1;
                a.st->T = it0 + i;
                stop = 1;
            }
        }
        __syncthreads();
    }
}

// scales = 1 / inv (the reference returns 1 / (1 / s)), zeros = z of iteration T, in group order.
__global__ __launch_bounds__(kHqqBlock) void k_hqq_write(HqqArgs a, int g, float* scales, float* zeros, int* t_out) {
    const int64_t t = (int64_t)blockIdx.x * kHqqBlock + threadIdx.x;
    const int T = a.st->T;
    if (t == 0 && t_out) *t_out = T;
    if (t >= a.G) return;
    const int64_t gi = group_of(a, t, g);
    scales[gi] = 1.0f / a.inv[t];
    zeros[gi] = T < 0 ? a.z0[t] : a.zs[(int64_t)(T % a.kc) * a.G + t];
}

struct HqqLayout {
    int64_t G, nw;
    int kc;
    size_t part, state, inv, z0, zs, total;
};

static bool hqq_layout(int64_t R, int64_t K, int axis, int64_t g, int iters, HqqLayout& L) {
    if (R <= 0 || K <= 0 || iters < 0 || (axis != 0 && axis != 1)) return false;
    if (g != 16 && g != 32 && g != 64 && g != 128) return false;
    if ((axis == 0 ? R : K) % g) return false;
    L.G = R * K / g;
    L.nw = ceil_div64(L.G, 64);
    L.kc = iters < 1 ? 1 : (iters < kHqqChunk ? iters : kHqqChunk);
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    L.part = 0;
    L.state = up((size_t)L.kc * L.nw * sizeof(double));
    L.inv = L.state + 256;
    L.z0 = up(L.inv + (size_t)L.G * sizeof(float));
    L.zs = up(L.z0 + (size_t)L.G * sizeof(float));
    L.total = up(L.zs + (size_t)L.kc * L.G * sizeof(float));
    return true;
}

template <typename T, int GS, bool LP1>
static int hqq_run(HqqArgs& a, int iters, double* errs, float* scales, float* zeros, int* t_out, hipStream_t st) {
    const unsigned grid = (unsigned)ceil_div64(a.G, kHqqBlock);
    const double n = (double)a.G * GS;
    int it0 = 0;
    bool first = true;
    do {
        const int nit = (iters - it0) < a.kc ? (iters - it0) : a.kc;
        hipLaunchKernelGGL((k_hqq_chunk<T, GS, LP1>), dim3(grid), dim3(kHqqBlock), 0, st, a, nit, (int)first);
        LLMC_LAUNCH_CHECK();
        if (nit > 0) {
            hipLaunchKernelGGL(k_hqq_finalize, dim3(1), dim3(kHqqBlock), 0, st, a, it0, nit, n, errs);
            LLMC_LAUNCH_CHECK();
        }
        first = false;
        it0 += nit;
    } while (it0 < iters);
    hipLaunchKernelGGL(k_hqq_write, dim3(grid), dim3(kHqqBlock), 0, st, a, GS, scales, zeros, t_out);
    LLMC_LAUNCH_CHECK();
    return LLMC_OK;
}

template <typename T, bool LP1>
static int hqq_by_g(HqqArgs& a, int64_t g, int iters, double* errs, float* s, float* z, int* t_out, hipStream_t st) {
    switch (g) {
        case 16: return hqq_run<T, 16, LP1>(a, iters, errs, s, z, t_out, st);
        case 32: return hqq_run<T, 32, LP1>(a, iters, errs, s, z, t_out, st);
        case 64: return hqq_run<T, 64, LP1>(a, iters, errs, s, z, t_out, st);
        default: return hqq_run<T, 128, LP1>(a, iters, errs, s, z, t_out, st);
    }
}

template <typename T>
static int hqq_by_lp(HqqArgs& a, int lp1, int64_t g, int iters, double* errs, float* s, float* z, int* t_out,
                     hipStream_t st) {
    return lp1 ? hqq_by_g<T, true>(a, g, iters, errs, s, z, t_out, st)
               : hqq_by_g<T, false>(a, g, iters, errs, s, z, t_out, st);
}

}  // namespace
}  // namespace llmc

using namespace llmc;

extern "C" size_t llmc_hqq_ws_bytes(int64_t R, int64_t K, int axis, int64_t group_size, int iters) {
    HqqLayout L;
    return hqq_layout(R, K, axis, group_size, iters, L) ? L.total : 0;
}

extern "C" int llmc_hqq_optimize(const void* W, int dt, int64_t R, int64_t K, int64_t ld, int axis,
                                 int64_t group_size, int sym, int round_zp, float qmin, float qmax, const float* s_in,
                                 const float* z_in, float c, float p1, int lp_norm_one, int iters, float* scales,
                                 float* zeros, double* errs, int* t_out, void* ws, llmc_stream_t stream) {
    LLMC_REQUIRE(dtype_ok(dt), "hqq_optimize: bad dtype");
    LLMC_REQUIRE(W && scales && zeros && ws, "hqq_optimize: null argument");
    LLMC_REQUIRE(R > 0 && K > 0 && ld >= K && iters >= 0, "hqq_optimize: bad shape");
    LLMC_REQUIRE(!z_in || s_in, "hqq_optimize: z_in without s_in");
    HqqLayout L;
    if (!hqq_layout(R, K, axis, group_size, iters, L)) {
        set_last_error_msg("hqq_optimize: per_group with group_size in {16, 32, 64, 128} dividing the grouped dimension, "
                           "axis 0 or 1");
        return LLMC_ENOTSUP;
    }
    LLMC_REQUIRE(L.G < (1ll << 40), "hqq_optimize: tensor too large");
    HqqArgs a;
    a.W = W;
    a.R = R;
    a.K = K;
    a.ld = ld;
    a.G = L.G;
    a.axis = axis;
    const int vb = 16 / dtype_size(dt);
    a.vec = axis == 1 && ld % vb == 0 && ((uintptr_t)W & 15) == 0;
    a.sym = sym;
    a.round_zp = round_zp;
    a.qmin = qmin;
    a.qmax = qmax;
    a.c = c;
    a.p1 = p1;
    // |d| < c^(1 / (1 - p1)) <=> c * |d|^p1 > |d| (p1 < 1). Below tau = that bound * (1 - 2^-10) the fp32 shrink term exceeds
    // |d| by more than 2^-10 relative, far beyond the rounding of pow and of the product, so relu(...) is +0 exactly.
    // Only used for p1 < 0 (lp_norm < 1, the shipped 0.7); tau = 0 sends every element through pow.
    double tau = 0.0;
    if (!lp_norm_one && p1 < 0.0f && c > 0.0f && isfinite(c)) tau = pow((double)c, 1.0 / (1.0 - (double)p1)) * (1.0 - 0x1p-10);
    a.tau = (float)tau;
    a.s_in = s_in;
    a.z_in = z_in;
    char* base = (char*)ws;
    a.part = (double*)(base + L.part);
    a.st = (HqqState*)(base + L.state);
    a.inv = (float*)(base + L.inv);
    a.z0 = (float*)(base + L.z0);
    a.zs = (float*)(base + L.zs);
    a.nw = L.nw;
    a.kc = L.kc;
    a.iters = iters;
    hipStream_t st = (hipStream_t)stream;
    DISPATCH_DT(dt, return hqq_by_lp<T>(a, lp_norm_one, group_size, iters, errs, scales, zeros, t_out, st));
}
