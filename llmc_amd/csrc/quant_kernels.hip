// quant_kernels.hip — HBM-bound quantizer kernels (K5/K6/K7 of SURVEY.md §2.3):
//   min/max -> scale/zero, round/clamp (fake + real), LSB-first int packing, the AutoAWQ GEMM packer (K7b).
// Layout: W is a contiguous [G, g] view (one quantization group per row). A wave64 is cut into
// 64/LPR sub-groups of LPR lanes, one row per sub-group, 16 B per lane per load (coalesced: a sub-group
// reads LPR*16 contiguous bytes). Rows are distributed over a grid-stride of waves.
// Row kernels: quant_rows behind k_quant_rows* (any g; qparams only, fake values or codes, optionally a column multiplier) and
// k_quant_dynamic_small (g = LPR * 16 B exactly); launch_quant_rows is the one place that chooses between them.
#include "common.h"
#include "quant_group.h"
#include "quant_math.h"

namespace llmc {

static constexpr int kBlock = 256;
static constexpr int kMaxGrid = 256 * 8;

// k_quant_static / quant_rows: fake values as store_vec writes them. Codes are written element by element in source, because
// the hosts' vec_ok asks for a 16-B aligned `out` only where fake values go; the compiler is free to merge neighbouring element
// stores of the vector into wider ones that need the element's alignment only (gfx950 global stores are unaligned-capable), and
// it does: that is intended, k_quant_static has always been compiled this way.
template <int KIND, typename O, int VEC>
__device__ __forceinline__ void store_out(void* out, int64_t i, const Vec<O, VEC>& o) {
    O* op = (O*)out + i;
    if constexpr (KIND == LLMC_OUT_FAKE) {
        store_vec<O, VEC>(op, o);
    } else {
#pragma unroll
        for (int k = 0; k < VEC; ++k) op[k] = o.v[k];
    }
}
// --------------------------------------------------------------------------------------------
// row scan: min/max of one row by LPR lanes
// --------------------------------------------------------------------------------------------
// one vector of the row at column c; SCALE: times the column multiplier, w' = rnd(w * cs[col]) in the tensor dtype (from_f32
// is that one rounding)
template <typename T, int VEC, bool SCALE>
__device__ __forceinline__ Vec<T, VEC> load_row_vec(const T* row, const T* cs, int c) {
    Vec<T, VEC> v = load_vec<T, VEC>(row + c);
    if constexpr (SCALE) {
        const Vec<T, VEC> sv = load_vec<T, VEC>(cs + c);
#pragma unroll
        for (int i = 0; i < VEC; ++i)
            v.v[i] = from_f32<T>(to_f32<T>(v.v[i]) * to_f32<T>(sv.v[i]));
    }
    return v;
}
// KEEP_FIRST: `first` receives this lane's first vector, if the lane owns one (sl * VEC < g)
template <typename T, int VEC, bool SCALE, bool KEEP_FIRST>
__device__ __forceinline__ void row_minmax(const T* row, const T* cs, int g, int sl, int lpr, float& mn, float& mx,
                                           Vec<T, VEC>& first) {
    mn = INFINITY;
    mx = -INFINITY;
    bool have_first = false;
    for (int c = sl * VEC; c < g; c += lpr * VEC) {
        Vec<T, VEC> v = load_row_vec<T, VEC, SCALE>(row, cs, c);
        if constexpr (KEEP_FIRST) {
            if (!have_first) {
                first = v;
                have_first = true;
            }
        }
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            float f = to_f32<T>(v.v[i]);
            mn = fminf(mn, f);
            mx = fmaxf(mx, f);
        }
    }
    mn = wave_min(mn, lpr);
    mx = wave_max(mx, lpr);
}

// K5 / K5+K6 fused / AWQ's scale + fake-quant, for rows of any length: one body.
//   pass 1  min/max of the row (second row pass hits L1/L2; the first 16 B per lane stay in registers, which covers
//           g <= LPR*VEC, i.e. every per_group case), then scales / zeros [G] in the tensor dtype where asked for
//   pass 2  quantize and store: fake values or codes of KIND. KIND = OUT_NONE (file-local, not an LLMC_OUT_* of the ABI)
//           compiles pass 2 out: llmc_minmax_qparams' instantiation carries no quantizer code.
//   SCALE   fake_quantize_weight of AWQ's search (awq.py:147-164): every load is w' = rnd(w * cs[col]) (the in-place mul_ in
//           the model dtype); cs is [gpr, g], one row of K multipliers cut like the weight rows (gpr groups per row).
// A sub-group past the last row computes on row G - 1 (its lanes take part in the wave's shuffles) and stores nothing.
static constexpr int OUT_NONE = -1;
template <typename T, int VEC, int KIND, bool SCALE>
__device__ __forceinline__ void quant_rows(const T* __restrict__ W, const T* __restrict__ cs, int64_t G, int g, int gpr,
                                           int lpr, int sym, int round_zp, float qmin, float qmax, void* __restrict__ out,
                                           T* __restrict__ scales, T* __restrict__ zeros) {
    constexpr int DT = dt_of<T>::value;
    const int lane = threadIdx.x & 63;
    const int rpw = 64 / lpr;
    const int sub = lane / lpr, sl = lane % lpr;
    const int64_t wave = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * (kBlock / 64);
    for (int64_t r0 = wave * rpw; r0 < G; r0 += nwaves * rpw) {
        const int64_t row = r0 + sub;
        const bool valid = row < G;
        const int64_t rr = valid ? row : G - 1;
        const T* rp = W + rr * g;
        const T* cp = SCALE ? cs + (rr % gpr) * g : nullptr;
        float mn, mx;
        Vec<T, VEC> first;
        row_minmax<T, VEC, SCALE, KIND != OUT_NONE>(rp, cp, g, sl, lpr, mn, mx, first);
        const bool lead = valid && sl == 0;         // the lane that stores the row's qparams
        if (KIND == OUT_NONE && !lead) continue;    // qparams only: no other lane needs them
        const QParams qp = qparams_from_minmax(mn, mx, DT, sym, SCALE ? 1 : round_zp, qmin, qmax);
        if constexpr (!SCALE) {                     // SCALE serves llmc_awq_scale_fakequant: no qparams out, round_zp = 1
            if (lead) {
                if (KIND == OUT_NONE || scales) scales[row] = from_f32<T>(qp.s);    // llmc_minmax_qparams requires scales
                if (zeros) zeros[row] = from_f32<T>(qp.z);
            }
        }
        if constexpr (KIND != OUT_NONE) {
            if (!valid) continue;
            // The scalar statement, not a GroupQuant: with one in this loop two instantiations measured slower than the parent's
            // (scalar bf16 +2.5 %, scaled f16 +0.3 %; profiles/quant_group_refactor.txt). No fractional-zero-point arm:
            // llmc_quant_dynamic refuses round_zp = 0, only the qparams above take it.
            const Divisor dv = make_divisor(qp.s, fmaxf(fabsf(mn), fabsf(mx)));
            bool use_first = true;
            for (int c = sl * VEC; c < g; c += lpr * VEC) {
                const Vec<T, VEC> v = use_first ? first : load_row_vec<T, VEC, SCALE>(rp, cp, c);
                use_first = false;
                Vec<typename out_elem<KIND, T>::type, VEC> o;
                quant_vec<KIND>(o, v, dv, qp.s, qp.z, DT, DT, qmin, qmax);
                store_out<KIND>(out, rr * g + c, o);
            }
        }
    }
}

// The kernels of quant_rows: one entry point per argument list, nothing else. An instantiation that carried the arguments of
// the other two measured slower than the kernel it replaced (qparams only: 18.48 -> 18.74 us at 4096 x 14336 bf16) with the
// same instructions; with its own argument list it does not (profiles/quant_rows_refactor.txt).
template <typename T, int VEC>
__global__ __launch_bounds__(kBlock) void k_quant_rows_qparams(const T* __restrict__ W, int64_t G, int g, int lpr, int sym,
                                                               int round_zp, float qmin, float qmax,
                                                               T* __restrict__ scales, T* __restrict__ zeros) {
    quant_rows<T, VEC, OUT_NONE, false>(W, nullptr, G, g, 1, lpr, sym, round_zp, qmin, qmax, nullptr, scales, zeros);
}
template <typename T, int VEC, int KIND>
__global__ __launch_bounds__(kBlock) void k_quant_rows(const T* __restrict__ W, int64_t G, int g, int lpr, int sym,
                                                       int round_zp, float qmin, float qmax, void* __restrict__ out,
                                                       T* __restrict__ scales, T* __restrict__ zeros) {
    quant_rows<T, VEC, KIND, false>(W, nullptr, G, g, 1, lpr, sym, round_zp, qmin, qmax, out, scales, zeros);
}
template <typename T, int VEC>
__global__ __launch_bounds__(kBlock) void k_quant_rows_scaled(const T* __restrict__ W, const T* __restrict__ cs, int64_t G,
                                                              int g, int gpr, int lpr, int sym, float qmin, float qmax,
                                                              T* __restrict__ out) {
    quant_rows<T, VEC, LLMC_OUT_FAKE, true>(W, cs, G, g, gpr, lpr, sym, 1, qmin, qmax, out, nullptr, nullptr);
}

// two-stage variant for few, very long rows (per_tensor / huge per_channel)
static constexpr int kChunk = 8192;
template <typename T, int VEC>
__global__ __launch_bounds__(kBlock) void k_minmax_partial(const T* __restrict__ W, int64_t G, int64_t g,
                                                           int64_t nch, float2* __restrict__ part) {
    __shared__ float red[2 * (kBlock / 64)];
    for (int64_t u = blockIdx.x; u < G * nch; u += gridDim.x) {
        int64_t row = u / nch, ch = u % nch;
        int64_t c0 = ch * kChunk, c1 = c0 + kChunk < g ? c0 + kChunk : g;
        const T* p = W + row * g;
        float mn = INFINITY, mx = -INFINITY;
        for (int64_t c = c0 + (int64_t)threadIdx.x * VEC; c < c1; c += (int64_t)kBlock * VEC) {
            Vec<T, VEC> v = load_vec<T, VEC>(p + c);
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                float f = to_f32<T>(v.v[i]);
                mn = fminf(mn, f);
                mx = fmaxf(mx, f);
            }
        }
        block_minmax<kBlock>(red, mn, mx);
        if (threadIdx.x == 0) part[u] = make_float2(mn, mx);
    }
}
static constexpr int kFinalBlock = 1024;     // threads of k_minmax_final: its stride, its LDS words and its launch
template <typename T>
__global__ void k_minmax_final(const float2* __restrict__ part, int64_t G, int64_t nch, int sym,
                               int round_zp, float qmin, float qmax, T* __restrict__ scales,
                               T* __restrict__ zeros) {
    constexpr int DT = dt_of<T>::value;
    __shared__ float red[2 * (kFinalBlock / 64)];
    int64_t row = blockIdx.x;
    float mn = INFINITY, mx = -INFINITY;
    for (int64_t c = threadIdx.x; c < nch; c += kFinalBlock) {
        float2 p = part[row * nch + c];
        mn = fminf(mn, p.x);
        mx = fmaxf(mx, p.y);
    }
    block_minmax<kFinalBlock>(red, mn, mx);
    if (threadIdx.x == 0) {
        QParams q = qparams_from_minmax(mn, mx, DT, sym, round_zp, qmin, qmax);
        scales[row] = from_f32<T>(q.s);
        if (zeros) zeros[row] = from_f32<T>(q.z);
    }
}

// K6 static: given qparams
template <typename T, int VEC, int KIND>
__global__ __launch_bounds__(kBlock) void k_quant_static(const T* __restrict__ W, int64_t G, int g,
                                                         const void* __restrict__ scales, int sdt,
                                                         const void* __restrict__ zeros, int zdt,
                                                         float qmin, float qmax, void* __restrict__ out) {
    constexpr int WDT = dt_of<T>::value;
    const int sd = sdt & 3, zd = zdt & 3;
    const int64_t nvec_row = g / VEC;
    const int64_t total = G * nvec_row;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * kBlock) {
        int64_t row = i / nvec_row;
        int64_t c = (i - row * nvec_row) * VEC;
        float s = load_as_f32(scales, row, sd);
        float z = zeros ? load_as_f32(zeros, row, zd) : 0.0f;
        Vec<T, VEC> v = load_vec<T, VEC>(W + row * g + c);
        float am = 0.0f;   // bound of |x| over this thread's elements for the hoisted divisor (quant_math.h)
#pragma unroll
        for (int k = 0; k < VEC; ++k) am = fmaxf(am, fabsf(to_f32<T>(v.v[k])));
        const GroupQuant<true> q = GroupQuant<true>::from_qparams(s, z, zeros != nullptr, WDT, sdt, zdt, am);
        Vec<typename out_elem<KIND, T>::type, VEC> o;
        quant_vec<KIND>(o, v, q, qmin, qmax);
        store_out<KIND>(out, row * g + c, o);
    }
}

// ---- fast path for short rows (per_group: g == LPR * VEC exactly, one 16-B vector per lane per row):
// UNR independent row-sets per wave iteration keep 4 loads per lane in flight (the generic loop has one and
// measured 2.2-2.9 TB/s; HBM latency x bandwidth needs ~12 KB in flight per SIMD).
static constexpr int UNR = 4;
template <typename T, int VEC, int KIND, bool SCALE>
__global__ __launch_bounds__(kBlock) void k_quant_dynamic_small(const T* __restrict__ W, const T* __restrict__ cs,
                                                                int64_t G, int g, int gpr, int lpr, int sym,
                                                                int round_zp, float qmin, float qmax,
                                                                void* __restrict__ out, T* __restrict__ scales,
                                                                T* __restrict__ zeros) {
    constexpr int DT = dt_of<T>::value;
    const int lane = threadIdx.x & 63;
    const int rpw = 64 / lpr;
    const int sub = lane / lpr, sl = lane % lpr;
    const int64_t wave = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * (kBlock / 64);
    for (int64_t r0 = wave * rpw * UNR; r0 < G; r0 += nwaves * rpw * UNR) {
        Vec<T, VEC> v[UNR];
        bool valid[UNR];
        int64_t rows[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int64_t row = r0 + u * rpw + sub;
            valid[u] = row < G;
            rows[u] = valid[u] ? row : G - 1;
            v[u] = load_vec<T, VEC>(W + rows[u] * g + sl * VEC);
        }
        if (SCALE) {
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                Vec<T, VEC> sv = load_vec<T, VEC>(cs + (rows[u] % gpr) * g + sl * VEC);
#pragma unroll
                for (int i = 0; i < VEC; ++i)
                    v[u].v[i] = from_f32<T>(rndc<DT>(to_f32<T>(v[u].v[i]) * to_f32<T>(sv.v[i])));
            }
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            float mn = INFINITY, mx = -INFINITY;
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                const float f = to_f32<T>(v[u].v[i]);
                mn = fminf(mn, f);
                mx = fmaxf(mx, f);
            }
            mn = wave_min(mn, lpr);
            mx = wave_max(mx, lpr);
            const GroupQuant<> q = GroupQuant<>::from_minmax(mn, mx, DT, sym, round_zp, qmin, qmax);
            if (valid[u] && sl == 0) {
                if (scales) scales[rows[u]] = from_f32<T>(q.s);
                if (zeros) zeros[rows[u]] = from_f32<T>(q.z);
            }
            if (!valid[u] || out == nullptr) continue;
            using O = typename out_elem<KIND, T>::type;
            Vec<O, VEC> o;
            quant_vec<KIND>(o, v[u], q, qmin, qmax);
            store_vec_wide<O, VEC>((O*)out + rows[u] * g + sl * VEC, o);   // the launch condition guarantees a 16-B aligned `out`
        }
    }
}

static inline bool small_ok(int64_t g, int vec) {
    int64_t lpr = g / vec;
    return g % vec == 0 && lpr >= 1 && lpr <= 64 && (lpr & (lpr - 1)) == 0;
}

// K7: LSB-first packing. One thread per output word; 32/bits consecutive codes -> one int32.
template <typename C, bool VECOK>
__global__ __launch_bounds__(kBlock) void k_pack_lsb(const C* __restrict__ codes, int64_t R, int64_t K,
                                                     int bits, int64_t Kp, int32_t* __restrict__ packed) {
    const int pf = 32 / bits;
    const int off = 1 << (bits - 1);
    const int64_t total = R * Kp;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * kBlock) {
        int64_t r = i / Kp, j = i - r * Kp;
        const C* p = codes + r * K + j * pf;
        uint32_t w = 0;
        if (j * pf + pf <= K) {
            if constexpr (sizeof(C) == 4 && VECOK) {
                if (pf == 8) {
                    int4 a = *reinterpret_cast<const int4*>(p);
                    int4 b = *reinterpret_cast<const int4*>(p + 4);
                    int v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
                    for (int k = 0; k < 8; ++k) w |= (uint32_t)((v[k] + off) & 0xff) << (bits * k);
                } else {
                    for (int k = 0; k < pf; ++k) w |= (uint32_t)(((int)p[k] + off) & 0xff) << (bits * k);
                }
            } else {
                for (int k = 0; k < pf; ++k) w |= (uint32_t)(((int)p[k] + off) & 0xff) << (bits * k);
            }
        } else {
            for (int k = 0; k < pf && j * pf + k < K; ++k)
                w |= (uint32_t)(((int)p[k] + off) & 0xff) << (bits * k);
        }
        packed[i] = (int32_t)w;
    }
}

// K7b: the AutoAWQ GEMM packer (module_utils.py:1004-1065): one thread per output word
template <typename T>
__global__ __launch_bounds__(kBlock) void k_pack_awq_w(const T* __restrict__ W, const void* __restrict__ scales, int sdt,
                                                       const int32_t* __restrict__ zeros, int64_t R, int64_t K,
                                                       int64_t g, int32_t* __restrict__ qweight) {
    constexpr int WDT = dt_of<T>::value;
    const int p = promote(WDT, LLMC_F16);
    const int64_t R8 = R / 8, ng = K / g;
    const int64_t total = K * R8;
    const int order[8] = {0, 2, 4, 6, 1, 3, 5, 7};
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {
        const int64_t rw = i / K, k = i - rw * K;   // k fastest: coalesced reads of W rows
        const int64_t gi = k / g;
        uint32_t word = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int64_t r = rw * 8 + order[j];
            const float s = rnd(load_as_f32(scales, r * ng + gi, sdt), LLMC_F16);   // scales.to(float16)
            const float sz = rnd((float)zeros[r * ng + gi] * s, LLMC_F16);           // zeros * scales
            float t = rnd(to_f32<T>(W[r * K + k]) + sz, p);
            t = rnd(t / s, p);
            const int code = (int)rintf(t);
            word |= ((uint32_t)code) << (4 * j);
        }
        qweight[k * R8 + rw] = (int32_t)word;
    }
}
__global__ __launch_bounds__(kBlock) void k_pack_awq_z(const void* __restrict__ scales, int sdt,
                                                       const int32_t* __restrict__ zeros, int64_t R, int64_t ng,
                                                       int32_t* __restrict__ qzeros, uint16_t* __restrict__ sout) {
    const int64_t R8 = R / 8;
    const int order[8] = {0, 2, 4, 6, 1, 3, 5, 7};
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < ng * R; i += (int64_t)gridDim.x * kBlock) {
        const int64_t gi = i / R, r = i - gi * R;
        sout[gi * R + r] = f32_to_f16_bits(load_as_f32(scales, r * ng + gi, sdt));
        if (r < R8) {
            uint32_t word = 0;
#pragma unroll
            for (int j = 0; j < 8; ++j) word |= ((uint32_t)zeros[(r * 8 + order[j]) * ng + gi]) << (4 * j);
            qzeros[gi * R8 + r] = (int32_t)word;
        }
    }
}

static inline int choose_lpr(int64_t g, int vec) {
    int lpr = pow2_ceil(ceil_div64(g, vec));
    if (lpr > 64) lpr = 64;
    if (lpr < 1) lpr = 1;
    return lpr;
}

static inline bool use_two_stage(int64_t G, int64_t g) { return g >= 4 * kChunk && G < 4096; }

static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// The launch ladder of the row kernels for a contiguous [G, g] view with g < 2^31: small -> 16-byte vectors -> scalar.
//   vector  rows of whole 16-B vectors; W, the multipliers cs (SCALE) and, for fake values, `out` 16-B aligned. Codes are
//           stored element by element, so their `out` may lie anywhere; OUT_NONE has no `out`.
//   small   vector, g = lpr * 16 B with lpr a power of two <= 64, and `out` 16-B aligned for codes too (k_quant_dynamic_small
//           stores them 8 - 32 bytes at a time). It has no qparams-only instantiation: a null `out` says so at run time.
template <typename T, int KIND, bool SCALE>
static int launch_quant_rows(const void* W, const void* cs, int64_t G, int64_t g, int gpr, int sym, int round_zp, float qmin,
                             float qmax, void* out, void* scales, void* zeros, hipStream_t st) {
    constexpr int V16 = 16 / sizeof(T);
    const bool vec_ok = g % V16 == 0 && aligned16(W) && (!SCALE || aligned16(cs)) &&
                        (KIND != LLMC_OUT_FAKE || aligned16(out));
    if (vec_ok && small_ok(g, V16) && aligned16(out)) {
        constexpr int SK = KIND == OUT_NONE ? LLMC_OUT_FAKE : KIND;
        const int lpr = (int)(g / V16);
        const int grid = capped_grid(ceil_div64(G, (64 / lpr) * UNR), kBlock / 64, kMaxGrid);
        hipLaunchKernelGGL((k_quant_dynamic_small<T, V16, SK, SCALE>), dim3(grid), dim3(kBlock), 0, st, (const T*)W,
                           (const T*)cs, G, (int)g, gpr, lpr, sym, round_zp, qmin, qmax, out, (T*)scales, (T*)zeros);
    } else {
        const int lpr = choose_lpr(g, vec_ok ? V16 : 1);
        const int grid = capped_grid(ceil_div64(G, 64 / lpr), kBlock / 64, kMaxGrid);
        if constexpr (KIND == OUT_NONE) {
            const auto kernel = vec_ok ? k_quant_rows_qparams<T, V16> : k_quant_rows_qparams<T, 1>;
            hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), 0, st, (const T*)W, G, (int)g, lpr, sym, round_zp, qmin, qmax,
                               (T*)scales, (T*)zeros);
        } else if constexpr (SCALE) {
            const auto kernel = vec_ok ? k_quant_rows_scaled<T, V16> : k_quant_rows_scaled<T, 1>;
            hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), 0, st, (const T*)W, (const T*)cs, G, (int)g, gpr, lpr, sym, qmin,
                               qmax, (T*)out);
        } else {
            const auto kernel = vec_ok ? k_quant_rows<T, V16, KIND> : k_quant_rows<T, 1, KIND>;
            hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), 0, st, (const T*)W, G, (int)g, lpr, sym, round_zp, qmin, qmax, out,
                               (T*)scales, (T*)zeros);
        }
    }
    LLMC_LAUNCH_CHECK();
    return LLMC_OK;
}

}  // namespace llmc

using namespace llmc;

extern "C" size_t llmc_minmax_qparams_ws_bytes(int64_t G, int64_t g) {
    if (G <= 0 || g <= 0) return 0;
    if (!use_two_stage(G, g)) return 0;
    return (size_t)(G * ceil_div64(g, kChunk)) * sizeof(float2);
}

// few, very long rows: per-chunk partial min/max into the workspace, then one block per row
template <typename T>
static int minmax_two_stage_t(const void* W, int64_t G, int64_t g, int sym, int round_zp, float qmin, float qmax,
                              void* scales, void* zeros, void* ws, hipStream_t st) {
    constexpr int V16 = 16 / sizeof(T);
    const bool vec_ok = g % V16 == 0 && aligned16(W);
    const int64_t nch = ceil_div64(g, kChunk);
    const int grid = capped_grid(G * nch, 1, kMaxGrid);
    if (vec_ok)
        hipLaunchKernelGGL((k_minmax_partial<T, V16>), dim3(grid), dim3(kBlock), 0, st, (const T*)W, G, g, nch,
                           (float2*)ws);
    else
        hipLaunchKernelGGL((k_minmax_partial<T, 1>), dim3(grid), dim3(kBlock), 0, st, (const T*)W, G, g, nch,
                           (float2*)ws);
    LLMC_LAUNCH_CHECK();
    hipLaunchKernelGGL((k_minmax_final<T>), dim3((unsigned)G), dim3(kFinalBlock), 0, st, (const float2*)ws, G, nch, sym,
                       round_zp, qmin, qmax, (T*)scales, (T*)zeros);
    LLMC_LAUNCH_CHECK();
    return LLMC_OK;
}

extern "C" int llmc_minmax_qparams(const void* W, int dt, int64_t G, int64_t g, int sym, int round_zp,
                                   float qmin, float qmax, void* scales, void* zeros, void* ws,
                                   llmc_stream_t stream) {
    LLMC_REQUIRE(dtype_ok(dt), "minmax_qparams: bad dtype");
    LLMC_REQUIRE(W && scales && G > 0 && g > 0, "minmax_qparams: null/empty argument");
    LLMC_REQUIRE(sym || zeros, "minmax_qparams: zeros required for asymmetric");
    hipStream_t st = (hipStream_t)stream;
    if (use_two_stage(G, g)) {
        LLMC_REQUIRE(ws != nullptr, "minmax_qparams: workspace required for long rows");
        DISPATCH_DT(dt, return minmax_two_stage_t<T>(W, G, g, sym, round_zp, qmin, qmax, scales, zeros, ws, st));
    }
    LLMC_REQUIRE(g < (1ll << 31), "minmax_qparams: row too long");
    DISPATCH_DT(dt, return launch_quant_rows<T, OUT_NONE, false>(W, nullptr, G, g, 1, sym, round_zp, qmin, qmax, nullptr,
                                                                 scales, zeros, st));
}


// calib_algo = 'mse' (BaseQuantizer.get_mse_range, quant.py:145-203) + get_qparams on the searched range.
// One wave per row of g elements. The reference works on tensor.float(): ranges, qparams and the fake-quant are
// fp32. Its candidate ranges COMPOUND: best_min_val aliases _min_val, so after an improvement at step i the next
// candidate is p_{i+1} times the already shrunk range (oracle/quant_ref.py:mse_range pins this against the goldens).
// Every caller of the search (k_mse_qparams, k_mse_panel) runs this one function, so a row gives the same bits
// whichever kernel searched it. Returns the searched (min, max) and their qparams, valid in every lane.
template <typename T>
__device__ __forceinline__ QParams mse_search_row(const T* __restrict__ w, int g, int lane, int sym, int round_zp,
                                                  float qmin, float qmax, int nsteps, int grid, float norm,
                                                  float& min_out, float& max_out) {
    float mn = INFINITY, mx = -INFINITY;
    for (int c = lane; c < g; c += 64) {
        const float x = to_f32<T>(w[c]);
        mn = fminf(mn, x);
        mx = fmaxf(mx, x);
    }
    float cur_min = wave_min(mn, 64), cur_max = wave_max(mx, 64);
    const float row_absmax = fmaxf(fabsf(cur_min), fabsf(cur_max));
    float best = INFINITY;
    for (int i = 0; i < nsteps; ++i) {
        const float p = (float)(1.0 - (double)i / (double)grid);   // python float -> fp32 scalar operand
        const float xmin = p * cur_min, xmax = p * cur_max;
        const QParams q = qparams_from_minmax(xmin, xmax, LLMC_F32, sym, round_zp, qmin, qmax);
        const Divisor dv = make_divisor(q.s, row_absmax);
        float acc = 0.0f;
        for (int c = lane; c < g; c += 64) {
            const float x = to_f32<T>(w[c]);
            const float code = quant_code(x, dv, q.z, LLMC_F32, LLMC_F32, qmin, qmax);
            const float d = fabsf(dequant_code(code, q.s, q.z, LLMC_F32) - x);
            acc += powf(d, norm);
        }
        const float err = wave_sum(acc, 64);
        if (err < best) {
            best = err;
            cur_min = xmin;
            cur_max = xmax;
        }
    }
    min_out = cur_min;
    max_out = cur_max;
    return qparams_from_minmax(cur_min, cur_max, LLMC_F32, sym, round_zp, qmin, qmax);
}

// One wave per row of the contiguous [G, g] view.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_mse_qparams(const T* __restrict__ W, int64_t G, int g, int sym,
                                                        int round_zp, float qmin, float qmax, int nsteps, int grid,
                                                        float norm, float* __restrict__ scales,
                                                        float* __restrict__ zeros, float* __restrict__ min_out,
                                                        float* __restrict__ max_out) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * (kBlock / 64);
    for (int64_t row = wave; row < G; row += nwaves) {
        float cur_min, cur_max;
        const QParams q = mse_search_row<T>(W + row * g, g, lane, sym, round_zp, qmin, qmax, nsteps, grid, norm,
                                            cur_min, cur_max);
        if (lane == 0) {
            scales[row] = q.s;
            if (zeros) zeros[row] = q.z;
            if (min_out) min_out[row] = cur_min;
            if (max_out) max_out[row] = cur_max;
        }
    }
}

// The same search over the groups of a strided fp32 panel W[r, c0 : c0 + width] (row stride ld), in place: one wave
// per (row, group), group j covers columns c0 + j*gsz .. min(c0 + (j+1)*gsz, c0 + width). GPTQ's column loop runs it
// on the running weights at each block start (gptq_loop.hip). Results go to scales / zeros [r * ng + g0 + j].
__global__ __launch_bounds__(kBlock) void k_mse_panel(const float* __restrict__ W, int64_t R, int64_t ld, int64_t c0,
                                                      int width, int gsz, int sym, int round_zp, float qmin,
                                                      float qmax, int nsteps, int grid, float norm,
                                                      float* __restrict__ scales, float* __restrict__ zeros, int ng,
                                                      int g0) {
    const int lane = threadIdx.x & 63;
    const int nb = (width + gsz - 1) / gsz;
    const int64_t G = R * nb;
    const int64_t wave = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * (kBlock / 64);
    for (int64_t t = wave; t < G; t += nwaves) {
        const int64_t row = t / nb;
        const int j = (int)(t - row * nb);
        const int gw = min(gsz, width - j * gsz);
        float cur_min, cur_max;
        const QParams q = mse_search_row<float>(W + row * ld + c0 + (int64_t)j * gsz, gw, lane, sym, round_zp, qmin,
                                                qmax, nsteps, grid, norm, cur_min, cur_max);
        if (lane == 0) {
            scales[row * ng + g0 + j] = q.s;
            if (zeros) zeros[row * ng + g0 + j] = q.z;
        }
    }
}

extern "C" int llmc_mse_qparams(const void* W, int dt, int64_t G, int64_t g, int sym, int round_zp, float qmin,
                                float qmax, int nsteps, int grid, float norm, float* scales, float* zeros,
                                float* min_out, float* max_out, llmc_stream_t stream) {
    LLMC_REQUIRE(dtype_ok(dt), "mse_qparams: bad dtype");
    LLMC_REQUIRE(W && scales && G > 0 && g > 0 && g < (1ll << 31), "mse_qparams: null/empty argument");
    LLMC_REQUIRE(sym || zeros, "mse_qparams: zeros required for asymmetric");
    LLMC_REQUIRE(nsteps >= 1 && grid >= 1, "mse_qparams: nsteps and grid must be positive");
    hipStream_t st = (hipStream_t)stream;
    const int nblk = capped_grid(G, kBlock / 64, kMaxGrid);
    DISPATCH_DT(dt, hipLaunchKernelGGL((k_mse_qparams<T>), dim3(nblk), dim3(kBlock), 0, st, (const T*)W, G, (int)g, sym,
                                       round_zp, qmin, qmax, nsteps, grid, norm, scales, zeros, min_out, max_out));
    LLMC_LAUNCH_CHECK();
    return LLMC_OK;
}

extern "C" int llmc_mse_qparams_panel(const float* W, int64_t R, int64_t ld, int64_t c0, int64_t width,
                                      int64_t group_size, int sym, int round_zp, float qmin, float qmax, int nsteps,
                                      int grid, float norm, float* scales, float* zeros, int64_t ng, int64_t g0,
                                      llmc_stream_t stream) {
    LLMC_REQUIRE(W && scales && R > 0 && width > 0 && c0 >= 0 && width <= ld - c0,
                 "mse_qparams_panel: null/empty argument or panel outside the row");
    LLMC_REQUIRE(sym || zeros, "mse_qparams_panel: zeros required for asymmetric");
    LLMC_REQUIRE(nsteps >= 1 && grid >= 1, "mse_qparams_panel: nsteps and grid must be positive");
    if (!(group_size == 16 || group_size == 32 || group_size == 64 || group_size == 128)) {
        set_last_error_msg("mse_qparams_panel: group_size must be 16, 32, 64 or 128");
        return LLMC_ENOTSUP;
    }
    LLMC_REQUIRE(width < (1ll << 31), "mse_qparams_panel: panel too wide");
    const int64_t nb = ceil_div64(width, group_size);
    LLMC_REQUIRE(g0 >= 0 && ng >= g0 + nb && ng < (1ll << 31), "mse_qparams_panel: groups outside scales' row");
    hipStream_t st = (hipStream_t)stream;
    const int nblk = capped_grid(R * nb, kBlock / 64, kMaxGrid);
    hipLaunchKernelGGL(k_mse_panel, dim3(nblk), dim3(kBlock), 0, st, W, R, ld, c0, (int)width, (int)group_size, sym,
                       round_zp, qmin, qmax, nsteps, grid, norm, scales, zeros, (int)ng, (int)g0);
    LLMC_LAUNCH_CHECK();
    return LLMC_OK;
}

template <typename T, int KIND>
static int quant_static_tk(const void* W, int64_t G, int64_t g, const void* scales, int sdt,
                           const void* zeros, int zdt, float qmin, float qmax, void* out, hipStream_t st) {
    constexpr int V16 = 16 / sizeof(T);
    bool vec_ok = (g % V16 == 0) && (((uintptr_t)W & 15) == 0) &&
                  (KIND != LLMC_OUT_FAKE || ((uintptr_t)out & 15) == 0);
    LLMC_REQUIRE(g < (1ll << 31), "quant_static: row too long");
    if (vec_ok) {
        int grid = capped_grid(G * (g / V16), kBlock, kMaxGrid);
        hipLaunchKernelGGL((k_quant_static<T, V16, KIND>), dim3(grid), dim3(kBlock), 0, st, (const T*)W, G,
                           (int)g, scales, sdt, zeros, zdt, qmin, qmax, out);
    } else {
        int grid = capped_grid(G * g, kBlock, kMaxGrid);
        hipLaunchKernelGGL((k_quant_static<T, 1, KIND>), dim3(grid), dim3(kBlock), 0, st, (const T*)W, G,
                           (int)g, scales, sdt, zeros, zdt, qmin, qmax, out);
    }
    LLMC_LAUNCH_CHECK();
    return LLMC_OK;
}
template <typename T>
static int quant_static_t(const void* W, int64_t G, int64_t g, const void* scales, int sdt,
                          const void* zeros, int zdt, float qmin, float qmax, int kind, void* out,
                          hipStream_t st) {
    DISPATCH_OUT_KIND(kind, return quant_static_tk<T, KIND>(W, G, g, scales, sdt, zeros, zdt, qmin, qmax, out, st));
    set_last_error_msg("quant_static: bad out_kind");
    return LLMC_EINVAL;
}

extern "C" int llmc_quant_static(const void* W, int wdt, int64_t G, int64_t g, const void* scales, int sdt,
                                 const void* zeros, int zdt, float qmin, float qmax, int out_kind,
                                 void* out, llmc_stream_t stream) {
    LLMC_REQUIRE(dtype_ok(wdt) && dtype_ok(sdt & ~LLMC_SCALAR_QPARAM) && (!zeros || dtype_ok(zdt & ~(LLMC_SCALAR_QPARAM | LLMC_FRACTIONAL_ZP))),
                 "quant_static: bad dtype");
    LLMC_REQUIRE(W && scales && out && G > 0 && g > 0, "quant_static: null/empty argument");
    hipStream_t st = (hipStream_t)stream;
    DISPATCH_DT(wdt, return quant_static_t<T>(W, G, g, scales, sdt, zeros, zdt, qmin, qmax, out_kind, out, st));
}

extern "C" size_t llmc_quant_dynamic_ws_bytes(int64_t G, int64_t g) {
    if (G <= 0 || g <= 0) return 0;
    if (!use_two_stage(G, g)) return 0;
    // partial min/max + a private copy of scales/zeros when the caller does not want them
    return llmc_minmax_qparams_ws_bytes(G, g) + (size_t)G * 8 + 64;
}

template <typename T>
static int quant_dynamic_t(const void* W, int64_t G, int64_t g, int sym, int round_zp, float qmin,
                           float qmax, int kind, void* out, void* scales, void* zeros, hipStream_t st) {
    DISPATCH_OUT_KIND(kind, return launch_quant_rows<T, KIND, false>(W, nullptr, G, g, 1, sym, round_zp, qmin, qmax, out, scales,
                                                                     zeros, st));
    set_last_error_msg("quant_dynamic: bad out_kind");
    return LLMC_EINVAL;
}

extern "C" int llmc_quant_dynamic(const void* W, int dt, int64_t G, int64_t g, int sym, int round_zp,
                                  float qmin, float qmax, int out_kind, void* out, void* scales_out,
                                  void* zeros_out, void* ws, llmc_stream_t stream) {
    LLMC_REQUIRE(dtype_ok(dt), "quant_dynamic: bad dtype");
    LLMC_REQUIRE(W && out && G > 0 && g > 0, "quant_dynamic: null/empty argument");
    LLMC_REQUIRE(round_zp == 1, "quant_dynamic: only round_zp=True is supported");
    hipStream_t st = (hipStream_t)stream;
    if (use_two_stage(G, g)) {
        // few long rows (per_tensor): min/max by the two-stage reduction, then the static kernel
        LLMC_REQUIRE(ws != nullptr, "quant_dynamic: workspace required for long rows");
        char* wsb = (char*)ws;
        size_t off = (llmc_minmax_qparams_ws_bytes(G, g) + 63) & ~(size_t)63;
        void* s = scales_out ? scales_out : (void*)(wsb + off);
        void* z = sym ? nullptr : (zeros_out ? zeros_out : (void*)(wsb + off + (size_t)G * 4));
        int rc = llmc_minmax_qparams(W, dt, G, g, sym, round_zp, qmin, qmax, s, sym ? zeros_out : z, ws, stream);
        if (rc) return rc;
        return llmc_quant_static(W, dt, G, g, s, dt, z, dt, qmin, qmax, out_kind, out, stream);
    }
    LLMC_REQUIRE(g < (1ll << 31), "quant_dynamic: row too long");
    void* zo = sym ? nullptr : zeros_out;
    int rc;
    DISPATCH_DT(dt, rc = quant_dynamic_t<T>(W, G, g, sym, round_zp, qmin, qmax, out_kind, out, scales_out, zo, st));
    if (rc) return rc;
    if (sym && zeros_out) LLMC_HIP_CHECK(hipMemsetAsync(zeros_out, 0, (size_t)G * dtype_size(dt), st));
    return LLMC_OK;
}

// fake_quantize_weight of AWQ's search: k_quant_rows_scaled / k_quant_dynamic_small with the column multiplier, fake values only
extern "C" int llmc_awq_scale_fakequant(const void* W, const void* s, int dt, int64_t R, int64_t K, int64_t g,
                                        int sym, float qmin, float qmax, void* out, llmc_stream_t stream) {
    LLMC_REQUIRE(dtype_ok(dt), "awq_scale_fakequant: bad dtype");
    LLMC_REQUIRE(W && s && out && R > 0 && K > 0, "awq_scale_fakequant: null/empty argument");
    if (g <= 0) g = K;
    LLMC_REQUIRE(K % g == 0 && g < (1ll << 31), "awq_scale_fakequant: K must be a multiple of the group size");
    hipStream_t st = (hipStream_t)stream;
    const int64_t gpr = K / g;      // groups per weight row: group r of the [R * gpr, g] view takes the multipliers s[(r % gpr) * g ...]
    DISPATCH_DT(dt, return launch_quant_rows<T, LLMC_OUT_FAKE, true>(W, s, R * gpr, g, (int)gpr, sym, 1, qmin, qmax, out, nullptr,
                                                                     nullptr, st));
}

extern "C" int llmc_pack_lsb(const void* codes, int code_kind, int64_t R, int64_t K, int bits,
                             int32_t* packed, llmc_stream_t stream) {
    LLMC_REQUIRE(codes && packed && R > 0 && K > 0, "pack_lsb: null/empty argument");
    LLMC_REQUIRE(bits == 4 || bits == 8, "pack_lsb: bits must be 4 or 8");
    LLMC_REQUIRE(code_kind == LLMC_OUT_I32 || code_kind == LLMC_OUT_I8, "pack_lsb: bad code container");
    hipStream_t st = (hipStream_t)stream;
    int pf = 32 / bits;
    int64_t Kp = ceil_div64(K, pf);
    int grid = capped_grid(R * Kp, kBlock, kMaxGrid);
    if (code_kind == LLMC_OUT_I32) {
        bool vec_ok = (K % 4 == 0) && (((uintptr_t)codes & 15) == 0);  // 16-B loads need aligned rows
        if (vec_ok)
            hipLaunchKernelGGL((k_pack_lsb<int32_t, true>), dim3(grid), dim3(kBlock), 0, st,
                               (const int32_t*)codes, R, K, bits, Kp, packed);
        else
            hipLaunchKernelGGL((k_pack_lsb<int32_t, false>), dim3(grid), dim3(kBlock), 0, st,
                               (const int32_t*)codes, R, K, bits, Kp, packed);
    } else {
        hipLaunchKernelGGL((k_pack_lsb<int8_t, false>), dim3(grid), dim3(kBlock), 0, st, (const int8_t*)codes,
                           R, K, bits, Kp, packed);
    }
    LLMC_LAUNCH_CHECK();
    return LLMC_OK;
}

extern "C" int llmc_pack_awq_gemm(const void* weight, int wdt, const void* scales, int sdt, const int32_t* zeros,
                                  int64_t R, int64_t K, int64_t g, int32_t* qweight, int32_t* qzeros,
                                  void* scales_out_f16, llmc_stream_t stream) {
    LLMC_REQUIRE(dtype_ok(wdt) && dtype_ok(sdt), "pack_awq_gemm: bad dtype");
    LLMC_REQUIRE(weight && scales && zeros && qweight && qzeros && scales_out_f16 && R > 0 && K > 0 && g > 0,
                 "pack_awq_gemm: null/empty argument (AutoAWQ needs asymmetric zeros)");
    LLMC_REQUIRE(R % 8 == 0 && K % g == 0, "pack_awq_gemm: R must be a multiple of 8 and K of the group size");
    hipStream_t st = (hipStream_t)stream;
    const int grid = capped_grid(K * (R / 8), kBlock, 8192);
    DISPATCH_DT(wdt, hipLaunchKernelGGL((k_pack_awq_w<T>), dim3(grid), dim3(kBlock), 0, st, (const T*)weight, scales, sdt, zeros, R,
                                        K, g, qweight));
    LLMC_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_pack_awq_z, dim3(capped_grid((K / g) * R, kBlock, 8192)), dim3(kBlock), 0, st, scales, sdt, zeros, R, K / g, qzeros,
                       (uint16_t*)scales_out_f16);
    LLMC_LAUNCH_CHECK();
    return LLMC_OK;
}
