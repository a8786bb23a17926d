// mixed_quant.hip — IntegerQuantizer.fake_quant_act_dynamic / fake_quant_weight_dynamic with `int_indices` / `fp_indices`
// (llmc quant.py:754-783, 833-869; the methods QUIK and LLM.int8()): some columns are fake-quantized, some pass through in
// 16 bit, the rest are zero. The reference spells it gather -> quantize -> zeros_like -> two scatters; here a row is read from
// HBM once (16-byte loads), waits in LDS, and is written once. The group step is quant_group.h's, so a group gives bit for bit
// what llmc_quant_dynamic (round_zp) or llmc_minmax_qparams + llmc_quant_static (fractional zero point) give on the gathered
// copy.
//
// Two kernels:
//   k_mixed_mask  one group per row (per_token / per_channel): the group is "every column whose role has bit 0 set", no
//                 order is needed. A team of lanes owns a row; each lane keeps its own vectors in LDS between the reduction and
//                 the rounding (it reads back only what it wrote: no LDS traffic between lanes), and stores the finished
//                 vectors to HBM directly. Teams: 1 - 64 lanes of a wave (several rows per workgroup) or the workgroup.
//   k_mixed_idx   groups in the order of int_idx (per_group; QUIK's list is ordered by activation scale, not by column). The
//                 workgroup's rows are copied to LDS (role 0 zeroed on the way), groups are spread over sub-wave lane teams
//                 like quant_rows' rows (lpr lanes per group, wave_min / wave_max), which gather and write back inside LDS,
//                 then the rows are copied out. The gather is a 2- or 4-byte ds_read per lane at arbitrary addresses: a
//                 random order costs bank conflicts (lanes of one 32-lane half on one bank, cdna LDS banking), not uncoalesced
//                 HBM accesses; int_idx itself is read coalesced and, like role, is shared by all rows (L2).
#include "common.h"
#include "quant_group.h"
#include "quant_math.h"

namespace llmc {

static constexpr int MB = 256;                    // threads per workgroup
static constexpr int MQ_LDS_MAX = 160 * 1024;     // gfx950: LDS of a CU, and the most one workgroup may ask for
static constexpr int MQ_RED = 64;                 // workgroup-reduction scratch in front of the rows (dynamic region only)
static constexpr int MQ_MULTI_ROW_LDS = 64 * 1024;   // k_mixed_idx takes several rows per workgroup up to this many bytes

// the roles of V consecutive columns (V = 8 / 4: one aligned load; the host checks role's alignment)
template <int V> struct RoleVec {
    uint8_t r[V];
};
template <int V> __device__ __forceinline__ RoleVec<V> load_role(const uint8_t* p) {
    RoleVec<V> r;
    if constexpr (V == 8) {
        const uint2 raw = *reinterpret_cast<const uint2*>(p);
        __builtin_memcpy(&r, &raw, 8);
    } else if constexpr (V == 4) {
        const uint32_t raw = *reinterpret_cast<const uint32_t*>(p);
        __builtin_memcpy(&r, &raw, 4);
    } else {
#pragma unroll
        for (int i = 0; i < V; ++i) r.r[i] = p[i];
    }
    return r;
}

// A group takes either branch of round_zp at run time (GroupQuant<true>): round_zp = 0 is the reference's fractional zero point,
// exactly as k_quant_static evaluates LLMC_FRACTIONAL_ZP. The select is written out here, fractional arm first, as it always
// was: q.fake() states it the other way round (the column kernels' order), and with that block order k_mixed_idx measured
// 0.6 % slower than the parent commit's, above the run-to-run spread (profiles/quant_group_refactor.txt). With this select and
// the pairwise block_minmax both kernels compile to the parent's instruction stream.
using MixedQuant = GroupQuant<true>;
template <typename T> __device__ __forceinline__ T fake_value(T x, const MixedQuant& q, float qmin, float qmax) {
    const float f = to_f32<T>(x);
    const float c = q.fz ? quant_code_fz(f, q.dv, q.z, q.p1, q.p2, qmin, qmax) : quant_code(f, q.dv, q.z, q.p1, q.p2, qmin, qmax);
    return from_f32<T>(dequant_code(c, q.s, q.z, q.p2));
}

// X and out may be the same buffer: a workgroup reads its rows completely before it writes them, and no other reads them.
template <typename T, int V>
__global__ __launch_bounds__(MB) void k_mixed_mask(const T* X, int64_t N, int K, const uint8_t* __restrict__ role, int ts,
                                                   int sym, int round_zp, float qmin, float qmax, T* out) {
    extern __shared__ __attribute__((aligned(16))) char mq_smem[];
    constexpr int DT = dt_of<T>::value;
    float* red = (float*)mq_smem;
    T* rows = (T*)(mq_smem + MQ_RED);
    const int rpb = MB / ts;
    const int team = threadIdx.x / ts, tl = threadIdx.x % ts;
    const int64_t row = (int64_t)blockIdx.x * rpb + team;
    const bool valid = row < N;                          // a team past the last row computes on row N - 1 and stores nothing
    const int64_t rr = valid ? row : N - 1;
    const T* xp = X + rr * K;
    T* lp = rows + (size_t)team * K;
    float mn = INFINITY, mx = -INFINITY;
    for (int c = tl * V; c < K; c += ts * V) {
        const Vec<T, V> v = load_vec<T, V>(xp + c);
        const RoleVec<V> r = load_role<V>(role + c);
        store_vec<T, V>(lp + c, v);
#pragma unroll
        for (int i = 0; i < V; ++i) {
            if (r.r[i] & 1) {
                const float f = to_f32<T>(v.v[i]);
                mn = fminf(mn, f);
                mx = fmaxf(mx, f);
            }
        }
    }
    if (ts <= 64) {
        mn = wave_min(mn, ts);
        mx = wave_max(mx, ts);
    } else {
        block_minmax<MB, true>(red, mn, mx);
    }
    if (!valid) return;
    const MixedQuant q = MixedQuant::from_minmax(mn, mx, DT, sym, round_zp, qmin, qmax);
    T* op = out + rr * K;
    for (int c = tl * V; c < K; c += ts * V) {
        const Vec<T, V> v = load_vec<T, V>(lp + c);
        const RoleVec<V> r = load_role<V>(role + c);
        Vec<T, V> o;
#pragma unroll
        for (int i = 0; i < V; ++i)
            o.v[i] = r.r[i] == 1 ? fake_value<T>(v.v[i], q, qmin, qmax) : (r.r[i] == 0 ? zero_of<T>() : v.v[i]);
        store_vec<T, V>(op + c, o);
    }
}

template <typename T, int V>
__global__ __launch_bounds__(MB) void k_mixed_idx(const T* X, int64_t N, int K, const uint8_t* __restrict__ role,
                                                  const int32_t* __restrict__ idx, int ng, int g, int lpr, int rpb, int sym,
                                                  int round_zp, float qmin, float qmax, T* out) {
    extern __shared__ __attribute__((aligned(16))) char mq_smem[];
    constexpr int DT = dt_of<T>::value;
    float* red = (float*)mq_smem;
    T* rows = (T*)(mq_smem + MQ_RED);
    const int64_t row0 = (int64_t)blockIdx.x * rpb;
    const int nr = (int)(N - row0 < rpb ? N - row0 : rpb);
    const int64_t base = row0 * K;
    const int total = nr * K;                 // the workgroup's rows are one contiguous piece; V divides K
    for (int e = threadIdx.x * V; e < total; e += MB * V) {
        Vec<T, V> v = load_vec<T, V>(X + base + e);
        const RoleVec<V> r = load_role<V>(role + e % K);
#pragma unroll
        for (int i = 0; i < V; ++i)
            if (r.r[i] == 0) v.v[i] = zero_of<T>();
        store_vec<T, V>(rows + e, v);
    }
    __syncthreads();
    const int items = nr * ng;                // (row, group) pairs of this workgroup
    if (lpr <= 64) {
        const int nteams = MB / lpr;
        const int team = threadIdx.x / lpr, sl = threadIdx.x % lpr;
        for (int it0 = 0; it0 < items; it0 += nteams) {
            const bool valid = it0 + team < items;          // idle teams recompute the last item (shuffles need every lane)
            const int it = valid ? it0 + team : items - 1;
            const int r = it / ng, j = it - r * ng;
            T* lp = rows + (size_t)r * K;
            const int32_t* ip = idx + (size_t)j * g;
            float mn = INFINITY, mx = -INFINITY;
            for (int e = sl; e < g; e += lpr) {
                const int col = ip[e];
                if ((unsigned)col >= (unsigned)K) continue;
                const float f = to_f32<T>(lp[col]);
                mn = fminf(mn, f);
                mx = fmaxf(mx, f);
            }
            mn = wave_min(mn, lpr);
            mx = wave_max(mx, lpr);
            if (!valid) continue;
            const MixedQuant q = MixedQuant::from_minmax(mn, mx, DT, sym, round_zp, qmin, qmax);
            for (int e = sl; e < g; e += lpr) {
                const int col = ip[e];
                if ((unsigned)col >= (unsigned)K) continue;
                if (role[col] == 1) lp[col] = fake_value<T>(lp[col], q, qmin, qmax);
            }
        }
    } else {                                  // long groups: the workgroup is the team
        for (int it = 0; it < items; ++it) {
            const int r = it / ng, j = it - r * ng;
            T* lp = rows + (size_t)r * K;
            const int32_t* ip = idx + (size_t)j * g;
            float mn = INFINITY, mx = -INFINITY;
            for (int e = threadIdx.x; e < g; e += MB) {
                const int col = ip[e];
                if ((unsigned)col >= (unsigned)K) continue;
                const float f = to_f32<T>(lp[col]);
                mn = fminf(mn, f);
                mx = fmaxf(mx, f);
            }
            block_minmax<MB, true>(red, mn, mx);
            const MixedQuant q = MixedQuant::from_minmax(mn, mx, DT, sym, round_zp, qmin, qmax);
            for (int e = threadIdx.x; e < g; e += MB) {
                const int col = ip[e];
                if ((unsigned)col >= (unsigned)K) continue;
                if (role[col] == 1) lp[col] = fake_value<T>(lp[col], q, qmin, qmax);
            }
        }
    }
    __syncthreads();
    for (int e = threadIdx.x * V; e < total; e += MB * V) store_vec<T, V>(out + base + e, load_vec<T, V>(rows + e));
}

static inline bool mq_aligned(const void* p, int a) { return ((uintptr_t)p & (uintptr_t)(a - 1)) == 0; }

template <typename T>
static int mixed_t(const void* X, int64_t N, int64_t K, const uint8_t* role, const int32_t* idx, int64_t n_int, int64_t g,
                   int sym, int round_zp, float qmin, float qmax, void* out, hipStream_t st) {
    constexpr int V16 = 16 / sizeof(T);
    const bool vec_ok = K % V16 == 0 && mq_aligned(X, 16) && mq_aligned(out, 16) && mq_aligned(role, V16);
    const int64_t row_bytes = K * (int64_t)sizeof(T);
    if (idx == nullptr) {
        const int64_t nvec = vec_ok ? K / V16 : K;
        int ts = pow2_ceil(ceil_div64(nvec, 4));          // about four vectors per lane
        if (ts > 64) ts = MB;
        const int rpb = MB / ts;
        const int64_t blocks = ceil_div64(N, rpb);
        LLMC_REQUIRE(blocks < (1ll << 31), "quant_dynamic_mixed: too many rows");
        const size_t lds = (size_t)(MQ_RED + rpb * row_bytes);
        const auto kernel = vec_ok ? k_mixed_mask<T, V16> : k_mixed_mask<T, 1>;
        if (int rc = ensure_dynamic_lds((const void*)kernel, MQ_LDS_MAX)) return rc;
        hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(MB), lds, st, (const T*)X, N, (int)K, role, ts, sym, round_zp,
                           qmin, qmax, (T*)out);
    } else {
        const int64_t ng = n_int / g;
        int lpr = MB;                                     // groups above 1024 columns: the workgroup is the team
        if (g <= 1024) {
            lpr = pow2_ceil(ceil_div64(g, 8));            // about eight columns per lane
            if (lpr > 64) lpr = 64;
        }
        const int nteams = lpr <= 64 ? MB / lpr : 1;
        int64_t rpb = ceil_div64(nteams, ng);             // enough rows to give every team a group
        const int64_t cap = MQ_MULTI_ROW_LDS / row_bytes;
        if (rpb > cap) rpb = cap;
        if (rpb > N) rpb = N;
        if (rpb < 1) rpb = 1;
        const int64_t blocks = ceil_div64(N, rpb);
        LLMC_REQUIRE(blocks < (1ll << 31), "quant_dynamic_mixed: too many rows");
        const size_t lds = (size_t)(MQ_RED + rpb * row_bytes);
        const auto kernel = vec_ok ? k_mixed_idx<T, V16> : k_mixed_idx<T, 1>;
        if (int rc = ensure_dynamic_lds((const void*)kernel, MQ_LDS_MAX)) return rc;
        hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(MB), lds, st, (const T*)X, N, (int)K, role, idx, (int)ng, (int)g,
                           lpr, (int)rpb, sym, round_zp, qmin, qmax, (T*)out);
    }
    LLMC_LAUNCH_CHECK();
    return LLMC_OK;
}

}  // namespace llmc

using namespace llmc;

extern "C" int llmc_quant_dynamic_mixed_fits(int dt, int64_t K) {
    if (!dtype_ok(dt) || K <= 0) return 0;
    return MQ_RED + K * (int64_t)dtype_size(dt) <= MQ_LDS_MAX ? 1 : 0;
}

extern "C" int llmc_quant_dynamic_mixed(const void* X, int dt, int64_t N, int64_t K, const uint8_t* role,
                                        const int32_t* int_idx, int64_t n_int, int64_t g, int sym, int round_zp, float qmin,
                                        float qmax, void* out, llmc_stream_t stream) {
    LLMC_REQUIRE(dtype_ok(dt), "quant_dynamic_mixed: bad dtype");
    LLMC_REQUIRE(X && role && out && N > 0 && K > 0, "quant_dynamic_mixed: null/empty argument");
    LLMC_REQUIRE(n_int > 0 && g > 0 && n_int % g == 0, "quant_dynamic_mixed: n_int must be a positive multiple of g");
    LLMC_REQUIRE(n_int <= K, "quant_dynamic_mixed: more integer columns than columns (duplicate entries)");
    LLMC_REQUIRE(int_idx || g == n_int, "quant_dynamic_mixed: int_idx may be null only with one group per row");
    if (!llmc_quant_dynamic_mixed_fits(dt, K)) {
        set_last_error_msg("quant_dynamic_mixed: the row does not fit the LDS of a CU");
        return LLMC_ENOTSUP;
    }
    hipStream_t st = (hipStream_t)stream;
    DISPATCH_DT(dt, return mixed_t<T>(X, N, K, role, int_idx, n_int, g, sym, round_zp, qmin, qmax, out, st));
    return LLMC_OK;
}
