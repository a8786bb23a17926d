// kv_cache.hip — the quantized KV cache's update (kvquant.py:44-87, 233-289 of the reference) as one pass: dequantize the stored
// rows, append the new ones, and (REQUANT) derive every row's codes and qparams again from those values, in place.
// The reference does dequant(whole cache) -> cat -> contiguous -> amax / amin -> quant(whole cache) on 16-bit float codes: about
// ten passes over [B, H, T, D]. Here an old element costs 1 byte read (its code) and 2 + 1 bytes written (the returned value and
// the new code); qparams add 2 x 2 x sizeof(T) / g bytes.
// A sibling of k_quant_dynamic_small (quant_kernels.hip): a group is lpr = g / VEC lanes of one 16-byte vector each, a wave takes
// 64 / lpr groups, UNR of them in flight per lane. The arithmetic is quant_group.h's (GroupQuant::from_minmax, code) and
// quant_math.h's dequant_code; the vectors are vec16.h's.
// Grid: x walks the T * D / g groups of one (b, h), y = b * H + h, z = keys / values.
#include "common.h"
#include "quant_group.h"
#include "quant_math.h"

namespace llmc {

static constexpr int kKvBlock = 256;
static constexpr int kKvMaxGridX = 256 * 8;
static constexpr int kKvUnr = 4;

// one of the two tensors of an update (keys, values)
struct KvSet {
    uint8_t* codes;      // [B * H, cap, D], one code per byte (two's complement when qmin < 0)
    void* scales;        // [B * H, cap, D / g] of the tensor dtype
    void* zeros;         // same, null when symmetric
    const void* rows;    // the new rows [B, H, n_new, D] with element strides sb, sh, st
    void* out;           // [B, H, T, D] contiguous, may be null with REQUANT
};
struct KvArgs {
    KvSet set[2];
    int H, T_old, T, cap, D, g, gpr, gpr_shift, lpr;
    int64_t sb, sh, st;
    int sym, is_signed, new_fake;
    float qmin, qmax;
};

// the VEC code bytes beside a lane's VEC elements of T: one 8- or 4-byte access (p is VEC-byte aligned)
template <int VEC> __device__ __forceinline__ Vec<uint8_t, VEC> load_codes(const uint8_t* p) {
    Vec<uint8_t, VEC> r;
    std::conditional_t<VEC == 8, uint2, uint32_t> raw = *reinterpret_cast<const decltype(raw)*>(p);
    __builtin_memcpy(&r, &raw, VEC);
    return r;
}

template <typename T, bool REQUANT>
__global__ __launch_bounds__(kKvBlock) void k_kv_update(const KvArgs a) {
    constexpr int DT = dt_of<T>::value;
    constexpr int VEC = 16 / sizeof(T);
    constexpr int UNR = kKvUnr;
    const KvSet& S = a.set[blockIdx.z];
    const int bh = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int rpw = 64 / a.lpr;
    const int sub = lane / a.lpr, sl = lane % a.lpr;
    const int total = a.T * a.gpr;                       // groups of this (b, h); the host checked that it fits
    const int64_t wave = (int64_t)blockIdx.x * (kKvBlock / 64) + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * (kKvBlock / 64);
    const T* rows = (const T*)S.rows + (int64_t)(bh / a.H) * a.sb + (int64_t)(bh % a.H) * a.sh;
    T* out = S.out ? (T*)S.out + (int64_t)bh * a.T * a.D : nullptr;
    uint8_t* codes = S.codes + (int64_t)bh * a.cap * a.D;
    T* scales = (T*)S.scales + (int64_t)bh * a.cap * a.gpr;
    T* zeros = S.zeros ? (T*)S.zeros + (int64_t)bh * a.cap * a.gpr : nullptr;

    for (int64_t i0 = wave * rpw * UNR; i0 < total; i0 += nwaves * rpw * UNR) {
        Vec<T, VEC> v[UNR];
        Vec<uint8_t, VEC> c[UNR];
        float s[UNR], z[UNR];
        bool valid[UNR], old[UNR];
        int t[UNR], col[UNR], j[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int64_t iw = i0 + u * rpw + sub;
            valid[u] = iw < total;
            const int i = valid[u] ? (int)iw : total - 1;            // a clamped group is loaded again and stores nothing
            t[u] = a.gpr_shift >= 0 ? i >> a.gpr_shift : i / a.gpr;
            j[u] = i - t[u] * a.gpr;
            col[u] = j[u] * a.g + sl * VEC;
            old[u] = t[u] < a.T_old;
            if (old[u]) {
                c[u] = load_codes<VEC>(codes + (int64_t)t[u] * a.D + col[u]);
                s[u] = to_f32<T>(scales[(int64_t)t[u] * a.gpr + j[u]]);
                z[u] = zeros ? to_f32<T>(zeros[(int64_t)t[u] * a.gpr + j[u]]) : 0.0f;
            } else {
                v[u] = load_vec<T, VEC>(rows + (int64_t)(t[u] - a.T_old) * a.st + col[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            if (old[u]) {
#pragma unroll
                for (int k = 0; k < VEC; ++k) {
                    const int b = a.is_signed ? (int)(int8_t)c[u].v[k] : (int)c[u].v[k];
                    v[u].v[k] = from_f32<T>(dequant_code((float)b, s[u], z[u], DT));
                }
            }
            T* op = out ? out + (int64_t)t[u] * a.D + col[u] : nullptr;
            if constexpr (!REQUANT) {
                if (valid[u]) store_vec<T, VEC>(op, v[u]);
            } else {
                float mn = INFINITY, mx = -INFINITY;
#pragma unroll
                for (int k = 0; k < VEC; ++k) {
                    const float f = to_f32<T>(v[u].v[k]);
                    mn = fminf(mn, f);
                    mx = fmaxf(mx, f);
                }
                mn = wave_min(mn, a.lpr);                // every lane of the wave takes part: clamped groups carry real data
                mx = wave_max(mx, a.lpr);
                const GroupQuant<> q = GroupQuant<>::from_minmax(mn, mx, DT, a.sym, 1, a.qmin, a.qmax);
                if (!valid[u]) continue;                 // the store is updated in place: nothing is written twice
                if (sl == 0) {
                    scales[(int64_t)t[u] * a.gpr + j[u]] = from_f32<T>(q.s);
                    if (zeros) zeros[(int64_t)t[u] * a.gpr + j[u]] = from_f32<T>(q.z);
                }
                const bool fake = a.new_fake && !old[u];
                Vec<uint8_t, VEC> o;
#pragma unroll
                for (int k = 0; k < VEC; ++k) {
                    const float code = q.code(to_f32<T>(v[u].v[k]), a.qmin, a.qmax);
                    o.v[k] = (uint8_t)(int)code;
                    if (fake) v[u].v[k] = from_f32<T>(dequant_code(code, q.s, q.z, q.p2));
                }
                store_vec_wide<uint8_t, VEC>(codes + (int64_t)t[u] * a.D + col[u], o);
                if (op) store_vec<T, VEC>(op, v[u]);
            }
        }
    }
}

static inline bool kv_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace llmc

using namespace llmc;

extern "C" int llmc_kv_cache_update(int dt, int64_t B, int64_t H, int64_t T_old, int64_t n_new, int64_t cap, int64_t D,
                                    int64_t g, int sym, int round_zp, float qmin, float qmax, int flags, void* k_codes,
                                    void* k_scales, void* k_zeros, const void* k_new, void* k_out, void* v_codes,
                                    void* v_scales, void* v_zeros, const void* v_new, void* v_out, int64_t new_stride_b,
                                    int64_t new_stride_h, int64_t new_stride_t, llmc_stream_t stream) {
    LLMC_REQUIRE(dtype_ok(dt), "kv_cache_update: bad dtype");
    LLMC_REQUIRE((flags & ~(LLMC_KV_REQUANT | LLMC_KV_NEW_FAKE)) == 0, "kv_cache_update: unknown flag");
    const bool requant = (flags & LLMC_KV_REQUANT) != 0, new_fake = (flags & LLMC_KV_NEW_FAKE) != 0;
    LLMC_REQUIRE(!new_fake || requant, "kv_cache_update: NEW_FAKE needs REQUANT");
    LLMC_REQUIRE(B > 0 && H > 0 && T_old >= 0 && n_new >= 0 && T_old + n_new > 0 && D > 0 && g > 0 && D % g == 0,
                 "kv_cache_update: bad geometry");
    const int64_t T = T_old + n_new;
    LLMC_REQUIRE(cap >= T_old && (!requant || cap >= T), "kv_cache_update: the store's capacity is below the row count");
    LLMC_REQUIRE(qmin <= qmax && qmin == floorf(qmin) && qmax == floorf(qmax), "kv_cache_update: bad code range");
    const bool have_v = v_codes || v_scales || v_zeros || v_new || v_out;
    const void* sets[2][5] = {{k_codes, k_scales, k_zeros, k_new, k_out}, {v_codes, v_scales, v_zeros, v_new, v_out}};
    for (int i = 0; i < (have_v ? 2 : 1); ++i) {
        LLMC_REQUIRE(sets[i][0] && sets[i][1], "kv_cache_update: null code store or scales");
        LLMC_REQUIRE((sets[i][2] == nullptr) == (sym != 0), "kv_cache_update: zeros must be given exactly when asymmetric");
        LLMC_REQUIRE(n_new == 0 || sets[i][3], "kv_cache_update: null new rows");
        LLMC_REQUIRE(sets[i][4] || requant, "kv_cache_update: null out without REQUANT");
        LLMC_REQUIRE(kv_aligned16(sets[i][0]) && kv_aligned16(sets[i][3]) && kv_aligned16(sets[i][4]),
                     "kv_cache_update: codes, new rows and out must be 16-byte aligned");
    }
    auto refuse = [](const char* msg) {
        set_last_error_msg(msg);
        return LLMC_ENOTSUP;
    };
    if (round_zp != 1) return refuse("kv_cache_update: only round_zp=True is fused");
    if (qmin < -128.0f || qmax > 255.0f || (qmin < 0.0f && qmax > 127.0f)) return refuse("kv_cache_update: codes of at most 8 bits");
    const int64_t vec = 16 / dtype_size(dt);
    const int64_t lpr = g / vec;
    if (g % vec != 0 || lpr > 64 || (lpr & (lpr - 1)) != 0)
        return refuse("kv_cache_update: a group must be 16 bytes times a power of two <= 64");
    if (n_new > 0 && (new_stride_b % vec != 0 || new_stride_h % vec != 0 || new_stride_t % vec != 0 || new_stride_b < 0 ||
                      new_stride_h < 0 || new_stride_t < 0))
        return refuse("kv_cache_update: rows of the new states must be 16-byte aligned");
    const int64_t gpr = D / g;
    if (B * H > 65535 || T * gpr >= (1ll << 31) || cap * D >= (1ll << 40)) return refuse("kv_cache_update: cache too large for one launch");

    KvArgs a;
    for (int i = 0; i < 2; ++i)
        a.set[i] = KvSet{(uint8_t*)sets[i][0], (void*)sets[i][1], (void*)sets[i][2], sets[i][3], (void*)sets[i][4]};
    a.H = (int)H;
    a.T_old = (int)T_old;
    a.T = (int)T;
    a.cap = (int)cap;
    a.D = (int)D;
    a.g = (int)g;
    a.gpr = (int)gpr;
    a.gpr_shift = -1;
    for (int sft = 0; sft < 31; ++sft)
        if ((1ll << sft) == gpr) a.gpr_shift = sft;
    a.lpr = (int)lpr;
    a.sb = new_stride_b;
    a.sh = new_stride_h;
    a.st = new_stride_t;
    a.sym = sym != 0;
    a.is_signed = qmin < 0.0f;
    a.new_fake = new_fake;
    a.qmin = qmin;
    a.qmax = qmax;
    const int per_block = (int)(64 / lpr) * kKvUnr * (kKvBlock / 64);
    const dim3 grid(capped_grid(T * gpr, per_block, kKvMaxGridX), (unsigned)(B * H), have_v ? 2 : 1);
    hipStream_t st = (hipStream_t)stream;
    if (requant) {
        DISPATCH_DT(dt, hipLaunchKernelGGL((k_kv_update<T, true>), grid, dim3(kKvBlock), 0, st, a));
    } else {
        DISPATCH_DT(dt, hipLaunchKernelGGL((k_kv_update<T, false>), grid, dim3(kKvBlock), 0, st, a));
    }
    LLMC_LAUNCH_CHECK();
    return LLMC_OK;
}
