// kv_sink.hip — the attention-sink KV cache's update (SinkKVCache.update, kvsparse.py:569-648 of the reference) as one pass over
// keys and values: the sink rows are copied, the kept window is shifted and (keys, with rope) rotated again by the shift, the new
// rows are appended. The reference slices, multiplies by cos, builds rotate_half with a cat, multiplies by sin, adds and cats
// [sink, kept, new], then slices and cats the values: about a dozen launches and five passes over [B, H, W, D]. The arithmetic
// stays as it is there (a key that survived k steps carries k roundings); here a cached element is read once and written once.
// A lane owns the 16-byte vector at column c < rot / 2 and its partner at c + rot / 2 (rotate_half pairs exactly these), so
// every element is loaded once; columns >= rot (partial_rotation_size) are one vector per lane. Pure streaming: no LDS, no
// cross-lane traffic. Grid: x grid-strides over the (b * H + h, row, vector slot) items, z = keys / values.
#include "common.h"
#include "vec16.h"

namespace llmc {

static constexpr int kSinkBlock = 256;
static constexpr int kSinkMaxGrid = 256 * 8;         // blocks of one launch, keys and values together: 8 per CU

// one of the two tensors of an update (keys, values)
struct SinkSet {
    const void* src;     // [B * H, src_cap, D]
    void* dst;           // [B * H, dst_cap, D]
    const void* rows;    // the new rows [B, H, n_new, D] with element strides sb, sh, st
};
struct SinkArgs {
    SinkSet set[2];
    const void* cos;     // [n_keep, rot] of the tensor dtype, null without rope
    const void* sin;
    int H, D, Tn, n_sink, keep_from, n_keep, rot, P, S, S_shift;
    uint32_t items;
    int64_t src_cap, dst_cap, dst_row0, sb, sh, st;
};

// a * b and a + b rounded to T, as one ATen op each: no contraction into an fma on the fp32 path
template <typename T> __device__ __forceinline__ float mul_t(float a, float b) {
    return to_f32<T>(from_f32<T>(__fmul_rn(a, b)));
}
template <typename T> __device__ __forceinline__ T add_t(float a, float b) {
    return from_f32<T>(__fadd_rn(a, b));
}

template <typename T>
__global__ __launch_bounds__(kSinkBlock) void k_kv_sink(const SinkArgs a) {
    constexpr int VEC = 16 / sizeof(T);
    const SinkSet& S = a.set[blockIdx.z];
    const bool rope = blockIdx.z == 0 && a.cos != nullptr;
    const int half = a.rot >> 1;
    const T* src = (const T*)S.src;
    const T* rows = (const T*)S.rows;
    T* dst = (T*)S.dst;
    const uint32_t stride = gridDim.x * kSinkBlock;
    for (uint32_t i = blockIdx.x * kSinkBlock + threadIdx.x; i < a.items; i += stride) {
        const uint32_t row = a.S_shift >= 0 ? i >> a.S_shift : i / (uint32_t)a.S;
        const int slot = (int)(i - row * (uint32_t)a.S);
        const int bh = (int)(row / (uint32_t)a.Tn);
        const int r = (int)(row - (uint32_t)bh * (uint32_t)a.Tn);
        const bool pair = slot < a.P;
        const int c = pair ? slot * VEC : a.rot + (slot - a.P) * VEC;
        const int k = r - a.n_sink;                  // the row's place in the kept window when 0 <= k < n_keep
        const T* sp;
        if (k < 0) sp = src + ((int64_t)bh * a.src_cap + r) * a.D;
        else if (k < a.n_keep) sp = src + ((int64_t)bh * a.src_cap + a.keep_from + k) * a.D;
        else sp = rows + (int64_t)(bh / a.H) * a.sb + (int64_t)(bh % a.H) * a.sh + (int64_t)(k - a.n_keep) * a.st;
        T* dp = dst + ((int64_t)bh * a.dst_cap + a.dst_row0 + r) * a.D + c;
        Vec<T, VEC> lo = load_vec<T, VEC>(sp + c), hi;
        if (pair) hi = load_vec<T, VEC>(sp + c + half);
        if (rope && pair && k >= 0 && k < a.n_keep) {
            const T* cp = (const T*)a.cos + (int64_t)k * a.rot + c;
            const T* np = (const T*)a.sin + (int64_t)k * a.rot + c;
            const Vec<T, VEC> cl = load_vec<T, VEC>(cp), ch = load_vec<T, VEC>(cp + half);
            const Vec<T, VEC> sl = load_vec<T, VEC>(np), sh = load_vec<T, VEC>(np + half);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const float x1 = to_f32<T>(lo.v[e]), x2 = to_f32<T>(hi.v[e]);
                // rotate_half = cat(-x2, x1): out = rnd(rnd(x * cos) + rnd(rotate_half * sin))
                lo.v[e] = add_t<T>(mul_t<T>(x1, to_f32<T>(cl.v[e])), mul_t<T>(-x2, to_f32<T>(sl.v[e])));
                hi.v[e] = add_t<T>(mul_t<T>(x2, to_f32<T>(ch.v[e])), mul_t<T>(x1, to_f32<T>(sh.v[e])));
            }
        }
        store_vec<T, VEC>(dp, lo);
        if (pair) store_vec<T, VEC>(dp + half, hi);
    }
}

static inline bool sink_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace llmc

using namespace llmc;

extern "C" int llmc_kv_sink_update(int dt, int64_t B, int64_t H, int64_t D, int64_t n_sink, int64_t keep_from, int64_t n_keep,
                                   int64_t n_new, int64_t src_cap, int64_t dst_cap, int64_t dst_row0, int64_t rot,
                                   const void* cos, const void* sin, const void* k_src, void* k_dst, const void* k_new,
                                   const void* v_src, void* v_dst, const void* v_new, int64_t new_stride_b,
                                   int64_t new_stride_h, int64_t new_stride_t, llmc_stream_t stream) {
    LLMC_REQUIRE(dtype_ok(dt), "kv_sink_update: bad dtype");
    LLMC_REQUIRE(B > 0 && H > 0 && D > 0 && n_sink >= 0 && keep_from >= 0 && n_keep >= 0 && n_new >= 0 && dst_row0 >= 0 &&
                     n_sink + n_keep + n_new > 0,
                 "kv_sink_update: bad geometry");
    const int64_t Tn = n_sink + n_keep + n_new;
    const bool moves = n_sink + n_keep > 0;
    LLMC_REQUIRE((cos == nullptr) == (sin == nullptr), "kv_sink_update: cos and sin come together");
    const bool rope = cos != nullptr;
    if (!rope) rot = 0;
    LLMC_REQUIRE(!rope || (rot > 0 && rot <= D && rot % 2 == 0), "kv_sink_update: rot must be even and in (0, D]");
    LLMC_REQUIRE(dst_row0 + Tn <= dst_cap, "kv_sink_update: the destination's capacity is below the row count");
    LLMC_REQUIRE(!moves || (n_sink <= src_cap && (n_keep == 0 || keep_from + n_keep <= src_cap)),
                 "kv_sink_update: the sink or kept rows lie beyond the source's rows");
    const bool have_v = v_src || v_dst || v_new;
    const void* sets[2][3] = {{k_src, k_dst, k_new}, {v_src, v_dst, v_new}};
    for (int i = 0; i < (have_v ? 2 : 1); ++i) {
        LLMC_REQUIRE(sets[i][1], "kv_sink_update: null destination");
        LLMC_REQUIRE(!moves || sets[i][0], "kv_sink_update: null source");
        LLMC_REQUIRE(n_new == 0 || sets[i][2], "kv_sink_update: null new rows");
        LLMC_REQUIRE(!moves || sets[i][0] != sets[i][1], "kv_sink_update: in place only when nothing is moved (n_sink == n_keep == 0)");
    }
    LLMC_REQUIRE(!have_v || k_dst != v_dst, "kv_sink_update: keys and values share a destination");
    auto refuse = [](const char* msg) {
        set_last_error_msg(msg);
        return LLMC_ENOTSUP;
    };
    const int64_t vec = 16 / dtype_size(dt);
    if (D % vec != 0) return refuse("kv_sink_update: a row must be whole 16-byte vectors");
    if ((rot / 2) % vec != 0) return refuse("kv_sink_update: rot / 2 must be whole 16-byte vectors");
    for (int i = 0; i < (have_v ? 2 : 1); ++i)
        if (!sink_aligned16(sets[i][1]) || (moves && !sink_aligned16(sets[i][0])) || (n_new > 0 && !sink_aligned16(sets[i][2])))
            return refuse("kv_sink_update: source, destination and new rows must be 16-byte aligned");
    if (rope && !(sink_aligned16(cos) && sink_aligned16(sin))) return refuse("kv_sink_update: cos and sin must be 16-byte aligned");
    if (n_new > 0 && (new_stride_b % vec != 0 || new_stride_h % vec != 0 || new_stride_t % vec != 0 || new_stride_b < 0 ||
                      new_stride_h < 0 || new_stride_t < 0))
        return refuse("kv_sink_update: rows of the new states must be 16-byte aligned");
    const int64_t P = rot / 2 / vec, S = P + (D - rot) / vec;
    if (B * H * Tn * S >= (1ll << 31) || src_cap * D >= (1ll << 40) || dst_cap * D >= (1ll << 40))
        return refuse("kv_sink_update: cache too large for one launch");

    SinkArgs a;
    for (int i = 0; i < 2; ++i) a.set[i] = SinkSet{sets[i][0], (void*)sets[i][1], sets[i][2]};
    a.cos = cos;
    a.sin = sin;
    a.H = (int)H;
    a.D = (int)D;
    a.Tn = (int)Tn;
    a.n_sink = (int)n_sink;
    a.keep_from = (int)keep_from;
    a.n_keep = (int)n_keep;
    a.rot = (int)rot;
    a.P = (int)P;
    a.S = (int)S;
    a.S_shift = -1;
    for (int sft = 0; sft < 31; ++sft)
        if ((1ll << sft) == S) a.S_shift = sft;
    a.items = (uint32_t)(B * H * Tn * S);
    a.src_cap = src_cap;
    a.dst_cap = dst_cap;
    a.dst_row0 = dst_row0;
    a.sb = new_stride_b;
    a.sh = new_stride_h;
    a.st = new_stride_t;
    const int nz = have_v ? 2 : 1;
    const int cap = opt(OPT_KV_SINK_MAX_GRID) > 0 ? opt(OPT_KV_SINK_MAX_GRID) : kSinkMaxGrid / nz;
    const dim3 grid(capped_grid(a.items, kSinkBlock, cap), 1, nz);
    DISPATCH_DT(dt, hipLaunchKernelGGL((k_kv_sink<T>), grid, dim3(kSinkBlock), 0, (hipStream_t)stream, a));
    LLMC_LAUNCH_CHECK();
    return LLMC_OK;
}
