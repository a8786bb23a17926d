// i8_linear.hip — the W8A8 integer Linear: A [M, K] and B [N, K] int8 codes whose scales are constant along K (one per token or
// one per tensor for A, one per output channel or one per tensor for B), the stored form deploy('vllm_quant' | 'sgl_quant' | ...)
// writes for the reference's backend/{vllm,sglang}/{smoothquant,awq,rtn}_w8a8 configurations (an extension: its real-quant
// Linears raise in forward).
//   llmc_i8_scaled_gemm     acc[m, n] = sum_k a[m, k] b[n, k] in int32 on the integer matrix pipe,
//                           C[m, n] = rnd_out(fl(fl(float(acc) * a_s[m]) * b_s[n])), then the bias in the output dtype
// float(acc) is v_cvt_f32_i32, round to nearest even. Nothing is de-quantized in the K loop: it holds loads, LDS traffic and
// matrix instructions only; both scales act in the epilogue. The tile and decode rungs' structure is scaled8_gemm.h's, shared
// with fp8_linear.hip; this file states the number format (I8Code), the split-K rung, the ladder and the entry points.
//
// Matrix instructions: v_mfma_i32_32x32x32_i8 (tile rung) and v_mfma_i32_16x16x64_i8 (decode rungs), 16 operand bytes per lane
// and instruction. The int32 accumulator is exact: there is no accumulation window like the fp8 forms' (DESIGN.md K22 / K24), any
// order of adding gives the same bits, and a zeroed operand byte adds exactly 0, which is what lets K be ragged (K % 16 == 0).
// K <= 65536 keeps the worst case 128 * 128 * K = 2^30 below 2^31.
//
// Rungs (which shape takes which: I8_LADDER below, one table): scaled8_gemm.h's tile128 and decode, and
//   decode_split  the decode rung with K also cut into S slices across workgroups (grid N / 16 x S) for layers with too few column
//                 tiles to fill the chip. A slice stores its int32 tile to the caller's workspace [S, M, N] with plain vector
//                 stores; k_i8_split_reduce adds the S partials and applies the epilogue. No atomics, no counters: two launches.
#include "scaled8_gemm.h"

namespace llmc {

struct I8Code {
    typedef int acc_t;
    static constexpr bool RAGGED_K = true;
    static __device__ __forceinline__ i32x16 mac32(i32x4 a, i32x4 b, i32x16 c) { return mfma_i32_32x32x32_i8(a, b, c); }
    static __device__ __forceinline__ i32x4 mac16(i32x4 a, i32x4 b, i32x4 c) { return mfma_i32_16x16x64_i8(a, b, c); }
    static __device__ __forceinline__ float to_float(int acc) { return (float)acc; }
};
struct I8Args : Scaled8Args {
    int32_t* ws;              // decode_split: the slices' partial tiles [S, M, N]
    int kb_per;               // decode_split: K blocks of 128 per slice
};

template <int DT, int WM, int WN>
__global__ __launch_bounds__(256) void k_i8_scaled_tile(I8Args a) { s8_tile_body<I8Code, DT, WM, WN>(a); }

template <int DT, int MT, bool SPLIT>
__global__ __launch_bounds__(64 * S8D_WAVES) void k_i8_scaled_decode(I8Args a) { s8_decode_body<I8Code, DT, MT, SPLIT>(a); }

// decode_split, second launch: one thread per output adds its S partials and applies the epilogue
template <int DT>
__global__ __launch_bounds__(256) void k_i8_split_reduce(I8Args a, int S) {
    const int64_t mn = a.M * a.N, i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= mn) return;
    int s = 0;
    for (int sl = 0; sl < S; ++sl) s += a.ws[sl * mn + i];
    const int64_t row = i / a.N, col = i - row * a.N;
    s8_store<I8Code, DT>(a, row, col, s, a.As[a.as_rows ? row : 0], a.Bs[a.bs_rows ? col : 0]);
}

// ---------------------------------------------------------------------------------------------------------------
// which rung takes which shape: the first row whose bounds hold. Set from tools/bench_i8_linear.py (profiles/i8_linear.txt):
// up to 64 tokens the decode rung is 2.8 to 9 times faster than the tile rung on three of the four Llama-3-8B shapes (1.3 to 2.3
// times on 14336 x 4096 up to 32 tokens). decode_split beats decode only on the k / v shape (1024 x 4096: 64 column tiles for 256
// CUs) with 2 or 4 row tiles: 8.5 against 9.7 us at 32 tokens, 11.0 against 14.9 us at 64, with S = 4 (one workgroup per CU; S = 2
// and 8 are slower); at 16 tokens and below the second launch costs more than the idle CUs (7.8 against 6.9 us), and from
// N = 4096 up it loses at every token count. So: 17 .. 64 tokens, N / 16 <= CUs / 4, K >= 4096, the only place it was seen to win.
// With 4 row tiles the decode rung is instruction-bound, and on the widest shape (14336 x 4096: 112 tiles of 128 columns) the tile
// rung passes it at 64 tokens, 45.2 against 51.4 us (at 32 tokens 41.1 against 32.4; on 4096 x 4096 at 64 tokens 43.4 against
// 15.5): 33 .. 64 tokens with N >= 14336 go to tile128. Both kernels' times grow with K alike, so the row has no K bound.
// ---------------------------------------------------------------------------------------------------------------
enum { I8_DECODE = 0, I8_TILE128 = 1, I8_DECODE_SPLIT = 2, I8_NRUNGS = 3 };
static constexpr int I8_SPLIT_MAX = 16;         // most K slices
struct I8Rung {
    int64_t min_m, max_m;   // min_m <= M <= max_m
    int cu_share;           // > 0: the column tiles (N / 16) fill at most 1 / cu_share of the CUs
    int64_t min_k;          // K >= min_k
    int64_t min_n;          // N >= min_n
    int rung;
};
static const I8Rung I8_LADDER[] = {
    {17, S8_DECODE_MAX_M, 4, 4096, 1, I8_DECODE_SPLIT},
    {33, S8_DECODE_MAX_M, 0, 0, 14336, I8_TILE128},
    {1, S8_DECODE_MAX_M, 0, 0, 1, I8_DECODE},
    {1, INT64_MAX, 0, 0, 1, I8_TILE128},
};

static int i8_pick_rung(int64_t M, int64_t N, int64_t K) {
    const int64_t ct = ceil_div64(N, S8D_N);
    for (const I8Rung& r : I8_LADDER)
        if (M >= r.min_m && M <= r.max_m && K >= r.min_k && N >= r.min_n && (r.cu_share == 0 || ct * r.cu_share <= device_cu_count())) return r.rung;
    return I8_TILE128;
}

// decode_split's K blocks per slice: one workgroup per CU (option i8_split_slices = n > 0: n slices), at most I8_SPLIT_MAX
// slices, none of them empty. The slice count is ceil(nkb / the result).
static int i8_split_kb_per(int64_t N, int64_t K) {
    const int64_t nkb = ceil_div64(K, S8_KB), ct = ceil_div64(N, S8D_N);
    int64_t s = opt(OPT_I8_SPLIT_SLICES) > 0 ? opt(OPT_I8_SPLIT_SLICES) : ceil_div64(device_cu_count(), ct);
    s = s > I8_SPLIT_MAX ? I8_SPLIT_MAX : s;
    s = s > nkb ? nkb : s;
    return (int)ceil_div64(nkb, s < 1 ? 1 : s);
}
static int i8_split_slices(int64_t N, int64_t K) { return (int)ceil_div64(ceil_div64(K, S8_KB), i8_split_kb_per(N, K)); }

template <int DT, bool SPLIT>
static void i8_launch_decode(const I8Args& a, dim3 grid, hipStream_t st) {
    s8_launch_decode(a, grid, st, k_i8_scaled_decode<DT, 1, SPLIT>, k_i8_scaled_decode<DT, 2, SPLIT>, k_i8_scaled_decode<DT, 4, SPLIT>);
}

template <int DT>
static int i8_launch(I8Args& a, int rung, hipStream_t st) {
    const unsigned ct = (unsigned)ceil_div64(a.N, S8D_N);
    if (rung == I8_DECODE) {
        i8_launch_decode<DT, false>(a, dim3(ct), st);
    } else if (rung == I8_DECODE_SPLIT) {
        a.kb_per = i8_split_kb_per(a.N, a.K);
        const int S = i8_split_slices(a.N, a.K);
        i8_launch_decode<LLMC_F32, true>(a, dim3(ct, (unsigned)S), st);     // the partial tiles are int32 whatever DT
        LLMC_LAUNCH_CHECK();
        hipLaunchKernelGGL((k_i8_split_reduce<DT>), dim3((unsigned)ceil_div64(a.M * a.N, 256)), dim3(256), 0, st, a, S);
    } else {
        s8_launch_tile128(a, st, k_i8_scaled_tile<DT, 2, 2>);
    }
    LLMC_LAUNCH_CHECK();
    return LLMC_OK;
}

}  // namespace llmc

using namespace llmc;

// the workspace decode_split needs for a shape (0 where no decode rung takes it): S int32 tiles [M, N]; a pure host call
extern "C" size_t llmc_i8_scaled_gemm_ws_bytes(int64_t M, int64_t N, int64_t K) {
    if (M < 1 || N < 1 || K < 1 || M > S8_DECODE_MAX_M || K > 65536 || N >= (1ll << 31)) return 0;
    return (size_t)i8_split_slices(N, K) * (size_t)M * (size_t)N * sizeof(int32_t);
}

// rung: -1 = the ladder chooses; 0 .. I8_NRUNGS - 1 = that rung whatever the shape (the measuring tool and the tests)
extern "C" int llmc_i8_scaled_gemm_on_rung(const void* A8, const float* a_s, int64_t a_s_n, const void* B8, const float* b_s,
                                           int64_t b_s_n, int64_t M, int64_t N, int64_t K, int out_dt, const void* bias, void* C,
                                           void* ws, size_t ws_bytes, int rung_arg, llmc_stream_t stream) {
    I8Args a;
    const int forced = rung_arg;
    if (const int rc = s8_check_operands("i8_scaled_gemm", A8, a_s, B8, b_s, C, M, N, K, out_dt)) return rc;
    LLMC_REQUIRE(forced >= -1 && forced < I8_NRUNGS && (forced < 0 || forced == I8_TILE128 || M <= S8_DECODE_MAX_M),
                 "i8_scaled_gemm: no such rung (the decode rungs take M <= 64)");
    if (const int rc = s8_check_scales("i8_scaled_gemm", a_s_n, b_s_n, M, N)) return rc;
    s8_fill_args(a, A8, a_s, a_s_n, B8, b_s, b_s_n, M, N, K, bias, C);
    a.ws = (int32_t*)ws;
    a.kb_per = 0;
    LLMC_REQUIRE((((uintptr_t)A8 | (uintptr_t)B8) & 15) == 0 && (((uintptr_t)a_s | (uintptr_t)b_s | (uintptr_t)ws) & 3) == 0 &&
                 ((uintptr_t)C & (out_dt == LLMC_F32 ? 3 : 1)) == 0 && ((uintptr_t)bias & (out_dt == LLMC_F32 ? 3 : 1)) == 0,
                 "i8_scaled_gemm: codes need 16-byte, scales and workspace 4-byte, C and bias element alignment");
    if (K % 16) {
        set_last_error_msg("i8_scaled_gemm: K must be a multiple of 16 (one lane's operand bytes; callers de-quantize and run the 16-bit GEMM)");
        return LLMC_ENOTSUP;
    }
    if (K > 65536) {
        set_last_error_msg("i8_scaled_gemm: K must be at most 65536 (128 * 128 * K has to stay below 2^31 in the int32 accumulator)");
        return LLMC_ENOTSUP;
    }
    if (N >= (1ll << 31) || ceil_div64(M, 128) * ceil_div64(N, 128) >= (1ll << 31)) {
        set_last_error_msg("i8_scaled_gemm: N and the tile count must be below 2^31");
        return LLMC_ENOTSUP;
    }
    const int rung = forced >= 0 ? forced : i8_pick_rung(M, N, K);
    if (rung == I8_DECODE_SPLIT)
        LLMC_REQUIRE(ws && ws_bytes >= llmc_i8_scaled_gemm_ws_bytes(M, N, K),
                     "i8_scaled_gemm: the decode_split rung needs a workspace of llmc_i8_scaled_gemm_ws_bytes(M, N, K) bytes");
    hipStream_t st = (hipStream_t)stream;
    return s8_with_out_dt(out_dt, [&](auto dt) { return i8_launch<decltype(dt)::value>(a, rung, st); });
}

extern "C" int llmc_i8_scaled_gemm(const void* A8, const float* a_s, int64_t a_s_n, const void* B8, const float* b_s, int64_t b_s_n,
                                   int64_t M, int64_t N, int64_t K, int out_dt, const void* bias, void* C, void* ws, size_t ws_bytes,
                                   llmc_stream_t stream) {
    return llmc_i8_scaled_gemm_on_rung(A8, a_s, a_s_n, B8, b_s, b_s_n, M, N, K, out_dt, bias, C, ws, ws_bytes, -1, stream);
}

// the rung the ladder gives a shape (0 decode, 1 tile128, 2 decode_split): a pure host call, for tools and tests
extern "C" int llmc_i8_scaled_gemm_rung(int64_t M, int64_t N, int64_t K) { return i8_pick_rung(M, N, K); }
