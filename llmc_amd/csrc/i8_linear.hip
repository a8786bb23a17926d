// i8_linear.hip — the W8A8 integer Linear: A [M, K] and B [N, K] int8 codes whose scales are constant along K (one per token or
// one per tensor for A, one per output channel or one per tensor for B), the stored form deploy('vllm_quant' | 'sgl_quant' | ...)
// writes for the reference's backend/{vllm,sglang}/{smoothquant,awq,rtn}_w8a8 configurations (an extension: its real-quant
// Linears raise in forward).
//   llmc_i8_scaled_gemm     acc[m, n] = sum_k a[m, k] b[n, k] in int32 on the integer matrix pipe,
//                           C[m, n] = rnd_out(fl(fl(float(acc) * a_s[m]) * b_s[n])), then the bias in the output dtype
// float(acc) is v_cvt_f32_i32, round to nearest even. Nothing is de-quantized in the K loop: it holds loads, LDS traffic and
// matrix instructions only; both scales act in the epilogue, in the order of fp8_linear.hip's fl_store.
//
// Matrix instructions: v_mfma_i32_32x32x32_i8 (tile rung) and v_mfma_i32_16x16x64_i8 (decode rungs), 16 operand bytes per lane
// and instruction. The int32 accumulator is exact: there is no accumulation window like the fp8 forms' (DESIGN.md K22 / K24), any
// order of adding gives the same bits, and a zeroed operand byte adds exactly 0. K <= 65536 keeps the worst case
// 128 * 128 * K = 2^30 below 2^31. Which k a lane's bytes stand for does not matter as long as both operands use the same bytes.
//
// Ragged K (K % 16 == 0, not % 128): a 16-byte chunk past the end of a row is loaded from the row's last chunk instead (in
// bounds) and B's copy is zeroed by an AND mask on the loaded words; A's copy then multiplies zeros. Rows past the edge are
// clamped to the last row and not masked at all: their outputs are never stored. (No `valid ? v : 0` select of a whole uint4:
// fp8_linear.hip records that it sent the staged values to scratch. The build must report ScratchSize 0 for these kernels.)
//
// Rungs (which shape takes which: I8_LADDER below, one table):
//   tile128       128 x 128 outputs per workgroup, 4 waves as 2 x 2, 2 x 2 accumulators of 32 x 32 (i32x16) each. One K block of 128
//                 bytes per row and step, global -> registers (issued a step ahead) -> LDS -> one 32x32x32 instruction per 16-byte
//                 fragment read (the fp8 kernel splits the same 16 bytes over two instructions). XCD-aware tile order and m-tile
//                 groups as in k_fp8_scaled_tile.
//                 LDS row padding: a fragment read is one ds_read_b128 per lane; the LDS serves 64 banks x 4 B = 256 B a cycle,
//                 that is 16 lanes of 16 B, and the 16 lanes of one pass read the same k chunk of 16 consecutive rows. With a row
//                 stride of LD bytes lane r of a pass starts at bank (r * LD / 4) mod 64 and covers 4 banks, so the 16 lanes cover
//                 the 64 banks once iff r -> (r * LD / 16) mod 16 is a bijection, iff LD / 16 is odd. LD = 128 (8, even) puts all
//                 16 lanes on 8 banks; the smallest odd multiple above the 128 data bytes is 9: LD = 144, starts 0, 36, 8, 44, ...
//                 (9 r mod 16) * 4. The staging writes (8 chunks of a row, then the next row) are conflict-free for the same reason.
//   decode        M <= 64. One workgroup of 8 waves per 16 output columns and all rows; wave w takes the K blocks w, w + 8, ... of
//                 128 bytes, operands straight from global memory to registers, two K blocks in flight per wave; the 8 partial tiles
//                 meet in LDS. 1, 2 or 4 row tiles of 16.
//   decode_split  the decode rung with K also cut into S slices across workgroups (grid N / 16 x S) for layers with too few column
//                 tiles to fill the chip. A slice stores its int32 tile to the caller's workspace [S, M, N] with plain vector
//                 stores; k_i8_split_reduce adds the S partials and applies the epilogue. No atomics, no counters: two launches.
#include "common.h"
#include <stdint.h>
#include "mfma_common.h"

namespace llmc {

struct I8Args {
    const uint8_t* A; const float* As; const uint8_t* B; const float* Bs;
    int64_t M, N, K;
    int as_rows, bs_rows;     // 1: one scale per row of A / B, 0: one for the tensor
    const void* bias; void* C;
    int32_t* ws;              // decode_split: the slices' partial tiles [S, M, N]
    int ntm, ntn;             // tile rung: tile counts
    int kb_per;               // decode_split: K blocks of 128 per slice
};

static constexpr int I8_KB = 128;          // bytes of K per staged block (tile rung) / per wave turn (decode rungs)

// C[row, col] from an accumulator value: the conversion, the two scale products in their fixed order, one rounding, then the bias
template <int DT>
__device__ __forceinline__ void i8_store(const I8Args& a, int64_t row, int64_t col, int acc, float sa, float sb) {
    float y = rndc<DT>(((float)acc * sa) * sb);
    if (a.bias) y = rndc<DT>(y + load_as_f32(a.bias, col, DT));
    store_from_f32(a.C, row * a.N + col, DT, y);
}

// the 16-byte chunk at byte k of a row: all ones and k when it lies inside the row, else zero and the row's last chunk
__device__ __forceinline__ uint32_t i8_chunk(int64_t k, int64_t K, int64_t& at) {
    const uint32_t v = k < K ? 0xffffffffu : 0u;
    at = v ? k : K - 16;
    return v;
}
__device__ __forceinline__ i32x4 i8_and(i32x4 v, uint32_t m) {
    return i32x4{v[0] & (int)m, v[1] & (int)m, v[2] & (int)m, v[3] & (int)m};
}

// ---------------------------------------------------------------------------------------------------------------
// tile rung (WM x WN accumulators of 32 x 32 per wave; the ladder uses 2 x 2)
// ---------------------------------------------------------------------------------------------------------------
static constexpr int I8_LD = 144;
static constexpr int I8_GROUP_M = 8;      // m tiles that sweep the n tiles together (they share the B panels in L2)

template <int DT, int WM, int WN>
__global__ __launch_bounds__(256) void k_i8_scaled_tile(I8Args a) {
    constexpr int BM = 64 * WM, BN = 64 * WN;
    __shared__ __attribute__((aligned(16))) uint8_t lds[(BM + BN) * I8_LD];
    uint8_t* la = lds;
    uint8_t* lb = lds + BM * I8_LD;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int wm = wv >> 1, wn = wv & 1;

    // tile of this workgroup: consecutive workgroup ids go round the 8 XCDs, so the ids an XCD sees are made consecutive tiles
    // (a bijection for any tile count), and tiles run in groups of I8_GROUP_M m tiles that sweep n together
    int tm, tn;
    {
        const int nt = a.ntm * a.ntn;
        const int q = nt >> 3, r = nt & 7, x = blockIdx.x & 7;
        const int id = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (blockIdx.x >> 3);
        const int per = I8_GROUP_M * a.ntn;
        const int first = (id / per) * I8_GROUP_M;
        const int gsz = a.ntm - first < I8_GROUP_M ? a.ntm - first : I8_GROUP_M;
        const int in = id % per;
        tm = first + in % gsz;
        tn = in / gsz;
    }
    const int64_t m0 = (int64_t)tm * BM, n0 = (int64_t)tn * BN;
    const int nkb = (int)((a.K + I8_KB - 1) / I8_KB);

    i32x16 acc[WM][WN];
#pragma unroll
    for (int m = 0; m < WM; ++m)
#pragma unroll
        for (int n = 0; n < WN; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][n][r] = 0;

    // staging: thread t moves the 16-byte chunk (t & 7) of rows (t >> 3) + 32 q
    const int srow = tid >> 3, sch = (tid & 7) * 16;
    const uint8_t* pa[2 * WM];
    const uint8_t* pb[2 * WN];
#pragma unroll
    for (int q = 0; q < 2 * WM; ++q) {
        const int64_t row = m0 + srow + 32 * q;
        pa[q] = a.A + (row < a.M ? row : a.M - 1) * a.K;
    }
#pragma unroll
    for (int q = 0; q < 2 * WN; ++q) {
        const int64_t row = n0 + srow + 32 * q;
        pb[q] = a.B + (row < a.N ? row : a.N - 1) * a.K;
    }
    // the mask of a staged chunk is applied when the registers go to LDS, a step after the load was issued: nothing waits for
    // the load before this step's MFMAs
    i32x4 ra[2 * WM], rb[2 * WN];
    uint32_t rkv;
    auto gload = [&](int kb) {
        int64_t at;
        rkv = i8_chunk((int64_t)kb * I8_KB + sch, a.K, at);
#pragma unroll
        for (int q = 0; q < 2 * WM; ++q) ra[q] = *reinterpret_cast<const i32x4*>(pa[q] + at);
#pragma unroll
        for (int q = 0; q < 2 * WN; ++q) rb[q] = *reinterpret_cast<const i32x4*>(pb[q] + at);
    };
    gload(0);
    for (int kb = 0; kb < nkb; ++kb) {
        __syncthreads();                      // every wave is done with the previous step's panels
#pragma unroll
        for (int q = 0; q < 2 * WM; ++q) *reinterpret_cast<i32x4*>(la + (srow + 32 * q) * I8_LD + sch) = ra[q];
#pragma unroll
        for (int q = 0; q < 2 * WN; ++q) *reinterpret_cast<i32x4*>(lb + (srow + 32 * q) * I8_LD + sch) = i8_and(rb[q], rkv);
        __syncthreads();
        if (kb + 1 < nkb) gload(kb + 1);      // lands under this step's MFMAs
#pragma unroll
        for (int kc = 0; kc < 4; ++kc) {
            const int off = (lane & 31) * I8_LD + kc * 32 + 16 * (lane >> 5);
            i32x4 fa[WM], fb[WN];
#pragma unroll
            for (int m = 0; m < WM; ++m) fa[m] = *reinterpret_cast<const i32x4*>(la + (wm * 32 * WM + m * 32) * I8_LD + off);
#pragma unroll
            for (int n = 0; n < WN; ++n) fb[n] = *reinterpret_cast<const i32x4*>(lb + (wn * 32 * WN + n * 32) * I8_LD + off);
#pragma unroll
            for (int m = 0; m < WM; ++m)
#pragma unroll
                for (int n = 0; n < WN; ++n) acc[m][n] = mfma_i32_32x32x32_i8(fa[m], fb[n], acc[m][n]);
        }
    }

    // epilogue: accumulator register r of lane l is row (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31 of its 32 x 32 tile
#pragma unroll
    for (int n = 0; n < WN; ++n) {
        const int64_t col = n0 + wn * 32 * WN + n * 32 + (lane & 31);
        if (col >= a.N) continue;
        const float sb = a.Bs[a.bs_rows ? col : 0];
#pragma unroll
        for (int m = 0; m < WM; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t row = m0 + wm * 32 * WM + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if (row < a.M) i8_store<DT>(a, row, col, acc[m][n][r], a.As[a.as_rows ? row : 0], sb);
            }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// decode rungs: M <= 16 MT rows, 16 columns per workgroup, the K blocks [kb_lo, kb_hi) dealt round the I8D_WAVES waves.
// SPLIT: blockIdx.y is the K slice and the int32 tile goes to the workspace instead of through the epilogue.
// ---------------------------------------------------------------------------------------------------------------
static constexpr int I8D_WAVES = 8;
static constexpr int I8D_N = 16;

template <int MT> struct I8DecodeOperands {
    i32x4 b[2], x[MT][2];
    uint32_t kv[2];           // b[e]'s mask, applied where b[e] is used: an AND at the load would wait for the load there
};

template <int DT, int MT, bool SPLIT>
__global__ __launch_bounds__(64 * I8D_WAVES) void k_i8_scaled_decode(I8Args a) {
    __shared__ int red[I8D_WAVES * MT * 256];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int r = lane & 15, g = lane >> 4;
    const int64_t n0 = (int64_t)blockIdx.x * I8D_N;
    const int nkb = (int)((a.K + I8_KB - 1) / I8_KB);
    const int kb_lo = SPLIT ? (int)blockIdx.y * a.kb_per : 0;
    const int kb_hi = SPLIT ? (kb_lo + a.kb_per < nkb ? kb_lo + a.kb_per : nkb) : nkb;      // kb_lo < kb_hi: no slice is empty

    // lane (r, g) takes bytes 32 g .. 32 g + 31 of its row's K block, for the weight row n0 + r and the activation rows
    // 16 mt + r alike, as two chunks of 16, one instruction each
    const uint8_t* bp = a.B + (n0 + r < a.N ? n0 + r : a.N - 1) * a.K;
    const uint8_t* ap[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) ap[mt] = a.A + (16 * mt + r < a.M ? (int64_t)(16 * mt + r) : a.M - 1) * a.K;
    // a K block index past the end is clamped (the load stays in bounds, its products are not formed)
    auto load = [&](I8DecodeOperands<MT>& o, int kb) {
        const int64_t k0 = (int64_t)(kb < kb_hi ? kb : kb_hi - 1) * I8_KB + 32 * g;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            int64_t at;
            o.kv[e] = i8_chunk(k0 + 16 * e, a.K, at);
            o.b[e] = *reinterpret_cast<const i32x4*>(bp + at);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) o.x[mt][e] = *reinterpret_cast<const i32x4*>(ap[mt] + at);
        }
    };
    i32x4 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[mt] = i32x4{0, 0, 0, 0};
    auto mac = [&](const I8DecodeOperands<MT>& o) {
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const i32x4 b = i8_and(o.b[e], o.kv[e]);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) acc[mt] = mfma_i32_16x16x64_i8(o.x[mt][e], b, acc[mt]);
        }
    };
    I8DecodeOperands<MT> s0, s1;
    load(s0, kb_lo + wv);
    load(s1, kb_lo + wv + I8D_WAVES);
    for (int kb = kb_lo + wv; kb < kb_hi; kb += 2 * I8D_WAVES) {
        mac(s0);
        load(s0, kb + 2 * I8D_WAVES);
        if (kb + I8D_WAVES < kb_hi) mac(s1);
        load(s1, kb + 3 * I8D_WAVES);
    }

    // the waves' tiles meet in LDS. Accumulator register q of lane l is row 4 (l >> 4) + q, column l & 15.
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int q = 0; q < 4; ++q) red[(wv * MT + mt) * 256 + q * 64 + lane] = acc[mt][q];
    __syncthreads();
    for (int e = tid; e < MT * 256; e += 64 * I8D_WAVES) {
        int s = red[e];
#pragma unroll
        for (int w = 1; w < I8D_WAVES; ++w) s += red[w * MT * 256 + e];
        const int ln = e & 63;
        const int64_t row = 16 * (e >> 8) + 4 * (ln >> 4) + ((e >> 6) & 3), col = n0 + (ln & 15);
        if (row < a.M && col < a.N) {
            if constexpr (SPLIT) a.ws[((int64_t)blockIdx.y * a.M + row) * a.N + col] = s;
            else i8_store<DT>(a, row, col, s, a.As[a.as_rows ? row : 0], a.Bs[a.bs_rows ? col : 0]);
        }
    }
}

// decode_split, second launch: one thread per output adds its S partials and applies the epilogue
template <int DT>
__global__ __launch_bounds__(256) void k_i8_split_reduce(I8Args a, int S) {
    const int64_t mn = a.M * a.N, i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= mn) return;
    int s = 0;
    for (int sl = 0; sl < S; ++sl) s += a.ws[sl * mn + i];
    const int64_t row = i / a.N, col = i - row * a.N;
    i8_store<DT>(a, row, col, s, a.As[a.as_rows ? row : 0], a.Bs[a.bs_rows ? col : 0]);
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
static constexpr int I8_DECODE_MAX_M = 64;      // what the decode kernels are compiled for (MT <= 4)
static constexpr int I8_SPLIT_MAX = 16;         // most K slices
struct I8Rung {
    int64_t min_m, max_m;   // min_m <= M <= max_m
    int cu_share;           // > 0: the column tiles (N / 16) fill at most 1 / cu_share of the CUs
    int64_t min_k;          // K >= min_k
    int64_t min_n;          // N >= min_n
    int rung;
};
static const I8Rung I8_LADDER[] = {
    {17, I8_DECODE_MAX_M, 4, 4096, 1, I8_DECODE_SPLIT},
    {33, I8_DECODE_MAX_M, 0, 0, 14336, I8_TILE128},
    {1, I8_DECODE_MAX_M, 0, 0, 1, I8_DECODE},
    {1, INT64_MAX, 0, 0, 1, I8_TILE128},
};

static int i8_pick_rung(int64_t M, int64_t N, int64_t K) {
    const int64_t ct = ceil_div64(N, I8D_N);
    for (const I8Rung& r : I8_LADDER)
        if (M >= r.min_m && M <= r.max_m && K >= r.min_k && N >= r.min_n && (r.cu_share == 0 || ct * r.cu_share <= device_cu_count())) return r.rung;
    return I8_TILE128;
}

// decode_split's K blocks per slice: one workgroup per CU (option i8_split_slices = n > 0: n slices), at most I8_SPLIT_MAX
// slices, none of them empty. The slice count is ceil(nkb / the result).
static int i8_split_kb_per(int64_t N, int64_t K) {
    const int64_t nkb = ceil_div64(K, I8_KB), ct = ceil_div64(N, I8D_N);
    int64_t s = opt(OPT_I8_SPLIT_SLICES) > 0 ? opt(OPT_I8_SPLIT_SLICES) : ceil_div64(device_cu_count(), ct);
    s = s > I8_SPLIT_MAX ? I8_SPLIT_MAX : s;
    s = s > nkb ? nkb : s;
    return (int)ceil_div64(nkb, s < 1 ? 1 : s);
}
static int i8_split_slices(int64_t N, int64_t K) { return (int)ceil_div64(ceil_div64(K, I8_KB), i8_split_kb_per(N, K)); }

template <int DT, bool SPLIT>
static void i8_launch_decode(const I8Args& a, dim3 grid, hipStream_t st) {
    const dim3 block(64 * I8D_WAVES);
    if (a.M <= 16) hipLaunchKernelGGL((k_i8_scaled_decode<DT, 1, SPLIT>), grid, block, 0, st, a);
    else if (a.M <= 32) hipLaunchKernelGGL((k_i8_scaled_decode<DT, 2, SPLIT>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((k_i8_scaled_decode<DT, 4, SPLIT>), grid, block, 0, st, a);
}

template <int DT>
static int i8_launch(I8Args& a, int rung, hipStream_t st) {
    const unsigned ct = (unsigned)ceil_div64(a.N, I8D_N);
    if (rung == I8_DECODE) {
        i8_launch_decode<DT, false>(a, dim3(ct), st);
    } else if (rung == I8_DECODE_SPLIT) {
        a.kb_per = i8_split_kb_per(a.N, a.K);
        const int S = i8_split_slices(a.N, a.K);
        i8_launch_decode<LLMC_F32, true>(a, dim3(ct, (unsigned)S), st);     // the partial tiles are int32 whatever DT
        LLMC_LAUNCH_CHECK();
        hipLaunchKernelGGL((k_i8_split_reduce<DT>), dim3((unsigned)ceil_div64(a.M * a.N, 256)), dim3(256), 0, st, a, S);
    } else {
        a.ntm = (int)ceil_div64(a.M, 128);
        a.ntn = (int)ceil_div64(a.N, 128);
        hipLaunchKernelGGL((k_i8_scaled_tile<DT, 2, 2>), dim3((unsigned)(a.ntm * a.ntn)), dim3(256), 0, st, a);
    }
    LLMC_LAUNCH_CHECK();
    return LLMC_OK;
}

}  // namespace llmc

using namespace llmc;

// the workspace decode_split needs for a shape (0 where no decode rung takes it): S int32 tiles [M, N]; a pure host call
extern "C" size_t llmc_i8_scaled_gemm_ws_bytes(int64_t M, int64_t N, int64_t K) {
    if (M < 1 || N < 1 || K < 1 || M > I8_DECODE_MAX_M || K > 65536 || N >= (1ll << 31)) return 0;
    return (size_t)i8_split_slices(N, K) * (size_t)M * (size_t)N * sizeof(int32_t);
}

// rung: -1 = the ladder chooses; 0 .. I8_NRUNGS - 1 = that rung whatever the shape (the measuring tool and the tests)
extern "C" int llmc_i8_scaled_gemm_on_rung(const void* A8, const float* a_s, int64_t a_s_n, const void* B8, const float* b_s,
                                           int64_t b_s_n, int64_t M, int64_t N, int64_t K, int out_dt, const void* bias, void* C,
                                           void* ws, size_t ws_bytes, int rung_arg, llmc_stream_t stream) {
    LLMC_REQUIRE(A8 && a_s && B8 && b_s && C && M > 0 && N > 0 && K > 0, "i8_scaled_gemm: null/empty argument");
    const int forced = rung_arg;
    LLMC_REQUIRE(out_dt == LLMC_F16 || out_dt == LLMC_BF16 || out_dt == LLMC_F32, "i8_scaled_gemm: bad output dtype");
    LLMC_REQUIRE(forced >= -1 && forced < I8_NRUNGS && (forced < 0 || forced == I8_TILE128 || M <= I8_DECODE_MAX_M),
                 "i8_scaled_gemm: no such rung (the decode rungs take M <= 64)");
    LLMC_REQUIRE((a_s_n == M || a_s_n == 1) && (b_s_n == N || b_s_n == 1),
                 "i8_scaled_gemm: a_s holds M scales (per token) or 1, b_s holds N scales (per channel) or 1");
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
    I8Args a;
    a.A = (const uint8_t*)A8; a.As = a_s; a.B = (const uint8_t*)B8; a.Bs = b_s;
    a.M = M; a.N = N; a.K = K; a.bias = bias; a.C = C; a.ws = (int32_t*)ws;
    // one scale for a one-row operand is both "per row" and "per tensor": index 0 either way
    a.as_rows = a_s_n == M && M > 1 ? 1 : 0;
    a.bs_rows = b_s_n == N && N > 1 ? 1 : 0;
    a.ntm = a.ntn = a.kb_per = 0;
    hipStream_t st = (hipStream_t)stream;
    switch (out_dt) {
        case LLMC_F16: return i8_launch<LLMC_F16>(a, rung, st);
        case LLMC_BF16: return i8_launch<LLMC_BF16>(a, rung, st);
        default: return i8_launch<LLMC_F32>(a, rung, st);
    }
}

extern "C" int llmc_i8_scaled_gemm(const void* A8, const float* a_s, int64_t a_s_n, const void* B8, const float* b_s, int64_t b_s_n,
                                   int64_t M, int64_t N, int64_t K, int out_dt, const void* bias, void* C, void* ws, size_t ws_bytes,
                                   llmc_stream_t stream) {
    return llmc_i8_scaled_gemm_on_rung(A8, a_s, a_s_n, B8, b_s, b_s_n, M, N, K, out_dt, bias, C, ws, ws_bytes, -1, stream);
}

// the rung the ladder gives a shape (0 decode, 1 tile128, 2 decode_split): a pure host call, for tools and tests
extern "C" int llmc_i8_scaled_gemm_rung(int64_t M, int64_t N, int64_t K) { return i8_pick_rung(M, N, K); }
