// scaled8_gemm.h — the structure the 8-bit scaled GEMMs share, written once: A [M, K] and B [N, K] one-byte codes, scales constant
// along K, C[m, n] = rnd_out(fl(fl(float(acc[m, n]) * a_s[m]) * b_s[n])) then the bias. Included by fp8_linear.hip and
// i8_linear.hip, which keep their instruction's arithmetic, their ladder and their entry points. A number format is a `Code`:
//     acc_t                        the accumulator scalar (also the LDS element of the decode rung's partial tiles)
//     mac32(a, b, c), mac16(..)    multiply-accumulate a lane's 16 operand bytes into a 32 x 32 / 16 x 16 accumulator (mac16: only
//                                  where the format runs s8_decode_body)
//     to_float(acc)                the accumulator as the fp32 number the epilogue scales
//     RAGGED_K                     K % 16 == 0 is enough (a zeroed byte of B adds exactly 0); false: K % 128 == 0, no chunk mask
// Which k a lane's operand bytes stand for does not matter as long as both operands use the same bytes.
//
// Edges. A row of A only ever reaches its own row of C, a row of B its own column: rows past M / N are clamped to the last row for
// the load (in bounds), not masked, and their outputs never stored. (No `valid ? v : 0` select of a whole 16-byte vector: it once
// made hipcc keep the staged values in scratch memory, 160 bytes a lane and 16 scratch accesses per K step. The build must report
// ScratchSize 0 for every kernel made from these bodies.) RAGGED_K: a 16-byte chunk past the end of a row is loaded from the
// row's last chunk instead and B's copy is zeroed by an AND mask on the loaded words; A's copy then multiplies zeros.
//
// Everything device-side is __forceinline__ into the including file's __global__ kernels, whose names profiles and traces carry.
#pragma once
#include "common.h"
#include <stdint.h>
#include "mfma_common.h"

namespace llmc {

struct Scaled8Args {
    const uint8_t* A; const float* As; const uint8_t* B; const float* Bs;
    int64_t M, N, K;
    int as_rows, bs_rows;     // 1: one scale per row of A / B, 0: one for the tensor
    const void* bias; void* C;
    int ntm, ntn;             // tile rung: tile counts
};

static constexpr int S8_KB = 128;          // bytes of K per staged block (tile rung) / per wave turn (decode rung)

// C[row, col] from an accumulator value: the conversion, the two scale products in their fixed order, one rounding, then the bias
template <class Code, int DT>
__device__ __forceinline__ void s8_store(const Scaled8Args& a, int64_t row, int64_t col, typename Code::acc_t acc, float sa, float sb) {
    float y = rndc<DT>((Code::to_float(acc) * sa) * sb);
    if (a.bias) y = rndc<DT>(y + load_as_f32(a.bias, col, DT));
    store_from_f32(a.C, row * a.N + col, DT, y);
}

// the 16-byte chunk at byte k of a row: all ones and k when it lies inside the row, else zero and the row's last chunk
template <class Code>
__device__ __forceinline__ uint32_t s8_chunk(int64_t k, int64_t K, int64_t& at) {
    if constexpr (Code::RAGGED_K) {
        const uint32_t v = k < K ? 0xffffffffu : 0u;
        at = v ? k : K - 16;
        return v;
    } else {
        at = k;
        return 0xffffffffu;
    }
}
__device__ __forceinline__ i32x4 s8_and(i32x4 v, uint32_t m) {
    return i32x4{v[0] & (int)m, v[1] & (int)m, v[2] & (int)m, v[3] & (int)m};
}

// ---------------------------------------------------------------------------------------------------------------
// tile rung: 64 WM x 64 WN outputs per workgroup, 4 waves as 2 x 2, WM x WN accumulators of 32 x 32 per wave (the ladders use
// 2 x 2: 128 x 128). One K block of 128 bytes per row and step, global -> registers (issued a step ahead) -> LDS -> one mac32
// per 16-byte fragment read.
// LDS row padding: a fragment read is one ds_read_b128 per lane; the LDS serves 64 banks x 4 B = 256 B a cycle, that is 16 lanes
// of 16 B, and the 16 lanes of one pass read the same k chunk of 16 consecutive rows. With a row stride of LD bytes lane r of a
// pass starts at bank (r * LD / 4) mod 64 and covers 4 banks, so the 16 lanes cover the 64 banks once iff r -> (r * LD / 16)
// mod 16 is a bijection, iff LD / 16 is odd. LD = 128 (8, even) puts all 16 lanes on 8 banks; the smallest odd multiple above
// the 128 data bytes is 9: LD = 144, starts 0, 36, 8, 44, ... (9 r mod 16) * 4. The staging writes (8 chunks of a row, then the
// next row) are conflict-free for the same reason.
// ---------------------------------------------------------------------------------------------------------------
static constexpr int S8_LD = 144;
static constexpr int S8_GROUP_M = 8;      // m tiles that sweep the n tiles together (they share the B panels in L2)

// tile of this workgroup: consecutive workgroup ids go round the 8 XCDs, so the ids an XCD sees are made consecutive tiles
// (a bijection for any tile count), and tiles run in groups of S8_GROUP_M m tiles that sweep n together
__device__ __forceinline__ void s8_tile_of_workgroup(const Scaled8Args& a, int& tm, int& tn) {
    const int nt = a.ntm * a.ntn;
    const int q = nt >> 3, r = nt & 7, x = blockIdx.x & 7;
    const int id = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (blockIdx.x >> 3);
    const int per = S8_GROUP_M * a.ntn;
    const int first = (id / per) * S8_GROUP_M;
    const int gsz = a.ntm - first < S8_GROUP_M ? a.ntm - first : S8_GROUP_M;
    const int in = id % per;
    tm = first + in % gsz;
    tn = in / gsz;
}

template <class Code, int DT, int WM, int WN, class Args>
__device__ __forceinline__ void s8_tile_body(const Args a) {
    typedef typename Code::acc_t acc16 __attribute__((ext_vector_type(16)));
    constexpr int BM = 64 * WM, BN = 64 * WN;
    __shared__ __attribute__((aligned(16))) uint8_t lds[(BM + BN) * S8_LD];
    uint8_t* la = lds;
    uint8_t* lb = lds + BM * S8_LD;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);      // the same in every lane: held in a scalar register
    const int wm = wv >> 1, wn = wv & 1;

    int tm, tn;
    s8_tile_of_workgroup(a, tm, tn);
    const int64_t m0 = (int64_t)tm * BM, n0 = (int64_t)tn * BN;
    const int nkb = (int)((a.K + S8_KB - 1) / S8_KB);

    acc16 acc[WM][WN];
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
        rkv = s8_chunk<Code>((int64_t)kb * S8_KB + sch, a.K, at);
#pragma unroll
        for (int q = 0; q < 2 * WM; ++q) ra[q] = *reinterpret_cast<const i32x4*>(pa[q] + at);
#pragma unroll
        for (int q = 0; q < 2 * WN; ++q) rb[q] = *reinterpret_cast<const i32x4*>(pb[q] + at);
    };
    gload(0);
    for (int kb = 0; kb < nkb; ++kb) {
        __syncthreads();                      // every wave is done with the previous step's panels
#pragma unroll
        for (int q = 0; q < 2 * WM; ++q) *reinterpret_cast<i32x4*>(la + (srow + 32 * q) * S8_LD + sch) = ra[q];
#pragma unroll
        for (int q = 0; q < 2 * WN; ++q) *reinterpret_cast<i32x4*>(lb + (srow + 32 * q) * S8_LD + sch) = s8_and(rb[q], rkv);
        __syncthreads();
        if (kb + 1 < nkb) gload(kb + 1);      // lands under this step's MFMAs
#pragma unroll
        for (int kc = 0; kc < 4; ++kc) {
            const int off = (lane & 31) * S8_LD + kc * 32 + 16 * (lane >> 5);
            i32x4 fa[WM], fb[WN];
#pragma unroll
            for (int m = 0; m < WM; ++m) fa[m] = *reinterpret_cast<const i32x4*>(la + (wm * 32 * WM + m * 32) * S8_LD + off);
#pragma unroll
            for (int n = 0; n < WN; ++n) fb[n] = *reinterpret_cast<const i32x4*>(lb + (wn * 32 * WN + n * 32) * S8_LD + off);
#pragma unroll
            for (int m = 0; m < WM; ++m)
#pragma unroll
                for (int n = 0; n < WN; ++n) acc[m][n] = Code::mac32(fa[m], fb[n], acc[m][n]);
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
                if (row < a.M) s8_store<Code, DT>(a, row, col, acc[m][n][r], a.As[a.as_rows ? row : 0], sb);
            }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// decode rung: M <= 16 MT rows. One workgroup of S8D_WAVES waves per 16 output columns and all rows; the K blocks [kb_lo, kb_hi)
// are dealt round the waves (wave w takes w, w + 8, ...), operands straight from global memory to registers (each weight byte is
// used by one wave only: LDS would be a round trip for nothing), two K blocks in flight per wave. The waves' partial tiles meet
// in LDS and are added in wave order 0..7: no atomics, the same bits on every run. (fp8_linear.hip keeps a decode kernel of its
// own and says why.) SPLIT (Args then has ws [S, M, N] and kb_per): blockIdx.y is the K slice of kb_per blocks, and the tile of
// acc_t goes to the workspace with plain vector stores instead of through the epilogue.
// ---------------------------------------------------------------------------------------------------------------
static constexpr int S8D_WAVES = 8;
static constexpr int S8D_N = 16;
static constexpr int S8_DECODE_MAX_M = 64;      // what the decode bodies are launched for (MT <= 4)

template <int MT> struct S8DecodeOperands {
    i32x4 b[2], x[MT][2];
    uint32_t kv[2];           // b[e]'s mask, applied where b[e] is used: an AND at the load would wait for the load there
};

template <class Code, int DT, int MT, bool SPLIT, class Args>
__device__ __forceinline__ void s8_decode_body(const Args a) {
    typedef typename Code::acc_t acc_t;
    typedef acc_t acc4 __attribute__((ext_vector_type(4)));
    __shared__ acc_t red[S8D_WAVES * MT * 256];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int r = lane & 15, g = lane >> 4;
    const int64_t n0 = (int64_t)blockIdx.x * S8D_N;
    const int nkb = (int)((a.K + S8_KB - 1) / S8_KB);
    int kb_lo = 0, kb_hi = nkb;
    if constexpr (SPLIT) {
        kb_lo = (int)blockIdx.y * a.kb_per;
        if (kb_lo + a.kb_per < nkb) kb_hi = kb_lo + a.kb_per;      // kb_lo < kb_hi: no slice is empty
    }

    // lane (r, g) takes bytes 32 g .. 32 g + 31 of its row's K block, for the weight row n0 + r and the activation rows
    // 16 mt + r alike, as two chunks of 16, one mac16 each
    const uint8_t* bp = a.B + (n0 + r < a.N ? n0 + r : a.N - 1) * a.K;
    const uint8_t* ap[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) ap[mt] = a.A + (16 * mt + r < a.M ? (int64_t)(16 * mt + r) : a.M - 1) * a.K;
    // a K block index past the end is clamped (the load stays in bounds, its products are not formed)
    auto load = [&](S8DecodeOperands<MT>& o, int kb) {
        const int64_t k0 = (int64_t)(kb < kb_hi ? kb : kb_hi - 1) * S8_KB + 32 * g;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            int64_t at;
            o.kv[e] = s8_chunk<Code>(k0 + 16 * e, a.K, at);
            o.b[e] = *reinterpret_cast<const i32x4*>(bp + at);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) o.x[mt][e] = *reinterpret_cast<const i32x4*>(ap[mt] + at);
        }
    };
    acc4 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[mt] = acc4{0, 0, 0, 0};
    auto mac = [&](const S8DecodeOperands<MT>& o) {
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const i32x4 b = s8_and(o.b[e], o.kv[e]);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) acc[mt] = Code::mac16(o.x[mt][e], b, acc[mt]);
        }
    };
    S8DecodeOperands<MT> s0, s1;
    load(s0, kb_lo + wv);
    load(s1, kb_lo + wv + S8D_WAVES);
    for (int kb = kb_lo + wv; kb < kb_hi; kb += 2 * S8D_WAVES) {
        mac(s0);
        load(s0, kb + 2 * S8D_WAVES);
        if (kb + S8D_WAVES < kb_hi) mac(s1);
        load(s1, kb + 3 * S8D_WAVES);
    }

    // the waves' tiles meet in LDS. Accumulator register q of lane l is row 4 (l >> 4) + q, column l & 15.
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int q = 0; q < 4; ++q) red[(wv * MT + mt) * 256 + q * 64 + lane] = acc[mt][q];
    __syncthreads();
    for (int e = tid; e < MT * 256; e += 64 * S8D_WAVES) {
        acc_t s = red[e];
#pragma unroll
        for (int w = 1; w < S8D_WAVES; ++w) s += red[w * MT * 256 + e];
        const int ln = e & 63;
        const int64_t row = 16 * (e >> 8) + 4 * (ln >> 4) + ((e >> 6) & 3), col = n0 + (ln & 15);
        if (row < a.M && col < a.N) {
            if constexpr (SPLIT) a.ws[((int64_t)blockIdx.y * a.M + row) * a.N + col] = s;
            else s8_store<Code, DT>(a, row, col, s, a.As[a.as_rows ? row : 0], a.Bs[a.bs_rows ? col : 0]);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// host side: the launches of the two rungs over a file's own kernels, the output dtype as a template argument, and what the
// entry points check and set alike
// ---------------------------------------------------------------------------------------------------------------
template <class Args> using S8Kernel = void (*)(Args);

// the decode rung on 1, 2 or 4 row tiles of 16 (k1, k2, k4: the file's decode kernel at MT = 1, 2, 4)
template <class Args>
static void s8_launch_decode(const Args& a, dim3 grid, hipStream_t st, S8Kernel<Args> k1, S8Kernel<Args> k2, S8Kernel<Args> k4) {
    hipLaunchKernelGGL(a.M <= 16 ? k1 : a.M <= 32 ? k2 : k4, grid, dim3(64 * S8D_WAVES), 0, st, a);
}

// the tile rung at 128 x 128 (k: the file's tile kernel at WM = WN = 2)
template <class Args>
static void s8_launch_tile128(Args& a, hipStream_t st, S8Kernel<Args> k) {
    a.ntm = (int)ceil_div64(a.M, 128);
    a.ntn = (int)ceil_div64(a.N, 128);
    hipLaunchKernelGGL(k, dim3((unsigned)(a.ntm * a.ntn)), dim3(256), 0, st, a);
}

// f(integral_constant<int, out_dt>): the output dtype as a compile-time constant
template <class F>
static int s8_with_out_dt(int out_dt, F&& f) {
    switch (out_dt) {
        case LLMC_F16: return f(std::integral_constant<int, LLMC_F16>{});
        case LLMC_BF16: return f(std::integral_constant<int, LLMC_BF16>{});
        default: return f(std::integral_constant<int, LLMC_F32>{});
    }
}

// The checks of an entry point in which only its name `fn` differs: LLMC_OK, or LLMC_EINVAL with the message set. The file's own
// rung check stands between the two, which keeps the order in which the entry points have always answered.
static int s8_fail(const char* fn, const char* what) {
    char msg[192];
    snprintf(msg, sizeof(msg), "%s: %s", fn, what);
    set_last_error_msg(msg);
    return LLMC_EINVAL;
}
static int s8_check_operands(const char* fn, const void* A8, const float* a_s, const void* B8, const float* b_s, const void* C, int64_t M,
                             int64_t N, int64_t K, int out_dt) {
    if (!(A8 && a_s && B8 && b_s && C && M > 0 && N > 0 && K > 0)) return s8_fail(fn, "null/empty argument");
    if (!(out_dt == LLMC_F16 || out_dt == LLMC_BF16 || out_dt == LLMC_F32)) return s8_fail(fn, "bad output dtype");
    return LLMC_OK;
}
static int s8_check_scales(const char* fn, int64_t a_s_n, int64_t b_s_n, int64_t M, int64_t N) {
    if ((a_s_n == M || a_s_n == 1) && (b_s_n == N || b_s_n == 1)) return LLMC_OK;
    return s8_fail(fn, "a_s holds M scales (per token) or 1, b_s holds N scales (per channel) or 1");
}

// the fields every rung reads, from checked arguments
static void s8_fill_args(Scaled8Args& a, const void* A8, const float* a_s, int64_t a_s_n, const void* B8, const float* b_s, int64_t b_s_n,
                         int64_t M, int64_t N, int64_t K, const void* bias, void* C) {
    a.A = (const uint8_t*)A8; a.As = a_s; a.B = (const uint8_t*)B8; a.Bs = b_s;
    a.M = M; a.N = N; a.K = K; a.bias = bias; a.C = C;
    // one scale for a one-row operand is both "per row" and "per tensor": index 0 either way
    a.as_rows = a_s_n == M && M > 1 ? 1 : 0;
    a.bs_rows = b_s_n == N && N > 1 ? 1 : 0;
    a.ntm = a.ntn = 0;
}

}  // namespace llmc
