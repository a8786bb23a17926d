// fp8_linear.hip — the plain W8A8-FP8 Linear: A [M, K] and B [N, K] OCP e4m3fn codes whose scales are constant along K (one per
// token or one per tensor for A, one per output channel or one per tensor for B), the stored form of the reference's
// configs/quantization/backend/{vllm,sglang}/fp8 configurations (an extension: its real-quant Linears raise in forward).
//   llmc_fp8_scaled_gemm    acc[m, n] = sum_k a[m, k] b[n, k] in fp32 on the fp8 matrix pipe,
//                           C[m, n] = rnd_out(fl(fl(acc * a_s[m]) * b_s[n])), then the bias in the output dtype
// Both scales leave the K loop: it holds loads, LDS traffic and matrix instructions only (llmc_fp8_block_gemm pays two VALU ops
// per element and 128-deep K block for its block scales).
//
// Matrix instruction: the NON-scaled forms v_mfma_f32_32x32x16_fp8_fp8 (tile rung) and v_mfma_f32_16x16x32_fp8_fp8 (decode rung).
// A product of two e4m3 numbers is exact in fp32, but neither form of the instruction adds all products at fp32 width. Measured
// here with one-product probes: the non-scaled forms align the 8 products of one lane's 8 operand bytes to the
// largest of them and cut off what lies more than 13 binary places below its leading bit (256 + 2^-5 exact, 256 + 2^-6 -> 256);
// the groups of different lanes, different instructions and the accumulator are added at fp32 width (256 + 2^-15 exact). That
// is the window DESIGN.md K22 found in the block-scaled f8f6f4 form, there over a lane's 32 products. Loss, one-sided, at most:
//     non-scaled     7 * 2^-13 of sum |a b|  (2^-10.2)        block-scaled   31 * 2^-13 of sum |a b|  (2^-8.0), at twice the rate
// Feeding either form one exponent class at a time (llmc_mx_gemm) makes the sums exact at 3 x and more the instructions. The
// non-scaled forms were chosen: the smaller loss, below one rounding of a 16-bit output for sums without cancellation; it is
// stated in include/llmc_hip.h and is the leading term of the bound the tests hold the kernel to (tests/fp8_linear_oracle.py).
// Data whose products of one group lie within 13 binary places of each other is summed exactly.
//
// Rungs (which shape takes which: FL_LADDER below, one table):
//   decode   M <= 64. One workgroup of 8 waves per 16 output columns and all rows; wave w takes the K blocks w, w + 8, ... of 128
//            bytes, operands straight from global memory to registers (each weight byte is used by one wave only: LDS would be a
//            round trip for nothing), two K blocks in flight per wave. The eight partial tiles meet in LDS and are added in wave
//            order 0..7: no atomics, the same bits on every run. N / 16 workgroups of 512 threads fill the chip from N = 4096 up.
//   tile128  128 x 128 outputs per workgroup, 4 waves as 2 x 2, 2 x 2 accumulators of 32 x 32 each. One K block of 128 bytes per
//            row and step, global -> registers (issued a step ahead) -> LDS (rows padded to 144 B: the 16-byte fragment reads of
//            16 consecutive rows cover the 64 banks once) -> two MFMAs per 16-byte read. (A 256 x 128 tile of the same structure,
//            128 accumulator registers and one wave per SIMD, was measured and dropped: 1.4 to 1.7 times slower at every shape.)
// Which k a lane's operand bytes stand for does not matter as long as both operands use the same bytes; every kernel here hands a
// lane 16 consecutive bytes per load and feeds them to two consecutive instructions.
#include "common.h"
#include <stdint.h>
#include "mfma_common.h"

namespace llmc {

struct Fp8ScaledArgs {
    const uint8_t* A; const float* As; const uint8_t* B; const float* Bs;
    int64_t M, N, K;
    int as_rows, bs_rows;     // 1: one scale per row of A / B, 0: one for the tensor
    const void* bias; void* C;
    int ntm, ntn;
};

// C[row, col] from an accumulator value: the two scale products in their fixed order, one rounding, then the bias
template <int DT>
__device__ __forceinline__ void fl_store(const Fp8ScaledArgs& a, int64_t row, int64_t col, float acc, float sa, float sb) {
    float y = rndc<DT>((acc * sa) * sb);
    if (a.bias) y = rndc<DT>(y + load_as_f32(a.bias, col, DT));
    store_from_f32(a.C, row * a.N + col, DT, y);
}

// ---------------------------------------------------------------------------------------------------------------
// tile rung (WM x WN accumulators of 32 x 32 per wave; the ladder uses 2 x 2)
// ---------------------------------------------------------------------------------------------------------------
static constexpr int FL_LD = 144;
static constexpr int FL_GROUP_M = 8;      // m tiles that sweep the n tiles together (they share the B panels in L2)

template <int DT, int WM, int WN>
__global__ __launch_bounds__(256) void k_fp8_scaled_tile(Fp8ScaledArgs a) {
    constexpr int BM = 64 * WM, BN = 64 * WN;
    __shared__ __attribute__((aligned(16))) uint8_t lds[(BM + BN) * FL_LD];
    uint8_t* la = lds;
    uint8_t* lb = lds + BM * FL_LD;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int wm = wv >> 1, wn = wv & 1;

    // tile of this workgroup: consecutive workgroup ids go round the 8 XCDs, so the ids an XCD sees are made consecutive tiles
    // (a bijection for any tile count), and tiles run in groups of FL_GROUP_M m tiles that sweep n together
    int tm, tn;
    {
        const int nt = a.ntm * a.ntn;
        const int q = nt >> 3, r = nt & 7, x = blockIdx.x & 7;
        const int id = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (blockIdx.x >> 3);
        const int per = FL_GROUP_M * a.ntn;
        const int first = (id / per) * FL_GROUP_M;
        const int gsz = a.ntm - first < FL_GROUP_M ? a.ntm - first : FL_GROUP_M;
        const int in = id % per;
        tm = first + in % gsz;
        tn = in / gsz;
    }
    const int64_t m0 = (int64_t)tm * BM, n0 = (int64_t)tn * BN;
    const int nkb = (int)(a.K / 128);

    f32x16 acc[WM][WN];
#pragma unroll
    for (int m = 0; m < WM; ++m)
#pragma unroll
        for (int n = 0; n < WN; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.0f;

    // staging: thread t moves the 16-byte chunk (t & 7) of rows (t >> 3) + 32 q; rows past the edge are clamped to the last row
    // for the load (always in bounds) and zeroed by an AND mask on the loaded words. (A `valid ? loaded : zero` select of the
    // whole uint4 made hipcc keep the staged values in scratch memory: 160 bytes a lane, 8 scratch loads and 8 scratch stores
    // per K step. The build must report ScratchSize 0 for these kernels.)
    const int srow = tid >> 3, sch = (tid & 7) * 16;
    const uint8_t* pa[2 * WM];
    const uint8_t* pb[2 * WN];
    uint32_t va[2 * WM], vb[2 * WN];       // all ones: the row exists
#pragma unroll
    for (int q = 0; q < 2 * WM; ++q) {
        const int64_t row = m0 + srow + 32 * q;
        va[q] = row < a.M ? 0xffffffffu : 0u;
        pa[q] = a.A + (va[q] ? row : a.M - 1) * a.K + sch;
    }
#pragma unroll
    for (int q = 0; q < 2 * WN; ++q) {
        const int64_t row = n0 + srow + 32 * q;
        vb[q] = row < a.N ? 0xffffffffu : 0u;
        pb[q] = a.B + (vb[q] ? row : a.N - 1) * a.K + sch;
    }
    uint4 ra[2 * WM], rb[2 * WN];
    auto gload = [&](int kb) {
        const int64_t k0 = (int64_t)kb * 128;
#pragma unroll
        for (int q = 0; q < 2 * WM; ++q) {
            const uint4 v = *reinterpret_cast<const uint4*>(pa[q] + k0);
            ra[q] = uint4{v.x & va[q], v.y & va[q], v.z & va[q], v.w & va[q]};
        }
#pragma unroll
        for (int q = 0; q < 2 * WN; ++q) {
            const uint4 v = *reinterpret_cast<const uint4*>(pb[q] + k0);
            rb[q] = uint4{v.x & vb[q], v.y & vb[q], v.z & vb[q], v.w & vb[q]};
        }
    };
    gload(0);
    for (int kb = 0; kb < nkb; ++kb) {
        __syncthreads();                      // every wave is done with the previous step's panels
#pragma unroll
        for (int q = 0; q < 2 * WM; ++q) *reinterpret_cast<uint4*>(la + (srow + 32 * q) * FL_LD + sch) = ra[q];
#pragma unroll
        for (int q = 0; q < 2 * WN; ++q) *reinterpret_cast<uint4*>(lb + (srow + 32 * q) * FL_LD + sch) = rb[q];
        __syncthreads();
        if (kb + 1 < nkb) gload(kb + 1);      // lands under this step's MFMAs
#pragma unroll
        for (int kc = 0; kc < 4; ++kc) {
            const int off = (lane & 31) * FL_LD + kc * 32 + 16 * (lane >> 5);
            uint4 fa[WM], fb[WN];
#pragma unroll
            for (int m = 0; m < WM; ++m) fa[m] = *reinterpret_cast<const uint4*>(la + (wm * 32 * WM + m * 32) * FL_LD + off);
#pragma unroll
            for (int n = 0; n < WN; ++n) fb[n] = *reinterpret_cast<const uint4*>(lb + (wn * 32 * WN + n * 32) * FL_LD + off);
#pragma unroll
            for (int m = 0; m < WM; ++m)
#pragma unroll
                for (int n = 0; n < WN; ++n) {
                    const long a0 = (long)(((uint64_t)fa[m].y << 32) | fa[m].x), a1 = (long)(((uint64_t)fa[m].w << 32) | fa[m].z);
                    const long b0 = (long)(((uint64_t)fb[n].y << 32) | fb[n].x), b1 = (long)(((uint64_t)fb[n].w << 32) | fb[n].z);
                    acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8(a0, b0, acc[m][n], 0, 0, 0);
                    acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8(a1, b1, acc[m][n], 0, 0, 0);
                }
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
                if (row < a.M) fl_store<DT>(a, row, col, acc[m][n][r], a.As[a.as_rows ? row : 0], sb);
            }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// decode rung: M <= 16 MT rows, 16 columns per workgroup, the K blocks dealt round the FD_WAVES waves
// ---------------------------------------------------------------------------------------------------------------
static constexpr int FD_WAVES = 8;
static constexpr int FD_N = 16;

template <int MT> struct Fp8DecodeOperands {
    uint4 b[2], x[MT][2];
};

template <int DT, int MT>
__global__ __launch_bounds__(64 * FD_WAVES) void k_fp8_scaled_decode(Fp8ScaledArgs a) {
    __shared__ float red[FD_WAVES * MT * 256];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int r = lane & 15, g = lane >> 4;
    const int64_t n0 = (int64_t)blockIdx.x * FD_N;
    const int nkb = (int)(a.K / 128);

    // lane (r, g) takes bytes 32 g .. 32 g + 31 of its row's K block, for the weight row n0 + r and the activation rows
    // 16 mt + r alike; rows past the edge are clamped for the load and zeroed afterwards
    const bool bv = n0 + r < a.N;
    const uint8_t* bp = a.B + (bv ? n0 + r : a.N - 1) * a.K + 32 * g;
    const uint8_t* ap[MT];
    bool av[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        av[mt] = 16 * mt + r < a.M;
        ap[mt] = a.A + (av[mt] ? (int64_t)(16 * mt + r) : a.M - 1) * a.K + 32 * g;
    }
    const uint4 zero4 = {0, 0, 0, 0};
    // a K block index past the end is clamped (the load stays in bounds, its products are not formed)
    auto load = [&](Fp8DecodeOperands<MT>& o, int kb) {
        const int64_t k0 = (int64_t)(kb < nkb ? kb : nkb - 1) * 128;
#pragma unroll
        for (int e = 0; e < 2; ++e) o.b[e] = *reinterpret_cast<const uint4*>(bp + k0 + 16 * e);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int e = 0; e < 2; ++e) o.x[mt][e] = *reinterpret_cast<const uint4*>(ap[mt] + k0 + 16 * e);
    };
    f32x4 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[mt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    auto mac = [&](const Fp8DecodeOperands<MT>& o) {
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const uint4 b = bv ? o.b[e] : zero4;
            const long b0 = (long)(((uint64_t)b.y << 32) | b.x), b1 = (long)(((uint64_t)b.w << 32) | b.z);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                const uint4 x = av[mt] ? o.x[mt][e] : zero4;
                const long x0 = (long)(((uint64_t)x.y << 32) | x.x), x1 = (long)(((uint64_t)x.w << 32) | x.z);
                acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(x0, b0, acc[mt], 0, 0, 0);
                acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(x1, b1, acc[mt], 0, 0, 0);
            }
        }
    };
    Fp8DecodeOperands<MT> s0, s1;
    load(s0, wv);
    load(s1, wv + FD_WAVES);
    for (int kb = wv; kb < nkb; kb += 2 * FD_WAVES) {
        mac(s0);
        load(s0, kb + 2 * FD_WAVES);
        if (kb + FD_WAVES < nkb) mac(s1);
        load(s1, kb + 3 * FD_WAVES);
    }

    // the K slices meet in LDS and are added in wave order. Accumulator register q of lane l is row 4 (l >> 4) + q, column l & 15.
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int q = 0; q < 4; ++q) red[(wv * MT + mt) * 256 + q * 64 + lane] = acc[mt][q];
    __syncthreads();
    for (int e = tid; e < MT * 256; e += 64 * FD_WAVES) {
        float s = red[e];
#pragma unroll
        for (int w = 1; w < FD_WAVES; ++w) s += red[w * MT * 256 + e];
        const int ln = e & 63;
        const int64_t row = 16 * (e >> 8) + 4 * (ln >> 4) + ((e >> 6) & 3), col = n0 + (ln & 15);
        if (row < a.M && col < a.N) fl_store<DT>(a, row, col, s, a.As[a.as_rows ? row : 0], a.Bs[a.bs_rows ? col : 0]);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// which rung takes which shape: the first row whose bounds hold. Set from tools/bench_fp8_linear.py (profiles/fp8_linear.txt): at
// 64, 16 and 1 tokens the decode rung is 1.6 to 18 times faster than the tile rung on every Llama-3-8B shape; 64 is also the most
// the decode kernel is compiled for.
// ---------------------------------------------------------------------------------------------------------------
enum { FL_DECODE = 0, FL_TILE128 = 1, FL_NRUNGS = 2 };
static constexpr int FL_DECODE_MAX_M = 64;      // what the decode kernel is compiled for (MT <= 4)
struct Fp8Rung {
    int64_t max_m;          // M <= max_m
    int rung;
};
static const Fp8Rung FL_LADDER[] = {
    {FL_DECODE_MAX_M, FL_DECODE},
    {INT64_MAX, FL_TILE128},
};

static int fl_pick_rung(int64_t M, int64_t N) {
    (void)N;
    for (const Fp8Rung& r : FL_LADDER)
        if (M <= r.max_m) return r.rung;
    return FL_TILE128;
}

template <int DT>
static int fl_launch(Fp8ScaledArgs& a, int rung, hipStream_t st) {
    if (rung == FL_DECODE) {
        const dim3 grid((unsigned)ceil_div64(a.N, FD_N)), block(64 * FD_WAVES);
        if (a.M <= 16) hipLaunchKernelGGL((k_fp8_scaled_decode<DT, 1>), grid, block, 0, st, a);
        else if (a.M <= 32) hipLaunchKernelGGL((k_fp8_scaled_decode<DT, 2>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((k_fp8_scaled_decode<DT, 4>), grid, block, 0, st, a);
    } else {
        a.ntm = (int)ceil_div64(a.M, 128);
        a.ntn = (int)ceil_div64(a.N, 128);
        hipLaunchKernelGGL((k_fp8_scaled_tile<DT, 2, 2>), dim3((unsigned)(a.ntm * a.ntn)), dim3(256), 0, st, a);
    }
    LLMC_LAUNCH_CHECK();
    return LLMC_OK;
}

}  // namespace llmc

using namespace llmc;

// rung: -1 = the ladder chooses; 0 .. FL_NRUNGS - 1 = that rung whatever the shape (the measuring tool and the tests)
extern "C" int llmc_fp8_scaled_gemm_on_rung(const void* A8, const float* a_s, int64_t a_s_n, const void* B8, const float* b_s,
                                            int64_t b_s_n, int64_t M, int64_t N, int64_t K, int out_dt, const void* bias, void* C,
                                            int rung_arg, llmc_stream_t stream) {
    LLMC_REQUIRE(A8 && a_s && B8 && b_s && C && M > 0 && N > 0 && K > 0, "fp8_scaled_gemm: null/empty argument");
    const int forced = rung_arg;
    LLMC_REQUIRE(out_dt == LLMC_F16 || out_dt == LLMC_BF16 || out_dt == LLMC_F32, "fp8_scaled_gemm: bad output dtype");
    LLMC_REQUIRE(forced >= -1 && forced < FL_NRUNGS && (forced != FL_DECODE || M <= FL_DECODE_MAX_M),
                 "fp8_scaled_gemm: no such rung (the decode rung takes M <= 64)");
    LLMC_REQUIRE((a_s_n == M || a_s_n == 1) && (b_s_n == N || b_s_n == 1),
                 "fp8_scaled_gemm: a_s holds M scales (per token) or 1, b_s holds N scales (per channel) or 1");
    LLMC_REQUIRE((((uintptr_t)A8 | (uintptr_t)B8) & 15) == 0 && (((uintptr_t)a_s | (uintptr_t)b_s) & 3) == 0 &&
                 ((uintptr_t)C & (out_dt == LLMC_F32 ? 3 : 1)) == 0 && ((uintptr_t)bias & (out_dt == LLMC_F32 ? 3 : 1)) == 0,
                 "fp8_scaled_gemm: codes need 16-byte, scales 4-byte, C and bias element alignment");
    if (K % 128) {
        set_last_error_msg("fp8_scaled_gemm: K must be a multiple of 128 (one staged K block; callers de-quantize and run the 16-bit GEMM)");
        return LLMC_ENOTSUP;
    }
    if (K >= (1ll << 24) || ceil_div64(M, 128) * ceil_div64(N, 16) >= (1ll << 31)) {
        set_last_error_msg("fp8_scaled_gemm: K must be below 2^24 and the tile count below 2^31");
        return LLMC_ENOTSUP;
    }
    Fp8ScaledArgs a;
    a.A = (const uint8_t*)A8; a.As = a_s; a.B = (const uint8_t*)B8; a.Bs = b_s;
    a.M = M; a.N = N; a.K = K; a.bias = bias; a.C = C;
    // one scale for a one-row operand is both "per row" and "per tensor": index 0 either way
    a.as_rows = a_s_n == M && M > 1 ? 1 : 0;
    a.bs_rows = b_s_n == N && N > 1 ? 1 : 0;
    a.ntm = a.ntn = 0;
    const int rung = forced >= 0 ? forced : fl_pick_rung(M, N);
    hipStream_t st = (hipStream_t)stream;
    switch (out_dt) {
        case LLMC_F16: return fl_launch<LLMC_F16>(a, rung, st);
        case LLMC_BF16: return fl_launch<LLMC_BF16>(a, rung, st);
        default: return fl_launch<LLMC_F32>(a, rung, st);
    }
}

extern "C" int llmc_fp8_scaled_gemm(const void* A8, const float* a_s, int64_t a_s_n, const void* B8, const float* b_s, int64_t b_s_n,
                                    int64_t M, int64_t N, int64_t K, int out_dt, const void* bias, void* C, llmc_stream_t stream) {
    return llmc_fp8_scaled_gemm_on_rung(A8, a_s, a_s_n, B8, b_s, b_s_n, M, N, K, out_dt, bias, C, -1, stream);
}

// the rung the ladder gives a shape (0 decode, 1 tile128): a pure host call, for tools and tests
extern "C" int llmc_fp8_scaled_gemm_rung(int64_t M, int64_t N) { return fl_pick_rung(M, N); }
