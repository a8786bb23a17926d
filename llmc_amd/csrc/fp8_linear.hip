// fp8_linear.hip — the plain W8A8-FP8 Linear: A [M, K] and B [N, K] OCP e4m3fn codes whose scales are constant along K (one per
// token or one per tensor for A, one per output channel or one per tensor for B), the stored form of the reference's
// configs/quantization/backend/{vllm,sglang}/fp8 configurations (an extension: its real-quant Linears raise in forward).
//   llmc_fp8_scaled_gemm    acc[m, n] = sum_k a[m, k] b[n, k] in fp32 on the fp8 matrix pipe,
//                           C[m, n] = rnd_out(fl(fl(acc * a_s[m]) * b_s[n])), then the bias in the output dtype
// Both scales leave the K loop: it holds loads, LDS traffic and matrix instructions only (llmc_fp8_block_gemm pays two VALU ops
// per element and 128-deep K block for its block scales). The tile rung's structure, the epilogue and the launches are scaled8_gemm.h's, shared
// with i8_linear.hip; this file states the number format (Fp8Code), its decode kernel, the ladder and the entry points.
//
// Matrix instruction: the NON-scaled forms v_mfma_f32_32x32x16_fp8_fp8 (tile rung) and v_mfma_f32_16x16x32_fp8_fp8 (decode rung),
// two consecutive instructions on a lane's 16 consecutive bytes.
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
#include "scaled8_gemm.h"

namespace llmc {

// K % 128 == 0 only: a zeroed byte of B against a NaN code of A is NaN, so a ragged chunk cannot be masked away as int8's is
struct Fp8Code {
    typedef float acc_t;
    static constexpr bool RAGGED_K = false;
    static __device__ __forceinline__ f32x16 mac32(i32x4 a, i32x4 b, f32x16 c) { return mfma_f32_32x32x16_fp8_x2(a, b, c); }
    static __device__ __forceinline__ float to_float(float acc) { return acc; }
};
struct Fp8ScaledArgs : Scaled8Args {};      // the kernels' full names, as profiles and traces carry them, include this name

template <int DT, int WM, int WN>
__global__ __launch_bounds__(256) void k_fp8_scaled_tile(Fp8ScaledArgs a) { s8_tile_body<Fp8Code, DT, WM, WN>(a); }

// The decode rung keeps a kernel of its own: s8_decode_body's loop, with two instructions per 16 bytes and the rows past M / N
// selected to zero where they are used. Measured (profiles/scaled8_refactor.txt): s8_decode_body<Fp8Code, ..>, and this kernel
// with nothing but its two selects taken out, run 1.4 to 4.9 % slower at 64 and 16 tokens: without the selects hipcc asks for the
// second operand set's chunks in two rounds with a full memory wait each, with them for all ten loads at once.
template <int MT> struct Fp8DecodeOperands {
    uint4 b[2], x[MT][2];
};

template <int DT, int MT>
__global__ __launch_bounds__(64 * S8D_WAVES) void k_fp8_scaled_decode(Fp8ScaledArgs a) {
    __shared__ float red[S8D_WAVES * MT * 256];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int r = lane & 15, g = lane >> 4;
    const int64_t n0 = (int64_t)blockIdx.x * S8D_N;
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
    load(s1, wv + S8D_WAVES);
    for (int kb = wv; kb < nkb; kb += 2 * S8D_WAVES) {
        mac(s0);
        load(s0, kb + 2 * S8D_WAVES);
        if (kb + S8D_WAVES < nkb) mac(s1);
        load(s1, kb + 3 * S8D_WAVES);
    }

    // the K slices meet in LDS and are added in wave order. Accumulator register q of lane l is row 4 (l >> 4) + q, column l & 15.
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int q = 0; q < 4; ++q) red[(wv * MT + mt) * 256 + q * 64 + lane] = acc[mt][q];
    __syncthreads();
    for (int e = tid; e < MT * 256; e += 64 * S8D_WAVES) {
        float s = red[e];
#pragma unroll
        for (int w = 1; w < S8D_WAVES; ++w) s += red[w * MT * 256 + e];
        const int ln = e & 63;
        const int64_t row = 16 * (e >> 8) + 4 * (ln >> 4) + ((e >> 6) & 3), col = n0 + (ln & 15);
        if (row < a.M && col < a.N) s8_store<Fp8Code, DT>(a, row, col, s, a.As[a.as_rows ? row : 0], a.Bs[a.bs_rows ? col : 0]);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// which rung takes which shape: the first row whose bounds hold. Set from tools/bench_fp8_linear.py (profiles/fp8_linear.txt): at
// 64, 16 and 1 tokens the decode rung is 1.6 to 18 times faster than the tile rung on every Llama-3-8B shape (N / 16 workgroups
// of 512 threads fill the chip from N = 4096 up); 64 is also the most the decode kernel is compiled for. (A 256 x 128 tile of
// tile128's structure, 128 accumulator registers and one wave per SIMD, was measured and dropped: 1.4 to 1.7 times slower at
// every shape.)
// ---------------------------------------------------------------------------------------------------------------
enum { FL_DECODE = 0, FL_TILE128 = 1, FL_NRUNGS = 2 };
struct Fp8Rung {
    int64_t max_m;          // M <= max_m
    int rung;
};
static const Fp8Rung FL_LADDER[] = {
    {S8_DECODE_MAX_M, FL_DECODE},
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
    if (rung == FL_DECODE)
        s8_launch_decode(a, dim3((unsigned)ceil_div64(a.N, S8D_N)), st, k_fp8_scaled_decode<DT, 1>, k_fp8_scaled_decode<DT, 2>,
                         k_fp8_scaled_decode<DT, 4>);
    else
        s8_launch_tile128(a, st, k_fp8_scaled_tile<DT, 2, 2>);
    LLMC_LAUNCH_CHECK();
    return LLMC_OK;
}

}  // namespace llmc

using namespace llmc;

// rung: -1 = the ladder chooses; 0 .. FL_NRUNGS - 1 = that rung whatever the shape (the measuring tool and the tests)
extern "C" int llmc_fp8_scaled_gemm_on_rung(const void* A8, const float* a_s, int64_t a_s_n, const void* B8, const float* b_s,
                                            int64_t b_s_n, int64_t M, int64_t N, int64_t K, int out_dt, const void* bias, void* C,
                                            int rung_arg, llmc_stream_t stream) {
    Fp8ScaledArgs a;
    const int forced = rung_arg;
    if (const int rc = s8_check_operands("fp8_scaled_gemm", A8, a_s, B8, b_s, C, M, N, K, out_dt)) return rc;
    LLMC_REQUIRE(forced >= -1 && forced < FL_NRUNGS && (forced != FL_DECODE || M <= S8_DECODE_MAX_M),
                 "fp8_scaled_gemm: no such rung (the decode rung takes M <= 64)");
    if (const int rc = s8_check_scales("fp8_scaled_gemm", a_s_n, b_s_n, M, N)) return rc;
    s8_fill_args(a, A8, a_s, a_s_n, B8, b_s, b_s_n, M, N, K, bias, C);
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
    const int rung = forced >= 0 ? forced : fl_pick_rung(M, N);
    hipStream_t st = (hipStream_t)stream;
    return s8_with_out_dt(out_dt, [&](auto dt) { return fl_launch<decltype(dt)::value>(a, rung, st); });
}

extern "C" int llmc_fp8_scaled_gemm(const void* A8, const float* a_s, int64_t a_s_n, const void* B8, const float* b_s, int64_t b_s_n,
                                    int64_t M, int64_t N, int64_t K, int out_dt, const void* bias, void* C, llmc_stream_t stream) {
    return llmc_fp8_scaled_gemm_on_rung(A8, a_s, a_s_n, B8, b_s, b_s_n, M, N, K, out_dt, bias, C, -1, stream);
}

// the rung the ladder gives a shape (0 decode, 1 tile128): a pure host call, for tools and tests
extern "C" int llmc_fp8_scaled_gemm_rung(int64_t M, int64_t N) { return fl_pick_rung(M, N); }
