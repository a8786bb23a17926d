// mx6_gemm.hip — the OCP MXFP6 path on gfx950's block-scaled matrix instruction (v_mfma_scale_f32_16x16x128_f8f6f4 with 6-bit
// operands): a Linear whose weight is stored as FloatQuantizer(bit='e3m2', float_semantics='ocp', scale_format='e8m0', per_group,
// group_size=32) writes it — e3m2 codes + one e8m0 scale byte per 32 elements — multiplied by an activation quantized on the fly
// into the same form. Next to mx_gemm.hip (MXFP4), which stays what it is. An extension beyond the reference, whose real-quant
// Linears raise in forward.
//   llmc_mx6_pack       codes [R, K], one per byte -> the dense form, 32 codes in 24 bytes per MX block, [R, 3K/4]
//   llmc_mx6_act_quant  X [M, K] bf16 / fp16 -> packed codes + e8m0 scales per 1 x 32 block, one pass (each element read once)
//   llmc_mx6_gemm       C [M, N] = sum over 32-deep blocks of 2^(a_s + b_s - 254) * (A_blk . B_blk^T), fp32 accumulation inside
//                       the instruction, which also applies the scales
// The dense form: a row is a little-endian bit stream, code i of the row at bits 6 i .. 6 i + 5 (code: s eee mm, sign on top). 16
// codes fill 3 dwords, an MX block 6 dwords = 24 bytes, and a lane's 6 operand registers are a plain copy of its block.
// Operand map of the instruction for format code 3 (e3m2), established with exact one-hot data on the GPU: one instruction fed by
// hand, e3m2 against an e2m1 operand whose map is known (mx_gemm.hip), then e3m2 against e3m2 with a different scale in every
// (row, block) — 2048 products each, all exact. With g = l >> 4:
//   operand  lane l holds row (A) / column (B) l & 15 and the 32 consecutive k 32 g .. + 31 in registers 0-5 of its 8 (6, 7 are not
//            read): k = 32 g + i in bits 6 i .. 6 i + 5 of the 192-bit little-endian value the six registers form
//   scale    byte `opsel` of lane l's scale register: the e8m0 scale of row l & 15, k block g, as for the other formats
//   C/D      column l & 15, rows 4 g + r
// In-block arithmetic (measured the same way): the instruction aligns the products of one 32-block to 2^(ea + eb) of the product
// with the largest exponent sum and cuts off what lies more than 13 binary places below that: 784 + 2^-5 (28 x 28 + ...) comes
// back exact, 784 + 2^-6 .. 2^-8 as 784; in the next block of the same instruction the small term survives. e3m2 x e3m2 products
// reach from 2^-8 to 784, so a block can lose bits: of 256 random full-range blocks 109 came back inexact (up to 2^-14 of
// sum |a b|). Remedy (m6_split): an e3m2 value with exponent e (a subnormal counts as e = -2) has its last bit at 2^(e - 2); against
// any e3m2 value (exponent <= 4, last bit >= 2^-4) the products of values with exponents e1 .. e2 lie between 2^(e1 - 6) and the
// alignment point 2^(e2 + 4): inside the window when e2 - e1 <= 3. So the A fragment goes through the instruction in TWO
// exponent classes, the other codes zeroed: exponent field 0 .. 3 (subnormals, 2^-2 .. 2^0) and 4 .. 7 (2^1 .. 2^4) — the top bit
// of the field. Each class sum is exact; the fp32 accumulator joins them. Two instructions per fragment pair: half the rate.
#include "common.h"
#include "float_quant_math.h"
#include "fp8_math.h"
#include "mfma_common.h"
#include "vec16.h"

#include <climits>

namespace llmc {
namespace {

constexpr int MFMA_FMT_E3M2 = 3;                                  // the instruction's cbsz / blgp code (mfma_common.h has 0, 1, 4)

// 16 codes (each below 64) -> 3 dwords of the dense form
__device__ __forceinline__ void m6_pack16(const uint32_t (&c)[16], uint32_t (&w)[3]) {
    w[0] = w[1] = w[2] = 0u;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int bit = 6 * i, j = bit >> 5, s = bit & 31;
        w[j] |= c[i] << s;
        if (s > 26) w[j + 1] |= c[i] >> (32 - s);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// llmc_mx6_pack: one thread per 16 codes (one 16-byte load, three dword stores)
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int M6P_B = 256;
__global__ __launch_bounds__(M6P_B) void k_mx6_pack(const uint8_t* __restrict__ codes, int64_t n16, uint8_t* __restrict__ packed) {
    for (int64_t i = (int64_t)blockIdx.x * M6P_B + threadIdx.x; i < n16; i += (int64_t)gridDim.x * M6P_B) {
        const uint4 raw = *reinterpret_cast<const uint4*>(codes + i * 16);
        const uint32_t in[4] = {raw.x, raw.y, raw.z, raw.w};
        uint32_t c[16], w[3];
#pragma unroll
        for (int k = 0; k < 16; ++k) c[k] = (in[k >> 2] >> (8 * (k & 3))) & 63u;
        m6_pack16(c, w);
        uint32_t* o = reinterpret_cast<uint32_t*>(packed + i * 12);
        o[0] = w[0], o[1] = w[1], o[2] = w[2];
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Activation quantizer. TWO lanes own a block of 32 (16 elements = two 16-byte vectors each), absmax by one DPP step inside
// the pair; a lane's 16 codes are exactly 3 dwords of the dense form, so every lane writes whole dwords (12 bytes, the pair 24
// contiguous ones) and nothing is exchanged. The alternative — four lanes per block as in k_mx_act_quant, 6 bytes each — needs
// a shuffle inside the quad to form dwords (or 2-byte stores); half the lanes per block costs nothing here, the kernel moves
// 2.8 bytes per element and is bound by memory either way. The pair's first lane writes the scale byte.
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int M6Q_B = 256;
template <typename T>
__global__ __launch_bounds__(M6Q_B) void k_mx6_act_quant(const T* __restrict__ X, int64_t nv, uint8_t* __restrict__ codes,
                                                         uint8_t* __restrict__ scales) {
    for (int64_t base = (int64_t)blockIdx.x * M6Q_B; base < nv; base += (int64_t)gridDim.x * M6Q_B) {     // uniform per workgroup
        const int64_t i = base + threadIdx.x;
        const bool active = i < nv;                            // nv is even: a pair is active as a whole
        Vec<T, 8> w[2];
        float m = 0.0f;
        if (active) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                w[h] = load_vec<T, 8>(X + i * 16 + h * 8);
#pragma unroll
                for (int k = 0; k < 8; ++k) m = fmaxf(m, fabsf(to_f32<T>(w[h].v[k])));
            }
        }
        m = fpx_seg_max(m, 2);
        if (!active) continue;
        const uint32_t c = e8m0_code(m, 4);                    // emax of e3m2: 28 = 1.75 * 2^4
        if ((i & 1) == 0) scales[i >> 1] = (uint8_t)c;
        const float rs = e8m0_recip(c);
        uint32_t q[16], o[3];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const float x = to_f32<T>(w[k >> 3].v[k & 7]);
            const float t = __builtin_fmaf(x, rs, 0.0f);
            q[k] = (uint32_t)fpx_encode<3, 2>(fpx_ocp_quantize<3, 2>(x != x ? x : t)) & 63u;
        }
        m6_pack16(q, o);
        uint32_t* dst = reinterpret_cast<uint32_t*>(codes + i * 12);
        dst[0] = o[0], dst[1] = o[1], dst[2] = o[2];
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// The two exponent classes of a fragment (the header has the why). A fragment is two 96-bit halves of 16 codes; bit 4 of a code
// is the top bit of its exponent field. From the marker bits b (one per code, at 6 i + 4) the 6-bit masks are
// (b << 2) - (b >> 4) = 2^(6 i + 6) - 2^(6 i) per marked code: no borrow passes from one code to another.
// ---------------------------------------------------------------------------------------------------------------------------
typedef unsigned __int128 u128;
__device__ __forceinline__ void m6_split(const uint32_t (&x)[6], i32x8& lo, i32x8& hi) {
    u128 b4 = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) b4 |= (u128)1 << (6 * i + 4);
    lo = i32x8{0, 0, 0, 0, 0, 0, 0, 0};
    hi = lo;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const u128 v = (u128)x[3 * h] | ((u128)x[3 * h + 1] << 32) | ((u128)x[3 * h + 2] << 64);
        const u128 b = v & b4;
        const u128 up = v & ((b << 2) - (b >> 4));
        const u128 dn = v ^ up;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            hi[3 * h + r] = (int)(uint32_t)(up >> (32 * r));
            lo[3 * h + r] = (int)(uint32_t)(dn >> (32 * r));
        }
    }
}

struct Mx6GemmArgs {
    const uint8_t* A; const uint8_t* As; const uint8_t* B; const uint8_t* Bs;
    int64_t M, N, K;
    const void* bias; void* C;
    int ntm;
};

// one rounding to the output dtype, then the bias in that dtype (llmc_mx_gemm's order)
template <int DT> __device__ __forceinline__ void m6_store(const Mx6GemmArgs& a, int64_t row, int64_t col, float v) {
    if (row < a.M && col < a.N) {
        float y = rndc<DT>(v);
        if (a.bias) y = rndc<DT>(y + load_as_f32(a.bias, col, DT));
        store_from_f32(a.C, row * a.N + col, DT, y);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Tile rung. Workgroup tile 128 (m) x 128 (n), 4 waves as 2 x 2, wave tile 64 x 64 = 4 x 4 accumulators of 16 x 16. A K
// sub-step is 128 deep: 96 bytes of a row, two instructions per accumulator (the two classes of the A fragment). Two stages of
// LDS-DMA: the pieces of stage s + 1 are issued right after the barrier that publishes stage s and land under its MFMAs.
// LDS image of a sub-step: A panel [128 rows][112 bytes], B panel [128][112], then the scale dwords [128 rows][4 blocks] of A
// and of B: 29 KiB. KSUB = 1 sub-step per stage: 58 KiB for the two stages, so that TWO workgroups share a CU's 160 KiB and one
// computes while the other waits at its barrier (KSUB = 2 would leave one workgroup of 4 waves per CU).
// The 96 bytes of a row are 6 of the 16-byte chunks an LDS-DMA lane moves; the panel gives a row 7 chunk slots (pitch 112). A
// panel is 896 slots = 14 pieces of 64 lanes; slot q = 64 p + lane is row q / 7, chunk q % 7, and the lanes of the seventh slot
// point past the descriptor's end (they bring zeros that nobody reads). Why 112: lane l reads its fragment — bytes 24 g .. + 23
// of row l & 15, g = l >> 4 — with three ds_read_b64, each served 32 lanes (g = 0, 1 or g = 2, 3) at a time over 64 banks of 4
// bytes = 32 slots of 8 bytes. Read j of lane (r, g) lies in slot (pitch / 8) r + 3 g + j:
//   pitch  96: 12 r mod 32 = 0 12 24 4 16 28 8 20 | 0 12 ...: rows r and r + 8 meet in one slot, every read is a 2-way conflict
//   pitch 112: 14 r mod 32 = 0 14 28 10 24 6 20 2 16 30 12 26 8 22 4 18: the 16 even residues once each; g = 1 adds 3 and takes
//              the 16 odd ones; j and the pair g = 2, 3 (+ 6) shift all 32 alike: 32 lanes, 32 slots
// (the 32-lane service of ds_read_b64 is the documented LDS rate, 128 bytes a clock per CU half, not something measured here).
// The price is 14 DMA pieces per panel where 12 would carry the data.
// Edges: the buffer descriptors end at the tile's last valid row, so rows past M / N arrive as zeros; the stores are masked.
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int M6_T = 128, M6_THREADS = 256;
constexpr int M6_RB = 96, M6_PITCH = 112, M6_PANEL = M6_T * M6_PITCH, M6_PIECES = M6_PANEL / 1024;
constexpr int M6_A_OFF = 0, M6_B_OFF = M6_PANEL, M6_SA_OFF = 2 * M6_PANEL, M6_SB_OFF = M6_SA_OFF + M6_T * 4;
constexpr int M6_SUB = M6_SB_OFF + M6_T * 4, M6_KSUB = 1, M6_STAGE = M6_KSUB * M6_SUB, M6_LDS = 2 * M6_STAGE;
constexpr int M6_NP = 2 * M6_PIECES / 4;                          // pieces of a sub-step per wave: 28 / 4
static_assert(M6_PANEL % 1024 == 0 && (2 * M6_PIECES) % 4 == 0, "whole DMA pieces, dealt evenly");

template <int DT>
__global__ __launch_bounds__(M6_THREADS) void k_mx6_gemm(Mx6GemmArgs a) {
    extern __shared__ __attribute__((aligned(16))) char m6_smem[];
    LDS_AS char* lds = (LDS_AS char*)m6_smem;
    const uint32_t lbase = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(uintptr_t)lds);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wv >> 1, wn = wv & 1;
    const int tm = blockIdx.x % a.ntm, tn = blockIdx.x / a.ntm;     // m fastest: the blocks in flight share weight panels
    const int64_t m0 = (int64_t)tm * M6_T, n0 = (int64_t)tn * M6_T;
    const int nk = (int)(a.K / 128);
    const uint32_t rowb = (uint32_t)(a.K / 4 * 3), srow = (uint32_t)(a.K / 32);                 // row bytes: codes, scales
    const int64_t mrows = a.M - m0 < M6_T ? a.M - m0 : M6_T, nrows = a.N - n0 < M6_T ? a.N - n0 : M6_T;
    const i32x4 ra = rsrc_words(a.A + m0 * rowb, mrows * rowb), rb = rsrc_words(a.B + n0 * rowb, nrows * rowb);
    // scales: waves 0, 1 move A's (rows 0-63, 64-127 of the tile), waves 2, 3 B's
    const i32x4 rs = wv < 2 ? rsrc_words(a.As + m0 * srow, mrows * srow) : rsrc_words(a.Bs + n0 * srow, nrows * srow);
    const uint32_t sdst = (uint32_t)((wv < 2 ? M6_SA_OFF : M6_SB_OFF) + (wv & 1) * 256);
    const uint32_t svoff = (uint32_t)((wv & 1) * 64 + lane) * srow;

    // DMA pieces: the 28 pieces of a sub-step (14 of A, then 14 of B: the B panel follows the A panel) are dealt round the four
    // waves, piece P = wv + 4 i. The row term stays in the vector offset (the part the descriptor's bound is checked against).
    uint32_t vo[M6_NP];
#pragma unroll
    for (int i = 0; i < M6_NP; ++i) {
        const int q = 64 * ((wv + 4 * i) % M6_PIECES) + lane, row = q / 7, ch = q % 7;
        vo[i] = ch == 6 ? 0x80000000u : (uint32_t)row * rowb + (uint32_t)(ch << 4);
    }
    auto dma_sub = [&](uint32_t sub, int ks) {                  // sub: LDS address of the sub-step's image
#pragma unroll
        for (int i = 0; i < M6_NP; ++i) {
            const int P = wv + 4 * i;
            dma_imm_at<0>(P < M6_PIECES ? ra : rb, vo[i], (uint32_t)ks * (uint32_t)M6_RB, sub + (uint32_t)P * 1024u);
        }
        dma_imm_at<0, 4>(rs, svoff, (uint32_t)ks * 4u, sub + sdst);
    };

    // fragment reads: row 16 t + (lane & 15) of the wave's 64, bytes 24 (lane >> 4) .. + 23 (the operand map above)
    const int fr = lane & 15, fq = lane >> 4;
    int offA[4], offB[4], offSA[4], offSB[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int rowa = wm * 64 + 16 * t + fr, rowb_ = wn * 64 + 16 * t + fr;
        offA[t] = M6_A_OFF + rowa * M6_PITCH + 24 * fq;
        offB[t] = M6_B_OFF + rowb_ * M6_PITCH + 24 * fq;
        offSA[t] = M6_SA_OFF + rowa * 4 + fq;
        offSB[t] = M6_SB_OFF + rowb_ * 4 + fq;
    }

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    auto mma_sub = [&](int sub) {                                // sub: byte offset of the sub-step's image in `lds`
        i32x8 fb[4];
        uint32_t fa[4][6];
        int sa[4], sb[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            fb[t] = i32x8{0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const u32x2 pa = *(LDS_AS const u32x2*)(lds + sub + offA[t] + 8 * j);
                const u32x2 pb = *(LDS_AS const u32x2*)(lds + sub + offB[t] + 8 * j);
                fa[t][2 * j] = pa.x, fa[t][2 * j + 1] = pa.y;
                fb[t][2 * j] = (int)pb.x, fb[t][2 * j + 1] = (int)pb.y;
            }
            sa[t] = (int)*(LDS_AS const uint8_t*)(lds + sub + offSA[t]);
            sb[t] = (int)*(LDS_AS const uint8_t*)(lds + sub + offSB[t]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            i32x8 fc[2];
            m6_split(fa[i], fc[0], fc[1]);
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[i][j] = mfma_scale_16x16x128<MFMA_FMT_E3M2, MFMA_FMT_E3M2>(fc[c], fb[j], acc[i][j], sa[i], sb[j]);
        }
    };

    const int nst = (nk + M6_KSUB - 1) / M6_KSUB;
    auto stage_dma = [&](int s) {
#pragma unroll
        for (int h = 0; h < M6_KSUB; ++h)
            if (s * M6_KSUB + h < nk) dma_sub(lbase + (uint32_t)((s & 1) * M6_STAGE + h * M6_SUB), s * M6_KSUB + h);
    };
    stage_dma(0);
    for (int s = 0; s < nst; ++s) {
        // my fragment reads of the stage about to be refilled are back, my DMA pieces of stage s have landed; then everybody's
        lds_wait_all();
        vm_wait<0>();
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        if (s + 1 < nst) stage_dma(s + 1);
#pragma unroll
        for (int h = 0; h < M6_KSUB; ++h)
            if (s * M6_KSUB + h < nk) mma_sub((s & 1) * M6_STAGE + h * M6_SUB);
    }

#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                m6_store<DT>(a, m0 + wm * 64 + 16 * i + 4 * fq + r, n0 + wn * 64 + 16 * j + fr, acc[i][j][r]);
}

// ---------------------------------------------------------------------------------------------------------------------------
// Decode rung, M <= 16: the 128-row tile would spend 7/8 of its instructions on rows that do not exist, and the weight stream
// decides the time. One workgroup per 16 output columns (N / 16 workgroups: 256 for a 4096-wide layer), 8 waves; the 128-deep
// sub-steps of K are dealt round the waves (wave w takes w, w + 8, ...). No LDS on the way in: under the operand map a lane's
// fragment is 24 contiguous bytes of its row, so every lane loads its own (three 8-byte loads; the four lanes of a row read 96
// contiguous bytes), the A rows from cache. The eight partial 16 x 16 tiles meet in LDS and wave 0 adds them in wave order: no
// atomics, the same bits on every run.
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int M6D_WAVES = 8, M6D_THREADS = 64 * M6D_WAVES, M6D_MAX_M = 16;

template <int DT>
__global__ __launch_bounds__(M6D_THREADS) void k_mx6_gemm_decode(Mx6GemmArgs a) {
    __shared__ f32x4 part[M6D_WAVES][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, fr = lane & 15, fq = lane >> 4;
    const int64_t n0 = (int64_t)blockIdx.x * 16;
    const int nk = (int)(a.K / 128);
    const int64_t rowb = a.K / 4 * 3, srow = a.K / 32;
    const bool va = fr < a.M, vb = n0 + fr < a.N;
    const uint8_t* pa = a.A + (va ? fr : 0) * rowb + 24 * fq;
    const uint8_t* pb = a.B + (vb ? n0 + fr : 0) * rowb + 24 * fq;
    const uint8_t* psa = a.As + (va ? fr : 0) * srow + fq;
    const uint8_t* psb = a.Bs + (vb ? n0 + fr : 0) * srow + fq;
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int ks = wv; ks < nk; ks += M6D_WAVES) {
        uint32_t fa[6] = {0u, 0u, 0u, 0u, 0u, 0u};
        i32x8 fb = {0, 0, 0, 0, 0, 0, 0, 0};
        int sa = 0, sb = 0;
        if (va) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const uint2 p = *reinterpret_cast<const uint2*>(pa + (int64_t)ks * M6_RB + 8 * j);
                fa[2 * j] = p.x, fa[2 * j + 1] = p.y;
            }
            sa = psa[ks * 4];
        }
        if (vb) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const uint2 p = *reinterpret_cast<const uint2*>(pb + (int64_t)ks * M6_RB + 8 * j);
                fb[2 * j] = (int)p.x, fb[2 * j + 1] = (int)p.y;
            }
            sb = psb[ks * 4];
        }
        i32x8 fc[2];
        m6_split(fa, fc[0], fc[1]);
#pragma unroll
        for (int c = 0; c < 2; ++c) acc = mfma_scale_16x16x128<MFMA_FMT_E3M2, MFMA_FMT_E3M2>(fc[c], fb, acc, sa, sb);
    }
    part[wv][lane] = acc;
    __syncthreads();
    if (wv != 0) return;
    f32x4 sum = part[0][lane];
#pragma unroll
    for (int w = 1; w < M6D_WAVES; ++w) sum = sum + part[w][lane];
#pragma unroll
    for (int r = 0; r < 4; ++r) m6_store<DT>(a, 4 * fq + r, n0 + fr, sum[r]);
}

// The ladder is data: the first rung whose max_m takes M runs.
struct M6Rung { int64_t max_m; const char* name; };
constexpr M6Rung M6_LADDER[] = {{M6D_MAX_M, "decode"}, {LLONG_MAX, "tile128"}};
constexpr int M6_RUNGS = (int)(sizeof(M6_LADDER) / sizeof(M6_LADDER[0]));

int m6_rung(int64_t M) {
    int r = 0;
    while (M > M6_LADDER[r].max_m) ++r;
    return r;
}

int m6_launch(const Mx6GemmArgs& a, int out_dt, int rung, hipStream_t st) {
    Mx6GemmArgs b = a;
    void* kargs[] = {(void*)&b};
    if (rung == 0) {
        const void* fn = out_dt == LLMC_F16 ? (const void*)k_mx6_gemm_decode<LLMC_F16>
                       : out_dt == LLMC_BF16 ? (const void*)k_mx6_gemm_decode<LLMC_BF16> : (const void*)k_mx6_gemm_decode<LLMC_F32>;
        LLMC_HIP_CHECK(hipLaunchKernel(fn, dim3((unsigned)ceil_div64(a.N, 16)), dim3(M6D_THREADS), kargs, 0, st));
        return LLMC_OK;
    }
    const void* fn = out_dt == LLMC_F16 ? (const void*)k_mx6_gemm<LLMC_F16>
                   : out_dt == LLMC_BF16 ? (const void*)k_mx6_gemm<LLMC_BF16> : (const void*)k_mx6_gemm<LLMC_F32>;
    if (int rc = ensure_dynamic_lds(fn, M6_LDS)) return rc;
    LLMC_HIP_CHECK(hipLaunchKernel(fn, dim3((unsigned)(a.ntm * ceil_div64(a.N, M6_T))), dim3(M6_THREADS), kargs, (size_t)M6_LDS, st));
    return LLMC_OK;
}

}  // namespace
}  // namespace llmc

using namespace llmc;

extern "C" int llmc_mx6_pack(const void* codes, int64_t R, int64_t K, void* packed, llmc_stream_t stream) {
    LLMC_REQUIRE(codes && packed && R > 0 && K > 0, "mx6_pack: null/empty argument");
    LLMC_REQUIRE(((uintptr_t)codes & 15) == 0 && ((uintptr_t)packed & 3) == 0, "mx6_pack: the codes need 16-byte, the packed form 4-byte alignment");
    if (K % 32) {
        set_last_error_msg("mx6_pack: K must be a multiple of the 32-element MX block");
        return LLMC_ENOTSUP;
    }
    const int64_t n16 = R * K / 16;
    hipLaunchKernelGGL(k_mx6_pack, dim3(capped_grid(n16, M6P_B, 8192)), dim3(M6P_B), 0, (hipStream_t)stream, (const uint8_t*)codes, n16,
                       (uint8_t*)packed);
    LLMC_LAUNCH_CHECK();
    return LLMC_OK;
}

extern "C" int llmc_mx6_act_quant(const void* X, int dt, int64_t M, int64_t K, void* out_codes, void* out_scales, llmc_stream_t stream) {
    LLMC_REQUIRE(X && out_codes && out_scales && M > 0 && K > 0, "mx6_act_quant: null/empty argument");
    LLMC_REQUIRE(dt == LLMC_F16 || dt == LLMC_BF16, "mx6_act_quant: X must be bf16 or fp16");
    LLMC_REQUIRE(((uintptr_t)X & 15) == 0 && ((uintptr_t)out_codes & 3) == 0, "mx6_act_quant: X needs 16-byte, the codes 4-byte alignment");
    if (K % 32) {
        set_last_error_msg("mx6_act_quant: K must be a multiple of the 32-element MX block");
        return LLMC_ENOTSUP;
    }
    hipStream_t st = (hipStream_t)stream;
    const int64_t nv = M * K / 16;
    const dim3 grid(capped_grid(nv, M6Q_B, 16384));
    if (dt == LLMC_BF16) hipLaunchKernelGGL((k_mx6_act_quant<bf16_t>), grid, dim3(M6Q_B), 0, st, (const bf16_t*)X, nv, (uint8_t*)out_codes, (uint8_t*)out_scales);
    else hipLaunchKernelGGL((k_mx6_act_quant<f16_t>), grid, dim3(M6Q_B), 0, st, (const f16_t*)X, nv, (uint8_t*)out_codes, (uint8_t*)out_scales);
    LLMC_LAUNCH_CHECK();
    return LLMC_OK;
}

extern "C" int llmc_mx6_gemm_rung(int64_t M, int64_t N, int64_t K) {
    (void)N, (void)K;
    return m6_rung(M);
}

extern "C" int llmc_mx6_gemm_on_rung(const void* A6, const void* a_s, const void* B6, const void* b_s, int64_t M, int64_t N, int64_t K,
                                     int out_dt, const void* bias, void* C, int rung, llmc_stream_t stream) {
    LLMC_REQUIRE(A6 && a_s && B6 && b_s && C && M > 0 && N > 0 && K > 0, "mx6_gemm: null/empty argument");
    LLMC_REQUIRE(out_dt == LLMC_F16 || out_dt == LLMC_BF16 || out_dt == LLMC_F32, "mx6_gemm: bad output dtype");
    LLMC_REQUIRE((((uintptr_t)A6 | (uintptr_t)B6) & 15) == 0 && (((uintptr_t)a_s | (uintptr_t)b_s) & 3) == 0 &&
                 ((uintptr_t)C & (out_dt == LLMC_F32 ? 3 : 1)) == 0 && ((uintptr_t)bias & (out_dt == LLMC_F32 ? 3 : 1)) == 0,
                 "mx6_gemm: codes need 16-byte, scales 4-byte, C and bias element alignment");
    LLMC_REQUIRE(rung >= -1 && rung < M6_RUNGS, "mx6_gemm: no such rung");
    LLMC_REQUIRE(rung != 0 || M <= M6D_MAX_M, "mx6_gemm: the decode rung takes M <= 16");
    if (K % 128) {
        set_last_error_msg("mx6_gemm: K must be a multiple of 128 (the depth of one block-scaled matrix instruction)");
        return LLMC_ENOTSUP;
    }
    if (K >= (1ll << 24) || ceil_div64(M, M6_T) * ceil_div64(N, M6_T) >= (1ll << 31) || ceil_div64(N, 16) >= (1ll << 31)) {
        set_last_error_msg("mx6_gemm: K must be below 2^24 and the tile count below 2^31");
        return LLMC_ENOTSUP;
    }
    Mx6GemmArgs a;
    a.A = (const uint8_t*)A6; a.As = (const uint8_t*)a_s; a.B = (const uint8_t*)B6; a.Bs = (const uint8_t*)b_s;
    a.M = M; a.N = N; a.K = K; a.bias = bias; a.C = C;
    a.ntm = (int)ceil_div64(M, M6_T);
    return m6_launch(a, out_dt, rung < 0 ? m6_rung(M) : rung, (hipStream_t)stream);
}

extern "C" int llmc_mx6_gemm(const void* A6, const void* a_s, const void* B6, const void* b_s, int64_t M, int64_t N, int64_t K,
                             int out_dt, const void* bias, void* C, llmc_stream_t stream) {
    return llmc_mx6_gemm_on_rung(A6, a_s, B6, b_s, M, N, K, out_dt, bias, C, -1, stream);
}
