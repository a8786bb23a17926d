// mx_gemm.hip — the OCP MX path on gfx950's block-scaled matrix instruction (v_mfma_scale_f32_16x16x128_f8f6f4): a Linear whose
// weight is stored as FloatQuantizer(bit='e2m1', float_semantics='ocp', scale_format='e8m0', per_group, group_size=32) writes
// it — e2m1 codes packed two per byte + one e8m0 scale byte per 32 elements — multiplied by an activation quantized on the fly
// into the same form (MXFP4) or into e4m3 codes with e8m0 block scales (MXFP8). An extension beyond the reference, whose
// real-quant Linears raise in forward.
//   llmc_mx_act_quant  X [M, K] bf16 / fp16 -> codes + e8m0 scales per 1 x 32 block, one pass (each element read once)
//   llmc_mx_gemm       C [M, N] = sum over 32-deep blocks of 2^(a_s + b_s - 254) * (A_blk . B_blk^T), fp32 accumulation inside
//                      the instruction, which also applies the scales: no accumulator update on the VALU per K block
// Rules of llmc_mx_act_quant (restated in tests/mx_oracle.py):
//   absmax    fmaxf over |x| from 0: a NaN element is ignored, an infinity gives the exponent field 255 (llmc_fpx_quant's rule)
//   scale     e8m0 byte clamp(exponent_field(absmax) - emax, 0, 254), 127 for an all-zero block; emax = 2 (e2m1) / 8 (e4m3)
//   element   t = x * 2^(127 - byte) (exact: fp32 product of a 16-bit value and a power of two)
//   e2m1      round to nearest even onto the OCP grid, saturating at +-6 (infinities too); a NaN gives 6 with the input's sign; the
//             sign survives on a zero. Bit for bit llmc_fpx_quant(ocp | e8m0, g = 32) + llmc_fp4_pack.
//   e4m3      round to nearest even, saturating at +-448 (infinities too); a NaN gives the NaN code 0x7f with the input's sign.
// Operand maps of the instruction (16x16x128; established with exact one-hot data, tests/test_mx_gemm_gpu.py). With g = l >> 4:
//   e2m1   lane l holds row (A) / column (B) l & 15 and the 32 consecutive k 32 g .. + 31 in 4 registers (16 bytes of a packed row)
//   e4m3   lane l holds the same row and TWO runs of 16 k: 16 g .. + 15 in registers 0-3 and 64 + 16 g .. + 15 in registers 4-7
//          (the instruction works through an 8-bit operand in two 64-deep halves) — NOT 32 consecutive k
//   scale  byte `opsel` of lane l's scale register is the e8m0 scale of row l & 15 and k block g (k 32 g .. + 31) whatever the
//          operand's format: for e4m3 that block lives in the registers of two other lane groups
//   C/D    column l & 15, rows 4 g + r, as the bf16 form of the shape
// and its arithmetic cuts small e4m3 products off inside a block (mg_e4m3_classes below: the kernel feeds it one exponent class
// of the activation at a time, three instructions per e4m3 fragment, so that nothing is cut).
#include "common.h"
#include "float_quant_math.h"
#include "fp8_math.h"
#include "mfma_common.h"
#include "vec16.h"

namespace llmc {
namespace {

constexpr int MX_E2M1 = 2, MX_E4M3 = 4;

// ---------------------------------------------------------------------------------------------------------------------------
// Activation quantizer: four lanes own a block of 32 (one 16-byte vector of 16-bit elements each), absmax by two DPP steps
// inside the quad, every lane writes its 4 bytes (e2m1) or 8 bytes (e4m3) of codes, the quad's first lane the scale byte.
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int AQ_B = 256;

// e4m3 codes of two scaled elements (x: the inputs, for the NaN rule). fmed3 clamps to +-448 (an infinity too); inside that
// range v_cvt_pk_fp8_f32 is the RNE cast (fp8_math.h)
__device__ __forceinline__ uint32_t mx_e4m3_pair(float x0, float t0, float x1, float t1) {
    const float c0 = x0 != x0 ? 0.0f : __builtin_amdgcn_fmed3f(t0, -448.0f, 448.0f);
    const float c1 = x1 != x1 ? 0.0f : __builtin_amdgcn_fmed3f(t1, -448.0f, 448.0f);
    uint32_t c = f32x2_to_e4m3fn(c0, c1);
    if (x0 != x0) c = (c & 0xff00u) | ((__float_as_uint(x0) >> 24) & 0x80u) | 0x7fu;
    if (x1 != x1) c = (c & 0x00ffu) | ((((__float_as_uint(x1) >> 24) & 0x80u) | 0x7fu) << 8);
    return c;
}

template <typename T, int FMT>
__global__ __launch_bounds__(AQ_B) void k_mx_act_quant(const T* __restrict__ X, int64_t nv, uint8_t* __restrict__ codes,
                                                       uint8_t* __restrict__ scales) {
    constexpr int EMAX = FMT == MX_E2M1 ? 2 : 8;
    for (int64_t base = (int64_t)blockIdx.x * AQ_B; base < nv; base += (int64_t)gridDim.x * AQ_B) {     // uniform per workgroup
        const int64_t i = base + threadIdx.x;
        const bool active = i < nv;                            // nv is a multiple of 4: a quad is active as a whole
        Vec<T, 8> w;
        float m = 0.0f;
        if (active) {
            w = load_vec<T, 8>(X + i * 8);
#pragma unroll
            for (int k = 0; k < 8; ++k) m = fmaxf(m, fabsf(to_f32<T>(w.v[k])));
        }
        m = fpx_seg_max(m, 4);
        if (!active) continue;
        const uint32_t c = e8m0_code(m, EMAX);
        if ((i & 3) == 0) scales[i >> 2] = (uint8_t)c;
        const float rs = e8m0_recip(c);
        float x[8], t[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            x[k] = to_f32<T>(w.v[k]);
            t[k] = __builtin_fmaf(x[k], rs, 0.0f);
        }
        if constexpr (FMT == MX_E2M1) {
            uint32_t o = 0;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float v = fpx_ocp_quantize<2, 1>(x[k] != x[k] ? x[k] : t[k]);
                o |= (uint32_t)(fpx_encode<2, 1>(v) & 0xfu) << (4 * k);
            }
            *reinterpret_cast<uint32_t*>(codes + i * 4) = o;
        } else {
            uint2 o;
            o.x = mx_e4m3_pair(x[0], t[0], x[1], t[1]) | (mx_e4m3_pair(x[2], t[2], x[3], t[3]) << 16);
            o.y = mx_e4m3_pair(x[4], t[4], x[5], t[5]) | (mx_e4m3_pair(x[6], t[6], x[7], t[7]) << 16);
            *reinterpret_cast<uint2*>(codes + i * 8) = o;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// GEMM. Workgroup tile 128 (m) x 128 (n), 4 waves as 2 x 2, wave tile 64 x 64 = 4 x 4 accumulators of 16 x 16. A K sub-step
// is 128 deep (one instruction per accumulator); a stage holds KSUB sub-steps (FP4 tiles are small: the LDS goes into depth
// per barrier, not into a wider tile), two stages: the LDS-DMA of stage s + 1 is issued right after the barrier that publishes
// stage s and lands under its MFMAs.
// LDS image of a sub-step: A panel [128 rows][AB bytes], B panel [128][64], then the scale bytes [128 rows][4 blocks] of A and
// of B. Panels are filled by 16-byte LDS-DMA pieces (1 KiB = 16 / 8 rows per wave instruction), the 16-byte chunk index XOR-ed
// with a per-row key on the DMA source address and on the fragment read, so that every ds_read_b128 lane group touches 16
// distinct bank slots. The scales travel as one dword per row and sub-step and are read back bytewise: lane l takes byte
// l >> 4 of its row's dword, the scale of k block l >> 4.
// Edges: the buffer descriptors end at the tile's last valid row, so rows past M / N arrive as zeros; the stores are masked.
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int MG_T = 128;
constexpr int MG_THREADS = 256;

template <int AFMT> struct MgGeo {
    static constexpr int AB = AFMT == MX_E2M1 ? 64 : 128;         // bytes of a row per sub-step
    static constexpr int KSUB = AFMT == MX_E2M1 ? 2 : 1;
    static constexpr int A_OFF = 0, B_OFF = MG_T * AB, SA_OFF = B_OFF + MG_T * 64, SB_OFF = SA_OFF + MG_T * 4;
    static constexpr int SUB = SB_OFF + MG_T * 4;
    static constexpr int STAGE = KSUB * SUB;
    static constexpr int LDS = 2 * STAGE;
};

// chunk keys: 64-byte rows (read at chunk g) by (row >> 2) & 3, 128-byte rows (read at chunks g and 4 + g) by (row >> 1) & 7,
// chosen against the ds_read_b128 lane groups {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and their upper-half twins
__device__ __forceinline__ int mg_key64(int row) { return (0x78 >> (2 * ((row >> 2) & 3))) & 3; }
__device__ __forceinline__ int mg_key128(int row) { return (0x64642020u >> (4 * ((row >> 1) & 7))) & 7; }

// The instruction aligns the products of one 32-block to the block's largest product and cuts off what lies more than 13
// binary places below its leading bit (measured with exact two-term sums: 256 + 2^-5 is exact, 256 + 2^-6 comes back as 256).
// e2m1 x e2m1 products span 8 binades and never reach that window; e4m3 x e2m1 products span 22. A product of an e4m3 value with
// exponent e (three mantissa bits) and an e2m1 value has its leading bit at most at 2^(e + 3) and its last bit at least at
// 2^(e - 4): activations whose exponents differ by at most 6 keep every product inside the window. So the e4m3 codes of a
// fragment go through the instruction in three exponent classes, the other bytes zeroed (code 0 = +0), each sum then exact
// and the three joined by the fp32 accumulator: exponent field 0 .. 7 (subnormals and 2^-6 .. 2^0: the subnormals share the
// last bit 2^-9 of field 1), 8 .. 14 (2^1 .. 2^7) and 15 (256 .. 448). Four codes of a register at once: a byte's mask from one
// bit b of it is ((b << k) - (b >> j)) | (b << k), 0x80 - 0x01 = 0x7f per set byte with no borrow between bytes, then bit 7.
__device__ __forceinline__ void mg_e4m3_classes(uint32_t x, int& lo, int& mid, int& hi) {
    const uint32_t b6 = x & 0x40404040u;                                    // exponent field >= 8
    const uint32_t m6 = ((b6 << 1) - (b6 >> 6)) | (b6 << 1);
    uint32_t q = x & (x >> 1);                                               // bit 3: field bits 0 & 1, bit 5: field bits 2 & 3
    q = q & (q >> 2) & 0x08080808u;                                          // bit 3: exponent field == 15
    const uint32_t m15 = ((q << 4) - (q >> 3)) | (q << 4);
    const uint32_t up = x & m6;
    hi = (int)(x & m15);
    mid = (int)(up ^ (uint32_t)hi);
    lo = (int)(x ^ up);
}

struct MxGemmArgs {
    const uint8_t* A; const uint8_t* As; const uint8_t* B; const uint8_t* Bs;
    int64_t M, N, K;
    const void* bias; void* C;
    int ntm;
};

template <int AFMT, int DT>
__global__ __launch_bounds__(MG_THREADS) void k_mx_gemm(MxGemmArgs a) {
    typedef MgGeo<AFMT> G;
    constexpr int AB = G::AB;
    extern __shared__ __attribute__((aligned(16))) char mg_smem[];
    LDS_AS char* lds = (LDS_AS char*)mg_smem;
    const uint32_t lbase = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(uintptr_t)lds);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wv >> 1, wn = wv & 1;
    const int tm = blockIdx.x % a.ntm, tn = blockIdx.x / a.ntm;     // m fastest: the blocks in flight share weight panels
    const int64_t m0 = (int64_t)tm * MG_T, n0 = (int64_t)tn * MG_T;
    const int nk = (int)(a.K / 128);
    const uint32_t arow = (uint32_t)(a.K * AB / 128), brow = (uint32_t)(a.K / 2), srow = (uint32_t)(a.K / 32);   // row bytes
    const int64_t mrows = a.M - m0 < MG_T ? a.M - m0 : MG_T, nrows = a.N - n0 < MG_T ? a.N - n0 : MG_T;
    const i32x4 ra = rsrc_words(a.A + m0 * arow, mrows * arow), rb = rsrc_words(a.B + n0 * brow, nrows * brow);
    // scales: waves 0, 1 move A's (rows 0-63, 64-127 of the tile), waves 2, 3 B's
    const i32x4 rs = wv < 2 ? rsrc_words(a.As + m0 * srow, mrows * srow) : rsrc_words(a.Bs + n0 * srow, nrows * srow);
    const uint32_t sdst = (uint32_t)((wv < 2 ? G::SA_OFF : G::SB_OFF) + (wv & 1) * 256);
    const uint32_t svoff = (uint32_t)((wv & 1) * 64 + lane) * srow;

    // DMA pieces. B (and an e2m1 A): piece p = 16 rows, lane = (row lane >> 2, slot lane & 3), this wave moves p = wv, wv + 4;
    // an e4m3 A: piece p = 8 rows, lane = (row lane >> 3, slot lane & 7), p = wv + 4 i, i = 0 .. 3. The row term stays in the
    // vector offset (the part the descriptor's bound is checked against).
    constexpr int NPA = AB == 64 ? 2 : 4;
    uint32_t vb[2], va[NPA];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int row = 16 * (wv + 4 * i) + (lane >> 2);
        vb[i] = (uint32_t)row * brow + (uint32_t)(((lane & 3) ^ mg_key64(row)) << 4);
    }
#pragma unroll
    for (int i = 0; i < NPA; ++i) {
        if constexpr (AB == 64) {
            const int row = 16 * (wv + 4 * i) + (lane >> 2);
            va[i] = (uint32_t)row * arow + (uint32_t)(((lane & 3) ^ mg_key64(row)) << 4);
        } else {
            const int row = 8 * (wv + 4 * i) + (lane >> 3);
            va[i] = (uint32_t)row * arow + (uint32_t)(((lane & 7) ^ mg_key128(row)) << 4);
        }
    }
    auto dma_sub = [&](uint32_t sub, int ks) {                  // sub: LDS address of the sub-step's image
        const uint32_t pdst = sub + (uint32_t)wv * 1024u;
#pragma unroll
        for (int i = 0; i < NPA; ++i) dma_imm_at<0>(ra, va[i], (uint32_t)ks * (uint32_t)AB, pdst + G::A_OFF + (uint32_t)i * 4096u);
#pragma unroll
        for (int i = 0; i < 2; ++i) dma_imm_at<0>(rb, vb[i], (uint32_t)ks * 64u, pdst + G::B_OFF + (uint32_t)i * 4096u);
        dma_imm_at<0, 4>(rs, svoff, (uint32_t)ks * 4u, sub + sdst);
    };

    // fragment reads: row 16 t + (lane & 15) of the wave's 64; chunk (lane >> 4) of a 64-byte row, chunks (lane >> 4) and
    // 4 + (lane >> 4) of a 128-byte row (the operand maps above)
    const int fr = lane & 15, fq = lane >> 4;
    int offB[4], offA0[4], offA1[4], offSA[4], offSB[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int rowb = wn * 64 + 16 * t + fr, rowa = wm * 64 + 16 * t + fr;
        offB[t] = G::B_OFF + rowb * 64 + ((fq ^ mg_key64(rowb)) << 4);
        if constexpr (AB == 64) {
            offA0[t] = G::A_OFF + rowa * 64 + ((fq ^ mg_key64(rowa)) << 4);
            offA1[t] = 0;
        } else {
            offA0[t] = G::A_OFF + rowa * 128 + ((fq ^ mg_key128(rowa)) << 4);
            offA1[t] = G::A_OFF + rowa * 128 + (((4 + fq) ^ mg_key128(rowa)) << 4);
        }
        offSA[t] = G::SA_OFF + rowa * 4 + fq;
        offSB[t] = G::SB_OFF + rowb * 4 + fq;
    }

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    auto mma_sub = [&](int sub) {                                // sub: byte offset of the sub-step's image in `lds`
        i32x8 fa[4], fb[4];
        int sa[4], sb[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const i32x4 b = *(LDS_AS const i32x4*)(lds + sub + offB[t]);
            fb[t] = i32x8{b[0], b[1], b[2], b[3], 0, 0, 0, 0};
            const i32x4 lo = *(LDS_AS const i32x4*)(lds + sub + offA0[t]);
            if constexpr (AB == 64) fa[t] = i32x8{lo[0], lo[1], lo[2], lo[3], 0, 0, 0, 0};
            else {
                const i32x4 hi = *(LDS_AS const i32x4*)(lds + sub + offA1[t]);
                fa[t] = i32x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
            }
            sa[t] = (int)*(LDS_AS const uint8_t*)(lds + sub + offSA[t]);
            sb[t] = (int)*(LDS_AS const uint8_t*)(lds + sub + offSB[t]);
        }
        if constexpr (AFMT == MX_E2M1) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[i][j] = mfma_scale_16x16x128<MFMA_FMT_E2M1, MFMA_FMT_E2M1>(fa[i], fb[j], acc[i][j], sa[i], sb[j]);
        } else {
            // e4m3: one instruction per exponent class of the activation codes (mg_e4m3_classes: why, and which)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                i32x8 fc[3];
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    int lo, mid, hi;
                    mg_e4m3_classes((uint32_t)fa[i][r], lo, mid, hi);
                    fc[0][r] = lo, fc[1][r] = mid, fc[2][r] = hi;
                }
#pragma unroll
                for (int c = 0; c < 3; ++c)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        acc[i][j] = mfma_scale_16x16x128<MFMA_FMT_E4M3, MFMA_FMT_E2M1>(fc[c], fb[j], acc[i][j], sa[i], sb[j]);
            }
        }
    };

    const int nst = (nk + G::KSUB - 1) / G::KSUB;
    auto stage_dma = [&](int s) {
#pragma unroll
        for (int h = 0; h < G::KSUB; ++h)
            if (s * G::KSUB + h < nk) dma_sub(lbase + (uint32_t)((s & 1) * G::STAGE + h * G::SUB), s * G::KSUB + h);
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
        for (int h = 0; h < G::KSUB; ++h)
            if (s * G::KSUB + h < nk) mma_sub((s & 1) * G::STAGE + h * G::SUB);
    }

    // epilogue: one rounding to the output dtype, then the bias in that dtype (llmc_fp8_block_gemm's order)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t col = n0 + wn * 64 + 16 * j + fr;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t row = m0 + wm * 64 + 16 * i + 4 * fq + r;
                if (row < a.M && col < a.N) {
                    float y = rndc<DT>(acc[i][j][r]);
                    if (a.bias) y = rndc<DT>(y + load_as_f32(a.bias, col, DT));
                    store_from_f32(a.C, row * a.N + col, DT, y);
                }
            }
        }
}

template <int AFMT> int mx_gemm_launch(const MxGemmArgs& a, int out_dt, hipStream_t st) {
    const void* fn = out_dt == LLMC_F16 ? (const void*)k_mx_gemm<AFMT, LLMC_F16>
                   : out_dt == LLMC_BF16 ? (const void*)k_mx_gemm<AFMT, LLMC_BF16> : (const void*)k_mx_gemm<AFMT, LLMC_F32>;
    if (int rc = ensure_dynamic_lds(fn, MgGeo<AFMT>::LDS)) return rc;
    MxGemmArgs b = a;
    void* kargs[] = {(void*)&b};
    const int64_t ntn = ceil_div64(a.N, MG_T);
    LLMC_HIP_CHECK(hipLaunchKernel(fn, dim3((unsigned)(a.ntm * ntn)), dim3(MG_THREADS), kargs, (size_t)MgGeo<AFMT>::LDS, st));
    return LLMC_OK;
}

}  // namespace
}  // namespace llmc

using namespace llmc;

extern "C" int llmc_mx_act_quant(const void* X, int dt, int64_t M, int64_t K, int fmt, void* out_codes, void* out_scales,
                                 llmc_stream_t stream) {
    LLMC_REQUIRE(X && out_codes && out_scales && M > 0 && K > 0, "mx_act_quant: null/empty argument");
    LLMC_REQUIRE(dt == LLMC_F16 || dt == LLMC_BF16, "mx_act_quant: X must be bf16 or fp16");
    LLMC_REQUIRE(((uintptr_t)X & 15) == 0 && ((uintptr_t)out_codes & 7) == 0, "mx_act_quant: X needs 16-byte, the codes 8-byte alignment");
    if (fmt != MX_E2M1 && fmt != MX_E4M3) {
        set_last_error_msg("mx_act_quant: format must be 2 (e2m1) or 4 (e4m3)");
        return LLMC_ENOTSUP;
    }
    if (K % 32) {
        set_last_error_msg("mx_act_quant: K must be a multiple of the 32-element MX block");
        return LLMC_ENOTSUP;
    }
    hipStream_t st = (hipStream_t)stream;
    const int64_t nv = M * K / 8;
    const dim3 grid(capped_grid(nv, AQ_B, 16384));
#define MX_AQ(T, F) hipLaunchKernelGGL((k_mx_act_quant<T, F>), grid, dim3(AQ_B), 0, st, (const T*)X, nv, (uint8_t*)out_codes, (uint8_t*)out_scales)
    if (dt == LLMC_BF16) { if (fmt == MX_E2M1) MX_AQ(bf16_t, MX_E2M1); else MX_AQ(bf16_t, MX_E4M3); }
    else { if (fmt == MX_E2M1) MX_AQ(f16_t, MX_E2M1); else MX_AQ(f16_t, MX_E4M3); }
#undef MX_AQ
    LLMC_LAUNCH_CHECK();
    return LLMC_OK;
}

extern "C" int llmc_mx_gemm(const void* A, int a_fmt, const void* a_s, const void* B4, const void* b_s, int64_t M, int64_t N,
                            int64_t K, int out_dt, const void* bias, void* C, llmc_stream_t stream) {
    LLMC_REQUIRE(A && a_s && B4 && b_s && C && M > 0 && N > 0 && K > 0, "mx_gemm: null/empty argument");
    LLMC_REQUIRE(out_dt == LLMC_F16 || out_dt == LLMC_BF16 || out_dt == LLMC_F32, "mx_gemm: bad output dtype");
    LLMC_REQUIRE((((uintptr_t)A | (uintptr_t)B4) & 15) == 0 && (((uintptr_t)a_s | (uintptr_t)b_s) & 3) == 0 &&
                 ((uintptr_t)C & (out_dt == LLMC_F32 ? 3 : 1)) == 0 && ((uintptr_t)bias & (out_dt == LLMC_F32 ? 3 : 1)) == 0,
                 "mx_gemm: codes need 16-byte, scales 4-byte, C and bias element alignment");
    if (a_fmt != MX_E2M1 && a_fmt != MX_E4M3) {
        set_last_error_msg("mx_gemm: activation format must be 2 (e2m1, packed) or 4 (e4m3)");
        return LLMC_ENOTSUP;
    }
    if (K % 128) {
        set_last_error_msg("mx_gemm: K must be a multiple of 128 (the depth of one block-scaled matrix instruction)");
        return LLMC_ENOTSUP;
    }
    if (K >= (1ll << 24) || ceil_div64(M, MG_T) * ceil_div64(N, MG_T) >= (1ll << 31)) {
        set_last_error_msg("mx_gemm: K must be below 2^24 and the tile count below 2^31");
        return LLMC_ENOTSUP;
    }
    MxGemmArgs a;
    a.A = (const uint8_t*)A; a.As = (const uint8_t*)a_s; a.B = (const uint8_t*)B4; a.Bs = (const uint8_t*)b_s;
    a.M = M; a.N = N; a.K = K; a.bias = bias; a.C = C;
    a.ntm = (int)ceil_div64(M, MG_T);
    hipStream_t st = (hipStream_t)stream;
    return a_fmt == MX_E2M1 ? mx_gemm_launch<MX_E2M1>(a, out_dt, st) : mx_gemm_launch<MX_E4M3>(a, out_dt, st);
}
