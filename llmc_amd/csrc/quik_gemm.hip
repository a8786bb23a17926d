// quik_gemm.hip — the QUIK real-quant Linear (deploy('quik_quant'), QuikRealQuantLinear): the K input channels of a Linear are
// split once, at calibration, into n_int channels that run as int8 codes and F outlier channels that stay in 16 bit. Stored
// form: W8 [N, Ki] int8 (the int channels in the order of int_ids, Ki = n_int rounded up to 64, padding code 0) with one fp32
// scale per output channel, and Wfp [N, Fp] bf16 / f16 (the outlier channels in the order of fp_ids, Fp = F rounded up to 32,
// padding +0). An extension: the reference has the fake-quant method only.
//   llmc_quik_act_split   x [M, K] -> a8 [M, Ki] int8 codes, a_s [M] fp32, a_fp [M, Fp] in x's dtype, one pass over x
//   llmc_quik_gemm        C[m, n] = rnd_out(fl(fl(float(sum_k a8[m, k] w8[n, k]) * a_s[m]) * w_s[n]) + sum_j a_fp[m, j] w_fp[n, j]),
//                         then the bias in the output dtype
// The int sum is exact int32 (K <= 65536: 128 * 128 * K = 2^30 stays below 2^31, as in i8_linear.hip); float() is v_cvt_f32_i32;
// the 16-bit products are accumulated in fp32 by the matrix instruction, on top of the scaled integer part.
//
// k_quik_split: a team of 64 lanes (four rows per workgroup) or the workgroup owns a row. Each 16-byte vector of x is read once
// together with its 8 entries of col_map and scattered to the row's permuted copy in LDS (2-byte ds_write: a random order costs
// bank conflicts, not HBM transactions); the min / max of the elements that land in an int slot are reduced on the way. The
// scale and the codes are then the integer quantizer's own group step (quant_math.h) on 16 consecutive slots per lane: bit for
// bit IntegerQuantizer(8, True, 'per_token').real_quant_weight_dynamic on the gathered copy. Padding slots are zeroed in LDS, so
// they come out as code 0 / +0 by the same path. Every store is a 16-byte vector (the scale: one dword).
//
// k_quik_tile (rung tile128): 128 x 128 outputs, 4 waves as 2 x 2, 2 x 2 accumulators of 32 x 32 per wave. One K loop over
// blocks of 128 bytes per row, first the ceil(Ki / 128) blocks of the codes (v_mfma_i32_32x32x32_i8), then the ceil(2 Fp / 128)
// blocks of the outliers (v_mfma_f32_32x32x16_bf16 / _f16: 64 elements per block). Both kinds of block have the same shape in
// bytes, 128 rows x 128 B per operand and 16 B per lane and instruction, so they go through the same two-stage LDS ring by the
// same LDS-DMA pieces and the same fragment reads; only the descriptors and the instruction differ. Between the phases the 64
// accumulator registers of a lane are retyped in place: v_cvt_f32_i32, times a_s[row], times w_s[column], and the result is the
// C operand of the first 16-bit MFMA. No second accumulator set, no second pass over C.
// LDS row pitch QK_LD = 144 for both phases: a fragment read is one ds_read_b128 per lane, 16 lanes (16 consecutive rows, one
// 16-byte chunk) per pass over the 64 banks; they cover the banks once iff r -> (r * LD / 16) mod 16 is a bijection, iff
// LD / 16 is odd (scaled8_gemm.h has the argument in full). The outlier phase reads rows of 64 16-bit elements = 128 B, the
// same 8 chunks as a row of codes, so the smallest odd multiple above the data, 9 chunks, serves it too; a pitch of its own
// (say 64 + 16 B for blocks of 32 elements) would halve the block and double the barriers for F = 256. An LDS-DMA instruction
// writes 64 consecutive 16-byte slots; slot s of a panel is row s / 9, chunk s % 9, and the lanes on chunk 8 (the padding) and
// on chunks past the end of a row are sent out of range (offset bit 31), which a buffer load answers with zeros: a zero code
// adds exactly 0 and a +0 outlier adds +0 to a sum, which is what lets Ki and Fp be ragged against the block. Rows past M / N
// are out of the descriptor's range as well; their outputs are never stored.
//
// k_quik_decode (rung decode, M <= 64): scaled8_gemm.h's decode structure, 16 output columns per workgroup and all rows, the
// weight streamed once from global memory to registers. The K blocks of both kinds are one list, codes first, dealt round the
// 8 waves; a wave runs v_mfma_i32_16x16x64_i8 on a block of codes into its int32 tile and v_mfma_f32_16x16x32_bf16 / _f16 on a
// block of outliers into its fp32 tile (lane (r, g) holds bytes 32 g .. + 31 of the block of row r for both operands, two
// instructions of 16 B). The waves' int32 tiles meet in LDS and are added (exact, any order), the sum is scaled; then the fp32
// tiles meet in the same LDS and are added onto it in wave order 0 .. 7. No atomics: the same bits on every run.
#include "scaled8_gemm.h"
#include "quant_group.h"

namespace llmc {

// ---------------------------------------------------------------------------------------------------------------
// the activation split
// ---------------------------------------------------------------------------------------------------------------
static constexpr int QS_B = 256;                   // threads per workgroup
static constexpr int QS_RED = 64;                  // block_minmax's words in front of the rows
static constexpr int QS_LDS_MAX = 160 * 1024;      // gfx950: the LDS of a CU

template <typename T>
__global__ __launch_bounds__(QS_B) void k_quik_split(const T* __restrict__ X, int64_t M, int K, const int32_t* __restrict__ col_map,
                                                     int Ki, int Fp, int ts, int8_t* __restrict__ codes,
                                                     float* __restrict__ scales, T* __restrict__ afp) {
    extern __shared__ __attribute__((aligned(16))) char qs_smem[];
    constexpr int DT = dt_of<T>::value;
    float* red = (float*)qs_smem;
    const int W = Ki + Fp;                                   // slots of a row: the int slots, then the fp slots
    const int team = threadIdx.x / ts, tl = threadIdx.x % ts;
    const int64_t row = (int64_t)blockIdx.x * (QS_B / ts) + team;
    const bool valid = row < M;                              // a team past the last row computes on row M - 1 and stores nothing
    const T* xp = X + (valid ? row : M - 1) * K;
    T* lp = (T*)(qs_smem + QS_RED) + (size_t)team * W;
    // the padding: at most the last 63 int slots and the last 31 fp slots, zeroed before the scatter overwrites the used ones
    for (int j = Ki - 63 + tl; j < Ki; j += ts) lp[j] = zero_of<T>();
    for (int j = W - 31 + tl; j < W; j += ts)
        if (j >= Ki) lp[j] = zero_of<T>();
    __syncthreads();
    float mn = INFINITY, mx = -INFINITY;
    for (int c = tl * 8; c < K; c += ts * 8) {
        const Vec<T, 8> v = load_vec<T, 8>(xp + c);
        const Vec<int32_t, 4> d0 = load_vec<int32_t, 4>(col_map + c), d1 = load_vec<int32_t, 4>(col_map + c + 4);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int d = i < 4 ? d0.v[i] : d1.v[i - 4];
            if ((unsigned)d >= (unsigned)W) continue;         // not a slot: the host's col_map never holds one
            lp[d] = v.v[i];
            if (d < Ki) {
                const float f = to_f32<T>(v.v[i]);
                mn = fminf(mn, f);
                mx = fmaxf(mx, f);
            }
        }
    }
    if (ts == 64) {
        mn = wave_min(mn, 64);
        mx = wave_max(mx, 64);
        __syncthreads();
    } else {
        block_minmax<QS_B, true>(red, mn, mx);                // its barriers publish the rows too
    }
    if (!valid) return;
    const QParams qp = qparams_from_minmax(mn, mx, DT, 1, 1, -128.0f, 127.0f);
    const Divisor dv = make_divisor(qp.s, fmaxf(fabsf(mn), fabsf(mx)));
    for (int j = tl * 16; j < Ki; j += ts * 16) {
        Vec<int8_t, 16> o;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const Vec<T, 8> v = load_vec<T, 8>(lp + j + 8 * h);
#pragma unroll
            for (int i = 0; i < 8; ++i) o.v[8 * h + i] = (int8_t)quant_code(to_f32<T>(v.v[i]), dv, 0.0f, DT, DT, -128.0f, 127.0f);
        }
        store_vec_wide<int8_t, 16>(codes + row * Ki + j, o);
    }
    for (int j = tl * 8; j < Fp; j += ts * 8) store_vec<T, 8>(afp + row * Fp + j, load_vec<T, 8>(lp + Ki + j));
    if (tl == 0) scales[row] = qp.s;
}

static bool quik_split_fits(int dt, int64_t K, int64_t Ki, int64_t Fp) {
    if (!(dt == LLMC_F16 || dt == LLMC_BF16) || K <= 0 || K % 8 || Ki <= 0 || Ki % 64 || Fp < 0 || Fp % 32) return false;
    const int64_t rpb = K / 8 <= 256 ? 4 : 1;
    return QS_RED + rpb * (Ki + Fp) * 2 <= QS_LDS_MAX;
}

// ---------------------------------------------------------------------------------------------------------------
// the GEMM
// ---------------------------------------------------------------------------------------------------------------
struct QuikArgs : Scaled8Args {      // A / B: the codes a8 [M, K] / w8 [N, K] (K = Ki), As [M], Bs [N]
    const uint8_t* Afp;              // the outliers [M, Fp] and
    const uint8_t* Bfp;              // their weight columns [N, Fp], 16 bit
    int64_t Fp;
    int out_dt;
};

// the 16 x 16 form of the 16-bit MFMA: lane l holds 8 consecutive k of row / column l & 15, k group l >> 4; register q of lane l
// is row 4 (l >> 4) + q, column l & 15, as in the integer form of the same tile
template <int DT> __device__ __forceinline__ f32x4 mfma16_f32_16x16x32(i32x4 a, i32x4 b, f32x4 c) {
    if constexpr (DT == LLMC_BF16)
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

// C[row, col] from the finished fp32 sum: one rounding, then the bias in the output dtype
__device__ __forceinline__ void quik_store(const QuikArgs& a, int64_t row, int64_t col, float acc) {
    float y = rnd(acc, a.out_dt);
    if (a.bias) y = rnd(y + load_as_f32(a.bias, col, a.out_dt), a.out_dt);
    store_from_f32(a.C, row * a.N + col, a.out_dt, y);
}

static constexpr int QK_LD = S8_LD;                      // LDS row pitch of both phases (the file's head says why)
static constexpr int QK_CH = QK_LD / 16;                 // 16-byte slots per row: 8 of data, 1 of padding
static constexpr int QK_PANEL = 128 * QK_LD;             // one operand's rows of a block: 18 DMA instructions of 1024 B
static constexpr int QK_PANEL_DMA = QK_PANEL / 1024;
static constexpr int QK_STAGE = 2 * QK_PANEL;
static constexpr int QK_TILE_LDS = 2 * QK_STAGE;         // 73728 B: two workgroups per CU
static constexpr int QK_DMA_PER_WAVE = 2 * QK_PANEL_DMA / 4;
static constexpr uint32_t QK_OOB = 0x80000000u;          // an offset no descriptor of a tile reaches (their ranges are <= 8 MiB)
static_assert(QK_PANEL % 1024 == 0 && (2 * QK_PANEL_DMA) % 4 == 0, "a panel is whole DMA instructions, dealt evenly to 4 waves");

template <int FDT>
__global__ __launch_bounds__(256) void k_quik_tile(QuikArgs a) {
    extern __shared__ __attribute__((aligned(16))) char qk_smem[];
    LDS_AS char* lds = (LDS_AS char*)qk_smem;
    const uint32_t lds0 = (uint32_t)(uintptr_t)lds;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wv >> 1, wn = wv & 1;

    int tm, tn;
    s8_tile_of_workgroup(a, tm, tn);
    const int64_t m0 = (int64_t)tm * 128, n0 = (int64_t)tn * 128;
    const int64_t rows_a = a.M - m0 < 128 ? a.M - m0 : 128, rows_b = a.N - n0 < 128 ? a.N - n0 : 128;
    const uint32_t rb_i = (uint32_t)a.K, rb_f = (uint32_t)(2 * a.Fp);        // bytes of a row in each phase
    const int nkb_i = (int)((rb_i + S8_KB - 1) / S8_KB), nkb = nkb_i + (int)((rb_f + S8_KB - 1) / S8_KB);

    // the descriptors end with the tile's last row: a row past M / N arrives as zeros
    const buf_rsrc ra_i = uniform_rsrc(a.A + m0 * rb_i, (uint32_t)(rows_a * rb_i));
    const buf_rsrc rw_i = uniform_rsrc(a.B + n0 * rb_i, (uint32_t)(rows_b * rb_i));
    const buf_rsrc ra_f = uniform_rsrc(a.Afp + m0 * rb_f, (uint32_t)(rows_a * rb_f));
    const buf_rsrc rw_f = uniform_rsrc(a.Bfp + n0 * rb_f, (uint32_t)(rows_b * rb_f));

    // DMA instruction i = wv + 4 j of a stage (0 .. 17: the A panel, 18 .. 35: the B panel) fills slots 64 (i % 18) .. + 63
    int srow[QK_DMA_PER_WAVE], sch[QK_DMA_PER_WAVE];
#pragma unroll
    for (int j = 0; j < QK_DMA_PER_WAVE; ++j) {
        const int s = ((wv + 4 * j) % QK_PANEL_DMA) * 64 + lane;
        srow[j] = s / QK_CH;
        sch[j] = (s % QK_CH) * 16;
    }
    auto issue = [&](int kb) {
        const bool fp = kb >= nkb_i;
        const uint32_t rb = fp ? rb_f : rb_i, k0 = (uint32_t)(fp ? kb - nkb_i : kb) * S8_KB;
        const uint32_t dst = lds0 + (uint32_t)(kb & 1) * QK_STAGE;
#pragma unroll
        for (int j = 0; j < QK_DMA_PER_WAVE; ++j) {
            const int i = wv + 4 * j;
            const bool in = sch[j] < S8_KB && k0 + (uint32_t)sch[j] < rb;
            const uint32_t voff = in ? (uint32_t)srow[j] * rb + (uint32_t)sch[j] : QK_OOB;
            const uint32_t to = dst + (uint32_t)i * 1024u;
            if (i < QK_PANEL_DMA) {
                if (fp) dma16_to(ra_f, voff, k0, to);
                else dma16_to(ra_i, voff, k0, to);
            } else {
                if (fp) dma16_to(rw_f, voff, k0, to);
                else dma16_to(rw_i, voff, k0, to);
            }
        }
    };

    // one accumulator set: int32 bits during the codes' blocks, fp32 from the retyping on
    f32x16 acc[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) acc[m][n] = __builtin_bit_cast(f32x16, i32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0});

    // accumulator register r of lane l is row (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31 of its 32 x 32 tile
    auto retype = [&]() {
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            const int64_t col = n0 + wn * 64 + n * 32 + (lane & 31);
            const float sb = a.Bs[col < a.N ? col : a.N - 1];
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                const i32x16 iv = __builtin_bit_cast(i32x16, acc[m][n]);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int64_t row = m0 + wm * 64 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                    acc[m][n][r] = ((float)iv[r] * a.As[row < a.M ? row : a.M - 1]) * sb;
                }
            }
        }
    };

    // one step of the K loop on block kb; INT: a block of codes
    auto step = [&](int kb, auto is_int) {
        constexpr bool INT = decltype(is_int)::value;
        vm_wait<0>();                         // this wave's pieces of block kb have landed
        __syncthreads();                      // block kb is published; every wave is done with block kb - 1's stage
        if (kb + 1 < nkb) issue(kb + 1);      // lands under this block's MFMAs
        LDS_AS char* la = lds + (kb & 1) * QK_STAGE;
        LDS_AS char* lb = la + QK_PANEL;
#pragma unroll
        for (int kc = 0; kc < 4; ++kc) {
            const int off = (lane & 31) * QK_LD + kc * 32 + 16 * (lane >> 5);
            i32x4 fa[2], fb[2];
#pragma unroll
            for (int m = 0; m < 2; ++m) fa[m] = *(LDS_AS i32x4*)(la + (wm * 64 + m * 32) * QK_LD + off);
#pragma unroll
            for (int n = 0; n < 2; ++n) fb[n] = *(LDS_AS i32x4*)(lb + (wn * 64 + n * 32) * QK_LD + off);
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int n = 0; n < 2; ++n) {
                    if constexpr (INT)
                        acc[m][n] = __builtin_bit_cast(f32x16, mfma_i32_32x32x32_i8(fa[m], fb[n], __builtin_bit_cast(i32x16, acc[m][n])));
                    else
                        acc[m][n] = Mfma<FDT>::run(__builtin_bit_cast(s16x8, fa[m]), __builtin_bit_cast(s16x8, fb[n]), acc[m][n]);
                }
        }
    };
    issue(0);
    for (int kb = 0; kb < nkb_i; ++kb) step(kb, std::true_type{});
    retype();                                 // the first outlier block's DMA is in flight meanwhile
    for (int kb = nkb_i; kb < nkb; ++kb) step(kb, std::false_type{});

#pragma unroll
    for (int n = 0; n < 2; ++n) {
        const int64_t col = n0 + wn * 64 + n * 32 + (lane & 31);
        if (col >= a.N) continue;
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t row = m0 + wm * 64 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if (row < a.M) quik_store(a, row, col, acc[m][n][r]);
            }
    }
}

template <int MT> struct QuikDecodeOperands {
    i32x4 b[2], x[MT][2];
    uint32_t kv[2];           // b[e]'s mask, applied where b[e] is used
};

template <int FDT, int MT>
__global__ __launch_bounds__(64 * S8D_WAVES) void k_quik_decode(QuikArgs a) {
    constexpr int NE = (MT * 256 + 64 * S8D_WAVES - 1) / (64 * S8D_WAVES);      // outputs per thread
    __shared__ int red[S8D_WAVES * MT * 256];            // the waves' tiles: int32 first, then the bits of fp32
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, g = lane >> 4;
    const int64_t n0 = (int64_t)blockIdx.x * S8D_N;
    const int64_t rb_i = a.K, rb_f = 2 * a.Fp;
    const int nkb_i = (int)((rb_i + S8_KB - 1) / S8_KB), nkb = nkb_i + (int)((rb_f + S8_KB - 1) / S8_KB);

    const int64_t brow = n0 + r < a.N ? n0 + r : a.N - 1;
    int64_t arow[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) arow[mt] = 16 * mt + r < a.M ? 16 * mt + r : a.M - 1;
    // block kb of the list: a block of codes (kb < nkb_i) or of outliers; an index past the end is clamped (the load stays in
    // bounds, its products are not formed). A 16-byte chunk past the end of a row is loaded from the row's last chunk and the
    // weight's copy is zeroed where it is used.
    auto load = [&](QuikDecodeOperands<MT>& o, int kb) {
        kb = kb < nkb ? kb : nkb - 1;
        const bool fp = kb >= nkb_i;
        const uint8_t* A = fp ? a.Afp : a.A;
        const uint8_t* B = fp ? a.Bfp : a.B;
        const int64_t rb = fp ? rb_f : rb_i, k0 = (int64_t)(fp ? kb - nkb_i : kb) * S8_KB + 32 * g;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int64_t k = k0 + 16 * e;
            o.kv[e] = k < rb ? 0xffffffffu : 0u;
            const int64_t at = o.kv[e] ? k : rb - 16;
            o.b[e] = *reinterpret_cast<const i32x4*>(B + brow * rb + at);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) o.x[mt][e] = *reinterpret_cast<const i32x4*>(A + arow[mt] * rb + at);
        }
    };
    i32x4 acci[MT];
    f32x4 accf[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        acci[mt] = i32x4{0, 0, 0, 0};
        accf[mt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    }
    auto mac = [&](const QuikDecodeOperands<MT>& o, int kb) {
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const i32x4 b = s8_and(o.b[e], o.kv[e]);
            if (kb < nkb_i) {
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) acci[mt] = mfma_i32_16x16x64_i8(o.x[mt][e], b, acci[mt]);
            } else {
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) accf[mt] = mfma16_f32_16x16x32<FDT>(o.x[mt][e], b, accf[mt]);
            }
        }
    };
    QuikDecodeOperands<MT> s0, s1;
    load(s0, wv);
    load(s1, wv + S8D_WAVES);
    for (int kb = wv; kb < nkb; kb += 2 * S8D_WAVES) {
        mac(s0, kb);
        load(s0, kb + 2 * S8D_WAVES);
        if (kb + S8D_WAVES < nkb) mac(s1, kb + S8D_WAVES);
        load(s1, kb + 3 * S8D_WAVES);
    }

    // the int32 tiles meet in LDS. Accumulator register q of lane l is row 4 (l >> 4) + q, column l & 15.
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int q = 0; q < 4; ++q) red[(wv * MT + mt) * 256 + q * 64 + lane] = acci[mt][q];
    __syncthreads();
    float y[NE];
#pragma unroll
    for (int j = 0; j < NE; ++j) {
        const int e = tid + 64 * S8D_WAVES * j;
        y[j] = 0.0f;
        if (e >= MT * 256) continue;
        int s = 0;
#pragma unroll
        for (int w = 0; w < S8D_WAVES; ++w) s += red[w * MT * 256 + e];
        const int ln = e & 63;
        const int64_t row = 16 * (e >> 8) + 4 * (ln >> 4) + ((e >> 6) & 3), col = n0 + (ln & 15);
        y[j] = ((float)s * a.As[row < a.M ? row : a.M - 1]) * a.Bs[col < a.N ? col : a.N - 1];
    }
    if (nkb > nkb_i) {                        // the fp32 tiles, through the same LDS, added in wave order
        __syncthreads();
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int q = 0; q < 4; ++q) red[(wv * MT + mt) * 256 + q * 64 + lane] = __float_as_int(accf[mt][q]);
        __syncthreads();
#pragma unroll
        for (int j = 0; j < NE; ++j) {
            const int e = tid + 64 * S8D_WAVES * j;
            if (e >= MT * 256) continue;
#pragma unroll
            for (int w = 0; w < S8D_WAVES; ++w) y[j] += __int_as_float(red[w * MT * 256 + e]);
        }
    }
#pragma unroll
    for (int j = 0; j < NE; ++j) {
        const int e = tid + 64 * S8D_WAVES * j;
        if (e >= MT * 256) continue;
        const int ln = e & 63;
        const int64_t row = 16 * (e >> 8) + 4 * (ln >> 4) + ((e >> 6) & 3), col = n0 + (ln & 15);
        if (row < a.M && col < a.N) quik_store(a, row, col, y[j]);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// which rung takes which shape: the first row whose bounds hold. REASONED, not yet measured on this kernel: the rows are
// i8_linear.hip's measured ones (both rungs here are that file's rungs plus the outlier blocks, which add the same share of work
// to each): up to 64 tokens the decode rung, except 33 .. 64 tokens on N >= 14336, where its four row tiles are instruction-bound
// and the tile rung passed it. tools/bench_quik.py (profiles/quik_gemm.txt) is the measurement to set them from.
// ---------------------------------------------------------------------------------------------------------------
enum { QK_DECODE = 0, QK_TILE128 = 1, QK_NRUNGS = 2 };
struct QuikRung {
    int64_t min_m, max_m;   // min_m <= M <= max_m
    int64_t min_n;          // N >= min_n
    int rung;
};
static const QuikRung QK_LADDER[] = {
    {33, S8_DECODE_MAX_M, 14336, QK_TILE128},
    {1, S8_DECODE_MAX_M, 1, QK_DECODE},
    {1, INT64_MAX, 1, QK_TILE128},
};
static int quik_pick_rung(int64_t M, int64_t N) {
    for (const QuikRung& r : QK_LADDER)
        if (M >= r.min_m && M <= r.max_m && N >= r.min_n) return r.rung;
    return QK_TILE128;
}

template <int FDT>
static int quik_launch(QuikArgs& a, int rung, hipStream_t st) {
    if (rung == QK_DECODE) {
        s8_launch_decode(a, dim3((unsigned)ceil_div64(a.N, S8D_N)), st, k_quik_decode<FDT, 1>, k_quik_decode<FDT, 2>, k_quik_decode<FDT, 4>);
    } else {
        if (int rc = ensure_dynamic_lds((const void*)k_quik_tile<FDT>, QK_TILE_LDS)) return rc;
        a.ntm = (int)ceil_div64(a.M, 128);
        a.ntn = (int)ceil_div64(a.N, 128);
        hipLaunchKernelGGL(k_quik_tile<FDT>, dim3((unsigned)(a.ntm * a.ntn)), dim3(256), QK_TILE_LDS, st, a);
    }
    LLMC_LAUNCH_CHECK();
    return LLMC_OK;
}

}  // namespace llmc

using namespace llmc;

extern "C" int llmc_quik_act_split_fits(int dt, int64_t K, int64_t Ki, int64_t Fp) { return quik_split_fits(dt, K, Ki, Fp) ? 1 : 0; }

extern "C" int llmc_quik_act_split(const void* X, int dt, int64_t M, int64_t K, const int32_t* col_map, int64_t Ki, int64_t Fp,
                                   void* codes, float* scales, void* a_fp, llmc_stream_t stream) {
    LLMC_REQUIRE(X && col_map && codes && scales && M > 0 && K > 0, "quik_act_split: null/empty argument");
    LLMC_REQUIRE(Ki >= 64 && Fp >= 0 && K <= Ki + Fp && K >= Ki + Fp - 94 && (a_fp || Fp == 0),
                 "quik_act_split: Ki + Fp is K plus the padding of both parts (at most 63 + 31 slots); a_fp may be null only when Fp is 0");
    LLMC_REQUIRE((((uintptr_t)X | (uintptr_t)col_map | (uintptr_t)codes | (uintptr_t)a_fp) & 15) == 0 && ((uintptr_t)scales & 3) == 0,
                 "quik_act_split: x, col_map, codes and a_fp need 16-byte, scales 4-byte alignment");
    LLMC_REQUIRE(M < (1ll << 31), "quik_act_split: too many rows");
    if (!quik_split_fits(dt, K, Ki, Fp)) {
        set_last_error_msg("quik_act_split: takes bf16 / f16 rows with K % 8 == 0 whose permuted copy fits the LDS of a CU");
        return LLMC_ENOTSUP;
    }
    const int ts = K / 8 <= 256 ? 64 : QS_B;                  // about four vectors per lane up to K = 2048, then the workgroup
    const int rpb = QS_B / ts;
    const size_t lds = (size_t)(QS_RED + rpb * (Ki + Fp) * 2);
    hipStream_t st = (hipStream_t)stream;
    if (dt == LLMC_BF16) {
        if (int rc = ensure_dynamic_lds((const void*)k_quik_split<bf16_t>, QS_LDS_MAX)) return rc;
        hipLaunchKernelGGL(k_quik_split<bf16_t>, dim3((unsigned)ceil_div64(M, rpb)), dim3(QS_B), lds, st, (const bf16_t*)X, M, (int)K,
                           col_map, (int)Ki, (int)Fp, ts, (int8_t*)codes, scales, (bf16_t*)a_fp);
    } else {
        if (int rc = ensure_dynamic_lds((const void*)k_quik_split<f16_t>, QS_LDS_MAX)) return rc;
        hipLaunchKernelGGL(k_quik_split<f16_t>, dim3((unsigned)ceil_div64(M, rpb)), dim3(QS_B), lds, st, (const f16_t*)X, M, (int)K,
                           col_map, (int)Ki, (int)Fp, ts, (int8_t*)codes, scales, (f16_t*)a_fp);
    }
    LLMC_LAUNCH_CHECK();
    return LLMC_OK;
}

// rung: -1 = the ladder chooses; 0 .. QK_NRUNGS - 1 = that rung whatever the shape (the measuring tool and the tests)
extern "C" int llmc_quik_gemm_on_rung(const void* A8, const float* a_s, const void* A_fp, const void* W8, const float* w_s,
                                      const void* W_fp, int64_t M, int64_t N, int64_t Ki, int64_t Fp, int fp_dt, int out_dt,
                                      const void* bias, void* C, int rung_arg, llmc_stream_t stream) {
    QuikArgs a;
    if (const int rc = s8_check_operands("quik_gemm", A8, a_s, W8, w_s, C, M, N, Ki, out_dt)) return rc;
    LLMC_REQUIRE(fp_dt == LLMC_F16 || fp_dt == LLMC_BF16, "quik_gemm: the outlier columns are f16 or bf16");
    LLMC_REQUIRE(Fp >= 0 && (Fp == 0 || (A_fp && W_fp)), "quik_gemm: Fp > 0 needs a_fp and w_fp");
    LLMC_REQUIRE(rung_arg >= -1 && rung_arg < QK_NRUNGS && (rung_arg != QK_DECODE || M <= S8_DECODE_MAX_M),
                 "quik_gemm: no such rung (the decode rung takes M <= 64)");
    LLMC_REQUIRE((((uintptr_t)A8 | (uintptr_t)W8 | (uintptr_t)A_fp | (uintptr_t)W_fp) & 15) == 0 && (((uintptr_t)a_s | (uintptr_t)w_s) & 3) == 0 &&
                 ((uintptr_t)C & (out_dt == LLMC_F32 ? 3 : 1)) == 0 && ((uintptr_t)bias & (out_dt == LLMC_F32 ? 3 : 1)) == 0,
                 "quik_gemm: codes and outlier columns need 16-byte, scales 4-byte, C and bias element alignment");
    if (Ki % 64 || Fp % 32) {
        set_last_error_msg("quik_gemm: Ki must be a multiple of 64 and Fp of 32 (the stored form pads to them)");
        return LLMC_ENOTSUP;
    }
    if (Ki > 65536 || Fp > 32768) {
        set_last_error_msg("quik_gemm: Ki must be at most 65536 (128 * 128 * Ki has to stay below 2^31 in the int32 accumulator) and Fp at most 32768");
        return LLMC_ENOTSUP;
    }
    if (N >= (1ll << 31) || ceil_div64(M, 128) * ceil_div64(N, 128) >= (1ll << 31)) {
        set_last_error_msg("quik_gemm: N and the tile count must be below 2^31");
        return LLMC_ENOTSUP;
    }
    s8_fill_args(a, A8, a_s, M, W8, w_s, N, M, N, Ki, bias, C);
    a.Afp = (const uint8_t*)A_fp;
    a.Bfp = (const uint8_t*)W_fp;
    a.Fp = Fp;
    a.out_dt = out_dt;
    const int rung = rung_arg >= 0 ? rung_arg : quik_pick_rung(M, N);
    hipStream_t st = (hipStream_t)stream;
    return fp_dt == LLMC_BF16 ? quik_launch<LLMC_BF16>(a, rung, st) : quik_launch<LLMC_F16>(a, rung, st);
}

extern "C" int llmc_quik_gemm(const void* A8, const float* a_s, const void* A_fp, const void* W8, const float* w_s, const void* W_fp,
                              int64_t M, int64_t N, int64_t Ki, int64_t Fp, int fp_dt, int out_dt, const void* bias, void* C,
                              llmc_stream_t stream) {
    return llmc_quik_gemm_on_rung(A8, a_s, A_fp, W8, w_s, W_fp, M, N, Ki, Fp, fp_dt, out_dt, bias, C, -1, stream);
}

// the rung the ladder gives a shape (0 decode, 1 tile128): a pure host call, for tools and tests
extern "C" int llmc_quik_gemm_rung(int64_t M, int64_t N) { return quik_pick_rung(M, N); }
