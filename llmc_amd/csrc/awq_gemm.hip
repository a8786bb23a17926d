// awq_gemm.hip — the W4A16 Linear on AutoAWQ's GEMM layout (the stored form deploy('autoawq_quant') writes; an extension: the
// reference's AutoawqRealQuantLinear raises in forward):
//   qweight int32 [K, R/8], qzeros int32 [K/g, R/8], scales f16 [K/g, R]; nibble i of a word holds column 8 c + ORDER[i],
//   ORDER = 0,2,4,6,1,3,5,7, so column 8 c + j sits in nibble INV[j], INV = 0,4,1,5,2,6,3,7.
//   code(k, n) = nibble INV[n % 8] of qweight[k][n / 8], as stored (a group maximum that spilled into the neighbouring nibble
//                at packing is whatever the nibbles hold); zero(k / g, n) the same from qzeros
//   W~[k][n]   = rnd_dt(float(code - zero) * float(scale[k / g][n]))      one rounding (the fp32 product is exact)
//   llmc_awq_gemm     y[M, R] = rnd_dt(sum_k x[m, k] W~[k, n] (+ bias[n])), fp32 accumulation on v_mfma_f32_32x32x16
//   llmc_awq_dequant  W~^T as [R, K] in f16 / bf16 / fp32 (the layout hip_linear takes)
//
// Opening the words: w & 0x0f0f0f0f holds the even nibbles (columns 0, 4, 1, 5 of the word) in its four bytes and
// (w >> 4) & 0x0f0f0f0f the odd ones (columns 2, 6, 3, 7): column j is byte 2 (j & 1) + (j >> 2) of half (j >> 1) & 1.
// One v_perm_b32 puts that byte of two words (k, k + 1) into the low bytes of two 16-bit halves, an OR
// with 0x64006400 makes them the f16 numbers 1024 + code; minus (1024 + zero) is exact, and one packed f16 product with the
// scale rounds once: bit for bit AutoAWQ's (q - z) * s in half precision. bf16 widens the exact difference to fp32, multiplies
// by the widened scale (exact) and rounds once with v_cvt_pk_bf16_f32.
//
// Operand map (both rungs). Lane (r = lane & 31, h = lane >> 5) of strip c0 (32 words = 256 columns) holds the eight words
// qweight[k0 + 8 h + 0..7][c0 + r]: an 8 k x 8 n block of codes, which is the B fragment (column l & 31, 8 consecutive k) of
// eight MFMAs at once: MFMA j takes nibble INV[j], i.e. the stride-8 column set 8 (c0 + r) + j. No transposition. In accumulator j
// lane r's C column is 8 (c0 + r) + j: a lane ends with 8 consecutive output columns per row.
//
// Rungs (which shape takes which: AG_LADDER; the Python layer keeps the measured table, awq_gemm_ops.LADDER):
//   stream  small M, weight-bound. One wave per (strip, M block of 32 MB rows, K slice); the fragments are de-quantized in
//           registers straight from the loaded words, one 16-k step in flight ahead. K is cut into slices of at least 64 so
//           that strips x slices x M blocks fills the chip; every slice writes fp32 partials, k_awq_reduce adds them in ascending
//           slice order (no atomics: the same bits on every run), adds the bias and rounds once.
//   tile    large M. A workgroup of 4 waves owns 128 rows x 256 columns. Per 64-k block wave w de-quantizes 16-k step w of the
//           weight tile ONCE into LDS in MFMA fragment order (slot (step, j, lane) of 16 bytes: written and read with
//           conflict-free 16-byte accesses), so the ~150 VALU instructions a lane spends per step are shared by the four M
//           blocks; x fragments come by LDS-DMA, also in fragment order (one DMA instruction = one (M block, step) fragment set;
//           rows past M lie outside the descriptor's range and arrive as zeros), double-buffered. Wave (wm, wj) multiplies M
//           blocks 2 wm, 2 wm + 1 by MFMAs j = 4 wj .. 4 wj + 3. K % 64 == 0. 64 KiB of LDS and at most 256 registers: two
//           workgroups per CU, so that one's de-quantize VALU work runs beside the other's MFMAs.
#include "common.h"
#include <stdint.h>
#include "mfma_common.h"
#include "vec16.h"

namespace llmc {

typedef __attribute__((ext_vector_type(2))) _Float16 f16x2;

struct AwqArgs {
    const uint16_t* x; const uint32_t* qw; const uint32_t* qz; const uint16_t* sc; const uint16_t* bias;
    uint16_t* y; float* ws;
    int64_t M, K, R, R8;        // R8 = R / 8 words per row
    int g, ng;
    int nstrips, nmb, nslices, slice_len, ntm;
};

// ---------------------------------------------------------------------------------------------------------------
// de-quantizing a lane's 8 k x 8 n block
// ---------------------------------------------------------------------------------------------------------------
// (1024 + byte b of lo, 1024 + byte b of hi) as two f16
__device__ __forceinline__ uint32_t awq_pair(uint32_t lo, uint32_t hi, uint32_t b) {
    return __builtin_amdgcn_perm(hi, lo, 0x0c000c00u | b | ((4u + b) << 16)) | 0x64006400u;
}

// where column j of a word sits once the word is split into its even (half 0) and odd (half 1) nibbles
__device__ __forceinline__ constexpr int awq_half(int j) { return (j >> 1) & 1; }
__device__ __forceinline__ constexpr uint32_t awq_byte(int j) { return (uint32_t)(2 * (j & 1) + (j >> 2)); }

// a group's parameters for the lane's 8 columns: zz[j] = (1024 + zero_j) twice in f16; ss[j] = scale_j twice in f16 (f16
// activations) or widened to fp32 (bf16)
template <int DT> struct AwqGroup {
    uint32_t zz[8], ss[8];
};
template <int DT> __device__ __forceinline__ void awq_group(AwqGroup<DT>& gp, uint32_t zw, uint4 sraw) {
    const uint32_t zt[2] = {zw & 0x0f0f0f0fu, (zw >> 4) & 0x0f0f0f0fu};
    const uint32_t s4[4] = {sraw.x, sraw.y, sraw.z, sraw.w};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        gp.zz[j] = awq_pair(zt[awq_half(j)], zt[awq_half(j)], awq_byte(j));
        const uint32_t sw = s4[j >> 1];
        if constexpr (DT == LLMC_F16) gp.ss[j] = __builtin_amdgcn_perm(sw, sw, (j & 1) ? 0x03020302u : 0x01000100u);
        else gp.ss[j] = __float_as_uint(f16_bits_to_f32((uint16_t)((j & 1) ? sw >> 16 : sw & 0xffffu)));
    }
}

// the eight B fragments of eight words of consecutive k: f[j] = W~[k .. k + 7][8 c + j] in DT
template <int DT> __device__ __forceinline__ void awq_frags(const uint32_t (&w)[8], const AwqGroup<DT>& gp, s16x8 (&f)[8]) {
    uint32_t t[2][8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        t[0][i] = w[i] & 0x0f0f0f0fu;
        t[1][i] = (w[i] >> 4) & 0x0f0f0f0fu;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        u32x4 o;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const uint32_t q = awq_pair(t[awq_half(j)][2 * p], t[awq_half(j)][2 * p + 1], awq_byte(j));
            const f16x2 d = __builtin_bit_cast(f16x2, q) - __builtin_bit_cast(f16x2, gp.zz[j]);       // exact
            if constexpr (DT == LLMC_F16) {
                o[p] = __builtin_bit_cast(uint32_t, d * __builtin_bit_cast(f16x2, gp.ss[j]));         // one rounding
            } else {
                // widened first (opaque: a product fused with the conversion would add +0 and lose the sign of a zero)
                const float s = __uint_as_float(gp.ss[j]);
                const f32x2 v = {opaque_f32((float)d[0]) * s, opaque_f32((float)d[1]) * s};
                o[p] = __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2));
            }
        }
        f[j] = __builtin_bit_cast(s16x8, o);
    }
}

// accumulator register q of lane (r, h) is row (q & 3) + 8 (q >> 2) + 4 h of its 32 x 32 tile
__device__ __forceinline__ int acc_row(int q, int h) { return (q & 3) + 8 * (q >> 2) + 4 * h; }

// ---------------------------------------------------------------------------------------------------------------
// stream rung
// ---------------------------------------------------------------------------------------------------------------
static constexpr int AG_STREAM_WAVES = 2048;     // waves the slices are cut for: 8 per CU of a 256-CU chip (a constant, so that
                                                 // the slice count, hence the order of the fp32 sum, does not depend on the device)
static constexpr int AG_MIN_SLICE = 64;          // k per slice at least (four 16-k steps beside a slice's set-up and its partial tile)

template <int DT, int MB>
__global__ __launch_bounds__(256) void k_awq_stream(AwqArgs a) {
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    // work item of this wave: strip fastest (neighbouring waves read neighbouring 128-byte segments of the same weight rows)
    const int64_t item = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (item >= (int64_t)a.nstrips * a.nmb * a.nslices) return;
    const int strip = (int)(item % a.nstrips);
    const int mb = (int)((item / a.nstrips) % a.nmb), slice = (int)(item / ((int64_t)a.nstrips * a.nmb));
    const int64_t wcol = (int64_t)strip * 32 + r;
    const bool cok = wcol < a.R8;                       // the last strip's guard: a lane past the edge works on the last word
    const int64_t wc = cok ? wcol : a.R8 - 1;           // (loads stay in bounds) and stores nothing
    const int64_t m0 = (int64_t)mb * 32 * MB;
    const int k_begin = slice * a.slice_len;
    const int k_end = (int64_t)k_begin + a.slice_len < a.K ? k_begin + a.slice_len : (int)a.K;

    const uint32_t* wp = a.qw + wc + (int64_t)(8 * h) * a.R8;
    const uint16_t* xp[MB];
    uint32_t xm[MB];                                     // all ones: the row exists (rows past M: clamped load, zeroed by the mask)
#pragma unroll
    for (int b = 0; b < MB; ++b) {
        const int64_t row = m0 + 32 * b + r;
        xm[b] = row < a.M ? 0xffffffffu : 0u;
        xp[b] = a.x + (xm[b] ? row : a.M - 1) * a.K + 8 * h;
    }
    auto load = [&](uint32_t (&w)[8], uint4 (&xf)[MB], int k0) {
#pragma unroll
        for (int i = 0; i < 8; ++i) w[i] = wp[(int64_t)(k0 + i) * a.R8];
#pragma unroll
        for (int b = 0; b < MB; ++b) {
            const uint4 v = *reinterpret_cast<const uint4*>(xp[b] + k0);
            xf[b] = uint4{v.x & xm[b], v.y & xm[b], v.z & xm[b], v.w & xm[b]};
        }
    };
    // a group's raw parameters: the lane's zero word and its 8 scales (16 bytes); loaded one group ahead
    uint32_t zraw;
    uint4 sraw;
    auto load_group = [&](int kg) {
        if (kg >= a.ng) kg = a.ng - 1;
        zraw = a.qz[(int64_t)kg * a.R8 + wc];
        sraw = *reinterpret_cast<const uint4*>(a.sc + (int64_t)kg * a.R + 8 * wc);
    };

    f32x16 acc[MB][8];
#pragma unroll
    for (int b = 0; b < MB; ++b)
#pragma unroll
        for (int j = 0; j < 8; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[b][j][q] = 0.0f;

    uint32_t w0[8], w1[8];
    uint4 x0[MB], x1[MB];
    AwqGroup<DT> gp;
    int kg = k_begin / a.g, gend = k_begin;              // gend: the k at which the next group starts (the first step opens one)
    load_group(kg);
    load(w0, x0, k_begin);
    for (int k0 = k_begin; k0 < k_end; k0 += 16) {
        load(w1, x1, k0 + 16 < k_end ? k0 + 16 : k0);   // the next step (the last one loads itself again: in bounds, unused)
        if (k0 >= gend) {
            awq_group<DT>(gp, zraw, sraw);
            ++kg;
            gend = kg * a.g;
            load_group(kg);
        }
        s16x8 f[8];
        awq_frags<DT>(w0, gp, f);
#pragma unroll
        for (int b = 0; b < MB; ++b) {
            const s16x8 xa = __builtin_bit_cast(s16x8, x0[b]);
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[b][j] = Mfma<DT>::run(xa, f[j], acc[b][j]);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) w0[i] = w1[i];
#pragma unroll
        for (int b = 0; b < MB; ++b) x0[b] = x1[b];
    }

    // the slice's fp32 partial tile: ws[slice][row][8 wcol .. + 7], two 16-byte stores per row
    if (!cok) return;
    float* part = a.ws + (int64_t)slice * a.M * a.R + 8 * wcol;
#pragma unroll
    for (int b = 0; b < MB; ++b)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int64_t row = m0 + 32 * b + acc_row(q, h);
            if (row >= a.M) continue;
            float4* p = reinterpret_cast<float4*>(part + row * a.R);
            p[0] = float4{acc[b][0][q], acc[b][1][q], acc[b][2][q], acc[b][3][q]};
            p[1] = float4{acc[b][4][q], acc[b][5][q], acc[b][6][q], acc[b][7][q]};
        }
}

// y = rnd(sum of the slices' partials in ascending order (+ bias)); thread = the 8 outputs of one word column
template <int DT>
__global__ __launch_bounds__(256) void k_awq_reduce(AwqArgs a) {
    const int64_t NR = a.M * a.R, i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 8;
    if (i0 >= NR) return;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = 0.0f;
    for (int s = 0; s < a.nslices; ++s) {
        const float4* p = reinterpret_cast<const float4*>(a.ws + (int64_t)s * NR + i0);
        const float4 a0 = p[0], a1 = p[1];
        v[0] += a0.x; v[1] += a0.y; v[2] += a0.z; v[3] += a0.w; v[4] += a1.x; v[5] += a1.y; v[6] += a1.z; v[7] += a1.w;
    }
    const int64_t c0 = i0 % a.R;        // R % 8 == 0: the 8 outputs lie in one row
    Vec<uint16_t, 8> o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float s = v[j] + (a.bias ? load_as_f32(a.bias, c0 + j, DT) : 0.0f);
        o.v[j] = DT == LLMC_BF16 ? f32_to_bf16_bits(s) : f32_to_f16_bits(s);
    }
    store_vec<uint16_t, 8>(a.y + i0, o);
}

// ---------------------------------------------------------------------------------------------------------------
// tile rung
// ---------------------------------------------------------------------------------------------------------------
static constexpr int AT_BM = 128, AT_KS = 64;
static constexpr int AT_B_BYTES = (AT_KS / 16) * 8 * 1024;        // 4 steps x 8 MFMAs x (64 lanes x 16 B)
static constexpr int AT_A_BYTES = (AT_BM / 32) * (AT_KS / 16) * 1024;     // 4 M blocks x 4 steps x (64 lanes x 16 B), twice

template <int DT>
__global__ __launch_bounds__(256, 2) void k_awq_tile(AwqArgs a) {
    __shared__ __attribute__((aligned(16))) char smem[AT_B_BYTES + 2 * AT_A_BYTES];
    LDS_AS char* lds = (LDS_AS char*)smem;
    const uint32_t lds0 = (uint32_t)(uintptr_t)lds;
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wv >> 1, wj = wv & 1;

    // tile of this workgroup: consecutive workgroup ids go round the 8 XCDs, so the ids one XCD sees are made consecutive tiles
    // (a bijection for any tile count); the M tiles of one strip are neighbours: they share the strip's words in that XCD's L2
    int tm, strip;
    {
        const int nt = a.ntm * a.nstrips;
        const int q = nt >> 3, rem = nt & 7, xcd = blockIdx.x & 7;
        const int id = (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + (blockIdx.x >> 3);
        tm = id % a.ntm;
        strip = id / a.ntm;
    }
    const int64_t m0 = (int64_t)tm * AT_BM;
    const int64_t wcol = (int64_t)strip * 32 + r;
    const bool cok = wcol < a.R8;
    const int64_t wc = cok ? wcol : a.R8 - 1;
    const int nkb = (int)(a.K / AT_KS);

    // B producer: wave wv de-quantizes 16-k step wv of every 64-k block
    const uint32_t* wp = a.qw + wc + (int64_t)(16 * wv + 8 * h) * a.R8;
    // A: wave wv stages the four fragment sets of M block wv. Lane (r, h) brings x[m0 + 32 wv + r][k + 8 h .. + 7]; the
    // descriptor ends with the last row of x, and only the vector offset is range-checked: a row past M arrives as zeros
    const int64_t left = (a.M - m0) * a.K * 2;
    const buf_rsrc rx = uniform_rsrc(a.x + m0 * a.K, clamp_u32(left));
    const uint32_t voff = (uint32_t)(((int64_t)(32 * wv + r) * a.K + 8 * h) * 2);

    uint32_t w[8], zraw;
    uint4 sraw;
    auto gload = [&](int kb) {
        const int64_t k0 = (int64_t)kb * AT_KS;
#pragma unroll
        for (int i = 0; i < 8; ++i) w[i] = wp[(k0 + i) * a.R8];
        const int kg = (int)((k0 + 16 * wv) / a.g);
        zraw = a.qz[(int64_t)kg * a.R8 + wc];
        sraw = *reinterpret_cast<const uint4*>(a.sc + (int64_t)kg * a.R + 8 * wc);
    };
    auto stage_x = [&](int kb) {
        const uint32_t dst = lds0 + AT_B_BYTES + (uint32_t)(kb & 1) * AT_A_BYTES + (uint32_t)wv * 4096u;
#pragma unroll
        for (int s = 0; s < 4; ++s) dma16_to(rx, voff, (uint32_t)((kb * AT_KS + 16 * s) * 2), dst + (uint32_t)s * 1024u);
    };

    f32x16 acc[2][4];
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[b][j][q] = 0.0f;

    stage_x(0);
    gload(0);
    for (int kb = 0; kb < nkb; ++kb) {
        {   // this wave's step of the weight tile, in fragment order (every wave is past the previous block's reads: the barrier
            // that ends the loop body)
            AwqGroup<DT> gp;
            awq_group<DT>(gp, zraw, sraw);
            s16x8 f[8];
            awq_frags<DT>(w, gp, f);
#pragma unroll
            for (int j = 0; j < 8; ++j) *(LDS_AS s16x8*)(lds + ((wv * 8 + j) * 64 + lane) * 16) = f[j];
        }
        vm_wait<0>();                         // this wave's x fragments of block kb have landed
        __syncthreads();                      // the weight tile and the x fragments of block kb are published
        if (kb + 1 < nkb) {                   // lands under this block's MFMAs; the x buffer it fills was last read in block kb - 1
            stage_x(kb + 1);
            gload(kb + 1);
        }
        LDS_AS char* la = lds + AT_B_BYTES + (kb & 1) * AT_A_BYTES;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            s16x8 fa[2];
#pragma unroll
            for (int b = 0; b < 2; ++b) fa[b] = *(LDS_AS s16x8*)(la + (((2 * wm + b) * 4 + s) * 64 + lane) * 16);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const s16x8 fb = *(LDS_AS s16x8*)(lds + ((s * 8 + 4 * wj + j) * 64 + lane) * 16);
#pragma unroll
                for (int b = 0; b < 2; ++b) acc[b][j] = Mfma<DT>::run(fa[b], fb, acc[b][j]);
            }
        }
        __syncthreads();                      // every wave is done with the weight tile before the next one is written
    }

    // epilogue: the lane's 4 consecutive columns 8 wcol + 4 wj .. + 3 of each row: bias in fp32, one rounding, one 8-byte store
    if (!cok) return;
    const int64_t col = 8 * wcol + 4 * wj;
    float bv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) bv[j] = a.bias ? load_as_f32(a.bias, col + j, DT) : 0.0f;
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int64_t row = m0 + 32 * (2 * wm + b) + acc_row(q, h);
            if (row >= a.M) continue;
            Vec<uint16_t, 4> o;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float s = acc[b][j][q] + bv[j];
                o.v[j] = DT == LLMC_BF16 ? f32_to_bf16_bits(s) : f32_to_f16_bits(s);
            }
            uint2 ov;
            __builtin_memcpy(&ov, &o, 8);
            *reinterpret_cast<uint2*>(a.y + row * a.R + col) = ov;
        }
}

// ---------------------------------------------------------------------------------------------------------------
// de-quantize: thread = 8 k x 4 words (32 columns). Consecutive threads take consecutive k octets, so that the 16-byte vectors
// a wave writes along K are contiguous per output row; the words are read as 8 rows x 16 bytes
// ---------------------------------------------------------------------------------------------------------------
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void k_awq_dequant(const uint32_t* __restrict__ qw, const uint32_t* __restrict__ qz,
                                                     const uint16_t* __restrict__ sc, int64_t K, int64_t R8, int g, T* __restrict__ out) {
    const int64_t K8 = K / 8, nq = (R8 + 3) / 4;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= K8 * nq) return;
    const int64_t k0 = (idx % K8) * 8, c0 = (idx / K8) * 4, kg = k0 / g, R = R8 * 8;
    Vec<uint32_t, 4> w[8], z;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        if constexpr (VEC) w[i] = load_vec<uint32_t, 4>(qw + (k0 + i) * R8 + c0);
        else
#pragma unroll
            for (int c = 0; c < 4; ++c) w[i].v[c] = c0 + c < R8 ? qw[(k0 + i) * R8 + c0 + c] : 0u;
    }
    if constexpr (VEC) z = load_vec<uint32_t, 4>(qz + kg * R8 + c0);
    else
#pragma unroll
        for (int c = 0; c < 4; ++c) z.v[c] = c0 + c < R8 ? qz[kg * R8 + c0 + c] : 0u;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if (c0 + c >= R8) break;
        const Vec<uint16_t, 8> s8 = load_vec<uint16_t, 8>(sc + kg * R + 8 * (c0 + c));
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int sh = 4 * ((j >> 1) + 4 * (j & 1));        // INV[j] = 0,4,1,5,2,6,3,7
            const int zero = (int)((z.v[c] >> sh) & 15u);
            const float s = f16_bits_to_f32(s8.v[j]);
            Vec<T, 8> o;
#pragma unroll
            for (int i = 0; i < 8; ++i) o.v[i] = from_f32<T>((float)((int)((w[i].v[c] >> sh) & 15u) - zero) * s);
            T* p = out + (8 * (c0 + c) + j) * K + k0;
            if constexpr (sizeof(T) == 4) store_vec_wide<T, 8>(p, o);
            else store_vec<T, 8>(p, o);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// host: slices, the ladder, launches
// ---------------------------------------------------------------------------------------------------------------
enum { AG_STREAM = 0, AG_TILE = 1, AG_NRUNGS = 2 };
// The first row whose bound holds, for callers of the C entry that name no rung. The measured dispatch (which also knows when
// awq_dequant + the 16-bit GEMM wins) is awq_gemm_ops.LADDER, set from profiles/awq_gemm.txt; this threshold is its stream row:
// up to 64 tokens the stream rung is 1.7 to 8 times faster than both the tile rung and the unpacked route on every measured shape.
struct AwqRung {
    int64_t max_m;
    int rung;
};
static const AwqRung AG_LADDER[] = {
    {64, AG_STREAM},
    {INT64_MAX, AG_TILE},
};
static int ag_pick_rung(int64_t M, int64_t K) {
    if (K % AT_KS) return AG_STREAM;
    for (const AwqRung& r : AG_LADDER)
        if (M <= r.max_m) return r.rung;
    return AG_TILE;
}

static int ag_stream_mb(int64_t M) { return M <= 32 ? 1 : 2; }
// how the stream rung cuts K: as many slices as fill AG_STREAM_WAVES, none shorter than AG_MIN_SLICE, and no more than keep the
// partial tiles (written and read once) at about the bytes of the weight; slices are whole 16-k steps, the last may be short
static void ag_stream_slices(int64_t M, int64_t K, int64_t R, int& nslices, int& slice_len) {
    const int64_t strips = ceil_div64(R, 256), nmb = ceil_div64(M, 32 * ag_stream_mb(M));
    int64_t want = AG_STREAM_WAVES / (strips * nmb);
    const int64_t by_len = K / AG_MIN_SLICE, by_bytes = K / (8 * M);
    if (want > by_len) want = by_len;
    if (want > by_bytes) want = by_bytes;
    if (want < 1) want = 1;
    slice_len = (int)(ceil_div64(ceil_div64(K, 16), want) * 16);
    nslices = (int)ceil_div64(K, slice_len);
}

template <int DT>
static int ag_launch(AwqArgs& a, int rung, hipStream_t st) {
    if (rung == AG_STREAM) {
        const int64_t waves = (int64_t)a.nstrips * a.nmb * a.nslices;
        const dim3 grid((unsigned)ceil_div64(waves, 4)), block(256);
        if (ag_stream_mb(a.M) == 1) hipLaunchKernelGGL((k_awq_stream<DT, 1>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((k_awq_stream<DT, 2>), grid, block, 0, st, a);
        LLMC_LAUNCH_CHECK();
        hipLaunchKernelGGL((k_awq_reduce<DT>), dim3((unsigned)ceil_div64(a.M * a.R, 2048)), dim3(256), 0, st, a);
    } else {
        hipLaunchKernelGGL((k_awq_tile<DT>), dim3((unsigned)(a.ntm * a.nstrips)), dim3(256), 0, st, a);
    }
    LLMC_LAUNCH_CHECK();
    return LLMC_OK;
}

// what both entries refuse (LLMC_ENOTSUP, nothing launched): callers compose the product from llmc_awq_dequant and the 16-bit GEMM
static bool ag_shape_notsup(const char* who, int64_t M, int64_t K, int64_t R) {
    if (K >= (1ll << 22) || R >= (1ll << 31) || M >= (1ll << 31) || ceil_div64(M, 32) * ceil_div64(R, 256) >= (1ll << 24)) {
        char msg[160];
        snprintf(msg, sizeof msg, "%s: K must be below 2^22, M and R below 2^31 and the 32 x 256 tile count below 2^24 (32-bit element indices)", who);
        set_last_error_msg(msg);
        return true;
    }
    return false;
}

}  // namespace llmc

using namespace llmc;

extern "C" size_t llmc_awq_gemm_ws_bytes(int64_t M, int64_t K, int64_t R) {
    if (M <= 0 || K <= 0 || R <= 0) return 0;
    int nslices, slice_len;
    ag_stream_slices(M, K, R, nslices, slice_len);
    return (size_t)nslices * (size_t)M * (size_t)R * 4;
}

// rung: -1 = the ladder; 0 stream, 1 tile = that rung whatever M (the measuring tool and the tests)
extern "C" int llmc_awq_gemm(const void* x, int dt, int64_t M, int64_t K, int64_t R, const int32_t* qweight, const int32_t* qzeros,
                             const void* scales, int64_t g, const void* bias, void* y, void* ws, llmc_stream_t stream, int rung) {
    LLMC_REQUIRE(x && qweight && qzeros && scales && y && M > 0 && K > 0 && R > 0 && g > 0, "awq_gemm: null/empty argument");
    LLMC_REQUIRE(dt == LLMC_F16 || dt == LLMC_BF16, "awq_gemm: x, y and bias are f16 or bf16");
    LLMC_REQUIRE(R % 8 == 0 && K % g == 0, "awq_gemm: R must be a multiple of 8 and K of the group size");
    LLMC_REQUIRE(rung >= -1 && rung < AG_NRUNGS, "awq_gemm: no such rung (-1 the ladder, 0 stream, 1 tile)");
    if (g % 16) {
        set_last_error_msg("awq_gemm: the group size must be a multiple of 16 (a 16-k MFMA step lies in one group)");
        return LLMC_ENOTSUP;
    }
    if (ag_shape_notsup("awq_gemm", M, K, R)) return LLMC_ENOTSUP;
    if ((((uintptr_t)x | (uintptr_t)y | (uintptr_t)scales | (uintptr_t)ws) & 15) || (((uintptr_t)qweight | (uintptr_t)qzeros) & 3) ||
        ((uintptr_t)bias & 1)) {
        set_last_error_msg("awq_gemm: x, y, scales and ws need 16-byte, the words 4-byte, the bias element alignment");
        return LLMC_ENOTSUP;
    }
    if (rung == AG_TILE && K % AT_KS) {
        set_last_error_msg("awq_gemm: the tile rung takes K % 64 == 0 (one staged K block); the stream rung takes any K");
        return LLMC_ENOTSUP;
    }
    if (rung < 0) rung = ag_pick_rung(M, K);
    LLMC_REQUIRE(rung != AG_STREAM || ws, "awq_gemm: the stream rung needs a workspace of llmc_awq_gemm_ws_bytes");
    AwqArgs a;
    a.x = (const uint16_t*)x; a.qw = (const uint32_t*)qweight; a.qz = (const uint32_t*)qzeros; a.sc = (const uint16_t*)scales;
    a.bias = (const uint16_t*)bias; a.y = (uint16_t*)y; a.ws = (float*)ws;
    a.M = M; a.K = K; a.R = R; a.R8 = R / 8; a.g = (int)g; a.ng = (int)(K / g);
    a.nstrips = (int)ceil_div64(R, 256);
    a.nmb = (int)ceil_div64(M, 32 * ag_stream_mb(M));
    a.ntm = (int)ceil_div64(M, AT_BM);
    ag_stream_slices(M, K, R, a.nslices, a.slice_len);
    hipStream_t st = (hipStream_t)stream;
    return dt == LLMC_F16 ? ag_launch<LLMC_F16>(a, rung, st) : ag_launch<LLMC_BF16>(a, rung, st);
}

extern "C" int llmc_awq_dequant(const int32_t* qweight, const int32_t* qzeros, const void* scales, int64_t K, int64_t R, int64_t g,
                                void* out, int out_dt, llmc_stream_t stream) {
    LLMC_REQUIRE(qweight && qzeros && scales && out && K > 0 && R > 0 && g > 0, "awq_dequant: null/empty argument");
    LLMC_REQUIRE(dtype_ok(out_dt), "awq_dequant: bad output dtype");
    LLMC_REQUIRE(R % 8 == 0 && K % g == 0, "awq_dequant: R must be a multiple of 8 and K of the group size");
    if (g % 8) {
        set_last_error_msg("awq_dequant: the group size must be a multiple of 8 (one 16-byte vector along K lies in one group)");
        return LLMC_ENOTSUP;
    }
    if (ag_shape_notsup("awq_dequant", 1, K, R)) return LLMC_ENOTSUP;
    if (K * R >= (1ll << 44)) {
        set_last_error_msg("awq_dequant: K * R must be below 2^44 (one thread per 8 k x 32 columns in a 1-D grid)");
        return LLMC_ENOTSUP;
    }
    if ((((uintptr_t)scales | (uintptr_t)out) & 15) || (((uintptr_t)qweight | (uintptr_t)qzeros) & 3)) {
        set_last_error_msg("awq_dequant: scales and out need 16-byte, the words 4-byte alignment");
        return LLMC_ENOTSUP;
    }
    const int64_t R8 = R / 8;
    const bool vec = R8 % 4 == 0 && ((((uintptr_t)qweight | (uintptr_t)qzeros) & 15) == 0);
    const dim3 grid((unsigned)ceil_div64((K / 8) * ceil_div64(R8, 4), 256)), block(256);
    hipStream_t st = (hipStream_t)stream;
    const uint32_t* qw = (const uint32_t*)qweight;
    const uint32_t* qz = (const uint32_t*)qzeros;
    DISPATCH_DT(out_dt,
                if (vec) hipLaunchKernelGGL((k_awq_dequant<T, true>), grid, block, 0, st, qw, qz, (const uint16_t*)scales, K, R8, (int)g, (T*)out);
                else hipLaunchKernelGGL((k_awq_dequant<T, false>), grid, block, 0, st, qw, qz, (const uint16_t*)scales, K, R8, (int)g, (T*)out));
    LLMC_LAUNCH_CHECK();
    return LLMC_OK;
}
