// awq_i8_gemm.hip — the W4A8 Linear on AutoAWQ's GEMM layout: the packed nibbles of awq_gemm.hip's stored form (qweight int32
// [K, R/8], qzeros int32 [K/g, R/8], scales f16 [K/g, R]; column 8 c + j of a word in nibble INV[j], see that file's header) times
// int8 activation codes a8 [M, K] with one fp32 scale per token or per tensor, on the int8 matrix instruction
// v_mfma_i32_32x32x32_i8 (an extension: the reference's AutoawqRealQuantLinear raises in forward).
//   d(k, n)   = code(k, n) - zero(k / g, n)                           integers in [-15, 15], nibbles read as stored
//   S_g(m, n) = sum over the k of group g of a8(m, k) d(k, n)          int32, exact
//   acc(m, n) = fmaf(float(S_g), float(scales[g][n]), acc) for g ascending, from 0        fp32, one v_fma_f32 per group
//   y(m, n)   = rnd_dt(a_s(m) * acc(m, n) + bias(n))                   fp32 product, then fp32 sum, one rounding to dt
// float(S_g) is exact: |S_g| <= g * 128 * 15 < 2^24 for g <= 8192. g % 32 == 0, so that no 32-deep MFMA step straddles a group.
//
// Operand map (both rungs; i8 operand layout of mfma_common.h: lane l holds 16 consecutive k bytes of row / column l & 31, k half
// l >> 5). Lane (r = lane & 31, h = lane >> 5) of strip c0 (32 words = 256 columns) holds the 16 words
// qweight[k0 + 16 h + 0..15][c0 + r]: a 16 k x 8 n block of nibbles, which is the B fragment (column r, 16 consecutive k, 16 bytes)
// of eight MFMAs at once: MFMA j takes the stride-8 column set 8 (c0 + r) + j. No transposition through LDS. In accumulator j lane
// r's C column is 8 (c0 + r) + j, so the group's scale is one number per accumulator tile and lane.
//
// Opening the nibbles. (w >> 4 hf) & 0x0f0f0f0f holds the codes of four columns of one k in its bytes (hf = 0: columns 0, 4, 1, 5
// of the word, hf = 1: 2, 6, 3, 7); the group's zero word opens the same way, so the zero points are taken off BEFORE the bytes
// move and need no replication: with c = 0x80808080 - zeros (no byte borrows: 0x80 - z >= 0x71), (codes + c) ^ 0x80808080 is the
// two's-complement code - zero in every byte (codes + c has no byte carries: at most 0x8f) — an AND, an ADD and an XOR per word
// and half. Then 4 x 4 byte transposes (8 v_perm_b32 each) make registers that hold four consecutive k of one column.
// Per 32-k step a lane spends 16 shifts, 32 ANDs, 32 ADDs, 32 XORs and 64 v_perm_b32 for 8 fragments.
//
// Rungs (which shape takes which: A8_LADDER; the Python layer keeps the measured table, awq_gemm_ops.I8_LADDER):
//   stream  small M, weight-bound. One wave per (strip, block of 32 rows, K slice of whole groups); the nibbles are opened in
//           registers straight from the loaded words, one 32-k step in flight ahead; the slice's fp32 partial tile goes to the
//           caller's workspace, k_awq8_reduce adds the slices in ascending order (no atomics: the same bits on every run), applies
//           a_s and the bias and rounds once.
//   tile    large M. A workgroup of 8 waves owns 128 rows x 256 columns. Per 128-k block wave w opens nibble half w & 1 of 32-k step
//           w >> 1 ONCE into LDS in MFMA fragment order (slot (step, j, lane) of 16 bytes), shared by the four row blocks; the
//           activation codes come by LDS-DMA in fragment order, double-buffered (rows past M lie outside the descriptor's range and
//           arrive as zeros). Wave (wm = w >> 1, wj = w & 1) multiplies row block wm by MFMAs j = 4 wj .. 4 wj + 3: 64 int32 and 64
//           fp32 accumulator registers. 64 KiB of LDS, one workgroup of 8 waves per CU.
#include "common.h"
#include <stdint.h>
#include "mfma_common.h"
#include "vec16.h"

namespace llmc {

struct Awq8Args {
    const int8_t* a8; const float* a_s; const uint32_t* qw; const uint32_t* qz; const uint16_t* sc; const uint16_t* bias;
    uint16_t* y; float* ws;
    int64_t M, K, R, R8;        // R8 = R / 8 words per row
    int as_rows;                // 1: one activation scale per row, 0: one in all
    int g, ng, gsteps;          // gsteps = g / 32 MFMA steps per group
    int nstrips, nmb, nslices, slice_groups, ntm;
};

// ---------------------------------------------------------------------------------------------------------------
// opening a lane's 16 k x 8 n block
// ---------------------------------------------------------------------------------------------------------------
// byte b of nibble half hf is column j of the word: hf = (j >> 1) & 1, b = 2 (j & 1) + (j >> 2)
__device__ __forceinline__ constexpr int awq8_col(int hf, int b) { return (b >> 1) + 2 * hf + 4 * (b & 1); }

// 0x80808080 - the zeros of nibble half HF of a zero word
template <int HF> __device__ __forceinline__ uint32_t awq8_zc(uint32_t zw) { return 0x80808080u - ((zw >> (4 * HF)) & 0x0f0f0f0fu); }

// the four B fragments of nibble half HF of 16 words of consecutive k: f[b] = d[k .. k + 15][column awq8_col(HF, b)] as int8
template <int HF> __device__ __forceinline__ void awq8_open(const uint32_t (&w)[16], uint32_t zc, i32x4 (&f)[4]) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        uint32_t d[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) d[i] = ((((w[4 * p + i] >> (4 * HF)) & 0x0f0f0f0fu) + zc) ^ 0x80808080u);
        // 4 x 4 byte transpose: d[i] byte b -> f[b][p] byte i
        const uint32_t lo01 = __builtin_amdgcn_perm(d[1], d[0], 0x05010400u), hi01 = __builtin_amdgcn_perm(d[1], d[0], 0x07030602u);
        const uint32_t lo23 = __builtin_amdgcn_perm(d[3], d[2], 0x05010400u), hi23 = __builtin_amdgcn_perm(d[3], d[2], 0x07030602u);
        f[0][p] = (int)__builtin_amdgcn_perm(lo23, lo01, 0x05040100u);
        f[1][p] = (int)__builtin_amdgcn_perm(lo23, lo01, 0x07060302u);
        f[2][p] = (int)__builtin_amdgcn_perm(hi23, hi01, 0x05040100u);
        f[3][p] = (int)__builtin_amdgcn_perm(hi23, hi01, 0x07060302u);
    }
}

// accumulator register q of lane (r, h) is row (q & 3) + 8 (q >> 2) + 4 h of its 32 x 32 tile
__device__ __forceinline__ int awq8_acc_row(int q, int h) { return (q & 3) + 8 * (q >> 2) + 4 * h; }

// a group is done: acc = fmaf(float(S_g), scale, acc), S_g = 0
__device__ __forceinline__ void awq8_fold(i32x16& s, float scale, f32x16& acc) {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        acc[q] = __builtin_fmaf((float)s[q], scale, acc[q]);
        s[q] = 0;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// stream rung
// ---------------------------------------------------------------------------------------------------------------
static constexpr int A8_STREAM_WAVES = 2048;     // waves the slices are cut for: 8 per CU of a 256-CU chip (a constant, so that
                                                 // the slice count, hence the order of the fp32 sum, does not depend on the device)
static constexpr int A8_MIN_SLICE = 64;          // k per slice at least

__global__ __launch_bounds__(256) void k_awq8_stream(Awq8Args a) {
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    // work item of this wave: strip fastest (neighbouring waves read neighbouring 128-byte segments of the same weight rows)
    const int64_t item = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (item >= (int64_t)a.nstrips * a.nmb * a.nslices) return;
    const int strip = (int)(item % a.nstrips);
    const int mb = (int)((item / a.nstrips) % a.nmb), slice = (int)(item / ((int64_t)a.nstrips * a.nmb));
    const int64_t wcol = (int64_t)strip * 32 + r;
    const bool cok = wcol < a.R8;                       // the last strip's guard: a lane past the edge works on the last word
    const int64_t wc = cok ? wcol : a.R8 - 1;           // (loads stay in bounds) and stores nothing
    const int64_t m0 = (int64_t)mb * 32;
    const int g_begin = slice * a.slice_groups;
    const int g_end = g_begin + a.slice_groups < a.ng ? g_begin + a.slice_groups : a.ng;
    const int k_begin = g_begin * a.g, k_end = g_end * a.g;

    const uint32_t* wp = a.qw + wc + (int64_t)(16 * h) * a.R8;
    const int64_t row = m0 + r;
    const uint32_t xm = row < a.M ? 0xffffffffu : 0u;   // all ones: the row exists (rows past M: clamped load, zeroed by the mask)
    const int8_t* xp = a.a8 + (xm ? row : a.M - 1) * a.K + 16 * h;
    auto load = [&](uint32_t (&w)[16], uint4& xf, int k0) {
#pragma unroll
        for (int i = 0; i < 16; ++i) w[i] = wp[(int64_t)(k0 + i) * a.R8];
        const uint4 v = *reinterpret_cast<const uint4*>(xp + k0);
        xf = uint4{v.x & xm, v.y & xm, v.z & xm, v.w & xm};
    };
    // a group's raw parameters: the lane's zero word and its 8 scales (16 bytes); loaded one group ahead
    uint32_t zraw;
    uint4 sraw;
    auto load_group = [&](int kg) {
        if (kg >= a.ng) kg = a.ng - 1;
        zraw = a.qz[(int64_t)kg * a.R8 + wc];
        sraw = *reinterpret_cast<const uint4*>(a.sc + (int64_t)kg * a.R + 8 * wc);
    };

    i32x16 si[8];
    f32x16 acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            si[j][q] = 0;
            acc[j][q] = 0.0f;
        }

    uint32_t w0[16], w1[16], zc[2] = {0u, 0u};
    uint4 x0, x1;
    float ss[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) ss[j] = 0.0f;
    int kg = g_begin, cnt = 0;                           // cnt: steps done in the open group
    load_group(kg);
    load(w0, x0, k_begin);
    for (int k0 = k_begin; k0 < k_end; k0 += 32) {
        load(w1, x1, k0 + 32 < k_end ? k0 + 32 : k0);   // the next step (the last one loads itself again: in bounds, unused)
        if (cnt == 0) {                                 // a group opens: its parameters, and the next group's on their way
            zc[0] = awq8_zc<0>(zraw);
            zc[1] = awq8_zc<1>(zraw);
            const uint32_t s4[4] = {sraw.x, sraw.y, sraw.z, sraw.w};
#pragma unroll
            for (int j = 0; j < 8; ++j) ss[j] = f16_bits_to_f32((uint16_t)((j & 1) ? s4[j >> 1] >> 16 : s4[j >> 1] & 0xffffu));
            load_group(kg + 1);
        }
        i32x4 f0[4], f1[4];
        awq8_open<0>(w0, zc[0], f0);
        awq8_open<1>(w0, zc[1], f1);
        const i32x4 xa = __builtin_bit_cast(i32x4, x0);
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            si[awq8_col(0, b)] = mfma_i32_32x32x32_i8(xa, f0[b], si[awq8_col(0, b)]);
            si[awq8_col(1, b)] = mfma_i32_32x32x32_i8(xa, f1[b], si[awq8_col(1, b)]);
        }
        if (++cnt == a.gsteps) {
#pragma unroll
            for (int j = 0; j < 8; ++j) awq8_fold(si[j], ss[j], acc[j]);
            cnt = 0;
            ++kg;
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) w0[i] = w1[i];
        x0 = x1;
    }

    // the slice's fp32 partial tile: ws[slice][row][8 wcol .. + 7], two 16-byte stores per row
    if (!cok) return;
    float* part = a.ws + (int64_t)slice * a.M * a.R + 8 * wcol;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int64_t orow = m0 + awq8_acc_row(q, h);
        if (orow >= a.M) continue;
        float4* p = reinterpret_cast<float4*>(part + orow * a.R);
        p[0] = float4{acc[0][q], acc[1][q], acc[2][q], acc[3][q]};
        p[1] = float4{acc[4][q], acc[5][q], acc[6][q], acc[7][q]};
    }
}

// y = rnd(a_s * (sum of the slices' partials in ascending order) + bias); thread = the 8 outputs of one word column
template <int DT>
__global__ __launch_bounds__(256) void k_awq8_reduce(Awq8Args a) {
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
    const int64_t row = i0 / a.R, c0 = i0 - row * a.R;        // R % 8 == 0: the 8 outputs lie in one row
    const float as = a.a_s[a.as_rows ? row : 0];
    Vec<uint16_t, 8> o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float s = as * v[j] + (a.bias ? load_as_f32(a.bias, c0 + j, DT) : 0.0f);
        o.v[j] = DT == LLMC_BF16 ? f32_to_bf16_bits(s) : f32_to_f16_bits(s);
    }
    store_vec<uint16_t, 8>(a.y + i0, o);
}

// ---------------------------------------------------------------------------------------------------------------
// tile rung
// ---------------------------------------------------------------------------------------------------------------
static constexpr int A8T_BM = 128, A8T_KB = 128, A8T_STEPS = A8T_KB / 32;
static constexpr int A8T_B_BYTES = A8T_STEPS * 8 * 1024;                  // 4 steps x 8 MFMAs x (64 lanes x 16 B)
static constexpr int A8T_A_BYTES = (A8T_BM / 32) * A8T_STEPS * 1024;      // 4 row blocks x 4 steps x (64 lanes x 16 B), twice

template <int DT>
__global__ __launch_bounds__(512) void k_awq8_tile(Awq8Args a) {
    __shared__ __attribute__((aligned(16))) char smem[A8T_B_BYTES + 2 * A8T_A_BYTES];
    LDS_AS char* lds = (LDS_AS char*)smem;
    const uint32_t lds0 = (uint32_t)(uintptr_t)lds;
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wv >> 1, wj = wv & 1;                // as a producer: 32-k step wm, nibble half wj

    // the row tiles of one strip are neighbours: they share the strip's words in L2
    const int tm = (int)(blockIdx.x % (unsigned)a.ntm), strip = (int)(blockIdx.x / (unsigned)a.ntm);
    const int64_t m0 = (int64_t)tm * A8T_BM;
    const int64_t wcol = (int64_t)strip * 32 + r;
    const bool cok = wcol < a.R8;
    const int64_t wc = cok ? wcol : a.R8 - 1;
    const int nsteps = (int)(a.K / 32), nkb = (nsteps + A8T_STEPS - 1) / A8T_STEPS;

    const uint32_t* wp = a.qw + wc + (int64_t)(32 * wm + 16 * h) * a.R8;
    // A: wave (wm, wj) stages the fragment sets of row block wm, steps 2 wj and 2 wj + 1. Lane (r, h) brings
    // a8[m0 + 32 wm + r][k + 16 h .. + 15]; the descriptor ends with the last row of a8: a row past M arrives as zeros
    const int64_t left = (a.M - m0) * a.K;
    const buf_rsrc rx = uniform_rsrc(a.a8 + m0 * a.K, clamp_u32(left));
    const uint32_t voff = (uint32_t)((int64_t)(32 * wm + r) * a.K + 16 * h);

    uint32_t w[16], zraw = 0u;
#pragma unroll
    for (int i = 0; i < 16; ++i) w[i] = 0u;
    auto gload = [&](int kb) {
        if (kb * A8T_STEPS + wm >= nsteps) return;      // a step past K (the last block of a ragged K): neither opened nor multiplied
        const int64_t k0 = (int64_t)kb * A8T_KB;
#pragma unroll
        for (int i = 0; i < 16; ++i) w[i] = wp[(k0 + i) * a.R8];
        zraw = a.qz[(int64_t)((k0 + 32 * wm) / a.g) * a.R8 + wc];
    };
    auto stage_a = [&](int kb) {
        const uint32_t dst = lds0 + A8T_B_BYTES + (uint32_t)(kb & 1) * A8T_A_BYTES + (uint32_t)wm * 4096u;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int s = 2 * wj + t;
            if (kb * A8T_STEPS + s < nsteps) dma16_to(rx, voff, (uint32_t)(kb * A8T_KB + 32 * s), dst + (uint32_t)s * 1024u);
        }
    };
    // the scales of the open group for the lane's 4 columns 8 wc + 4 wj .. + 3 (8 bytes), loaded when the group opens
    uint2 sraw;
    auto load_scales = [&](int kg) {
        if (kg >= a.ng) kg = a.ng - 1;
        sraw = *reinterpret_cast<const uint2*>(a.sc + (int64_t)kg * a.R + 8 * wc + 4 * wj);
    };

    i32x16 si[4];
    f32x16 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            si[j][q] = 0;
            acc[j][q] = 0.0f;
        }

    int kg = 0, cnt = 0;
    load_scales(0);
    stage_a(0);
    gload(0);
    for (int kb = 0; kb < nkb; ++kb) {
        if (kb * A8T_STEPS + wm < nsteps) {
            // this wave's half step of the weight tile, in fragment order (every wave is past the previous block's reads: the
            // barrier that ends the loop body)
            i32x4 f[4];
            if (wj) awq8_open<1>(w, awq8_zc<1>(zraw), f);
            else awq8_open<0>(w, awq8_zc<0>(zraw), f);
#pragma unroll
            for (int b = 0; b < 4; ++b) *(LDS_AS i32x4*)(lds + ((wm * 8 + awq8_col(wj, b)) * 64 + lane) * 16) = f[b];
        }
        vm_wait<0>();                         // this wave's a8 fragments of block kb have landed
        __syncthreads();                      // the weight tile and the a8 fragments of block kb are published
        if (kb + 1 < nkb) {                   // lands under this block's MFMAs; the a8 buffer it fills was last read in block kb - 1
            stage_a(kb + 1);
            gload(kb + 1);
        }
        LDS_AS char* la = lds + A8T_B_BYTES + (kb & 1) * A8T_A_BYTES;
#pragma unroll
        for (int s = 0; s < A8T_STEPS; ++s) {
            if (kb * A8T_STEPS + s >= nsteps) break;
            const i32x4 fa = *(LDS_AS i32x4*)(la + ((wm * A8T_STEPS + s) * 64 + lane) * 16);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const i32x4 fb = *(LDS_AS i32x4*)(lds + ((s * 8 + 4 * wj + j) * 64 + lane) * 16);
                si[j] = mfma_i32_32x32x32_i8(fa, fb, si[j]);
            }
            if (++cnt == a.gsteps) {
                const uint32_t s2[2] = {sraw.x, sraw.y};
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    awq8_fold(si[j], f16_bits_to_f32((uint16_t)((j & 1) ? s2[j >> 1] >> 16 : s2[j >> 1] & 0xffffu)), acc[j]);
                cnt = 0;
                load_scales(++kg);
            }
        }
        __syncthreads();                      // every wave is done with the weight tile before the next one is written
    }

    // epilogue: the lane's 4 consecutive columns 8 wcol + 4 wj .. + 3 of each row: a_s and the bias in fp32, one rounding, one 8-byte store
    if (!cok) return;
    const int64_t col = 8 * wcol + 4 * wj;
    float bv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) bv[j] = a.bias ? load_as_f32(a.bias, col + j, DT) : 0.0f;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int64_t row = m0 + 32 * wm + awq8_acc_row(q, h);
        if (row >= a.M) continue;
        const float as = a.a_s[a.as_rows ? row : 0];
        Vec<uint16_t, 4> o;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float s = as * acc[j][q] + bv[j];
            o.v[j] = DT == LLMC_BF16 ? f32_to_bf16_bits(s) : f32_to_f16_bits(s);
        }
        uint2 ov;
        __builtin_memcpy(&ov, &o, 8);
        *reinterpret_cast<uint2*>(a.y + row * a.R + col) = ov;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// host: slices, the ladder, launches
// ---------------------------------------------------------------------------------------------------------------
enum { A8_STREAM = 0, A8_TILE = 1, A8_NRUNGS = 2 };
// The first row whose bound holds, for callers that name no rung. The measured dispatch (which also knows where the W4A16 path on
// de-quantized codes wins) is awq_gemm_ops.I8_LADDER, set from profiles/awq_i8_gemm.txt.
struct Awq8Rung {
    int64_t max_m;
    int rung;
};
static const Awq8Rung A8_LADDER[] = {
    {64, A8_STREAM},
    {INT64_MAX, A8_TILE},
};
static int a8_pick_rung(int64_t M) {
    for (const Awq8Rung& r : A8_LADDER)
        if (M <= r.max_m) return r.rung;
    return A8_TILE;
}

// how the stream rung cuts K: as many slices as fill A8_STREAM_WAVES, whole groups each and none shorter than A8_MIN_SLICE, and no
// more than keep the partial tiles (written and read once) at about the bytes of the weight
static void a8_stream_slices(int64_t M, int64_t K, int64_t R, int64_t g, int& nslices, int& slice_groups) {
    const int64_t strips = ceil_div64(R, 256), nmb = ceil_div64(M, 32), ng = K / g;
    int64_t want = A8_STREAM_WAVES / (strips * nmb);
    const int64_t by_len = K / A8_MIN_SLICE, by_bytes = K / (8 * M);
    if (want > by_len) want = by_len;
    if (want > by_bytes) want = by_bytes;
    if (want > ng) want = ng;
    if (want < 1) want = 1;
    slice_groups = (int)ceil_div64(ng, want);
    nslices = (int)ceil_div64(ng, slice_groups);
}

static bool a8_shape_ok(int64_t M, int64_t K, int64_t R, int64_t g) {
    return M > 0 && K > 0 && R > 0 && g > 0 && R % 8 == 0 && K % g == 0 && g % 32 == 0 && g <= 8192 && K < (1ll << 22) &&
           R < (1ll << 31) && M < (1ll << 31) && ceil_div64(M, 32) * ceil_div64(R, 256) < (1ll << 24);
}

template <int DT>
static int a8_launch(Awq8Args& a, int rung, hipStream_t st) {
    if (rung == A8_STREAM) {
        const int64_t waves = (int64_t)a.nstrips * a.nmb * a.nslices;
        hipLaunchKernelGGL(k_awq8_stream, dim3((unsigned)ceil_div64(waves, 4)), dim3(256), 0, st, a);
        LLMC_LAUNCH_CHECK();
        hipLaunchKernelGGL((k_awq8_reduce<DT>), dim3((unsigned)ceil_div64(a.M * a.R, 2048)), dim3(256), 0, st, a);
    } else {
        hipLaunchKernelGGL((k_awq8_tile<DT>), dim3((unsigned)(a.ntm * a.nstrips)), dim3(512), 0, st, a);
    }
    LLMC_LAUNCH_CHECK();
    return LLMC_OK;
}

}  // namespace llmc

using namespace llmc;

// the stream rung's workspace: one fp32 [M, R] per K slice; 0 for a shape the entry point does not take. A pure host call
extern "C" size_t llmc_awq_i8_gemm_ws_bytes(int64_t M, int64_t K, int64_t R, int64_t g) {
    if (!a8_shape_ok(M, K, R, g)) return 0;
    int nslices, slice_groups;
    a8_stream_slices(M, K, R, g, nslices, slice_groups);
    return (size_t)nslices * (size_t)M * (size_t)R * 4;
}

// the rung the ladder gives M tokens (0 stream, 1 tile): a pure host call, for tools and tests
extern "C" int llmc_awq_i8_gemm_rung(int64_t M, int64_t K, int64_t R) {
    (void)K;
    (void)R;
    return a8_pick_rung(M);
}

// rung: -1 = the ladder; 0 stream, 1 tile = that rung whatever M (the measuring tool and the tests)
extern "C" int llmc_awq_i8_gemm_on_rung(const void* a8, const float* a_s, int64_t a_s_n, int64_t M, int64_t K, int64_t R,
                                        const int32_t* qweight, const int32_t* qzeros, const void* scales, int64_t g, int out_dt,
                                        const void* bias, void* y, void* ws, size_t ws_bytes, int rung, llmc_stream_t stream) {
    LLMC_REQUIRE(a8 && a_s && qweight && qzeros && scales && y && M > 0 && K > 0 && R > 0 && g > 0, "awq_i8_gemm: null/empty argument");
    LLMC_REQUIRE(out_dt == LLMC_F16 || out_dt == LLMC_BF16, "awq_i8_gemm: y and bias are f16 or bf16");
    LLMC_REQUIRE(R % 8 == 0 && K % g == 0, "awq_i8_gemm: R must be a multiple of 8 and K of the group size");
    LLMC_REQUIRE(a_s_n == 1 || a_s_n == M, "awq_i8_gemm: a_s holds one scale per token (M) or one");
    LLMC_REQUIRE(rung >= -1 && rung < A8_NRUNGS, "awq_i8_gemm: no such rung (-1 the ladder, 0 stream, 1 tile)");
    if (g % 32) {
        set_last_error_msg("awq_i8_gemm: the group size must be a multiple of 32 (a 32-k MFMA step lies in one group)");
        return LLMC_ENOTSUP;
    }
    if (g > 8192) {
        set_last_error_msg("awq_i8_gemm: the group size must be at most 8192 (a group's int32 sum is converted to fp32 exactly below 2^24)");
        return LLMC_ENOTSUP;
    }
    if (!a8_shape_ok(M, K, R, g)) {
        set_last_error_msg("awq_i8_gemm: K must be below 2^22, M and R below 2^31 and the 32 x 256 tile count below 2^24 (32-bit element indices)");
        return LLMC_ENOTSUP;
    }
    if ((((uintptr_t)a8 | (uintptr_t)y | (uintptr_t)scales | (uintptr_t)ws) & 15) ||
        (((uintptr_t)qweight | (uintptr_t)qzeros | (uintptr_t)a_s) & 3) || ((uintptr_t)bias & 1)) {
        set_last_error_msg("awq_i8_gemm: a8, y, scales and ws need 16-byte, the words and a_s 4-byte, the bias element alignment");
        return LLMC_ENOTSUP;
    }
    if (rung < 0) rung = a8_pick_rung(M);
    LLMC_REQUIRE(rung != A8_STREAM || (ws && ws_bytes >= llmc_awq_i8_gemm_ws_bytes(M, K, R, g)),
                 "awq_i8_gemm: the stream rung needs a workspace of llmc_awq_i8_gemm_ws_bytes(M, K, R, g) bytes");
    Awq8Args a;
    a.a8 = (const int8_t*)a8; a.a_s = a_s; a.qw = (const uint32_t*)qweight; a.qz = (const uint32_t*)qzeros;
    a.sc = (const uint16_t*)scales; a.bias = (const uint16_t*)bias; a.y = (uint16_t*)y; a.ws = (float*)ws;
    a.M = M; a.K = K; a.R = R; a.R8 = R / 8; a.as_rows = a_s_n == M && M > 1;
    a.g = (int)g; a.ng = (int)(K / g); a.gsteps = (int)(g / 32);
    a.nstrips = (int)ceil_div64(R, 256);
    a.nmb = (int)ceil_div64(M, 32);
    a.ntm = (int)ceil_div64(M, A8T_BM);
    a8_stream_slices(M, K, R, g, a.nslices, a.slice_groups);
    hipStream_t st = (hipStream_t)stream;
    return out_dt == LLMC_F16 ? a8_launch<LLMC_F16>(a, rung, st) : a8_launch<LLMC_BF16>(a, rung, st);
}
