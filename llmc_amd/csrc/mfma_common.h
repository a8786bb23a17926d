// mfma_common.h — the toolkit of the matrix-pipe kernels, each hardware rule of gfx950 written down once: vector types, the
// MFMA wrappers, counted waits, the transposing fragment read, buffer descriptors, the LDS-DMA pieces and the split of an
// fp32 value into three bf16 terms. Included by hessian_syrk.hip, linear_eval.hip, gemm3.hip, gemm3_wide.hip,
// sgemm_wide_tile.h (sgemm_wide.hip, gptq_loop.hip), fp8_block.hip, mx_gemm.hip and token_select.hip; sgemm.hip and cholesky.hip
// take the vector types.
// Everything here is __forceinline__: a kernel's instruction stream is what it was with the helper written out in place.
#pragma once
#include "common.h"

namespace llmc {

typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((__vector_size__(4 * sizeof(short)))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

#define LDS_AS __attribute__((address_space(3)))

template <int DT> struct Mfma;
template <> struct Mfma<LLMC_BF16> {
    static __device__ __forceinline__ f32x16 run(s16x8 a, s16x8 b, f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a),
                                                       __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    }
};
template <> struct Mfma<LLMC_F16> {
    static __device__ __forceinline__ f32x16 run(s16x8 a, s16x8 b, f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a),
                                                      __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    }
};

// ---- the block-scaled form v_mfma_scale_f32_16x16x128_f8f6f4: A and B in formats FA / FB (the instruction's cbsz / blgp codes),
// lane l holds row / column l & 15; an e2m1 operand's k 32 g .. + 31 (g = l >> 4) in the first 4 of its 8 registers, an e4m3 / e5m2
// operand's k 16 g .. + 15 in registers 0-3 and 64 + 16 g .. + 15 in registers 4-7; byte 0 of lane l's scale register is the e8m0
// scale (2^(byte - 127)) of row l & 15, k block g, for either format (csrc/mx_gemm.hip has the probe's account).
constexpr int MFMA_FMT_E4M3 = 0, MFMA_FMT_E5M2 = 1, MFMA_FMT_E2M1 = 4;
template <int FA, int FB> __device__ __forceinline__ f32x4 mfma_scale_16x16x128(i32x8 a, i32x8 b, f32x4 c, int scale_a, int scale_b) {
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, FA, FB, 0, scale_a, 0, scale_b);
}

// ---- waits. The LDS-DMA pieces below are inline asm, so hipcc's own vmcnt bookkeeping does not count them: the kernels wait
// by hand, for "all but the N youngest vector-memory requests of this wave" (requests complete in issue order).
template <int N> __device__ __forceinline__ void vm_wait() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
__device__ __forceinline__ void lds_wait_all() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// A kernel whose DMA destinations are immediates owns the whole LDS: its dynamic LDS must start at address 0.
__device__ __forceinline__ void require_lds_base_zero(LDS_AS char* lds) {
    if ((uint32_t)(uintptr_t)lds != 0u) __builtin_trap();
}

// ---- transposing fragment read of a k-major bf16 / f16 panel (k-rows of ROW_BYTES): two ds_read_b64_tr_b16, each turning four
// k-rows into four consecutive k of one row (channel) per lane; the second one starts four k-rows further down. Together: the 8
// consecutive k of one row that a 32x32x16 MFMA takes per lane.
template <int ROW_BYTES> __device__ __forceinline__ s16x8 tr_frag(LDS_AS char* p, int imm) {
    s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_AS s16x4*)(p + imm));
    s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_AS s16x4*)(p + imm + 4 * ROW_BYTES));
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// ---- buffer descriptors: base, stride 0, `bytes` of range (an access at or past it reads 0 / is dropped, which is how the
// kernels mask lanes: offset | 0x80000000), word 3 = RSRC_WORD3 (data format 32 bit, nothing else set).
constexpr int RSRC_WORD3 = 0x00020000;
typedef __amdgpu_buffer_rsrc_t buf_rsrc;
// For the raw_buffer_* builtins and the register-destination DMA piece. A descriptor lives in SGPRs: it is built from
// readfirstlane'd halves so that the compiler can prove it wave-uniform (else every use becomes a waterfall loop).
__device__ __forceinline__ buf_rsrc uniform_rsrc(const void* p, uint32_t bytes) {
    const uint64_t u = (uint64_t)p;
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)u);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(u >> 32));
    return __builtin_amdgcn_make_buffer_rsrc((void*)(((uint64_t)hi << 32) | lo), (short)0,
                                             __builtin_amdgcn_readfirstlane((int)bytes), RSRC_WORD3);
}
// The same four words filled by hand from kernel arguments (uniform by construction), for the asm pieces that take an i32x4.
// The low 32 bits of `bytes` are taken as given; CLAMP_4GIB: an extent that may pass 4 GiB (linear_eval.hip's operands) is
// clamped to 0xffffffff instead. (A switch here and not a clamp at the call: the order in which the four words are computed
// is part of the callers' instruction streams.)
constexpr bool CLAMP_4GIB = true;
__device__ __forceinline__ uint32_t clamp_u32(int64_t v) { return (uint32_t)(v > 0xffffffffll ? 0xffffffffll : v); }
template <bool CLAMP = false> __device__ __forceinline__ i32x4 rsrc_words(const void* p, int64_t bytes) {
    i32x4 r;
    r[0] = (int)(uint32_t)(uintptr_t)p;
    r[1] = (int)((uint32_t)((uintptr_t)p >> 32) & 0xffffu);
    r[2] = (int)(CLAMP ? clamp_u32(bytes) : (uint32_t)bytes);
    r[3] = RSRC_WORD3;
    return r;
}

// ---- LDS-DMA pieces: 64 lanes x 16 B from buffer(rsrc) + soff + voff[lane] to LDS at M0 + 16 * lane.
// Issued from inline asm ON PURPOSE: hipcc (ROCm 7.2) puts `s_waitcnt vmcnt(0)` in front of the first
// ds_read that follows a compiler-visible LDS-DMA (it cannot prove the two do not alias), which would
// serialise the prefetch of K-step k+1 with the MFMAs of K-step k. The asm form is invisible to that
// pass; completion is waited for by hand (vm_wait) before the barrier that publishes the stage.
// M0 (LDS base of the DMA) is written in the same statement; s_nop covers the M0->VMEM (and, in dma16, the SGPR->VMEM)
// wait states that hipcc does not pad inside an asm string.

// M0 saved and restored: for kernels in which the compiler may keep M0 live around the piece.
__device__ __forceinline__ void dma16(i32x4 rsrc, uint32_t voff, uint32_t lds_addr) {
    uint32_t keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %3\n\t"
        "s_nop 4\n\t"
        "buffer_load_dwordx4 %1, %2, 0 offen lds\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(voff), "s"(rsrc), "s"(lds_addr)
        : "memory");
}
// Destination in a register (M0 is not live across statements in the kernels that use the forms from here on).
__device__ __forceinline__ void dma16_to(buf_rsrc rsrc, uint32_t voff, uint32_t soff, uint32_t lds_addr) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %1, %3 offen lds"
                 :: "v"(voff), "s"(rsrc), "s"(lds_addr), "s"(soff) : "memory");
}
// Destination = immediate DST + the wave's offset `wvoff` (an SGPR), for kernels whose LDS starts at 0 (require_lds_base_zero);
// BYTES per lane: 16, or 4 (64 lanes x 4 B to M0 + 4 * lane).
template <int DST, int BYTES = 16>
__device__ __forceinline__ void dma_imm_at(i32x4 rsrc, uint32_t voff, uint32_t soff, uint32_t wvoff) {
    static_assert(BYTES == 16 || BYTES == 4, "one dwordx4 or one dword per lane");
    if constexpr (BYTES == 16)
        asm volatile("s_add_u32 m0, %3, %4\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %0 offen lds"
                     :: "s"(soff), "v"(voff), "s"(rsrc), "s"(wvoff), "n"(DST) : "memory", "scc");
    else
        asm volatile("s_add_u32 m0, %3, %4\n\ts_nop 0\n\tbuffer_load_dword %1, %2, %0 offen lds"
                     :: "s"(soff), "v"(voff), "s"(rsrc), "s"(wvoff), "n"(DST) : "memory", "scc");
}
// The same piece with its scalar source offset in an SGPR of its own that advances by `inc` for the piece's next stage right
// after use — written a whole stage before it is read again, so no hazard padding. LOAD / ADVANCE = false are k_syrk4's lab
// forms (the piece without its buffer_load; the source pinned in place).
template <int DST, bool LOAD = true, bool ADVANCE = true>
__device__ __forceinline__ void dma16_imm(i32x4 rsrc, uint32_t voff, uint32_t& soff, uint32_t inc, uint32_t wvoff) {
    if constexpr (LOAD && ADVANCE)
        asm volatile("s_add_u32 m0, %3, %4\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %0 offen lds\n\ts_add_u32 %0, %0, %5"
                     : "+s"(soff) : "v"(voff), "s"(rsrc), "s"(wvoff), "n"(DST), "s"(inc) : "memory", "scc");
    else if constexpr (LOAD)
        asm volatile("s_add_u32 m0, %3, %4\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %0 offen lds"
                     : "+s"(soff) : "v"(voff), "s"(rsrc), "s"(wvoff), "n"(DST) : "memory", "scc");
    else
        asm volatile("s_add_u32 m0, %1, %2\n\ts_nop 0\n\ts_add_u32 %0, %0, %3"
                     : "+s"(soff) : "s"(wvoff), "n"(DST), "s"(inc) : "memory", "scc");
}

// ---- the three bf16 terms of an fp32 value: hi = bf16(v), mid = bf16(v - hi), lo = bf16(v - hi - mid), every conversion
// round-to-nearest-even and every subtraction exact, so hi + mid + lo = v to 24 bits. The packed form (four values: one
// v_cvt_pk_bf16_f32 per pair and term, out[t] = term t of the four) and the scalar form compute the same three terms.
__device__ __forceinline__ void split3(f32x4 v, u32x2 (&out)[3]) {
    f32x2 a0 = {v[0], v[1]}, a1 = {v[2], v[3]};
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const bf16x2 h0 = __builtin_convertvector(a0, bf16x2);
        const bf16x2 h1 = __builtin_convertvector(a1, bf16x2);
        out[t].x = __builtin_bit_cast(uint32_t, h0);
        out[t].y = __builtin_bit_cast(uint32_t, h1);
        if (t < 2) {
            a0 = a0 - __builtin_convertvector(h0, f32x2);
            a1 = a1 - __builtin_convertvector(h1, f32x2);
        }
    }
}
__device__ __forceinline__ void split3(float v, uint16_t (&pl)[3]) {
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const uint16_t b = f32_to_bf16_bits(v);
        pl[t] = b;
        v = v - bf16_bits_to_f32(b);
    }
}
// four values split and written as 8-byte quadruples to the three planes of an LDS panel (PLANE_BYTES apart)
template <int PLANE_BYTES> __device__ __forceinline__ void split3_store(f32x4 v, LDS_AS char* plane0, int off) {
    u32x2 out[3];
    split3(v, out);
#pragma unroll
    for (int t = 0; t < 3; ++t) *(LDS_AS u32x2*)(plane0 + t * PLANE_BYTES + off) = out[t];
}

}  // namespace llmc
