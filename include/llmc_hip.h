/*
 * llmc_hip.h — C ABI of libllmc_hip.so: the MI355X (gfx950) implementation of llmc's per-Linear
 * weight-quantization hot path (GPTQ / AWQ / RTN quantizer arithmetic, packing).
 *
 * Conventions:
 *   - every pointer is a DEVICE pointer unless the name ends in `_host`;
 *   - the library never allocates or frees device memory: callers pass outputs and a workspace whose
 *     size comes from the matching `*_ws_bytes` query;
 *   - every entry point takes the hipStream_t to launch on (as void*) and never synchronises the device;
 *   - return value: 0 ok; LLMC_EINVAL bad shape/dtype/alignment; LLMC_ENOTSUP unsupported combination;
 *     LLMC_EIO a HIP runtime error (text via llmc_hip_last_error). No C++ exception crosses the ABI;
 *   - dtype codes: LLMC_F16 / LLMC_BF16 / LLMC_F32. "Tensor dtype" arithmetic follows ATen's rule the
 *     reference relies on: every elementwise op is evaluated in fp32 and rounded (RNE) to the op's
 *     result dtype, no FMA contraction, IEEE division.
 *
 * Each entry cites the reference code (paths relative to the llmc tree) it replaces.
 */
#ifndef LLMC_HIP_H_
#define LLMC_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LLMC_HIP_ABI_VERSION 1

#define LLMC_OK 0
#define LLMC_EINVAL (-22)
#define LLMC_ENOTSUP (-95)
#define LLMC_EIO (-5)

#define LLMC_F16 0
#define LLMC_BF16 1
#define LLMC_F32 2
#define LLMC_F64 3 /* llmc_hadamard only */
/* OR-ed into the dtype code of llmc_quant_static's scales / zeros: the operand is a 0-dim tensor in the reference
 * (per_tensor qparams): it is used at its own precision but ATen leaves it out of type promotion, so every op still
 * rounds to the weight dtype (quant.py:699-717 with the 0-dim scales of quant.py:132-136,555-556). */
#define LLMC_SCALAR_QPARAM 16
/* OR-ed into llmc_quant_static's zdt: round_zp = False (quant.py:557-558, 702-707): the zero point is not an integer and
 * the code is clamp(round(x / max(s, 1e-9) + z)) instead of clamp(round(x / s) + z). */
#define LLMC_FRACTIONAL_ZP 32

/* integer code container for llmc_quant_static / llmc_quant_dynamic */
#define LLMC_OUT_FAKE 0 /* dequantised values, written in the weight dtype              */
#define LLMC_OUT_I32 1  /* int32 codes   (reference: bit != 8  -> torch.int32)          */
#define LLMC_OUT_I8 2   /* int8 codes    (reference: bit == 8, qmin != 0 -> torch.int8) */
#define LLMC_OUT_U8 3   /* uint8 codes   (reference: bit == 8, qmin == 0 -> torch.uint8)*/

typedef void* llmc_stream_t; /* hipStream_t */

int llmc_hip_abi_version(void);
/* hash (16 hex digits) of the sources and compiler flags the library was built from; the Python loader recomputes it from
 * the sources next to the .so and refuses a stale library (llmc_amd/build.py:source_digest, llmc_amd/_ffi.py:lib) */
const char* llmc_hip_build_id(void);
/* copies the last HIP error string of the calling thread into buf (NUL-terminated); returns its length */
int llmc_hip_last_error(char* buf_host, size_t n);

/* Per calling-thread switch: may llmc_chol_inv_upper / llmc_gptq_quantize use an internal low-priority helper stream
 * to overlap their large trailing updates with their latency-bound chains (default 1)? A caller that already runs
 * several of them side by side on its own streams (the subsets of a block) turns it off for all but the longest
 * chain: every entry point still completes, in stream order, on the stream it was given. Returns the previous value.
 * No reference counterpart (the reference runs one default stream). */
int llmc_hip_set_helper_streams(int enable);

/* Per calling-thread: the Hessian kernel (llmc_hessian_accum*) is persistent, one workgroup per compute unit, and a
 * workgroup owns its CU (all VGPRs, 128 KiB LDS). n_cus > 0 makes it leave that many CUs (rounded up to a multiple of
 * 8, one per XCD) to kernels the caller runs on other streams meanwhile; 0 (default) = the whole device. Returns the
 * previous value. No reference counterpart. */
int llmc_hip_set_cu_reserve(int n_cus);

/* Explicit A/B switches, per calling thread, all 0 by default. The library reads NO environment variable: what used to be
 * LLMC_* variables (rounds 2-5) are these keys. Every value produces valid results; "same bits" = bit-identical to the default.
 *   k3_fp32           K3's large products on the fp32 MFMA pipe instead of split-bf16 (other rounding, same accuracy class)
 *   k3_no_gemm6       deep levels of the triangular inverse on k_gemm3 instead of gemm6 (other rounding)
 *   k3_no_planes      K3's far updates split inside every tile (k_gemm3) instead of pre-split planes + k_gemm3s; same bits
 *   k3_split_far      without a helper stream, an outer block's far update as two launches instead of one; same bits
 *   k4_split_far      without helper streams, a column group's far update as three launches instead of one; same bits
 *   k4_err_rowmajor   the column loop's error columns row-major instead of k-major; same bits
 *   gptq_generic      k_gptq_block: every wave on the generic IEEE-division path; same bits
 *   gemm3_nospec      never k_gemm3s; same bits.   gemm3s_min_tiles = n > 0: its tile-count threshold (tests)
 *   no_shortk         short products through the general fp32 GEMM; same bits
 *   linear_nosplit    the k-tiled GEMM never cuts a small product into k-slices (single pass: the row-major kernel's bits)
 *   fp8_exact_div     FP8 casts through the IEEE division + general encoder; same bits
 *   side_cu_mask      helper streams created with a CU mask (read when a caller stream's helper set is first created)
 *   k1_batch_off      llmc_hessian_accum_multi as one launch per problem instead of one tile queue; same bits
 *   k1_fp32_diag      diag(H) as the MFMA kernel's fp32 chain leaves it instead of the fp64-folded one (other diagonal)
 *   fp8_no_packed16   FP8 e4m3 cast of bf16 tensors (qtorch rounding, codes out): the float form of the division-free path; same bits
 *   gemm3s_no_dma     k_gemm3s (planes form): producer waves copy through registers instead of LDS-DMA; same bits
 *   gemm3_no_wide     K3's far updates on k_gemm3s instead of k_gemm3w (128 x 128 tiles, two workgroups per CU); same bits
 *   sgemm_no_wide     K4's far update: 1 = on k_sgemm (the kernel of rounds 2-5), 4 = k_sgemm_wide's 256 x 128 form (one workgroup
 *                     per CU) instead of its 128 x 128 form (two per CU, the default); same bits
 *   no_riders         without helper streams, a column group's far update as one launch over all later columns; default: the
 *                     128 x 128 tiles of its last columns ride on the next group's in-block launches instead (k_gptq_block_riders,
 *                     one tile per CU the chain leaves free); same bits
 *   kv_sink_max_grid  n > 0: llmc_kv_sink_update launches at most n blocks per tensor and grid-strides the rest (tests); same bits
 *   block_influence_max_grid  n > 0: llmc_block_influence's row kernel launches at most n blocks and grid-strides the rest (tests);
 *                     same bits
 * set: returns the previous value, or LLMC_EINVAL for an unknown key / negative value. get: the value, or LLMC_EINVAL.
 * option_name: the key of index 0, 1, ... (copied into buf), LLMC_EINVAL past the last one. No reference counterpart. */
int llmc_hip_set_option(const char* key, int value);
int llmc_hip_get_option(const char* key);
int llmc_hip_option_name(int index, char* buf_host, size_t n);

/* ------------------------------------------------------------------------------------------------
 * Quantizer arithmetic (llmc/compression/quantization/quant.py)
 * ---------------------------------------------------------------------------------------------- */

/* get_minmax_range + get_qparams (quant.py:132-143, 545-559) on a [G, g] view (reshape_tensor,
 * quant.py:612-642: per_group -> g = group_size, per_channel -> g = in_features, per_tensor -> G = 1).
 * scales / zeros: [G] in the tensor dtype `dt`. zeros may be NULL when sym (reference returns 0).
 * round_zp = 1 is the reference default; 0 gives zeros = qmin - min/scale. */
size_t llmc_minmax_qparams_ws_bytes(int64_t G, int64_t g);
int llmc_minmax_qparams(const void* W, int dt, int64_t G, int64_t g, int sym, int round_zp,
                        float qmin, float qmax, void* scales, void* zeros, void* ws,
                        llmc_stream_t stream);

/* calib_algo 'static_hist', data pass (quant.py:462-512): torch.histc(sample.float(), bins, min, max) -> out fp32 [bins]
 * counts; bin = int((x - min) * bins / (max - min)) in fp32, the right edge belongs to the last bin, values outside the
 * range are dropped, min == max widens the range by one on both sides (ATen). ws: llmc_histc_ws_bytes(bins). The merge
 * of the per-sample histograms and the range search (quant.py:279-460) work on `bins` numbers and stay host code. */
/* Per-sample min / max of n <= llmc_minmax_samples_max() calibration samples in one launch pair: what `sample.min()`,
 * `sample.max()` give for every sample in get_minmax_stats / get_moving_minmax / the first pass of the histogram observer
 * (quant.py:253-263, 524-543, 462-475). X_list_host[i]: device address of sample i (16-B aligned, its own allocation),
 * len_list_host[i] its element count; both arrays live on the HOST (they travel in the kernel arguments). mn / mx: fp32 [n]
 * on the device (the values are elements of the samples, exact in fp32); a NaN in a sample makes both of its results NaN,
 * like torch. ws: llmc_minmax_samples_ws_bytes(len_list_host, n). */
int llmc_minmax_samples_max(void);
size_t llmc_minmax_samples_ws_bytes(const int64_t* len_list_host, int n);
int llmc_minmax_samples(const void* const* X_list_host, const int64_t* len_list_host, int n, int dt, float* mn, float* mx,
                        void* ws, llmc_stream_t stream);

size_t llmc_histc_ws_bytes(int bins);
int llmc_histc(const void* x, int dt, int64_t n, int bins, float min, float max, float* out, void* ws,
               llmc_stream_t stream);

/* calib_algo 'mse': BaseQuantizer.get_mse_range (quant.py:145-203) followed by get_qparams (:545-559) on a [G, g]
 * view. The reference casts the tensor to fp32 first, so ranges and qparams are fp32 whatever `dt` is:
 * scales / zeros / min_out / max_out are fp32 [G] (zeros may be NULL when sym, min_out / max_out may be NULL).
 * nsteps = int(maxshrink * mse_grid) and grid = mse_grid as Python computes them; norm = 2.4 in the reference. */
int llmc_mse_qparams(const void* W, int dt, int64_t G, int64_t g, int sym, int round_zp, float qmin, float qmax,
                     int nsteps, int grid, float norm, float* scales, float* zeros, float* min_out, float* max_out,
                     llmc_stream_t stream);
/* The same search on the groups of a strided fp32 panel, in place: W[r, c0 : c0 + width] for r < R, row stride ld
 * (elements, ld >= c0 + width). Group j covers panel columns [j * group_size, min((j + 1) * group_size, width)): the last
 * group may be ragged. Each (row, group) gives bit for bit what llmc_mse_qparams gives on a contiguous fp32 copy of that
 * group. Results: scales / zeros fp32 [R, ng] at [r * ng + g0 + j] (zeros may be NULL when sym; ng >= g0 + groups).
 * group_size in {16, 32, 64, 128}, others LLMC_ENOTSUP. GPTQ's column loop with calib_algo 'mse' runs it per block. */
int llmc_mse_qparams_panel(const float* W, int64_t R, int64_t ld, int64_t c0, int64_t width, int64_t group_size, int sym,
                           int round_zp, float qmin, float qmax, int nsteps, int grid, float norm, float* scales,
                           float* zeros, int64_t ng, int64_t g0, llmc_stream_t stream);

/* calib_algo 'hqq' / method HQQ: optimize_weights_proximal (quant.py:588-610, hqq.py:36-60) after get_tensor_qparams
 * (quant.py:680-697) on the weight W [R, K] (row stride ld >= K elements, dtype dt), in place: no transposed copy.
 * axis 1 groups g consecutive elements of a row (group r * (K / g) + k / g); axis 0 groups g consecutive rows of one column
 * (the reference's W.T reshaped: group k * (R / g) + r / g). g = group_size in {16, 32, 64, 128} dividing the grouped
 * dimension, anything else LLMC_ENOTSUP. The start is get_qparams of the group's min / max in fp32 (bit for bit
 * llmc_minmax_qparams on W.float()), or the given s_in / z_in (fp32 [G], group order; z_in NULL = 0) when s_in is not NULL.
 * Each iteration, in fp32 with one rounding per op: q = clamp(round(W * inv + z)), W_r = (q - z) / inv (inv = 1 / s; quant.py:593-598), the shrink
 * sign(d) * relu(|d| - c * |d|^p1) (lp_norm_one: relu(|d| - c)), c = fp32(1 / beta) computed in double, p1 = fp32(lp_norm - 1),
 * pow evaluated in fp64 and rounded once; the new zero is the group mean in ATen's CPU inner-sum order. The error of an
 * iteration is mean |W - W_r| over the tensor, summed in fp64 in a fixed order and rounded to fp32; the first iteration
 * whose error is not below the best stops the loop and its zeros are returned (beta's decay by kappa has no effect in the
 * reference: its shrink reads self.beta). Outputs: scales = 1 / (1 / s), zeros, fp32 [G] in group order; errs (optional,
 * fp64 [iters]) the per-iteration mean errors up to the stop; t_out (optional, int32 [1]) the stop iteration (iters - 1
 * when the loop runs out, -1 when iters == 0). Stream-ordered, no host synchronisation. ws: llmc_hqq_ws_bytes. */
size_t llmc_hqq_ws_bytes(int64_t R, int64_t K, int axis, int64_t group_size, int iters);
int llmc_hqq_optimize(const void* W, int dt, int64_t R, int64_t K, int64_t ld, int axis, int64_t group_size, int sym,
                      int round_zp, float qmin, float qmax, const float* s_in, const float* z_in, float c, float p1,
                      int lp_norm_one, int iters, float* scales, float* zeros, double* errs, int* t_out, void* ws,
                      llmc_stream_t stream);

/* IntegerQuantizer.quant / quant_dequant with given qparams (quant.py:699-717), i.e. the arithmetic of
 * fake_quant_weight_static (quant.py:785-831) and real_quant_weight_static (quant.py:871-914).
 * W: [G, g] dtype wdt. scales [G] dtype sdt. zeros [G] dtype zdt, or NULL (== 0, the symmetric case).
 * out_kind LLMC_OUT_FAKE writes (q - z) * s cast to wdt; the others write integer codes.
 * Promotion follows torch: x/s in promote(wdt,sdt); +z in promote(.,zdt); rounding after each op. */
int llmc_quant_static(const void* W, int wdt, int64_t G, int64_t g, const void* scales, int sdt,
                      const void* zeros, int zdt, float qmin, float qmax, int out_kind, void* out,
                      llmc_stream_t stream);

/* fake_quant_weight_dynamic (quant.py:833-869) / real_quant_weight_dynamic (quant.py:916-953):
 * min/max -> qparams -> quant(-> dequant) in one pass over W. scales_out / zeros_out may be NULL
 * (fake path does not keep them); when given they are [G] in dtype dt. */
size_t llmc_quant_dynamic_ws_bytes(int64_t G, int64_t g);
int llmc_quant_dynamic(const void* W, int dt, int64_t G, int64_t g, int sym, int round_zp, float qmin,
                       float qmax, int out_kind, void* out, void* scales_out, void* zeros_out, void* ws,
                       llmc_stream_t stream);

/* VllmRealQuantLinear.pack (module_utils.py:836-862): codes [R, K] (int32 or int8 container) ->
 * packed int32 [R, ceil(K / (32/bits))]; u = (code + 2^(bits-1)) & 0xff, LSB-first nibbles/bytes,
 * zero padding on the right. code_kind is LLMC_OUT_I32 or LLMC_OUT_I8. */
int llmc_pack_lsb(const void* codes, int code_kind, int64_t R, int64_t K, int bits, int32_t* packed,
                  llmc_stream_t stream);

/* AutoawqRealQuantLinear.gemm_pack (module_utils.py:1004-1065): recompute codes
 * round((w + z*s) / s) in fp16 from weight [R, K] (f16), scales/zeros [R, K/g] as returned by
 * real_quant_weight_* (scales any float dtype -> cast to f16, zeros int32), transpose to [K, R] and
 * pack 8 nibbles per int32 along R with AWQ's order map [0,2,4,6,1,3,5,7].
 * qweight [K, R/8] int32, qzeros [K/g, R/8] int32, scales_out [K/g, R] f16. */
int llmc_pack_awq_gemm(const void* weight, int wdt, const void* scales, int sdt, const int32_t* zeros,
                       int64_t R, int64_t K, int64_t g, int32_t* qweight, int32_t* qzeros,
                       void* scales_out_f16, llmc_stream_t stream);

/* FloatQuantizer weight / activation path, e4m3 and e5m2 (quant.py:963-1003, 1043-1072, 1161-1221):
 * scale = absmax.clamp(1e-5) / finfo(float8 type).max (448 / 57344) per row of the [G, g] view (G = 1 per-tensor, G = R
 * per-channel / per-token), q = float_quantize(x / scale, e_bits, m_bits, 'nearest'). `fake` is a flag word:
 *   bit 0      write dequantised q * scale in dt to `out` instead of 8-bit codes
 *   bits 4-5   format: 0 = e4m3, 1 = e5m2 (quant.py:983-984, 1162-1163)
 *   bit 8      rounding semantics: 1 = qtorch.quant.float_quantize as llmc calls it (third-party, not vendored by the
 *              reference: QPyTorch 0.3.0's published CPU algorithm restated in csrc/fp8_math.h and oracle/quant_ref.py —
 *              IEEE-style formats, ties away from zero, saturation at 240 / 57344); 0 = torch's dtype cast
 *              (.to(torch.float8_e4m3fn / float8_e5m2): round to nearest even, OCP e4m3fn up to 448), which is what
 *              the reference's real-quant path ends in (quant.py:1183, 1211) and what its Triton kernels compute.
 *   bit 9      evaluate every element with the IEEE division and the general encoder. Results are identical with and
 *              without it: 16-bit e4m3 calls otherwise use w * fl(1 / scale) and send only the lanes near a rounding
 *              boundary (or outside the 8-bit format's normal range) through the division (tests/test_fp8_fast_gpu.py).
 *   bit 11     dynamic scales only: write back the scale as get_qparams forms it (quant.py:545-553) — one that underflows
 *              in fp16 stays 0 — instead of the value quant() leaves in place (`scales[scales == 0] = 1`, quant.py:1062).
 *              The elements are quantized with 1 either way. For get_tensor_qparams, which never reaches quant().
 * Codes are OCP e4m3fn / IEEE e5m2 bytes in both cases (every qtorch result is representable). scales [G] in dtype sdt:
 * ATen yields fp32 for the 0-dim per-tensor scale and the tensor dtype for per-channel.
 * static_scales != 0: `scales` is INPUT (fake_quant_act_static / real_quant_weight_static, quant.py:1083-1099). */
size_t llmc_fp8_quant_ws_bytes(int64_t G, int64_t g);
int llmc_fp8_quant(const void* W, int dt, int64_t G, int64_t g, int fake, void* out, void* scales, int sdt,
                   int static_scales, void* ws, llmc_stream_t stream);

/* FloatQuantizer on the narrow float grids (quant.py:963-1003 with qmax = tensor(6) / tensor(28), 1061-1081), one pass:
 * per row of the [G, g] view  absmax -> scale -> t = rnd_dt(w / scale) + 0 -> rounding onto the grid -> q * scale or a code.
 *   e2m1 (FP4): s ee m, bias 1, OCP values 0, 0.5, 1, 1.5, 2, 3, 4, 6;   e3m2 (FP6): s eee mm, bias 3, OCP max 28, smallest
 *   normal 0.25, subnormal step 0.0625. Neither has an infinity or a NaN.
 * `mode` is a flag word:
 *   bit 0      write dequantised q * scale in dt to `out` (fp32 product, one rounding) instead of one code per byte (the low
 *              4 / 6 bits, sign on top, the rest zero)
 *   bits 4-5   format: 2 = e2m1, 3 = e3m2 (0 / 1 are llmc_fp8_quant's; here they return LLMC_ENOTSUP)
 *   bit 8      rounding semantics: 0 = qtorch.quant.float_quantize(x, 2, 1) / (x, 3, 2) as the reference calls it (restated
 *              in csrc/fp8_math.h, see llmc_fp8_quant): ties away from zero, the top exponent code kept for infinity, so the
 *              largest value is 3 / 14 although the scale maps the row to +-6 / +-28 — 11 of e2m1's 15 levels; a zero
 *              result is +0. 1 = 'ocp': round to nearest even onto the OCP grid, subnormals included, saturating at +-6 /
 *              +-28 (infinities too); a NaN gives the maximum with the input's sign; the sign survives on a zero result.
 *   bit 9      scales are e8m0 bytes (OCP MX; with bit 8 only, else LLMC_ENOTSUP): code = clamp(floor(log2(absmax)) - emax
 *              + 127, 0, 254) with emax = 2 (e2m1) / 4 (e3m2), 127 for an all-zero row; scale = 2^(code - 127); the division
 *              is exact, so the quotient is not rounded to dt. `scales` is then uint8 [G] and sdt is ignored. Dynamic e8m0
 *              scales need rows the resident kernels take (below), else LLMC_ENOTSUP.
 *   bit 11     dynamic scales: write back get_qparams' own value (an underflowed scale stays 0), as in llmc_fp8_quant.
 * Other bits: LLMC_ENOTSUP. Dtype scales: absmax.clamp(1e-5) / qmax rounded to sdt; a zero scale quantizes with 1. The
 * reference's qmax is an INTEGER 0-dim tensor here, so the 0-dim per-tensor absmax / qmax keeps the tensor dtype (the FP8
 * formats' float qmax promotes it to fp32): callers pass sdt = dt for every granularity.
 * cols (may be null): [K] multipliers in dt for a 2-D weight [G * g / K, K] whose rows are split into groups (K % g == 0):
 * the element is first rnd_dt(w * cols[k]) — bit for bit llmc_mul_cols followed by the call without cols; W is not written.
 * Rows of at most 16384 elements (a multiple of the 16-byte vector, 16-B aligned W / out / cols) are read from HBM once:
 * the row waits in registers (g = vector x a power of two <= 64 lanes) or LDS between the reduction and the rounding.
 * Everything else takes llmc_minmax_qparams + a second read (ws of llmc_fpx_quant_ws_bytes, dynamic scales only; cols are
 * then LLMC_ENOTSUP unless the scales are static). */
size_t llmc_fpx_quant_ws_bytes(int64_t G, int64_t g);
int llmc_fpx_quant(const void* W, int dt, int64_t G, int64_t g, const void* cols, int64_t K, int mode, void* out,
                   void* scales, int sdt, int static_scales, void* ws, llmc_stream_t stream);

/* e2m1 codes [R, K] (one per byte, K even) -> [R, K / 2] bytes: element 2i in the low nibble, 2i + 1 in the high one (the
 * float4_e2m1fn_x2 / MX convention). */
int llmc_fp4_pack(const void* codes, int64_t R, int64_t K, void* packed, llmc_stream_t stream);

/* The stored form back to numbers: out[G, g] (odt) = decode(code) * scale[row] — an fp32 product rounded once, the
 * arithmetic of llmc_fpx_quant's fake output. fmt 2 = e2m1 (packed != 0: two codes per byte as llmc_fp4_pack writes them),
 * 3 = e3m2 (one code per byte only; dense FP6 packing is not provided). sdt: the scales' float dtype, or -1 for e8m0 bytes. */
int llmc_fpx_dequant(const void* codes, int fmt, int packed, const void* scales, int sdt, int64_t G, int64_t g, void* out,
                     int odt, llmc_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * GPTQ (llmc/compression/quantization/gptq.py)
 * ---------------------------------------------------------------------------------------------- */

/* GPTQ.add_batch (gptq.py:254-295):  H <- H * (n_before / n_after) + (2 / n_after) * X^T X
 * X: [T, K] tokens x channels (row stride ldx elements), 16-bit dtype dt (F16 / BF16); H: [K, K] fp32,
 * full symmetric on output. n_before / n_after are the reference's `nsamples` before and after the call
 * (counts of sequences, not tokens). Products are exact (16-bit x 16-bit in fp32), accumulation is fp32
 * on the MFMA pipe in a fixed, launch-independent order (deterministic). */
size_t llmc_hessian_accum_ws_bytes(int64_t T, int64_t K, int64_t ldx);
int llmc_hessian_accum(float* H, const void* X, int dt, int64_t T, int64_t K, int64_t ldx,
                       double n_before, double n_after, void* ws, llmc_stream_t stream);
/* The two launches of llmc_hessian_accum, separately (same ws): the MFMA kernel that writes per-unit
 * partial tiles, and the ordered reduction that folds them into H. Used by bench.py to time the MFMA
 * kernel alone with HIP events, and by callers that overlap the reduction with other work. */
int llmc_hessian_accum_partials(const void* X, int dt, int64_t T, int64_t K, int64_t ldx, void* ws,
                                llmc_stream_t stream);
int llmc_hessian_accum_reduce(float* H, int64_t T, int64_t K, int64_t ldx, double n_before, double n_after,
                              const void* ws, llmc_stream_t stream);

/* The same update from a LIST of samples that stay where they are (no staging copy): llmc's hooks call add_batch once
 * per calibration sample (calib.bs = 1, configs/quantization/methods/GPTQ/gptq_w_only.yml:12 -> 128 calls of
 * [1, 2048, K] per layer, gptq.py:254-295); a caller that keeps those tensors resident passes their addresses here and
 * gets ONE launch and ONE reduction for all of them:  X^T X = sum_i X_i^T X_i,  n_after - n_before = the number of
 * sequences in the list. X_list_host / T_list_host: HOST arrays of n device pointers (16-B aligned rows, common row
 * stride ldx and dtype dt) and their token counts (> 0; any lengths: every sample is walked in 128-token groups and
 * the last group of a sample is zero-filled by its buffer descriptor). n <= llmc_hessian_max_samples(). The host arrays
 * are consumed before the call returns (they travel in the kernel arguments: up to 8 KiB of them). The result is bit-identical to
 * llmc_hessian_accum on the concatenation of the samples whenever every T_i is a multiple of 128. ws from
 * llmc_hessian_accum_ptrs_ws_bytes (0 = invalid arguments). */
int llmc_hessian_max_samples(void);
size_t llmc_hessian_accum_ptrs_ws_bytes(const int64_t* T_list_host, int n, int64_t K, int64_t ldx);
int llmc_hessian_accum_ptrs(float* H, const void* const* X_list_host, const int64_t* T_list_host, int n, int dt,
                            int64_t K, int64_t ldx, double n_before, double n_after, void* ws, llmc_stream_t stream);
int llmc_hessian_accum_ptrs_partials(const void* const* X_list_host, const int64_t* T_list_host, int n, int dt,
                                     int64_t K, int64_t ldx, void* ws, llmc_stream_t stream);
int llmc_hessian_accum_ptrs_reduce(float* H, const int64_t* T_list_host, int n, int64_t K, int64_t ldx,
                                   double n_before, double n_after, const void* ws, llmc_stream_t stream);
/* Several Hessians in ONE launch pair (one unit queue): the problems' triangular tile grids fill the persistent grid's
 * rounds together — the three K = 4096 inputs of a Llama block pay one partially filled last round instead of three — and
 * the exact diagonal below. A problem = one llmc_hessian_accum_ptrs call: H [K, K], its sample list (host arrays of n device
 * pointers / token counts, consumed before the call returns), K, the common row stride ldx, the running-mean weights.
 * Up to llmc_hessian_max_problems() problems and llmc_hessian_max_samples() samples (all problems together) per call; one
 * dtype per call. The one-problem entry points above are wrappers of these (dstate = NULL).
 *
 * Exact diagonal (always on; no extra pass over the samples): in a DIAGONAL 256 x 256 tile of the kernel the upper-right
 * quadrant is the transpose of the lower-left one, so the reduction mirrors that one and the quadrant's wave spends its
 * MFMAs on the eight 32 x 32 blocks ON the diagonal, restarting its accumulators every 2048 tokens (every 256 in short units)
 * and folding each block's diagonal into fp64. diag(H) — what actorder sorts (gptq.py:58-83) and the damping averages
 * (gptq.py:169) — then sits within 2e-7 of the exact value (an fp32 rounding is 6e-8), instead of the 2-3e-6 an fp32 chain over a
 * whole token chunk leaves (twice the reference's sgemm; rounds 1-5 offered a second fp64 pass over the samples for this). dstate [K] fp64 (may
 * be NULL) carries the unrounded running diagonal across calls (overwritten when n_before == 0); without it H's own fp32
 * diagonal is the carried value. llmc_hip_set_option("k1_fp32_diag", 1) keeps the MFMA kernel's fp32 diagonal (A/B). */
typedef struct {
    float* H;
    double* dstate;
    const void* const* X_list_host;
    const int64_t* T_list_host;
    int n;
    int64_t K;
    int64_t ldx;
    double n_before;
    double n_after;
} llmc_hessian_problem_t;
int llmc_hessian_max_problems(void);
size_t llmc_hessian_accum_multi_ws_bytes(const llmc_hessian_problem_t* probs_host, int P);
int llmc_hessian_accum_multi_partials(const llmc_hessian_problem_t* probs_host, int P, int dt, void* ws, llmc_stream_t stream);
int llmc_hessian_accum_multi_reduce(const llmc_hessian_problem_t* probs_host, int P, const void* ws, llmc_stream_t stream);
int llmc_hessian_accum_multi_barrier_timeouts(const llmc_hessian_problem_t* probs_host, int P, const void* ws, unsigned* out_host,
                                              llmc_stream_t stream);
/* Diagnostic: how many round barriers of the LAST llmc_hessian_accum*_partials launch on `ws` (same T list, K, ldx) gave
 * up waiting because workgroups of its persistent grid were kept off their CUs by other streams. Synchronises `stream`
 * and writes the count to *out_host. 0 in a healthy run; > 0 leaves the result correct but the launch slower. */
int llmc_hessian_accum_barrier_timeouts(const void* ws, const int64_t* T_list_host, int n, int64_t K, int64_t ldx,
                                        unsigned* out_host, llmc_stream_t stream);

/* GPTQ.process_hessian_and_weights, first half (gptq.py:135-152, 169-171):
 *   dead = diag(H) == 0 -> H[dead,dead] = 1, W[:,dead] = 0; optional symmetric gather by perm
 *   (Hout = H[perm][:,perm], Wout = W[:,perm]); damp = percdamp * mean(diag) ; Hout += damp * I.
 * W [R, K] dtype wdt (model dtype or f32) -> Wout [R, K] fp32. perm may be NULL (identity).
 * H is modified in place only for the dead-column fix; Hout must not alias H.
 * Hout may be NULL (only W is gathered: layers that share an input share the factor), and W/Wout may
 * both be NULL (only H is prepared). */
size_t llmc_hessian_prep_ws_bytes(int64_t K);
int llmc_hessian_prep(float* H, const void* W, int wdt, int64_t R, int64_t K, const int64_t* perm,
                      float percdamp, float* Hout, float* Wout, void* ws, llmc_stream_t stream);

/* `W = tmp[:, invperm]` after the column loop (gptq.py:186-188) and any other fp32 column gather:
 * out[r][j] = in[r][idx[j]], in/out [R, K] fp32 contiguous, K % 4 == 0, K <= 40960 (one row staged in LDS), out must not alias in. */
int llmc_gather_cols(const float* in, int64_t R, int64_t K, const int64_t* idx, float* out, llmc_stream_t stream);

/* gptq.py:172-174: cholesky -> cholesky_inverse -> cholesky(upper). Computes the same upper factor U
 * (H^-1 = U^T U) by one reverse Cholesky H = R R^T (R upper) and one triangular inverse U = R^-1, in
 * fp32. A [K, K] is overwritten by U (strict lower triangle zeroed). info_dev: int32, 0 on success,
 * i+1 if the leading minor i is not positive definite. */
size_t llmc_chol_inv_upper_ws_bytes(int64_t K);
int llmc_chol_inv_upper(float* A, int64_t K, void* ws, int32_t* info_dev, llmc_stream_t stream);
/* The two calls above without the transposing pass between them (K^2 floats read + written; 0.5 ms at K = 14336):
 * llmc_hessian_prep_rev writes Hout index-reversed (Hout[i][j] = Hp[K-1-i][K-1-j]: the same gather with the permutation read
 * backwards; workspace llmc_hessian_prep_ws_bytes), which for a symmetric H is Hp reflected across its anti-diagonal — the
 * matrix llmc_chol_inv_upper builds first. llmc_chol_inv_upper_rev factors it in place (Arev is destroyed) and writes U to
 * Uout (a separate buffer; workspace llmc_chol_inv_upper_ws_bytes). U is bit-identical to the two-call form. */
int llmc_hessian_prep_rev(float* H, const void* W, int wdt, int64_t R, int64_t K, const int64_t* perm,
                          float percdamp, float* Hout, float* Wout, void* ws, llmc_stream_t stream);
int llmc_chol_inv_upper_rev(float* Arev, float* Uout, int64_t K, void* ws, int32_t* info_dev, llmc_stream_t stream);

/* GPTQ.weight_transform (gptq.py:199-244), the blocked column loop, with the quantizer of
 * search_column_qparams (gptq.py:359-366) fused at group starts.
 *   W      [R, K] fp32, (already permuted / dead-fixed), overwritten with the running updated weights
 *   Hinv   [K, K] fp32 upper factor U
 *   Wout   [R, K] fp32 = `tmp`: the error-compensated weight of each column at the time it was visited
 *   losses [R, K] fp32 = `Losses` (may be NULL)
 *   group_size: 0 = per_channel (one qparam pair per row, given in scales/zeros), else group size
 *   static_groups = 0: qparams re-derived from the current W at each group start and written to
 *     scales/zeros [R, K/group_size] (fp32) in processing (permuted) order;
 *   static_groups = 1: scales/zeros [R, K/group_size] are INPUT in original column order and
 *     col_group[i] (int32 [K], = perm[i]/group_size) selects the group of processed column i.
 *   sym: zeros ignored on input when static and sym (zero == 0).
 * blocksize must be 128 (the reference default in every shipped GPTQ config). */
size_t llmc_gptq_quantize_ws_bytes(int64_t R, int64_t K);
int llmc_gptq_quantize(float* W, const float* Hinv, int64_t R, int64_t K, int sym, float qmin,
                       float qmax, int64_t group_size, int static_groups, const int32_t* col_group,
                       float* scales, float* zeros, float* Wout, float* losses, int blocksize,
                       void* ws, llmc_stream_t stream);
/* OWQ form of the same loop (gptq.py:44-56, 66-83, 199-244 with n_nonout < columns): only the first n_quant columns are
 * visited; the trailing K - n_quant columns (kept in floating point) still receive every block's error feedback.
 * Dynamic groups are clipped at n_quant like `min(i + group_size, columns - n_out)` (gptq.py:216-221). */
int llmc_gptq_quantize_cols(float* W, const float* Hinv, int64_t R, int64_t K, int64_t n_quant, int sym, float qmin,
                       float qmax, int64_t group_size, int static_groups, const int32_t* col_group,
                       float* scales, float* zeros, float* Wout, float* losses, int blocksize,
                       void* ws, llmc_stream_t stream);
/* The same loop (arguments as llmc_gptq_quantize_cols) for a FloatQuantizer weight quantizer with use_qtorch (quant.py:963-1081;
 * the shipped gptq_fp8.yml): every visited column is rounded to an FP8 grid instead of an integer grid,
 *   q = float_quantize(w / s + 0, E, M, 'nearest') * s      with s = 1 where s == 0 (quant.py:1062),
 * fmt 0 = e4m3 (E, M = 4, 3; qtorch saturates at 240), 1 = e5m2 (5, 2; 57344); another fmt returns LLMC_ENOTSUP. The quantizer
 * is symmetric: there are no zero points.
 *   W      [R, K] fp32, overwritten with the running updated weights (columns from n_quant on: every block's feedback applied)
 *   Wout   [R, K] fp32 = `tmp`, losses [R, K] fp32 or NULL: written for the first n_quant columns
 *   group_size = 0 (per_channel): scales [R] fp32 is INPUT (a 16-bit scale promoted to fp32 is exact);
 *   static_groups = 1: scales [R, K/group_size] INPUT in original column order, col_group as above;
 *   static_groups = 0: group_size in {16, 32, 64, 128} (others LLMC_ENOTSUP); scales [R, ceil(K / group_size)] is OUTPUT in
 *     processing order, s = max(|min|, |max|).clamp(1e-5) / finfo(fmt).max of the group at its start (quant.py:545-553); groups the
 *     loop never visits (n_quant < K) keep their input values.
 * ws: llmc_gptq_quantize_ws_bytes(R, K) bytes, 256-B aligned. Runs on `stream`, complete in stream order; allocates nothing. */
int llmc_gptq_quantize_fp8_cols(float* W, const float* Hinv, int64_t R, int64_t K, int64_t n_quant, int fmt,
                                int64_t group_size, int static_groups, const int32_t* col_group, float* scales,
                                float* Wout, float* losses, int blocksize, void* ws, llmc_stream_t stream);
/* The same loop (n_quant as in llmc_gptq_quantize_cols) with calib_algo 'mse' dynamic groups: the qparams of a group
 * are searched (get_mse_range, as llmc_mse_qparams_panel) on W[:, i : min(i + group_size, n_quant)] as it stands when
 * the 128-column block holding column i begins, the values the reference's search sees (gptq.py:216-221). Once per
 * block, on `stream`, the groups starting in the block are searched, then the block runs with those qparams.
 * Outputs as for static_groups = 0: scales / zeros [R, ceil(K / group_size)] fp32 in processing order; groups the loop
 * never visits (n_quant < K) keep their input values. zeros may be NULL when sym. group_size in {16, 32, 64, 128}
 * (others LLMC_ENOTSUP); nsteps = int(maxshrink * mse_grid), grid = mse_grid, norm = 2.4 in the reference.
 * ws: llmc_gptq_quantize_mse_ws_bytes(R, K) bytes, 256-B aligned. */
size_t llmc_gptq_quantize_mse_ws_bytes(int64_t R, int64_t K);
int llmc_gptq_quantize_mse(float* W, const float* Hinv, int64_t R, int64_t K, int64_t n_quant, int sym, float qmin,
                           float qmax, int64_t group_size, int round_zp, int nsteps, int grid, float norm, float* scales,
                           float* zeros, float* Wout, float* losses, int blocksize, void* ws, llmc_stream_t stream);

/* SpQR.weight_transform (spqr.py:185-254) for asymmetric per-group weights (a symmetric weight quantizer crashes in the
 * reference's get_group_qparams): the blocked column loop with
 *   - leave-one-out outlier detection per group (spqr.py:186-203, 214-229) unless simplified_outliers or threshold = inf,
 *   - the round_zp = False quantizer (quant.py:555-559, 702-707),
 *   - the second-level scale / zero quantizers as the reference executes them on its [R, 1] tensors (spqr.py:323-345):
 *     stored scale = fl(fl(s / ss) * ss), ss = 1e-5 / (scale_qmax - scale_qmin), zero point likewise,
 *   - outlier mask err^2 > threshold, masked weights keep their value (spqr.py:239-244),
 *   - W[:, i+1:i2] -= err x Hinv[i, i+1:i2] in the block, W[:, i2:] -= Err1 @ Hinv[i1:i2, i2:] after it.
 * W [R, K] fp32 running weights (in/out), Hinv [K, K] fp32 upper factor, threshold = relative_threshold * outlier_scale
 * (caller computes spqr.py:205-206; INFINITY = no outliers), group_size in {16, 32, 64, 128}, blocksize 128.
 * Outputs: Wout (tmp) / losses [R, K] fp32, mask [R, K] uint8, scales / zeros [R, K/group_size] fp32 in processing
 * order. Bit-exact against oracle/csrc/spqr_canon.c, which is pinned bit-exactly to the reference (tests/golden/spqr.npz). */
size_t llmc_spqr_quantize_ws_bytes(int64_t R, int64_t K);
int llmc_spqr_quantize(float* W, const float* Hinv, int64_t R, int64_t K, float qmin, float qmax,
                       int64_t group_size, float threshold, int simplified_outliers, float scale_qmin,
                       float scale_qmax, float zero_qmin, float zero_qmax, float* scales, float* zeros,
                       float* Wout, float* losses, uint8_t* mask, int blocksize, void* ws,
                       llmc_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * AWQ (llmc/compression/quantization/awq.py, auto_clip.py)
 * ---------------------------------------------------------------------------------------------- */

/* Awq.get_act_scale (awq.py:74-85): mean over tokens of |x| per channel. X [N, K] dt -> out [K] dt
 * (fp32 accumulation, one rounding to dt at the end, as ATen's mean does). */
size_t llmc_awq_act_mean_ws_bytes(int64_t N, int64_t K);
int llmc_awq_act_mean(const void* X, int dt, int64_t N, int64_t K, void* out, void* ws,
                      llmc_stream_t stream);

/* Awq.get_weight_scale (awq.py:48-72) for one layer: mean over rows of |W| / rowgroup-max(|W|).
 * W [R, K] dt, groups of g along K (g = K for per-channel) -> out [K] dt: the layer's `layer_scale.mean(0)`;
 * the caller adds the layers' vectors and divides by their count (awq.py:66-72, [K]-sized torch ops). */
size_t llmc_awq_weight_mean_ws_bytes(int64_t R, int64_t K);
int llmc_awq_weight_mean(const void* W, int dt, int64_t R, int64_t K, int64_t g, void* out_dt, void* ws,
                         llmc_stream_t stream);

/* Awq.get_scales (awq.py:88-108): v2: s = x_mean^ratio clamp(1e-4); v1: x^r / w^(1-r) clamp(1e-4);
 * then s /= sqrt(max(s) * min(s)). x_mean / w_mean / out: [K] dt. w_mean may be NULL for v2. The exponents
 * ratio and 1-ratio are rounded to dt first, as ATen's CPU Tensor.pow(python_float) does. */
int llmc_awq_scales(const void* x_mean, const void* w_mean, int dt, int64_t K, double ratio, int version,
                    void* out, llmc_stream_t stream);

/* fake_quantize_weight + scaling_weight (awq.py:40-46,147-164): out = fakequant_dyn(W * s[None,:]) in dt. */
int llmc_awq_scale_fakequant(const void* W, const void* s, int dt, int64_t R, int64_t K, int64_t g,
                             int sym, float qmin, float qmax, void* out, llmc_stream_t stream);

/* scaling_input (base_blockwise_quantization.py:877-889): out = X / s[None,:] in dt. */
int llmc_div_cols(const void* X, const void* s, int dt, int64_t N, int64_t K, void* out,
                  llmc_stream_t stream);
/* The same quotient written in the k-tiled layout llmc_linear_eval_kt reads (see below): out[K/32][N][32], f16/bf16,
 * K % 32 == 0, out of place. Same bits as llmc_div_cols followed by llmc_ktile_pack. */
int llmc_div_cols_kt(const void* X, const void* s, int dt, int64_t N, int64_t K, void* out,
                     llmc_stream_t stream);
/* apply_scale helpers (base_blockwise_quantization.py:597-611,750-778): W *= s[None,:] ; v /= s. */
int llmc_mul_cols(void* W, const void* s, int dt, int64_t R, int64_t K, llmc_stream_t stream);

/* The fake-quant W4A16 matmul of Awq.search_scale_subset (awq.py:110-145, 229-236):
 *   Y = X [N, K] . Wq [R, K]^T  (16-bit in, fp32 accumulate on MFMA, rounded to dt like F.linear)
 * mode 0: store Y to Yout [N, R] (dt); Y0, when not NULL, is a bias [R] (dt) added to the fp32 sum before the single
 *         rounding, like F.linear / addmm    -- get_original_out, FakeQuantLinear.forward (module_utils.py:619-644)
 * mode 1: loss += sum((Y0 - Y)^2), diff formed in dt like the reference, squared and summed in fp32;
 *         *loss_sum (device fp32, caller zeroes) ; mean = loss_sum / (N*R) is taken by the caller. */
size_t llmc_linear_eval_ws_bytes(int64_t N, int64_t K, int64_t R);
int llmc_linear_eval(const void* X, const void* Wq, int dt, int64_t N, int64_t K, int64_t R, int mode,
                     void* Yout, const void* Y0, float* loss_sum, void* ws, llmc_stream_t stream);
/* The same product from K-TILED operands, layout T[K/32][rows][32] (the 32-k slice of every row contiguous): the
 * layout the one-wave-per-SIMD GEMM streams at whole cache lines. llmc_ktile_pack converts a row-major [rows, K]
 * 16-bit matrix; llmc_linear_eval_kt is llmc_linear_eval (same modes, outputs, Y0 and workspace, same bits) with
 * both operands k-tiled; K % 128 == 0. Used by the AWQ grid step, where x / s and fakequant(W * s) are produced
 * per evaluation anyway (awq.py:229-236).
 * mode | LLMC_LINEAR_YBLOCKED: Yout (mode 0) / Y0 (mode 1) is an opaque TILE-BLOCKED image of the [N, R] matrix,
 * llmc_linear_eval_yblocked_bytes(N, R) bytes: per 256 x 256 tile one contiguous 128 KiB in the kernel's own
 * accumulator order (tile, wave, 32 KiB-pieces, lane x 16 B), so that the reference output of the search
 * (get_original_out) is written with 16-B stores and re-read 20 times as one contiguous run per tile.
 * Small products (mode 0, row-major Yout, R % 8 == 0): when the output has fewer 256 x 256 tiles than 3/4 of the CUs and the
 * caller passes a workspace of llmc_linear_eval_ws_bytes(N, K, R) bytes, the k range is cut into 2..8 slices so that
 * tiles x slices fills the chip; the slices' fp32 partial tiles are summed in slice order and rounded once by a second
 * kernel. A reordering of the fp32 sum: within one rounding of the single-pass result. ws == NULL keeps the single pass. */
#define LLMC_LINEAR_YBLOCKED 4
size_t llmc_linear_eval_yblocked_bytes(int64_t N, int64_t R);
int llmc_ktile_pack(const void* src, int dt, int64_t rows, int64_t K, void* dst, llmc_stream_t stream);
int llmc_linear_eval_kt(const void* Xt, const void* Wt, int dt, int64_t N, int64_t K, int64_t R, int mode,
                        void* Yout, const void* Y0, float* loss_sum, void* ws, llmc_stream_t stream);

/* AutoClipper.auto_clip_layer (auto_clip.py:84-191), clip_version v1, w_only:
 *   W [R, K] dt; X [n_tok, K] dt (already token-subsampled); groups of g along K.
 *   for i_s in 0 .. n_shrink-1: max = org_max * (1 - i_s / n_grid), min = -max (clip_sym) or
 *   org_min * (1 - i_s/n_grid); q_w = fakequant_dyn(clamp(w, min, max));
 *   err = mean_tok((sum_g x*q_w - sum_g x*w)^2); keep argmin.  Outputs best_max / best_min [R, K/g] dt. */
size_t llmc_awq_clip_search_ws_bytes(int64_t R, int64_t K, int64_t g, int64_t n_tok);
int llmc_awq_clip_search(const void* W, const void* X, int dt, int64_t R, int64_t K, int64_t g,
                         int64_t n_tok, int n_grid, int n_shrink, int clip_sym, int sym, float qmin,
                         float qmax, void* best_max, void* best_min, void* ws, llmc_stream_t stream);
/* The same evaluation, returning the error table instead of its argmin: errs [n_shrink, R, K/g] (dt) = the
 * token-mean squared output error of every shrink level (auto_clip.py:150-180, `err`). Callers with SEVERAL calibration
 * batches (auto_clip_layer's `inputs` list) form err_mean = sum_i err_i / len(inputs) and the strict-< argmin
 * themselves, in the tensor dtype like the reference (auto_clip.py:176-184). */
int llmc_awq_clip_errs(const void* W, const void* X, int dt, int64_t R, int64_t K, int64_t g, int64_t n_tok,
                       int n_grid, int n_shrink, int clip_sym, int sym, float qmin, float qmax, void* errs,
                       llmc_stream_t stream);
/* The error table from GIVEN candidates — every group width (per_channel / per_tensor: g = K), every quantizer (integer,
 * FP8, learnable ranges of clip_version v2), optionally quantized activations (auto_clip.py:150-170 with
 * fake_quantize_weight :258-274 and fake_quantize_input :276-281 evaluated by the caller):
 *   Q [n_shrink, R, K] dt = the fake-quantized weights of every shrink level; XT [K, ldt] dt = the sampled tokens
 *   TRANSPOSED (token t of column k at XT[k * ldt + t], ldt % 8 == 0, 16-byte aligned, zero padded); XQT = the same
 *   layout of their fake-quantized form, or XT itself for weight-only;
 *   errs[s, r, j] = mean_tok((sum_g xq * Q[s] - sum_g x * W)^2) in dt, the sums in ATen's CPU orders
 *   (vectorized_inner_sum with its level cascade over g <= 262144 elements; the token mean as llmc_awq_clip_errs). */
int llmc_awq_clip_errs_cand(const void* W, const void* Q, const void* XT, const void* XQT, int dt, int64_t R,
                            int64_t K, int64_t g, int64_t n_tok, int64_t ldt, int n_shrink, void* errs,
                            llmc_stream_t stream);

/* apply_clip v1 (auto_clip.py:194-212): W = clamp(W, min, max) per (row, group). */
int llmc_clamp_groups(void* W, int dt, int64_t R, int64_t K, int64_t g, const void* min_val,
                      const void* max_val, llmc_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * FP8 block-wise (DeepSeek-V3 style): llmc/compression/quantization/kernel.py (Triton) and FloatQuantizer `per_block`
 * ------------------------------------------------------------------------------------------------ */
/* weight_cast_to_fp8 (kernel.py:58-86; quant.py:33-43) and FloatQuantizer per_block fake / real quant
 * (quant.py:132-143, 612-658, 1043-1072, 1195-1221). W [M, N] dt; one fp32 scale per block x block tile, row-major
 * [ceil(M/block), ceil(N/block)]: scale = max(absmax, clamp_min) / 448; q = e4m3fn(W / scale) (fp32 division, RNE).
 * clamp_min = 1e-5: FloatQuantizer (`.clamp(min=1e-5)`, zero scales replaced by 1); clamp_min = 0: the Triton kernel
 * (an all-zero block yields scale 0 and NaN codes, like 0 / 0 there). fake bit 0: out is dt = q * scale, else e4m3
 * bytes; fake bit 1: `scales` is an INPUT (the *_static forms, quant.py:1074-1160); fake bit 8: qtorch.float_quantize
 * rounding (FloatQuantizer) instead of the e4m3fn cast (the Triton kernels), see llmc_fp8_quant. */
int llmc_fp8_block_quant(const void* W, int dt, int64_t M, int64_t N, int block, float clamp_min, int fake, void* out,
                         float* scales, llmc_stream_t stream);
/* weight_cast_to_bf16 (kernel.py:89-143; quant.py:18-30): out[m, n] = float(W8[m, n]) * scales[m/block, n/block] in out_dt. */
int llmc_fp8_block_dequant(const void* W8, const float* scales, int64_t M, int64_t N, int block, int out_dt, void* out,
                           llmc_stream_t stream);
/* act_quant (kernel.py:7-55): X contiguous, n_elem elements, every `block` consecutive ones share scale = absmax / 448
 * (fp32, no clamp); out8 e4m3 bytes, scales [n_elem / block]. */
int llmc_fp8_act_quant(const void* X, int dt, int64_t n_elem, int block, void* out8, float* scales, llmc_stream_t stream);
/* fp8_gemm + block_wise_fp8_forward_func (kernel.py:146-242; module_utils.py:40-45): A8 [M, K] e4m3 with a_s [M, K/128],
 * B8 [N, K] e4m3 (a weight) with b_s [N/128, K/128]; C [M, N] out_dt = sum over 128-deep K blocks of
 * (A_kb . B_kb^T) * a_s * b_s, fp32 accumulation on the fp8 MFMA; bias [N] (out_dt) is added after the rounding.
 * The K-block update is the reference Triton kernel's, acc = fma(part * a_s, b_s, acc): bit-identical outputs, two VALU ops per
 * element and K block, which bound the kernel at 0.31-0.37 of the fp8 MFMA peak. out_dt | LLMC_FP8_GEMM_FUSED_SCALE (opt-in, for
 * callers that do not need bit-identity with the Triton kernel): acc = fma(part, fl(a_s * b_s), acc), one op — the same value up
 * to one fp32 rounding of the scale product per row and K block (the 256 x 256-tile kernel only; the small-shape kernel ignores it). */
#define LLMC_FP8_GEMM_FUSED_SCALE 0x100
int llmc_fp8_block_gemm(const void* A8, const float* a_s, const void* B8, const float* b_s, int64_t M, int64_t N,
                        int64_t K, int out_dt, const void* bias, void* C, llmc_stream_t stream);

/* ---- OCP MX (csrc/mx_gemm.hip; an extension: the reference's real-quant Linears raise in forward) ------------------------------
 * The stored form: element codes + one e8m0 scale byte (2^(byte - 127)) per 32 consecutive elements of a row. e2m1 codes are
 * packed two per byte, element 2i in the low nibble (llmc_fp4_pack's form); e4m3 codes (OCP e4m3fn) take one byte each.
 *
 * llmc_mx_act_quant: X [M, K] contiguous bf16 / fp16 (16-byte aligned), K % 32 == 0 -> out_codes ([M, K/2] for fmt 2 = e2m1,
 * [M, K] for fmt 4 = e4m3; 8-byte aligned) and out_scales [M, K/32] uint8, in one pass. Per 1 x 32 block:
 *   absmax  fmaxf over |x| starting from 0: a NaN element is ignored, an infinity gives the exponent field 255 (llmc_fpx_quant)
 *   scale   byte = clamp(floor(log2(absmax)) - emax + 127, 0, 254), 127 for an all-zero block; emax = 2 (e2m1), 8 (e4m3)
 *   t       x * 2^(127 - byte), exact
 *   e2m1    round to nearest even onto the OCP grid, saturating at +-6 (infinities too); a NaN gives 6 with the input's sign; the
 *           sign survives on a zero: bit for bit llmc_fpx_quant(mode = ocp | e8m0, g = 32) followed by llmc_fp4_pack
 *   e4m3    round to nearest even, saturating at +-448 (infinities too); a NaN gives the NaN code 0x7f with the input's sign
 * LLMC_ENOTSUP: another fmt, K % 32 != 0. LLMC_EINVAL: null / misaligned pointers, another dtype.
 *
 * llmc_mx_gemm: A [M, K] codes in a_fmt (2 = packed e2m1 [M, K/2], 4 = e4m3) with a_s [M, K/32]; B4 [N, K/2] packed e2m1 (a
 * weight) with b_s [N, K/32];
 *   C[m, n] = sum over 32-deep blocks kb of 2^(a_s[m, kb] + b_s[n, kb] - 254) * sum_{k in kb} a[m, k] * b[n, k]
 * accumulated in fp32 by v_mfma_scale_f32_16x16x128_f8f6f4, which applies the scales itself (no per-block accumulator update), rounded
 * once to out_dt (bf16, fp16, fp32); bias [N] (out_dt, may be null) is added after that rounding, like llmc_fp8_block_gemm.
 * Numerics (measured): the instruction aligns the products of one 32-block to the block's largest product and
 * cuts off what lies more than 13 binary places below its leading bit. e2m1 x e2m1 products never reach that window. e4m3
 * activation codes are therefore fed one exponent class at a time (fields 0-7, 8-14, 15: three instructions per fragment,
 * each sum exact, joined in the fp32 accumulator), at a third of the instruction's e4m3 rate.
 * Any M, N >= 1 (edge tiles masked). LLMC_ENOTSUP (nothing is launched): K % 128 != 0, K >= 2^24, another a_fmt.
 * LLMC_EINVAL: null operands, codes not 16-byte / scales not 4-byte aligned, another out_dt. */
int llmc_mx_act_quant(const void* X, int dt, int64_t M, int64_t K, int fmt, void* out_codes, void* out_scales,
                      llmc_stream_t stream);
int llmc_mx_gemm(const void* A, int a_fmt, const void* a_s, const void* B4, const void* b_s, int64_t M, int64_t N, int64_t K,
                 int out_dt, const void* bias, void* C, llmc_stream_t stream);

/* ---- plain W8A8-FP8 Linear (csrc/fp8_linear.hip; an extension: the reference's real-quant Linears raise in forward) -----------
 * The stored form of configs/quantization/backend/{vllm,sglang}/fp8: OCP e4m3fn codes whose scales are constant along K.
 * A8 [M, K] codes with a_s fp32 [a_s_n], a_s_n = M (one per token) or 1 (per tensor); B8 [N, K] codes (a weight) with b_s fp32
 * [b_s_n], b_s_n = N (one per output channel) or 1.
 *   acc[m, n] = sum_k a[m, k] * b[n, k]                   fp32, on the fp8 matrix pipe
 *   C[m, n]   = rnd_out(fl(fl(acc * a_s[m]) * b_s[n]))    the two fp32 products in this order, one rounding to out_dt
 * bias [N] (out_dt, may be null) is added after that rounding, like llmc_fp8_block_gemm and llmc_mx_gemm. out_dt: bf16, fp16, fp32.
 * Both scales act in the epilogue: the K loop has no VALU work (llmc_fp8_block_gemm pays two ops per element and K block).
 * Instruction: the non-scaled forms — v_mfma_f32_32x32x16_fp8_fp8 on the tile rung, v_mfma_f32_16x16x32_fp8_fp8 on the decode
 * rung. Numerics (measured): the instruction aligns the 8 products of one lane's 8 operand bytes to the largest of
 * them and cuts off what lies more than 13 binary places below its leading bit; groups, instructions and the accumulator are added
 * at fp32 width. The loss is one-sided and below 7 * 2^-13 of sum |a b|; on top come at most K fp32 additions. The block-scaled
 * f8f6f4 form (twice the rate) has the same window over 32 products (K22), a loss of up to 31 * 2^-13, and is not used. Data whose
 * products within a group lie within 13 binary places of each other, and whose partial sums are fp32 numbers, gives the exact
 * result rounded once.
 * Rungs (one table in the source, set from profiles/fp8_linear.txt): 0 decode, M <= 64 — 16 columns per workgroup, the K blocks of
 * 128 dealt round 8 waves whose partial tiles are added in wave order in LDS (no atomics: the same bits on every run); 1 tile128 —
 * 128 x 128 outputs per workgroup. llmc_fp8_scaled_gemm_on_rung runs rung r whatever the shape (r = -1:
 * the table; for the measuring tool and the tests; the decode rung with M > 64 is LLMC_EINVAL). llmc_fp8_scaled_gemm_rung: the rung the table gives a shape, a pure host call.
 * Any M, N >= 1 (edge tiles masked). LLMC_ENOTSUP (nothing is launched): K % 128 != 0, K >= 2^24 (or 2^31 tiles).
 * LLMC_EINVAL: null operands, codes not 16-byte / scales not 4-byte aligned, another out_dt, a_s_n / b_s_n not in the allowed set. */
int llmc_fp8_scaled_gemm(const void* A8, const float* a_s, int64_t a_s_n, const void* B8, const float* b_s, int64_t b_s_n,
                         int64_t M, int64_t N, int64_t K, int out_dt, const void* bias, void* C, llmc_stream_t stream);
int llmc_fp8_scaled_gemm_on_rung(const void* A8, const float* a_s, int64_t a_s_n, const void* B8, const float* b_s, int64_t b_s_n,
                                 int64_t M, int64_t N, int64_t K, int out_dt, const void* bias, void* C, int rung, llmc_stream_t stream);
int llmc_fp8_scaled_gemm_rung(int64_t M, int64_t N);

/* ---- SmoothQuant / OS+ (smoothquant.py:39-59, osplus.py:61-170) ------------------------------------------------------------
 * Column statistics of X [N, K] dt (N up to 2^31 rows): run[0:K] = max, run[K:2K] = min, run[2K:3K] = max |x| per column, fp32
 * (exact: they are values of dt). init != 0: the buffers are written; else the batch is folded into them (running max / min
 * over calibration batches; over the layers of a subset for |W|.max(dim=0)). NaN propagates like torch.amax. glob (optional,
 * fp32 [2]): max(0, max_k run_max), min(0, min_k run_min) — OS+'s amx / amn. Two stages without atomics: bit-exact whatever
 * the launch geometry. ws: llmc_col_stats_ws_bytes. */
size_t llmc_col_stats_ws_bytes(int64_t N, int64_t K);
int llmc_col_stats(const void* X, int dt, int64_t N, int64_t K, int init, float* run, float* glob, void* ws,
                   llmc_stream_t stream);
/* SmoothQuant.search_scale_subset: out[k] = (x^alpha / max(w, 1e-5)^(1 - alpha)).clamp(min=1e-5) in dt, every op rounded to
 * dt; x_absmax / w_absmax fp32 [K] (llmc_col_stats), x is cast to dt first. Exponents are cast to dt; 0.5 is a square
 * root, like ATen's pow. */
int llmc_smooth_scales(const float* x_absmax, const float* w_absmax, int dt, int64_t K, double alpha, double one_minus_alpha,
                       void* out, llmc_stream_t stream);
/* OS+ cur_scale of grid point `index` (osplus.py:118-131): st = thresholds[index] (dt, rounded on the host);
 * out[k] = max(cmx[k] > st ? cmx[k] / st : 1, cmn[k] < -st ? cmn[k] / -st : 1) in dt. cmx / cmn fp32 [K]. */
int llmc_osplus_scale(const float* cmx, const float* cmn, const void* thresholds, int64_t index, int dt, int64_t K, void* out,
                      llmc_stream_t stream);
/* out = fake_quant_act_dynamic(X / s[None, :]) per token (osplus.py:156-157) in one pass over X [N, K] dt: the same bits as
 * llmc_div_cols followed by llmc_quant_dynamic (kind 0: integer, sym / qmin / qmax as there, round_zp) or by llmc_fp8_quant
 * with dynamic per-row scales of dt (kind 1: fp8_mode = its `fake` argument's format and semantics bits). Takes rows of whole
 * 16-byte vectors up to 14 per thread of a 256-thread workgroup (K <= 28672 for 16-bit dt, 14336 for fp32) and 16-byte
 * aligned buffers; anything else LLMC_ENOTSUP (callers run the two kernels). llmc_osplus_act_step_tier: the vectors-per-thread
 * tier (2 / 4 / 8 / 14) a width is compiled for, 0 when the kernel does not take it; a pure host call. */
int llmc_osplus_act_step_tier(int dt, int64_t K);
int llmc_osplus_act_step(const void* X, const void* s, int dt, int64_t N, int64_t K, int kind, int sym, float qmin, float qmax,
                         int fp8_mode, void* out, llmc_stream_t stream);

/* ---- mixed int / fp columns (quant.py:754-783, 833-869 with int_indices / fp_indices: QUIK, LLM.int8()) ----------------------
 * Fake-quantize some columns of X [N, K] (contiguous, dtype dt) dynamically and leave the others alone, in one pass: a row is
 * read once, waits in LDS, is written once. role [K] says what becomes of a column: 0 = +0 is written (the reference's
 * zeros_like), 1 = integer column, 2 = X's own bits pass through (NaN payloads, infinities, -0 survive), 3 = passes through but
 * still counts in its group's min / max (a column named in both index lists: the reference's fp scatter comes second). The
 * integer columns are cut into n_int / g groups in the order of int_idx (int32 [n_int], values in [0, K); entries outside are
 * ignored): group j of a row is the columns int_idx[j * g .. (j + 1) * g). Each group gets get_minmax_range + get_qparams +
 * quant_dequant in dt: bit for bit llmc_quant_dynamic (LLMC_OUT_FAKE) on the contiguous gathered copy X[:, int_idx], written
 * back to the columns it came from; with round_zp = 0 bit for bit llmc_minmax_qparams + llmc_quant_static with
 * LLMC_FRACTIONAL_ZP on that copy. With g == n_int (one group per row) int_idx may be NULL: the group is then every column
 * whose role is 1 or 3. Duplicate entries in int_idx are undefined (as for torch's scatter); n_int > K is LLMC_EINVAL, as are
 * n_int <= 0 and n_int % g != 0. out == X is allowed. Only fake values: the reference has no real-quant path for mixed
 * columns. No workspace, no atomics, stream-ordered. Rows that do not fit the LDS of a CU (llmc_quant_dynamic_mixed_fits
 * answers 0: above about 81900 16-bit or 40950 fp32 columns; a pure host call) return LLMC_ENOTSUP: callers compose
 * llmc_quant_dynamic with gathers and scatters. */
int llmc_quant_dynamic_mixed_fits(int dt, int64_t K);
int llmc_quant_dynamic_mixed(const void* X, int dt, int64_t N, int64_t K, const uint8_t* role, const int32_t* int_idx,
                             int64_t n_int, int64_t g, int sym, int round_zp, float qmin, float qmax, void* out,
                             llmc_stream_t stream);

/* ---- dynamic quantization along columns (quant.py:833-869 with args['dim'] = 'ic': AdaDim's per-input-channel axis) -----------
 * W [R, K] row-major of dt with row stride ld >= K elements; a group is g consecutive rows of one column, group index
 * k * (R / g) + r / g: the order of reshape_tensor(W.T). g == R is per_channel along the input axis; any g >= 1 that divides R
 * is taken. out is contiguous [R, K] in W's own layout (not transposed), 16-byte aligned, and must not overlap W: fake values
 * in dt (LLMC_OUT_FAKE) or codes (LLMC_OUT_I32 / I8 / U8). scales_out / zeros_out: optional, [K * R / g] of dt in group order
 * (zeros_out of a symmetric quantizer: +0). Bit for bit llmc_quant_dynamic on the contiguous transposed copy of W, transposed
 * back; with round_zp = 0 bit for bit llmc_minmax_qparams + llmc_quant_static with LLMC_FRACTIONAL_ZP on that copy. The one
 * exception is the sign of a zero minimum, hence of a zero in zeros_out, which follows the order of the reduction as it does
 * between the row kernel's own paths. No transposed copy, no atomics: lanes walk columns 16 bytes at a time, a wave's load
 * covers four 256-byte row segments. Launch paths (llmc_quant_dynamic_cols_path answers which one a call takes, or a negative
 * LLMC_E*, without touching the GPU; llmc_quant_dynamic_cols_paths is their number):
 *   0  g <= 256: one workgroup takes min / max down a tile of g rows by a strip of columns, then re-reads the tile (from L2) and
 *      stores. One read from HBM and one write of W, no workspace.
 *   1  g > 256: the rows of a group are cut into slabs of 64; per-slab fp32 min / max go to ws, a small launch folds them per
 *      column (and writes scales_out / zeros_out), a third launch quantizes. Two reads and one write of W, all coalesced.
 *   2  W, ld or K do not allow 16-byte vectors (W not 16-byte aligned, ld or K not a multiple of 16 bytes: a ragged vector
 *      tail included): the same two structures one element per lane.
 * ws: llmc_quant_dynamic_cols_ws_bytes(R, K, g) bytes, 0 for g <= 256: (R / g) * (ceil(g / 64) + 1) * K * 8 otherwise.
 * LLMC_EINVAL (with a llmc_hip_last_error text, before anything is launched): bad dt, a null W or out, R, K or g < 1, g not
 * dividing R, ld < K, out unaligned or overlapping W, a bad out_kind, a missing workspace. */
size_t llmc_quant_dynamic_cols_ws_bytes(int64_t R, int64_t K, int64_t g);
int llmc_quant_dynamic_cols(const void* W, int dt, int64_t R, int64_t K, int64_t ld, int64_t g, int sym, int round_zp,
                            float qmin, float qmax, int out_kind, void* out, void* scales_out, void* zeros_out, void* ws,
                            llmc_stream_t stream);
int llmc_quant_dynamic_cols_paths(void);
int llmc_quant_dynamic_cols_path(const void* W, int dt, int64_t R, int64_t K, int64_t ld, int64_t g);

/* ---- Walsh-Hadamard transform (hadamard_utils.py:72-122 matmul_hadU / matmul_hadU_cuda, module_utils.py:460-503 Rotater) ------
 * x, y: contiguous [outer, n, inner] of dt (F16 / BF16 / F32 / F64); y == x is allowed. Along the middle axis
 *   y[o, a*m + j, c] = scale * sum_{b, i} hadK[a][b] * S_m[j][i] * x[o, b*m + i, c],   n = K0 * m,
 * S_m the Sylvester matrix of order m (a power of two, >= 1) in natural order, hadK a device [K0, K0] fp32 matrix of +-1 (null
 * when K0 == 1). Row transforms use inner = 1; transforms across heads or along a weight's output axis inner > 1. Additions and
 * subtractions only, accumulated in fp32 (fp64 for F64); scale (rounded to fp32 on the fp32 path) is applied once at the end,
 * then one rounding to dt. A row stays on chip between its load and its store. LLMC_ENOTSUP (llmc_hip_last_error names it):
 * K0 > 64, n / K0 not a power of two, a row too long to stay resident (n * 4 bytes, 8 for F64, plus the factor matrix above
 * 160 KiB, or n / K0 > 32768). Allocates nothing, runs in stream order. */
int llmc_hadamard(const void* x, void* y, int dt, int64_t outer, int64_t n, int64_t inner, const float* hadK, int K0,
                  double scale, llmc_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Sparsification (llmc/compression/sparsification/wanda.py, magnitude.py)
 * ---------------------------------------------------------------------------------------------- */

/* Wanda.get_row_scale (wanda.py:27-31): column sums of squares of X [N, K] (contiguous, dtype dt, N up to 2^31 rows).
 * acc [K] fp32: acc[k] = sum_n fp32(x[n, k])^2, every square and every add rounded to fp32. init != 0: acc is written;
 * else the batch is folded into it, acc[k] = acc[k] + batch[k]. out (optional, fp32 [K]): out[k] = acc[k] / (float)nsamples,
 * one IEEE fp32 division: the reference's scaler_row (which takes the square root of the sum and squares it again before it
 * divides: the same value up to those two roundings).
 * Two stages, no float atomics. The order of summation is a function of (N, K, dt) alone, so equal calls give equal bits:
 * the rows are cut into C = min(ceil(N / 64), max(1, 2048 / ceil(K / (64 * v)))) chunks of ceil(N / C) consecutive rows, v the
 * elements of a 16-byte vector of dt; in a chunk starting at row r0, wave w of 4 sums the rows r0 + w, r0 + w + 4, ... in
 * that order from 0, the chunk's value is ((s0 + s1) + s2) + s3, and the chunks are added in chunk order. The alignment of X
 * changes the loads (16-byte vectors when K % v == 0 and X is 16-byte aligned), not this order.
 * ws: llmc_col_sqsum_ws_bytes(N, K, dt) bytes (a pure host call; 0 for invalid arguments). */
size_t llmc_col_sqsum_ws_bytes(int64_t N, int64_t K, int dt);
int llmc_col_sqsum(const void* X, int dt, int64_t N, int64_t K, int init, float* acc, float* out, int64_t nsamples, void* ws,
                   llmc_stream_t stream);

/* Wanda.subset_transform's selection (wanda.py:46-56), in place on W [R, K] of dt with row stride ld >= K elements: a row is cut
 * into groups of m consecutive columns, and in each group the n_prune elements of smallest metric become +0 of dt.
 *   metric = fp32(|w|) * sqrtf(scaler_row[k]): exactly these two roundings (IEEE square root); scaler_row fp32 [K], null = the
 *   multiplier 1. A NaN metric (inf * 0 included) orders after +inf whatever its sign bit; ties go by lower column first. This is
 *   bit for bit the mask of torch.sort(metric, dim=-1, stable=True)[1][:, :n_prune] scattered back.
 *   m == K is the reference's per-row mode; m in {2, 4, 8, 16} with K % m == 0 is n:m semi-structured pruning (zero n_prune of
 *   every m); any other m returns LLMC_ENOTSUP.
 * Elements that are kept retain their own bits (-0, infinities, NaN payloads); columns K .. ld - 1 are never touched. mask_out
 * (optional): uint8 [R, K] contiguous, 1 where an element was pruned. n_prune == 0 touches no weight and clears mask_out;
 * n_prune == m zeroes everything. No workspace, no allocation, stream-ordered.
 * m == K reads W from HBM once and writes it once: the row and its 32-bit keys (the metric's bit pattern, NaN made the largest)
 * wait in registers while a most-significant-digit radix select (digits of 11, 11 and 9 bits, LDS histograms) finds the key of rank n_prune - 1
 * and the number of keys below it; a prefix count over the keys equal to it picks the first of them by column. Launch paths
 * (llmc_prune_rows_path answers which one a call takes, or a negative LLMC_E*, without touching the GPU; llmc_prune_rows_paths
 * is their number):
 *   0  one wave per row, four rows per workgroup: rows of up to 256 16-byte vectors (K <= 2048 16-bit, 1024 fp32)
 *   1  one 256-thread workgroup per row: up to 1024 vectors (K <= 8192 / 4096)
 *   2  one 1024-thread workgroup per row: up to 8192 vectors, K <= 32768
 *   3  m == K with operands that do not allow 16-byte vectors (W not 16-byte aligned, ld or K not a multiple of 16 bytes): the
 *      same three structures one element per lane, K <= 32768
 *   4  n:m, lane-local: a lane owns whole groups (one 16-byte vector, or m elements when m is wider); no LDS
 *   5  n:m one element per lane, for the operands of path 3
 * A row of more than 32768 columns with m == K returns LLMC_ENOTSUP (callers compose the reference's sequence).
 * LLMC_EINVAL, before anything is launched: bad dt, null W, R or K < 1, ld < K, m in the list but not dividing K, n_prune
 * outside [0, m]. */
int llmc_prune_rows(void* W, int dt, int64_t R, int64_t K, int64_t ld, const float* scaler_row, int64_t n_prune, int64_t m,
                    uint8_t* mask_out, llmc_stream_t stream);
int llmc_prune_rows_paths(void);
int llmc_prune_rows_path(int dt, int64_t R, int64_t K, int64_t ld, int64_t m, const void* W);

/* Magnitude.subset_transform (magnitude.py:26-31), in place on the strided view W [R, K] (row stride ld >= K) of dt: with
 * a = |W| over its R * K elements, thresh = the element of 0-based rank kth in ascending order (torch.sort(a.flatten())[0][kth]),
 * written to thresh_out (optional, one element of dt), and every element with a <= thresh becomes +0: all ties of the threshold
 * go, so at least kth + 1 zeros result. mask_out (optional): uint8 [R, K] contiguous, 1 where an element was zeroed. The weights
 * are assumed to hold no NaN (a NaN would count as larger than every number and survive). R * K < 2^32.
 * 16-bit dt: one pass builds a 32768-bin histogram of the sign-cleared bit patterns (per-workgroup LDS histograms merged into ws
 * with integer atomics: exact, hence deterministic), one workgroup scans it for the bin of rank kth, one pass masks. F32: two
 * 16-bit digits, a second histogram over the elements inside the first digit's bin. The call zeroes its own workspace; no host
 * synchronisation. ws: llmc_magnitude_prune_ws_bytes(dt, R, K) bytes, 4-byte aligned (a pure host call; 0 for invalid arguments).
 * LLMC_EINVAL, before anything is launched: bad dt, null W, R or K < 1, ld < K, kth outside [0, R * K) (the reference raises an
 * IndexError at sparsity 1.0), a missing workspace. */
size_t llmc_magnitude_prune_ws_bytes(int dt, int64_t R, int64_t K);
int llmc_magnitude_prune(void* W, int dt, int64_t R, int64_t K, int64_t ld, int64_t kth, void* thresh_out, uint8_t* mask_out,
                         void* ws, llmc_stream_t stream);

/* SparseGPT's fasterprune (Frantar & Alistarh 2023; the reference tree has no counterpart) in fp32 at blocksize 128: GPTQ's
 * blocked column loop with the quantizer replaced by a mask. Every elementwise operation rounds once, no fma:
 *   for i1 in 0, 128, ...: i2 = min(i1 + 128, K), count = i2 - i1, W1 = W[:, i1:i2] as it stands, d_c = Hinv[c][c]
 *     unstructured (prune_m == 0): s = fl(fl(W1 W1) / fl(d d)) of the block-start weights, kth = (int64)((double)(R count) *
 *       sparsity), thresh = the score of 0-based rank kth among the R * count scores, mask1 = s <= thresh (all ties go);
 *     n:m (prune_m = m in {2, 4, 8, 16}): at every column i with i % m == 0 the scores of columns i .. i + m - 1 of the RUNNING
 *       W1; in every row the prune_n lowest are masked, equal scores by lower column;
 *     per column c = i1 + i: q = mask1 ? +0 : w, Wout[:, c] = q, mask[:, c] = mask1, diff = fl(w - q),
 *       losses[:, c] = fl(fl(diff diff) / fl(d d)), err = fl(diff / d), W1[:, j] = fl(W1[:, j] - fl(err Hinv[c][i1 + j])), j > i;
 *     W[:, i2:] -= Err1 @ Hinv[i1:i2, i2:] on sgemm.hip's k-ordered fma chain.
 * W [R, K] fp32 running weights (in/out, GPTQ's convention: a block's own columns keep their block-start values), Hinv [K, K]
 * fp32 upper factor, Wout [R, K] fp32; losses [R, K] fp32 and mask [R, K] uint8 may be NULL. A pruned weight is +0, a kept one
 * keeps its bits. sparsity 0 prunes the minimum-score element(s) of each block, as the published code does. Non-finite weights
 * are outside the contract (they index nothing out of bounds). Per block: score + first-digit histogram, scan, second-digit
 * histogram, scan (integer atomics: exact, deterministic; the threshold never leaves the device), the block kernel, the trailing
 * sgemm; n:m skips the select. Runs on `stream`, complete in stream order; allocates nothing; no host synchronisation.
 * ws: llmc_sparsegpt_prune_ws_bytes(R, K) bytes, 256-B aligned (a pure host call; 0 for non-positive sizes).
 * Before anything is launched, LLMC_EINVAL: null W / Hinv / Wout / ws, R or K < 1, R >= 2^24, blocksize != 128, sparsity outside
 * [0, 1) when unstructured, prune_n outside [0, m]; LLMC_ENOTSUP: K % 4 != 0, m not in {2, 4, 8, 16}, K % m != 0.
 * Bit-exact against tests/sparsegpt_oracle.py. */
size_t llmc_sparsegpt_prune_ws_bytes(int64_t R, int64_t K);
int llmc_sparsegpt_prune(float* W, const float* Hinv, int64_t R, int64_t K, double sparsity, int64_t prune_n,
                         int64_t prune_m, float* Wout, float* losses, uint8_t* mask, int blocksize, void* ws,
                         llmc_stream_t stream);

/* NaiveQuantKVCache.update / KiviQuantKVCache.update (kvquant.py:44-87, 233-289) for keys and values in one launch: the stored
 * rows are dequantized, the new rows appended, and with LLMC_KV_REQUANT every row's codes and qparams are derived again from those
 * values, in place, as the reference's quantize(cat(dequantize(cache), new)) does. Per tensor (k_*, v_*; the v_* set may be all
 * NULL):
 *   codes   [B * H, cap, D] one code per byte: int8 when qmin < 0, uint8 otherwise (qmin >= -128, qmax <= 255 / 127)
 *   scales  [B * H, cap, D / g] of dt; zeros the same, NULL exactly when sym
 *   new     the rows [B, H, n_new, D] of dt with the element strides new_stride_b / _h / _t shared by both tensors (the
 *           [B, T, H, D].transpose(1, 2) view of an attention module is read in place); unit stride along D
 *   out     [B, H, T_old + n_new, D] contiguous of dt: what update() returns; may be NULL with LLMC_KV_REQUANT
 * Rows t < T_old: out = rnd(rnd(q - z) * s) (quant.py:709-712). Rows t >= T_old: out = the new row, or with LLMC_KV_NEW_FAKE
 * (needs LLMC_KV_REQUANT) its dequant(quant(.)) (the Naive cache's prefill). LLMC_KV_REQUANT: per group of g elements, min / max of
 * the row's `out` values before NEW_FAKE -> get_qparams (quant.py:545-559, minmax) -> codes and qparams stored to row t of the
 * same slots. Without it nothing in the store is written (Kivi between two flushes).
 * An old element costs 1 byte read and 2 + 1 written. Stream-ordered, no workspace, no allocation.
 * LLMC_EINVAL, before anything is launched: bad dt or flags, B, H, D, g < 1, D % g != 0, T_old + n_new < 1, cap < T_old (or
 * < T_old + n_new with REQUANT), a missing pointer, zeros given when sym or missing when not, codes / new / out not 16-byte aligned.
 * LLMC_ENOTSUP (callers compose the update from the quantizer's operators): round_zp != 1, codes of more than 8 bits, g not 16
 * bytes times a power of two <= 64, new-row strides that are not multiples of 16 bytes, B * H > 65535, T * D / g >= 2^31. */
#define LLMC_KV_REQUANT 1
#define LLMC_KV_NEW_FAKE 2
int llmc_kv_cache_update(int dt, int64_t B, int64_t H, int64_t T_old, int64_t n_new, int64_t cap, int64_t D, int64_t g, int sym,
                         int round_zp, float qmin, float qmax, int flags, void* k_codes, void* k_scales, void* k_zeros,
                         const void* k_new, void* k_out, void* v_codes, void* v_scales, void* v_zeros, const void* v_new,
                         void* v_out, int64_t new_stride_b, int64_t new_stride_h, int64_t new_stride_t, llmc_stream_t stream);

/* SinkKVCache.update (kvsparse.py:569-648: StreamingLLM's attention-sink window) for keys and values in one launch. src and dst
 * are [B * H, src_cap, D] and [B * H, dst_cap, D] buffers of dt per tensor (k_*, v_*; the v_* set may be all NULL). Per (b, h),
 * destination rows from dst_row0 on:
 *   [0, n_sink)             <- source rows [0, n_sink), copied
 *   the next n_keep rows    <- source rows [keep_from, keep_from + n_keep). Keys with cos / sin given ([n_keep, rot] contiguous
 *                              of dt): row i is rotated again, out = rnd(rnd(k * cos[i]) + rnd(rotate_half(k) * sin[i])) over the
 *                              first rot columns (rotate_half = cat(-k[rot / 2:rot], k[:rot / 2]); rnd rounds to dt, every
 *                              product and the sum on its own, no fused multiply-add); columns >= rot are copied
 *                              (partial_rotation_size). Values, and keys without cos / sin: copied.
 *   the next n_new rows     <- the new states [B, H, n_new, D] with the element strides new_stride_b / _h / _t shared by both
 *                              tensors (the [B, T, H, D].transpose(1, 2) view of an attention module is read in place)
 * A cached element is read once and written once. src == dst is allowed only with n_sink == n_keep == 0 (append in place at
 * dst_row0; src may then be NULL); src and dst must not overlap otherwise. Stream-ordered, no workspace, no allocation.
 * LLMC_EINVAL, before anything is launched: bad dt, B, H, D < 1, a negative count or row, nothing to write, cos without sin, rot
 * odd or outside (0, D] (rot is ignored without cos / sin), dst_row0 + n_sink + n_keep + n_new > dst_cap, n_sink or
 * keep_from + n_keep > src_cap, a missing pointer, src == dst while rows are moved.
 * LLMC_ENOTSUP (callers compose the update from tensor ops): D or rot / 2 not a multiple of the 16-byte vector, a source,
 * destination, table or new-row pointer or a new-row stride that is not 16-byte aligned, B * H * rows * vectors >= 2^31. */
int llmc_kv_sink_update(int dt, int64_t B, int64_t H, int64_t D, int64_t n_sink, int64_t keep_from, int64_t n_keep, int64_t n_new,
                        int64_t src_cap, int64_t dst_cap, int64_t dst_row0, int64_t rot, const void* cos, const void* sin,
                        const void* k_src, void* k_dst, const void* k_new, const void* v_src, void* v_dst, const void* v_new,
                        int64_t new_stride_b, int64_t new_stride_h, int64_t new_stride_t, llmc_stream_t stream);

/* ShortGPT.compute_bi (shortgpt.py:40-55: Block Influence, one cosine per token between a block's input and its output) without
 * the reference's N x N product. X, Y [N, d] of dt with unit column stride and row strides ldx, ldy >= d elements; each element
 * of the two is read once.
 *   per row: dot = sum x y, sx = sum x x, sy = sum y y in fp32, every product and every add rounded on its own (no fused
 *   multiply-add); sim = dot / (sqrtf(sx) * sqrtf(sy)), IEEE square roots and division (the reference's dot / (norm_in *
 *   norm_out)); a NaN sim becomes 0.5 and +-inf becomes +-FLT_MAX (nan_to_num(nan=0.5)); bi[row] = 1 - sim. bi fp32 [N] is
 *   always written.
 *   total (one fp64 on the device): the fp64 sum of bi[0 .. N - 1]; init != 0: written, else total = total + batch.
 * The order of summation, a function of (N, d, dt) alone, so equal calls give equal bits whatever the grid:
 *   a row is cut into slots of v = 16 / sizeof(dt) consecutive elements, the last one partial when d % v != 0. One wave owns the
 *   row; lane l folds the slots l, l + 64, l + 128, ... in that order, the elements of a slot in index order, onto three
 *   sums that start at +0: s = s + x y. The 64 lane values are joined by the xor butterfly with the offsets 32, 16, 8, 4, 2, 1:
 *   at every step lane l's value becomes v[l] + v[l ^ offset] (a lane without a slot holds +0).
 *   total: the rows are cut into chunks of 4096 consecutive rows. In a chunk starting at row r0, thread t of 256 adds
 *   bi[r0 + t], bi[r0 + t + 256], ... in that order onto an fp64 0; the 256 values are joined by the tree
 *   for s = 128, 64, ..., 1: v[t] = v[t] + v[t + s] (t < s). The chunk values are summed the same way: thread t of 256 adds
 *   the chunks t, t + 256, ..., then the same tree.
 * The alignment of the operands changes the loads, not this order: one 16-byte load per slot when d % v == 0 and X, Y, ldx and
 * ldy keep every row 16-byte aligned, element loads of the same slots otherwise.
 * Three launches on `stream`, complete in stream order; no atomics, no allocation, nothing read on the host.
 * ws: llmc_block_influence_ws_bytes(N) bytes, 8-byte aligned (a pure host call; 0 for invalid arguments).
 * LLMC_EINVAL, before anything is launched: bad dt, a null pointer, N < 1 or N > 2^31, d < 1, ldx or ldy < d.
 * LLMC_ENOTSUP: d >= 2^31 (the slot index of a row is a 32-bit integer).
 * Bit-exact against tests/shortgpt_oracle.py. */
size_t llmc_block_influence_ws_bytes(int64_t N);
int llmc_block_influence(const void* X, const void* Y, int dt, int64_t N, int64_t d, int64_t ldx, int64_t ldy, int init,
                         float* bi, double* total, void* ws, llmc_stream_t stream);

/* Pairwise cosine distance of token features (pairwise_cosine_similarity and the `1.0 -` of divprune, divprune.py:13-27 of the
 * reference's token_reduction package; the same matrix ToMe, DART, VisionZip, FastVID and DyCoke form). X [N, d] of dt with unit
 * column stride and row stride ldx >= d elements; D fp32 [N, N], contiguous.
 *   G = X X^T accumulated in fp32 on the matrix pipe (v_mfma_f32_32x32x16_bf16 / _f16; fp32 inputs take v_mfma_f32_32x32x2f32
 *   in the same template, so their products are fp32 products, not split ones). Both operands are rows of X, 8 (fp32: 4)
 *   consecutive k per lane: no transposed and no normalised copy of X is written.
 *   D[i][j] = 1 - G[i][j] / (sqrtf(G[i][i]) * sqrtf(G[j][j])), IEEE square roots, product, division and subtraction. G[i][i] is
 *   the diagonal element of the same accumulation, so D[i][i] is a rounding or two away from 0 and is not forced to 0; a zero
 *   row gives NaN in its row and column (0 / 0). Both as in the reference.
 *   Only the 128 x 128 tiles on or above the diagonal are multiplied; below the diagonal D is a copy, so D[i][j] and D[j][i]
 *   have equal bits (inside a diagonal tile both take the element above the diagonal).
 * The order of summation, a function of (N, d, dt) alone, so equal calls give equal bits:
 *   tiles = nt (nt + 1) / 2 with nt = ceil(N / 128); S = min(ceil(512 / tiles), ceil(d / 256)) slices are wanted; a slice is
 *   ks = ceil(ceil(d / S) / 32) * 32 consecutive k and there are ceil(d / ks) of them. Inside a slice k advances by 16 (fp32: 8)
 *   per step onto one accumulator per element that starts at +0; a step is one 32x32x16 instruction (fp32: four 32x32x2
 *   instructions, instruction e taking k0 + e and k0 + 4 + e); k at or past d enters as +0. The slices' fp32 values are then
 *   added in slice order starting from slice 0's.
 * Any alignment of X and ldx is accepted: 16-byte loads when X and ldx * sizeof(dt) are multiples of 16, element loads of the
 * same values otherwise; the order does not change.
 * Two launches on `stream`, complete in stream order; no atomics, no allocation, nothing read on the host.
 * ws: llmc_cosine_dist_ws_bytes(N, d) bytes, 16-byte aligned: the slices' partial tiles (a pure host call; 0 for arguments the
 * entry refuses).
 * LLMC_EINVAL, before anything is launched: bad dt, a null pointer, N < 1, d < 1, ldx < d.
 * LLMC_ENOTSUP: N > 46340 or d > 2^31 - 64 (an element index of D or of a row would leave 32 bits).
 * Error bound and exact cases: tests/divprune_oracle.py. */
size_t llmc_cosine_dist_ws_bytes(int64_t N, int64_t d);
int llmc_cosine_dist(const void* X, int dt, int64_t N, int64_t d, int64_t ldx, float* D, void* ws, llmc_stream_t stream);

/* DivPrune's greedy max-min selection (divprune.py:29-53) on a distance matrix D [N, N] of dt (f32, bf16 or f16: a matrix the
 * caller supplies keeps its dtype, values are only compared) with unit column stride and row stride ldd >= N elements.
 * sel int64 [k]. torch's ordering rules, stated outright:
 *   step 0: score[j] = the second smallest element of COLUMN j, a NaN sorting after every number (topk(2, dim=0, largest=False));
 *   step i >= 1: score[j] = min(score[j], D[sel[i - 1]][j]), a NaN in either operand giving NaN; before step 1 the scores are
 *   reset, so step 1's score is row sel[0] alone (the reference reduces the chosen rows only);
 *   every step: sel[i] = the index of the greatest score, a NaN greater than every number (and equal to another NaN), -0 equal to
 *   +0, the lowest index among equals (torch.argmax on the CPU). Nothing excludes an index already chosen: with duplicate tokens
 *   the reference selects again, and so does this; k > N is legal.
 * Two launches on `stream`: a pass over D for the step-0 statistic, then one workgroup of 1024 threads that runs all k steps,
 * each thread holding the running minimum of up to 16 columns in registers and a step reading one row of D (N * sizeof(dt)
 * bytes); the argmax is one reduction over (value, index) keys. No atomics, no allocation, nothing read on the host.
 * ws: llmc_maxmin_select_ws_bytes(N) bytes, 4-byte aligned (a pure host call; 0 for an N the entry refuses).
 * LLMC_EINVAL, before anything is launched: bad dt, N < 2 (the reference's topk(2) raises there), k < 0, ldd < N, a null pointer
 * with k > 0. k == 0 writes nothing and launches nothing.
 * LLMC_ENOTSUP: N > llmc_maxmin_select_max_n() = 16384, the columns one workgroup keeps resident (callers compose the
 * reference's loop). Bit-exact against tests/divprune_oracle.py: select. */
int llmc_maxmin_select_max_n(void);
size_t llmc_maxmin_select_ws_bytes(int64_t N);
int llmc_maxmin_select(const void* D, int dt, int64_t N, int64_t ldd, int64_t k, int64_t* sel, void* ws, llmc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* LLMC_HIP_H_ */
