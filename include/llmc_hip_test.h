/* llmc_hip_test.h — TEST-ONLY entry points of libllmc_hip.so (VERDICT r03 hygiene: not part of the product surface that
 * include/llmc_hip.h declares). tests/test_gptq_gpu.py and tools/bench_sgemm.py exercise the two internal GEMMs of K3 / K4
 * through them; nothing in llmc_amd/ calls them. */
#ifndef LLMC_HIP_TEST_H_
#define LLMC_HIP_TEST_H_
#include "llmc_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------
 * Test hooks (tests/test_gptq_gpu.py only): the internal fp32-MFMA GEMM used by K3/K4, and the split-bf16 GEMM
 * (C (op) op(A) B, TA / epilogue / hints as in llmc_test_sgemm, three bf16 terms per operand, six products) used by K3.
 * C (op) op(A)[M x Kd] . op(B)[Kd x N]; epilogue 0: C -= AB, 1: C = AB, 2: C = -AB.
 * ---------------------------------------------------------------------------------------------- */
int llmc_test_sgemm(const float* A, const float* B, float* C, int64_t lda, int64_t ldb, int64_t ldc, int M,
                    int N, int Kd, int TA, int TB, int epilogue, int a_upper, int a_lower, int b_upper,
                    int c_upper_only, llmc_stream_t stream);
/* The phased form K4's far update uses: C -= op(A)[:, p] B[p, :] for p = consecutive ranges of `phase_len` k (a multiple of 16),
 * one launch, bit-identical to Kd / phase_len separate llmc_test_sgemm calls. op(B) = N. */
int llmc_test_sgemm_phased(const float* A, const float* B, float* C, int64_t lda, int64_t ldb, int64_t ldc, int M, int N,
                           int Kd, int TA, int phase_len, llmc_stream_t stream);
int llmc_test_gemm3(const float* A, const float* B, float* C, int64_t lda, int64_t ldb, int64_t ldc, int M, int N,
                    int Kd, int TA, int epilogue, int a_upper, int b_upper, int c_upper_only, llmc_stream_t stream);
/* The k-major product (TA) of llmc_test_gemm3 in the form K3's large far updates use: both operands are first split into
 * their three bf16 planes in `ws` (6 * Kd * roundup8(max(M, N)) * 2 bytes, 16-B aligned), then multiplied by the
 * producer / MFMA-wave kernel (gemm3.hip, k_gemm3s). M % 8 == 0, N % 8 == 0, Kd a multiple of 64 and >= 128. Returns
 * LLMC_ENOTSUP when the product would not run on the planes: the shape is not eligible (too few tiles unless the option
 * gemm3s_min_tiles lowers the bar), or the launcher would refuse the arguments (misaligned operands, N % 4 != 0); nothing is split
 * or launched then. */
int llmc_test_gemm3_planes(const float* A, const float* B, float* C, int64_t lda, int64_t ldb, int64_t ldc, int M, int N,
                           int Kd, int epilogue, int c_upper_only, void* ws, llmc_stream_t stream);
/* tools/probes/gemm3s_probe.py: the s_memtime stamps (8 waves x 128 slots, int64) one workgroup of the last k_gemm3s
 * launch wrote under LLMC_GEMM3S_DBG=4, copied to host memory. */
int llmc_test_gemm3s_stamps(long long* host_out);
/* tests/test_chain_riders_plan.py: the launches llmc_gptq_quantize_cols issues on one stream (no helper streams) for these
 * shapes under the calling thread's options, in order, as records of 12 int32: kind (0 in-block kernel, 1 near update, 2 the
 * next group's columns of a far update cut in three (k4_split_far), 3 far update, 4 flush of queued rider tiles), column
 * group, the columns written [w0, w1), the err buffer read / written (-1: none), for an in-block launch that carries riders
 * their group, columns [r0, r1) and err buffer (group -1: none), and the range [k0, k1) of the group's 512 err columns that
 * riders or a flush apply (0, 0: all). Every field is read back from the arguments the launch would get. Pure host call.
 * Returns the number of records (only the first `cap` are written) or an error. */
int llmc_test_gptq_rider_plan(int64_t R, int64_t K, int64_t n_quant, int64_t group_size, int static_groups, int32_t* out,
                              int cap);
/* tests/test_gptq_pipe_plan.py: the same for the helper-stream schedule, whatever llmc_hip_set_helper_streams says. Records of 13
 * int32: the 12 fields above and the lane the launch is issued on (0 chain = the caller's stream, 1 bulk). Between them event
 * rows in issue order: kind 5 (record) or 6 (wait), the event's id (from 1, each recorded once) in the second field, the lane
 * that records or waits in the last. Lanes run in order; a wait puts what follows it on its lane behind everything the recording
 * lane had issued before the record. Pure host call. */
int llmc_test_gptq_pipe_plan(int64_t R, int64_t K, int64_t n_quant, int64_t group_size, int static_groups, int32_t* out,
                             int cap);
/* tests/test_chol_plan.py: the launches llmc_chol_inv_upper (rev: llmc_chol_inv_upper_rev) issues for this K under the calling
 * thread's options, in order; with_lanes: the helper-stream schedule, whatever llmc_hip_set_helper_streams says, else the
 * one-stream schedule. Records of 22 int32, with lanes 23:
 *   [0] kind: 0 antitranspose, 1 k_potrf_inv, 2 panel solve, 3 in-block update, 4 plane split, 7 far update, 8 k_place_diag_inv,
 *       9 k_zero_subdiag, 10 / 11 the X = A^-1 C / C = -X B^-1 product of an inverse level;
 *   [1] form: 0 the kernel named by the kind, 1 fp32 product (sgemm), 2 split-bf16 product (gemm3), 3 gemm6;
 *   [2..6] the rectangle written, [7..11] and [12..16] up to two rectangles read, [17..21] a second rectangle written
 *       (k_potrf_inv: the V block; gemm6: its workspace). A rectangle is buffer, rows [r0, r1), columns [c0, c1); buffer 0 the
 *       working matrix (K x K), 1 the V blocks (128 columns), 2 X / bf16 planes and 3 the gemm6 workspace (both flat: rows [0, 1),
 *       columns counted in floats), 4 the caller's other matrix (K x K: the input before, U after), -1 none. A batched product's
 *       rectangles are the hull of its first and last problem;
 *   [22] the lane (0 chain = the caller's stream, 1 bulk).
 * Every field is read back from the pointers and leading dimensions the launch would get. Event rows as in
 * llmc_test_gptq_pipe_plan: kind 5 / 6, the event's id in [1], every buffer -1, the lane last. Pure host call. Returns the number
 * of records (only the first `cap` are written) or an error. */
int llmc_test_chol_plan(int64_t K, int rev, int with_lanes, int32_t* out, int cap);
/* tests/test_gemm_route.py: which kernel llmc_test_sgemm / llmc_test_gemm3 / K3 / K4 would launch for a product, and how, under the
 * calling thread's options. Pure host call: the operands are fake addresses, 256-B aligned and far apart. in, 30 int64:
 *   [0] family (0 sgemm, 1 gemm3), [1..3] M, N, Kd, [4..6] lda, ldb, ldc, [7] TA, [8] TB (sgemm only), [9] epilogue,
 *   [10..13] a_upper, a_lower, b_upper, c_upper_only, [14] phase_len, [15] batch, [16..18] M_last, N_last, Kd_last, [19..21] sA, sB,
 *   sC, [22] planes given, [23] ldp, [24] plane_stride, [25] aliasing (0 none, 1 C == B, 2 C == A), [26..29] bytes added to the
 *   addresses of A, B, C, both planes.
 * out, 18 int32: status (0 or the error the launcher would return), kernel (0 k_sgemm, 1 k_sgemm_shortk, 2 k_sgemm_shortk_phased,
 *   3 / 4 k_sgemm_wide<2> / <4>, 5 k_gemm3, 6 k_gemm3s, 7 k_gemm3s on planes, 8 k_gemm3w), grid x, y, z, threads, dynamic LDS bytes,
 *   ta, tb, phased, edge (k_sgemm's instantiation), effective phase_len, planes_dma, sm_log, sn_log, sbm, nsb (the wide kernels'
 *   tile blocks), and the k_sgemm_wide form the arguments qualify for (0, 2, 4) whether or not a short-K kernel comes first.
 *   Everything after status is meaningful only for status 0 and a launch. Returns 1 when nothing would be launched (M, N or
 *   batch <= 0), else 0. */
int llmc_test_gemm_route(const int64_t* in, int32_t* out);
/* tests/test_linear_route.py, tests/test_linear_eval_exact_gpu.py: what llmc_linear_eval / llmc_linear_eval_kt would launch for a
 * call, under the calling thread's options (linear_nosplit). The launchers fill their kernel arguments from the same record. Pure
 * host call: the buffers are fake addresses, 16-B aligned and far apart. in, 16 int64:
 *   [0] entry (0 llmc_linear_eval, 1 llmc_linear_eval_kt), [1] dt, [2..4] N, K, R, [5] mode (flags), [6..9] Yout, Y0, loss_sum, ws
 *   given (0: NULL), [10..14] bytes added to the addresses of X, W, Yout, Y0, ws, [15] compute units of the device (0: ask the
 *   current device; 256 where there is none).
 * out, 12 int32: status (0 or the error the launcher would return, its message in llmc_hip_last_error), kernel (0 k_linear_eval, 1
 *   k_linear_eval4), grid, threads, sbm, sbn, nrounds (the tile order: each of the 8 XCDs works on one sbm x sbn block of tiles per
 *   round), ksplit (1: single pass), store (mode 0: 0 two-byte stores from the accumulators, 1 rows staged through LDS and stored
 *   16 B per lane, 2 tile-blocked, 3 fp32 k-slices + the reduction kernel; mode 1: -1), STAGE_Y (mode 1: 0 Y0 read from global
 *   memory, 1 row-major Y0 staged through LDS, 2 tile-blocked Y0 staged; mode 0: -1), tile rows (k-slices included) and tile
 *   columns. Everything after status is meaningful only for status 0. Returns 0, or LLMC_EINVAL for a NULL argument. */
int llmc_test_linear_route(const int64_t* in, int32_t* out);

#ifdef __cplusplus
}
#endif
#endif /* LLMC_HIP_TEST_H_ */
