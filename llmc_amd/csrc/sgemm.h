// sgemm.h — internal fp32 GEMM on the f32 MFMA pipe (v_mfma_f32_32x32x2_f32), used by the GPTQ
// Cholesky / triangular inverse (K3) and the GPTQ trailing update (K4).
//
// Numerics contract (relied on by K4's bit-exact parity): every output element is ONE accumulator that
// receives its products in ascending k order, acc = fma(a_k, b_k, acc) starting from +0 — exactly the
// chain MKL's sgemm produces for the reference on CPU (tests/test_oracle_golden.py pins that) — and the
// epilogue applies C = C - acc (or = acc / = -acc) as one further rounding.
#pragma once
#include "common.h"

namespace llmc {

enum SgemmEpilogue { SG_SUB = 0 /* C -= AB */, SG_SET = 1 /* C = AB */, SG_NEG = 2 /* C = -AB */ };

struct SgemmArgs {
    const float* A;  // op(A) is [M x Kd]; stored [M x Kd] (TA=false) or [Kd x M] (TA=true), row-major, ld = lda
    const float* B;  // op(B) is [Kd x N]; stored [Kd x N] (TB=false) or [N x Kd] (TB=true)
    float* C;        // [M x N], ldc
    int64_t lda, ldb, ldc;
    int M, N, Kd;
    int epilogue;
    // structure hints (skip work that multiplies known zeros; never changes a result bit)
    int a_upper;     // op(A)[i][k] == 0 for k < i  -> start k at the tile's first row
    int a_lower;     // op(A)[i][k] == 0 for k > i  -> stop k after the tile's last row
    int b_upper;     // op(B)[k][j] == 0 for k > j  -> stop k after the tile's last column
    int c_upper_only;  // only tiles that intersect j >= i are computed/stored (symmetric update, upper half)
    // phased accumulation (SG_SUB only): every `phase_len` k (a multiple of 16) the accumulator is subtracted
    // from the C tile held in registers and reset to +0:  C -= A[:, p] B[p, :] phase by phase, i.e. exactly what
    // Kd / phase_len separate launches would compute, with one read and one write of C. 0 = single phase.
    int phase_len;
    // batch: blockIdx.z-th problem at A + z*sA etc.; dims of the LAST problem may be smaller
    int64_t sA, sB, sC;
    int batch;
    int M_last, N_last, Kd_last;
    // gemm3 only (k-major A and B): the operands already split into bf16 planes (gemm3_split_planes) — hi | mid | lo planes of
    // `plane_stride` elements each, row stride ldp, pointing at the operand's first column. nullptr = split in the kernel.
    const void* planesA;
    const void* planesB;
    int64_t ldp, plane_stride;
    int planes_dma;   // set by gemm3_launch from the route
};

// Which kernel runs a product is data: a pure function of the arguments and the calling thread's options (gemm_route.hip; no device
// is read, nothing is launched; table: DESIGN.md "The GEMM routes"). The launchers launch what it says; callers that must know ask it too.
enum GemmKernel { GK_SGEMM, GK_SHORTK, GK_SHORTK_PHASED, GK_WIDE2, GK_WIDE4, GK_GEMM3, GK_GEMM3S, GK_GEMM3S_PRE, GK_GEMM3W };
// tile geometry the routers share with the kernels. k_sgemm: tile edge, K-step; k_sgemm_shortk[_phased]: tile edge, max K / phase
constexpr int GB = 128, GK = 16, SB = 64, SKD = 128;
constexpr int G3B = 128, G3K = 32, S_BM = 256, S_BN = 128, S_LDS = 144 * 1024;      // k_gemm3: tile edge, K-step; k_gemm3s: tile, LDS bytes
constexpr int G_B = 128, G_K = 16, G_LDS = 72 * 1024;     // k_gemm3w: tile edge, stage depth, LDS bytes
struct GemmRoute {
    int status; const char* msg;    // LLMC_OK, or the refusal and its message
    int kernel;                     // GemmKernel; meaningless unless status == LLMC_OK and !empty
    bool empty;                     // M, N or batch <= 0: nothing is launched, LLMC_OK
    unsigned gx, gy, gz; int threads, lds;      // launch geometry, dynamic LDS bytes
    bool ta, tb, phased, edge;      // k_sgemm's instantiation; ta / tb as given for the others
    int phase_len;                  // effective: a plain C -= AB on k_sgemm is ONE phase over the whole K loop (1 << 30)
    int planes_dma;                 // k_gemm3s: the planes form's producers copy by LDS-DMA (0: through registers, option gemm3s_no_dma)
    int sm_log, sn_log, sbm, nsb;   // wide kernels: an XCD's tile block = 2^sm_log x 2^sn_log tiles; tile blocks along M; tile blocks
    int wide_form;                  // sgemm: the k_sgemm_wide<MB> the arguments qualify for (0: none), even where a short-K kernel
                                    // takes the product first: K4's riders run that kernel's tile function themselves
    bool planes() const { return status == LLMC_OK && !empty && (kernel == GK_GEMM3S_PRE || kernel == GK_GEMM3W); }      // reads a.planesA / planesB
};
GemmRoute sgemm_route(const SgemmArgs& a, bool TA, bool TB);
// C (op) op(A) B on the 16-bit MFMA pipe with three bf16 terms per fp32 operand (gemm3.hip, gemm3_wide.hip): fp32-level accuracy, NOT the
// bitwise fma chain above — K3 only. op(B) = N; all hints, epilogues, batch; large k-major products read a.planesA / planesB where given
GemmRoute gemm3_route(const SgemmArgs& a, bool TA);
// launch on `st` what the router says, return LLMC_* status; below them the launch step of the routes whose kernels live in sgemm_wide.hip / gemm3_wide.hip
int sgemm_launch(const SgemmArgs& a, bool TA, bool TB, hipStream_t st);
int gemm3_launch(const SgemmArgs& a, bool TA, hipStream_t st);
int sgemm_wide_launch(const SgemmArgs& a, const GemmRoute& r, hipStream_t st);
int gemm3w_launch(const SgemmArgs& a, const GemmRoute& r, hipStream_t st);
// hi | mid | lo bf16 planes of a k-major fp32 panel [rows x n] (n % 8 == 0): planes + t * plane_stride + r * ldp + c
int gemm3_split_planes(const float* P, int64_t ld, int rows, int n, void* planes, int64_t ldp, int64_t plane_stride, hipStream_t st);

// C [M, N] = sign * A B (A [M, Kd] row-major, B [Kd, N] k-major, fp32) with the same three-bf16-term arithmetic on the
// one-wave-per-SIMD GEMM of linear_eval.hip: operands split ONCE into k-tiled stacked planes. For the large, deep levels of
// K3's triangular inverse. Kd % 256 == 0; ws: gemm6_ws_bytes, 256-B aligned.
size_t gemm6_ws_bytes(int M, int N, int Kd);
int gemm6_launch(const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, int M, int N, int Kd,
                 int a_upper, int b_upper, float sign, void* ws, hipStream_t st);

}  // namespace llmc
