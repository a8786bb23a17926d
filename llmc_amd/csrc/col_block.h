// col_block.h — the block scaffold of the row-resident column loops (spqr_loop.hip, sparsegpt_loop.hip): W [R, K] is walked in
// blocks of 128 columns against the upper factor U [K, K]. Inside a block a workgroup of 256 threads holds 16 rows: a wave owns
// 4 rows, 16 lanes per row, lane p owns columns p, p+16, ..., p+112 of the block (register e = column p + 16 e), so the 16
// columns of a stripe sit in the 16 lanes of the row at one register index. U[i1:i2, i1:i2] waits in LDS in that ownership
// order; a column step broadcasts its err over the row's lanes and every lane updates its 8 registers from one 32-byte read.
// After the block the host issues W[:, i2:] -= Err1 @ U[i1:i2, i2:] on sgemm.hip's k-ordered fp32 fma chain.
// (gptq_block_body.h has the same ownership with a staging of its own; it does not use this header.)
#pragma once
#include "common.h"
#include "sgemm.h"

namespace llmc {

constexpr int CB_BS = 128;   // columns of a block
constexpr int CB_NT = 256;   // threads per workgroup: 4 waves x 4 rows x 16 lanes

// v of lane po of every 16-lane row (ds_bpermute: po is a loop counter, the 16 steps of a stripe are a real loop — unrolled,
// the 128 steps with their IEEE divisions and hoisted LDS reads spill hundreds of registers)
__device__ __forceinline__ float row_lane(float v, int po) {
    const int src = ((int)(threadIdx.x & 48) | po) << 2;
    return __int_as_float(__builtin_amdgcn_ds_bpermute(src, __float_as_int(v)));
}

// column step i of the block: w[e] = w[e] - fl(e1 * U[i][p + 16 e]), one rounding per op; us = Us + p * 8. Columns up to i read 0.
__device__ __forceinline__ void col_rank1(float (&w)[8], float e1, const float* us, int i) {
    const float* ur = us + i * CB_BS;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float t = e1 * ur[e];
        w[e] = w[e] - t;
    }
}

// host: the blocks of [0, K) in order. launch(i1, count) enqueues the block's kernels (they leave the block's err in Err [R, 128])
// and returns an error code; the trailing update follows. The first error ends the walk.
template <typename Launch>
inline int col_blocks(float* W, const float* U, float* Err, int64_t R, int64_t K, hipStream_t st, Launch&& launch) {
    for (int64_t i1 = 0; i1 < K; i1 += CB_BS) {
        const int count = (int)(K - i1 < CB_BS ? K - i1 : CB_BS);
        if (int rc = launch((int)i1, count)) return rc;
        const int64_t i2 = i1 + count;
        if (i2 < K) {   // W[:, i2:] -= Err1 @ U[i1:i2, i2:]
            SgemmArgs g{};
            g.A = Err; g.lda = CB_BS;
            g.B = U + i1 * K + i2; g.ldb = K;
            g.C = W + i2; g.ldc = K;
            g.M = g.M_last = (int)R; g.N = g.N_last = (int)(K - i2); g.Kd = g.Kd_last = count;
            g.epilogue = SG_SUB; g.batch = 1;
            if (int rc = sgemm_launch(g, false, false, st)) return rc;
        }
    }
    return LLMC_OK;
}

}  // namespace llmc
