// gptq_loop_e5m2.hip — the in-block kernels of GPTQ's column loop for the e5m2 grid (qtorch rounding), a translation unit of
// their own so that they compile beside the integer ones (gptq_block_kernels.h; the loop itself is gptq_loop.hip).
#include "gptq_block_kernels.h"

namespace llmc {

int gptq_launch_in_block_e5m2(const GptqBlockArgs& a, int variant, int nt, int grid, const RiderArgs* ra, hipStream_t st) {
    return launch_in_block<QK_E5M2>(a, variant, nt, grid, ra, st);
}

}  // namespace llmc
