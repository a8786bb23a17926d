// gptq_loop_e4m3.hip — the in-block kernels of GPTQ's column loop for the e4m3 grid (qtorch rounding), a translation unit of
// their own so that they compile beside the integer ones (gptq_block_kernels.h; the loop itself is gptq_loop.hip).
#include "gptq_block_kernels.h"

namespace llmc {

int gptq_launch_in_block_e4m3(const GptqBlockArgs& a, int variant, int nt, int grid, const RiderArgs* ra, hipStream_t st) {
    return launch_in_block<QK_E4M3>(a, variant, nt, grid, ra, st);
}

}  // namespace llmc
