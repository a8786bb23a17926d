// sgemm_wide.hip — K4's phased far update with LDS-DMA operands and XCD-dealt tiles (round 6).
//
// The product:  C -= A^T B  phase by phase (phase = 128 k), A = a column group's error columns [Kd x M] k-major, B = the same
// rows of the inverse factor [Kd x N] k-major, C = the weight columns still to come (gptq.py:240-244 applied lazily: per element
// the same subtractions in the same order as one update per 128-column block). Same arithmetic as k_sgemm (sgemm.h): ONE
// accumulator per element and phase, products added in ascending k from +0 by v_mfma_f32_32x32x2_f32, then one rounding C - acc.
//
// Why another kernel: tools/probes/mfma_f32_peak.hip measures 0.99 of the 157.3-TFLOP/s fp32 MFMA peak with nothing else in the
// loop (one to four waves per SIMD, operands from LDS or not); k_sgemm reaches 0.58-0.72 on these shapes whatever its occupancy
// or K-step (profiles/r04_chain_pmc.txt, r05_sgemm_far_experiment.txt): its operands go through registers (83 VALU instructions
// per K-step: addresses, transposing writes, the phase end) and its tiles are dealt row by row over the XCDs. Here:
//   - operands by LDS-DMA (buffer_load_dwordx4 .. lds) into a four-slot ring of 16-k stages, two stages ahead: no staging
//     registers, no address arithmetic, no ds_write; MB + 2 DMA instructions per wave and stage. The loop is one MFMA and one
//     ds_read_b32 per slot;
//   - the C tile stays in registers; a phase's accumulators start from the inline constant +0 and are subtracted from C block by
//     block under the next phase's first MFMAs;
//   - a 1-D grid dealt so that the workgroups an XCD runs at a time are one 1024 x 1024 block of tiles (12-16 panels in that XCD's
//     L2 instead of one pair per tile), blocks of one B panel on neighbouring XCDs;
//   - the k-rows an MFMA operand read touches (lanes 0-31: k, lanes 32-63: k + 1) lie 1152 B apart in LDS: the other half of the banks.
// Two forms (template MB): 256 x 128 tiles with one workgroup per CU (128 x 64 per wave: accumulators + C = 256 of a wave's 512
// registers), and 128 x 128 tiles with two workgroups per CU, whose partner covers a workgroup's first DMA round trip, C loads,
// last subtraction and stores. Measured (profiles/r06_sgemm_wide_ab.txt): 0.74-0.87 of peak for the second form, 0.65-0.81 for the
// first, 0.59-0.72 for k_sgemm; inside the column loop -17 % / -11 % of k_sgemm's time. The second form is the default.
#include "sgemm_wide_tile.h"

namespace llmc {
namespace {

using namespace wide;

template <int MB>
__global__ __launch_bounds__(256, MB == 4 ? 1 : 2) void k_sgemm_wide(const WideArgs a) {
    using W = Wide<MB>;
    extern __shared__ __attribute__((aligned(16))) char smem_w[];
    // workgroup w runs on XCD w % 8 (round-robin dispatch); the PER_XCD consecutive workgroups of an XCD are one block of tiles
    const int w = blockIdx.x;
    const int g = (w / (8 * W::PER_XCD)) * 8 + (w & 7);
    if (g >= a.nsb) return;
    const int within = (w >> 3) % W::PER_XCD;
    const int ti = ((g % a.sbm) << a.sm_log) + (within >> a.sn_log), tj = ((g / a.sbm) << a.sn_log) + (within & ((1 << a.sn_log) - 1));
    if (ti >= a.tm || tj >= a.tn) return;
    wide_tile<MB>(a, ti, tj, smem_w, threadIdx.x);
}

}  // namespace

int sgemm_wide_launch(const SgemmArgs& a, const GemmRoute& r, hipStream_t st) {
    static_assert(Wide<4>::PER_XCD == 1 << 5 && Wide<2>::PER_XCD == 1 << 6, "sgemm_route's tile blocks");
    WideArgs w{};
    if (r.kernel == GK_WIDE4) wide_operands<4>(a, w); else wide_operands<2>(a, w);
    w.sm_log = r.sm_log; w.sn_log = r.sn_log; w.sbm = r.sbm; w.nsb = r.nsb;
    void (*const k)(WideArgs) = r.kernel == GK_WIDE4 ? k_sgemm_wide<4> : k_sgemm_wide<2>;
    if (int rc = ensure_dynamic_lds((const void*)k, r.lds)) return rc;
    hipLaunchKernelGGL(k, dim3(r.gx), dim3(r.threads), r.lds, st, w);
    LLMC_LAUNCH_CHECK();
    return LLMC_OK;
}

}  // namespace llmc
