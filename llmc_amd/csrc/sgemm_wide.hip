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

// form: 0 = none, 4 = 256 x 128 tiles (one workgroup per CU), 2 = 128 x 128 tiles (two per CU)
static int wide_form(const SgemmArgs& a, bool TA, bool TB) {
    if (!TA || TB || a.batch != 1 || a.epilogue != SG_SUB || a.phase_len != 128) return 0;
    if (a.a_upper || a.a_lower || a.b_upper || a.c_upper_only) return 0;
    if (a.M <= 0 || a.N <= 0 || a.M % 128 || a.N % W_BN || a.Kd % 128 || a.Kd < 128) return 0;
    if ((a.lda % 4) || (a.ldb % 4) || ((uintptr_t)a.A & 15) || ((uintptr_t)a.B & 15) || ((uintptr_t)a.C & 3)) return 0;
    const int64_t lim = (int64_t)1 << 31;
    if ((int64_t)a.Kd * a.lda * 4 >= lim || (int64_t)a.Kd * a.ldb * 4 >= lim || (int64_t)256 * a.ldc * 4 >= lim) return 0;
    if ((const void*)a.C == (const void*)a.A || (const void*)a.C == (const void*)a.B) return 0;
    const int v = opt(OPT_SGEMM_NO_WIDE);      // 0: the default form, 1: never, 2 / 4: that form where the shape allows it
    if (v == 1) return 0;
    if (v == 4) return a.M % 256 ? 2 : 4;
    return 2;      // measured (profiles/r06_sgemm_wide_ab.txt): two 128 x 128 workgroups per CU beat one 256 x 128 on every shape of the column loop
}
bool sgemm_wide_eligible(const SgemmArgs& a, bool TA, bool TB) { return wide_form(a, TA, TB) != 0; }

int sgemm_wide_form(const SgemmArgs& a, bool TA, bool TB) { return wide_form(a, TA, TB); }

template <int MB> static int wide_launch(const SgemmArgs& a, hipStream_t st) {
    using W = Wide<MB>;
    WideArgs w{};
    wide_operands<MB>(a, w);
    // The shape of an XCD's tile block: the one whose busiest XCD has the fewest tiles (block g goes to XCD g % 8; a ragged last
    // block column or a block count that is not a multiple of 8 leaves XCDs idle in the last round — the column loop's far updates
    // shrink by four tile columns per launch, most of them are a few rounds long), the squarest among equals (fewest panels in L2).
    int best_cost = 1 << 30, best_sm = 0;
    constexpr int LOGT = MB == 4 ? 5 : 6;
    for (int sm = 1; sm < LOGT; ++sm) {
        const int SM = 1 << sm, SN = 1 << (LOGT - sm);
        const int sbm = (w.tm + SM - 1) / SM, sbn = (w.tn + SN - 1) / SN;
        int load[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int g = 0; g < sbm * sbn; ++g) {
            const int bi = g % sbm, bj = g / sbm;
            load[g & 7] += (w.tm - bi * SM < SM ? w.tm - bi * SM : SM) * (w.tn - bj * SN < SN ? w.tn - bj * SN : SN);
        }
        int mx = 0;
        for (int x = 0; x < 8; ++x) mx = load[x] > mx ? load[x] : mx;
        const int cost = mx * 64 + (SM + SN);
        if (cost < best_cost) { best_cost = cost; best_sm = sm; }
    }
    w.sm_log = best_sm; w.sn_log = LOGT - best_sm;
    w.sbm = (w.tm + (1 << w.sm_log) - 1) >> w.sm_log;
    w.nsb = w.sbm * ((w.tn + (1 << w.sn_log) - 1) >> w.sn_log);
    const int rounds = (w.nsb + 7) / 8;
    if (int rc = ensure_dynamic_lds((const void*)k_sgemm_wide<MB>, W::LDS)) return rc;
    hipLaunchKernelGGL(k_sgemm_wide<MB>, dim3(rounds * 8 * W::PER_XCD), dim3(256), W::LDS, st, w);
    LLMC_LAUNCH_CHECK();
    return LLMC_OK;
}
int sgemm_wide_launch(const SgemmArgs& a, hipStream_t st) {
    return wide_form(a, true, false) == 4 ? wide_launch<4>(a, st) : wide_launch<2>(a, st);
}

}  // namespace llmc
