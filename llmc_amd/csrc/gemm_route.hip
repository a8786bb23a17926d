// gemm_route.hip — which kernel runs an internal product (sgemm.h): the two routers, pure host functions of the arguments and the
// calling thread's options. They read no device property and launch nothing, so llmc_test_gemm_route answers without a GPU.
#include "sgemm_wide_tile.h"

namespace llmc {
namespace {
GemmRoute refuse(GemmRoute r, int status, const char* msg) { r.status = status; r.msg = msg; return r; }
GemmRoute tiles(GemmRoute r, int kernel, const SgemmArgs& a, int bm, int bn, bool one_row = false) {
    r.kernel = kernel; r.gx = (a.N + bn - 1) / bn; r.gy = one_row ? 1 : (a.M + bm - 1) / bm; r.gz = a.batch;
    return r;
}
// The shape of an XCD's tile block for the 1-D grids of the wide kernels (block g goes to XCD g % 8, 2^logt tiles per block): the one whose busiest
// XCD has the fewest WORKING tiles — a ragged last block column or a block count that is not a multiple of 8 leaves XCDs idle in the last round, and
// with `upper` only the tiles on or right of the diagonal work — the squarest among equals (fewest panels in L2). The grid: whole rounds of 8 blocks.
GemmRoute tile_blocks(GemmRoute r, int kernel, int tm, int tn, int logt, bool upper, int lds) {
    int best_cost = 1 << 30;
    for (int sm = 1; sm < logt; ++sm) {
        const int SM = 1 << sm, SN = 1 << (logt - sm);
        const int sbm = (tm + SM - 1) / SM, sbn = (tn + SN - 1) / SN;
        int load[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int g = 0; g < sbm * sbn; ++g) {
            const int i0 = (g % sbm) * SM, j0 = (g / sbm) * SN;
            for (int i = i0; i < i0 + SM && i < tm; ++i) {
                const int jlo = upper && i > j0 ? i : j0, jhi = j0 + SN < tn ? j0 + SN : tn;
                if (jhi > jlo) load[g & 7] += jhi - jlo;
            }
        }
        int mx = 0;
        for (int x = 0; x < 8; ++x) mx = load[x] > mx ? load[x] : mx;
        const int cost = mx * 64 + (SM + SN);
        if (cost < best_cost) { best_cost = cost; r.sm_log = sm; }
    }
    r.sn_log = logt - r.sm_log;
    r.sbm = (tm + (1 << r.sm_log) - 1) >> r.sm_log;
    r.nsb = r.sbm * ((tn + (1 << r.sn_log) - 1) >> r.sn_log);
    r.kernel = kernel; r.lds = lds; r.gx = (unsigned)((r.nsb + 7) / 8 * 8) << logt; r.gy = r.gz = 1;
    return r;
}
// K4's phased far update (TA, op(B) = N, SG_SUB, phase 128, whole tiles) on k_sgemm_wide<MB>: 0 = not eligible, 4 = 256 x 128 tiles, 2 = 128 x 128 (two per CU)
int wide_form(const SgemmArgs& a, bool TA, bool TB) {
    if (!TA || TB || a.batch != 1 || a.epilogue != SG_SUB || a.phase_len != 128) return 0;
    if (a.a_upper || a.a_lower || a.b_upper || a.c_upper_only) return 0;
    if (a.M % 128 || a.N % wide::W_BN || a.Kd % 128 || a.Kd < 128 || ((uintptr_t)a.C & 3)) return 0;      // A, B: sgemm_route's refusal
    const int64_t lim = (int64_t)1 << 31;
    if ((int64_t)a.Kd * a.lda * 4 >= lim || (int64_t)a.Kd * a.ldb * 4 >= lim || (int64_t)256 * a.ldc * 4 >= lim) return 0;
    if ((const void*)a.C == (const void*)a.A || (const void*)a.C == (const void*)a.B) return 0;
    // option: 1 never, 4 that form where the shape allows it; else 2 (measured, profiles/r06_sgemm_wide_ab.txt: two 128 x 128 workgroups per CU
    // beat one 256 x 128 on every shape of the column loop)
    const int v = opt(OPT_SGEMM_NO_WIDE);
    return v == 1 ? 0 : v == 4 && a.M % 256 == 0 ? 4 : 2;
}
// k_gemm3s, the specialised kernel for large k-major products without operand hints; everything else stays on k_gemm3
bool gemm3s_eligible(const SgemmArgs& a) {
    if (opt(OPT_GEMM3_NOSPEC)) return false;
    if (a.a_upper || a.a_lower || a.b_upper) return false;
    if ((((uintptr_t)a.C) & 15) || a.ldc % 4 || a.sC % 4) return false;            // 16-B accesses to C
    if ((int64_t)S_BM * a.ldc * 4 >= (int64_t)0x7fffff00) return false;             // 32-bit offsets inside a C tile
    const int64_t kd = a.Kd > a.Kd_last ? a.Kd : a.Kd_last;
    const bool pre = a.planesA != nullptr;
    if (a.Kd % (2 * G3K) || a.Kd_last % (2 * G3K) || a.Kd < 4 * G3K || a.Kd_last < 4 * G3K) return false;   // an even number of K-steps, >= 4
    // the planes of ONE panel, 16-B rows; 32-bit offsets from the tile's first element
    if (pre && (a.batch != 1 || a.ldp % 8 || a.plane_stride % 8 || (((uintptr_t)a.planesA | (uintptr_t)a.planesB) & 15))) return false;
    const int64_t extent = pre ? (2 * a.plane_stride + (kd + G3K) * a.ldp) * 2 : (kd + G3K) * (a.lda > a.ldb ? a.lda : a.ldb) * 4;
    if (extent >= (int64_t)0x7fffff00) return false;
    // one workgroup per CU: worth it once the tiles that do work come near filling the chip
    const int64_t tm = (a.M + S_BM - 1) / S_BM, tn = (a.N + S_BN - 1) / S_BN;
    const int64_t tiles = a.c_upper_only ? tm * tn - tm * (tm - 1) : tm * tn;      // row r of tiles skips its first 2r columns
    const int mt = opt(OPT_GEMM3S_MIN_TILES);               // the tests lower it to reach the kernel with small shapes
    const int min_tiles = mt > 0 ? mt : (pre ? 48 : 256);   // bench: 48 -> 93.75, 160 -> 93.98 / 94.20, 600 -> 94.48, never -> 95.14 ms per step
    return tiles * a.batch >= min_tiles;
}
// k_gemm3w, the planes form on 128 x 128 tiles with two workgroups per CU: SG_SUB, whole tiles, planes given (asked after gemm3s_eligible)
bool gemm3w_eligible(const SgemmArgs& a) {
    if (opt(OPT_GEMM3_NO_WIDE)) return false;
    if (!a.planesA || !a.planesB || a.epilogue != SG_SUB || a.M % G_B || a.N % G_B) return false;
    if ((2 * a.plane_stride + ((int64_t)a.Kd + G_K) * a.ldp) * 2 >= (int64_t)0x7fffff00 || (int64_t)G_B * a.ldc * 4 >= (int64_t)0x7fffff00) return false;
    const int64_t tm = a.M / G_B, tn = a.N / G_B;
    const int64_t tiles = a.c_upper_only ? tm * tn - tm * (tm - 1) / 2 : tm * tn;
    const int mt = opt(OPT_GEMM3S_MIN_TILES);
    return tiles >= (mt > 0 ? mt : 1024);      // measured (profiles/r06_gemm3w_ab.txt): n = 3584 (406 tiles) 68 vs 54 us for k_gemm3s, n = 8192 (2080) 236-260 vs 268
}

}  // namespace
GemmRoute sgemm_route(const SgemmArgs& a, bool TA, bool TB) {
    GemmRoute r{}; r.threads = 256; r.ta = TA; r.tb = TB; r.phase_len = a.phase_len;
    if (a.M <= 0 || a.N <= 0 || a.batch <= 0) { r.empty = true; return r; }
    if ((a.lda % 4) || (a.ldb % 4) || ((uintptr_t)a.A & 15) || ((uintptr_t)a.B & 15) || (a.sA % 4) || (a.sB % 4))
        return refuse(r, LLMC_EINVAL, "sgemm: operands must be 16-B aligned with ld % 4 == 0");
    r.wide_form = wide_form(a, TA, TB);
    const bool in_place = (const void*)a.C == (const void*)a.B;
    const bool shortk = !TB && a.batch == 1 && !a.a_upper && !a.b_upper && !opt(OPT_NO_SHORTK);
    if (shortk && a.Kd <= SKD && (a.phase_len == 0 || a.phase_len >= a.Kd)) return tiles(r, GK_SHORTK, a, SB, SB, in_place);
    r.phased = true;      // few-tile phased products (phase = 128) on 64x64 tiles: the latency-critical slice of K4's far update
    if (shortk && a.epilogue == SG_SUB && a.phase_len == SKD && a.Kd % SKD == 0 && a.Kd > SKD && !a.a_lower &&
        (int64_t)((a.M + SB - 1) / SB) * ((a.N + SB - 1) / SB) <= 1024)
        return tiles(r, GK_SHORTK_PHASED, a, SB, SB);
    if (r.wide_form == 4) return tile_blocks(r, GK_WIDE4, a.M / 256, a.N / wide::W_BN, 5, false, wide::Wide<4>::LDS);
    if (r.wide_form == 2) return tile_blocks(r, GK_WIDE2, a.M / 128, a.N / wide::W_BN, 6, false, wide::Wide<2>::LDS);
    if (in_place && (a.M > GB || a.batch != 1)) return refuse(r, LLMC_EINVAL, "sgemm: in-place C = op(A) B needs a single row tile (M <= 128)");
    if (a.phase_len == 0 && a.epilogue == SG_SUB && !a.a_upper && !TB) r.phase_len = 1 << 30;
    r.phased = r.phase_len > 0;
    if (r.phased && (r.phase_len % GK || a.epilogue != SG_SUB || a.a_upper)) return refuse(r, LLMC_EINVAL, "sgemm: bad phased configuration");
    if (r.phased && TB) return refuse(r, LLMC_ENOTSUP, "sgemm: phased mode supports op(B) = N only");
    // interior-only instantiation when every tile and K range is whole (the shapes of the 128-aligned layers)
    auto whole = [&](int M, int N, int Kd) { return M % GB == 0 && N % GB == 0 && Kd % GK == 0; };
    r.edge = !(whole(a.M, a.N, a.Kd) && whole(a.M_last, a.N_last, a.Kd_last));
    return tiles(r, GK_SGEMM, a, GB, GB);
}

GemmRoute gemm3_route(const SgemmArgs& a, bool TA) {
    GemmRoute r{}; r.threads = 256; r.ta = TA;
    if (a.M <= 0 || a.N <= 0 || a.batch <= 0) { r.empty = true; return r; }
    if (a.phase_len != 0) return refuse(r, LLMC_EINVAL, "gemm3: no phased mode");
    if ((a.lda % 4) || (a.ldb % 4) || (a.N % 4) || (a.N_last % 4) || (TA && (a.M % 4 || a.M_last % 4)) || ((uintptr_t)a.A & 15) ||
        ((uintptr_t)a.B & 15) || (a.sA % 4) || (a.sB % 4))
        return refuse(r, LLMC_EINVAL, "gemm3: operands must be 16-B aligned with ld and sizes multiples of 4");
    if ((const void*)a.C == (const void*)a.B || (const void*)a.C == (const void*)a.A) return refuse(r, LLMC_EINVAL, "gemm3: no in-place product");
    if (!TA || !gemm3s_eligible(a)) return tiles(r, GK_GEMM3, a, G3B, G3B);
    if (gemm3w_eligible(a)) return tile_blocks(r, GK_GEMM3W, a.M / G_B, a.N / G_B, 6, a.c_upper_only != 0, G_LDS);
    r.threads = 512; r.lds = S_LDS; r.planes_dma = opt(OPT_GEMM3S_NO_DMA) ? 0 : 1;
    return tiles(r, a.planesA ? GK_GEMM3S_PRE : GK_GEMM3S, a, S_BM, S_BN);
}

}  // namespace llmc

// C ABI test hook (include/llmc_hip_test.h): the route of a product given as numbers, on addresses that are only compared and tested for alignment
extern "C" int llmc_test_gemm_route(const int64_t* in, int32_t* out) {
    if (!in || !out) return LLMC_EINVAL;
    char* const base = (char*)(uintptr_t)((uint64_t)1 << 40);
    const size_t span = (size_t)1 << 36;
    llmc::SgemmArgs a{};
    a.M = (int)in[1]; a.N = (int)in[2]; a.Kd = (int)in[3]; a.lda = in[4]; a.ldb = in[5]; a.ldc = in[6];
    a.epilogue = (int)in[9]; a.a_upper = (int)in[10]; a.a_lower = (int)in[11]; a.b_upper = (int)in[12]; a.c_upper_only = (int)in[13];
    a.phase_len = (int)in[14]; a.batch = (int)in[15]; a.M_last = (int)in[16]; a.N_last = (int)in[17]; a.Kd_last = (int)in[18];
    a.sA = in[19]; a.sB = in[20]; a.sC = in[21]; a.ldp = in[23]; a.plane_stride = in[24];
    a.A = (const float*)(base + in[26]); a.B = (const float*)(base + span + in[27]);
    a.C = in[25] == 1 ? (float*)a.B : in[25] == 2 ? (float*)a.A : (float*)(base + 2 * span + in[28]);
    if (in[22]) a.planesA = base + 3 * span + in[29], a.planesB = base + 4 * span + in[29];
    const llmc::GemmRoute r = in[0] ? llmc::gemm3_route(a, in[7] != 0) : llmc::sgemm_route(a, in[7] != 0, in[8] != 0);
    const int32_t v[18] = {r.status, r.kernel, (int32_t)r.gx, (int32_t)r.gy, (int32_t)r.gz, r.threads, r.lds, r.ta, r.tb, r.phased, r.edge,
                           r.phase_len, r.planes_dma, r.sm_log, r.sn_log, r.sbm, r.nsb, r.wide_form};
    memcpy(out, v, sizeof v);
    return r.empty ? 1 : 0;
}
