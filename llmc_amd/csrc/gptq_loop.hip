// gptq_loop.hip — K4: GPTQ.weight_transform (gptq.py:199-244), the blocked column loop.
//
// Rows of W are independent given U (= Hinv, the upper factor), so the serial part is 128 dependent
// column steps per 128-column block. In-block kernel: a wave owns 4 rows, 16 lanes per row, lane p owns
// columns p, p+16, ..., p+112 of the block (interleaved so every lane has the same amount of trailing
// work at every step). Step i: the owner's current w_i is broadcast inside the 16-lane group
// (ds_swizzle), every lane evaluates the quantizer chain and err = (w - q) / d redundantly, then updates
// its own later columns  w_j <- w_j - round(err * U[i][j])  (two roundings, like the reference's
// `W1[:, i:] -= err1.unsqueeze(1).matmul(Hinv1[i, i:].unsqueeze(0))`). The U block lives in LDS in the
// lanes' ownership order with its diagonal and lower part zeroed, so no predicate is needed and each
// lane's registers end up holding exactly `tmp` (the weight of each column at the time it was visited).
// Trailing update W[:, i2:] -= Err1 @ U[i1:i2, i2:] runs on the fp32 MFMA pipe (sgemm.hip) with the
// k-ordered fma chain that reproduces the reference's CPU sgemm bit for bit.
// (The other row-resident column loops, spqr_loop.hip and sparsegpt_loop.hip, share this scaffold through col_block.h.)
#include "gptq_block_kernels.h"
#include "pipe_lanes.h"

using namespace llmc;

static constexpr int GRP = 4;  // 128-column blocks per outer group (far updates are applied once per group; 8 measured the same: 12.4 vs 12.6 ms)
static constexpr int GW = BS * GRP;   // columns of an outer group = err columns of one err buffer

extern "C" size_t llmc_gptq_quantize_ws_bytes(int64_t R, int64_t K) {
    if (R <= 0 || K <= 0) return 0;
    return 3 * (size_t)((R + 3) & ~(int64_t)3) * GW * sizeof(float);   // err columns of three groups in flight (pipelined far updates)
}

extern "C" int llmc_gptq_quantize(float* W, const float* Hinv, int64_t R, int64_t K, int sym, float qmin,
                                  float qmax, int64_t group_size, int static_groups, const int32_t* col_group,
                                  float* scales, float* zeros, float* Wout, float* losses, int blocksize,
                                  void* ws, llmc_stream_t stream) {
    return llmc_gptq_quantize_cols(W, Hinv, R, K, K, sym, qmin, qmax, group_size, static_groups, col_group, scales,
                                   zeros, Wout, losses, blocksize, ws, stream);
}

// OWQ form (gptq.py:44-56,199-244 with n_nonout < columns): only the first n_quant columns are visited by the column
// loop; the trailing K - n_quant columns (the outlier columns OWQ keeps in floating point) still receive every
// block's error feedback `W[:, i2:] -= Err1 @ Hinv[i1:i2, i2:]`. Groups are clipped at n_quant like the reference's
// `min(i + group_size, columns - n_out)`.
// calib_algo = 'mse' with dynamic groups: the searched qparams of every group that starts in a block (gptq.py:216-221 ->
// get_mse_range). The reference searches W[:, i:i+g], which inside a block still holds the values the block started
// with, so each block's groups are searched on the running panel right before its in-block kernel, on the same stream.
struct MseSearch { int round_zp, nsteps, grid; float norm; };

// The host schedule (how it came about: DESIGN.md §3 "K4's host schedule"). Every weight receives the blocks' updates in the
// reference's order (block 0, 1, 2, ...), each as "W -= chain over the block's 128 k" (gptq.py:244): columns of the current outer
// group right after each block (near product), columns beyond it once per group (far product: GRP phases of 128 k, the C tile in
// registers), cut into PIECES on lanes. Column tiles are independent and every kernel that may run a piece computes an element the
// same way (one accumulator per phase from +0 in ascending k, one rounding C - acc): any cut on any lane gives the same bits as
// long as per element the updates arrive in block order — which the waits in gptq_cols_impl state and tests replay from the plans.
// The lanes (pipe_lanes.h): CHAIN carries the in-block kernel and near product per block and per group the far piece the next
// group needs; BULK the far pieces beyond the next group; RIDE pieces go on the in-block launches of the NEXT group.
struct Piece { int64_t c0, c1; int k0, k1; Lane lane; };    // columns [c0, c1), the group's err columns [k0, k1) (whole 128-k phases)
static constexpr int CARRIERS = GRP;      // in-block launches of a whole group
static_assert(CARRIERS % RIDER_PASSES == 0 && GRP % RIDER_PASSES == 0, "a group's carrying launches and phases divide into the passes");

// The far update [gend, K) of a group that ends at gend, in issue order.
//   merged (one stream, default): [gend, p0) on the chain and the tail [p0, K), p0 = max(gend2, K - 2 * rider_cols * 128), as RIDE
//     slices: per pass (ascending k) rider_cols tile columns per carrying launch, half a tile's k per launch. rider_cols = 0: p0 = K.
//   split (helper streams, or option k4_split_far on one stream): the next group's columns on the chain, then on the bulk lane the
//     columns of the group after next FIRST (all that the next group's own far update waits for), then the rest.
static int far_pieces(int64_t gend, int64_t K, bool merged, int rider_cols, Piece* p) {
    const int64_t gend2 = gend + GW < K ? gend + GW : K, gend3 = gend2 + GW < K ? gend2 + GW : K;
    if (!merged) {
        p[0] = Piece{gend, gend2, 0, GW, CHAIN}, p[1] = Piece{gend2, gend3, 0, GW, BULK}, p[2] = Piece{gend3, K, 0, GW, BULK};
        return 1 + (gend2 < K) + (gend3 < K);
    }
    const int64_t rw = (int64_t)rider_cols * 128, rspan = (CARRIERS / RIDER_PASSES) * rw;
    const int64_t p0 = (rider_cols > 0 && gend2 < K) ? (gend2 > K - rspan ? gend2 : K - rspan) : K;
    p[0] = Piece{gend, p0, 0, GW, CHAIN};
    int n = 1;
    const int kd = GW / RIDER_PASSES;
    for (int pass = 0; pass < RIDER_PASSES; ++pass)
        for (int64_t c = p0; c < K; c += rw) p[n++] = Piece{c, c + rw < K ? c + rw : K, pass * kd, (pass + 1) * kd, RIDE};
    return n;
}

// What every launch's arguments are made from: the call's pointers, dims, err layout and qparam mode. The three builders are the
// only pointer arithmetic of the loop.
struct ColCall {
    float* W; const float* U; float* Wout; float* losses; float* scales; float* zeros; const int32_t* col_group;
    int64_t R, K, NQ;
    // err columns of three groups in flight, K-MAJOR [GRP * 128][Rp] (16-B LDS writes when the GEMMs stage them as A; option
    // k4_err_rowmajor: [R][512], same bits)
    bool ekm; int64_t Rp, err_ld; float* ErrBuf[3];
    int ng, gsz, static_mode, sym; float qmin, qmax;
    const MseSearch* mse;
    int kind;     // QKind of the in-block step

    float* err(int group, int64_t k) const { return ErrBuf[group % 3] + (ekm ? k * Rp : k); }     // err column k of the group
    int64_t group_end(int64_t g0) const { return g0 + GW < NQ ? g0 + GW : NQ; }
    // columns updated right after every block: up to the end of the outer group; in the LAST group also the never-visited columns
    // beyond n_quant (their group-wide phased update could start on a ragged phase)
    int64_t near_end(int64_t g0) const { return group_end(g0) == NQ ? K : group_end(g0); }
    int count(int64_t i1) const { return (int)(NQ - i1 < BS ? NQ - i1 : BS); }

    GptqBlockArgs block(int64_t i1) const {
        GptqBlockArgs a;
        a.W = W; a.U = U; a.Wout = Wout; a.losses = losses;
        a.Err = err((int)(i1 / GW), i1 % GW); a.err_ld = (int)err_ld; a.err_kmajor = ekm ? 1 : 0;
        // mse: qparams searched per block into scales / zeros, then read like static groups in processing order
        a.scales = scales; a.zeros = zeros; a.col_group = mse ? nullptr : col_group; a.col_gsz = mse ? gsz : 1 << 30;
        a.R = R; a.K = (int)K; a.i1 = (int)i1; a.count = count(i1); a.ng = ng; a.gsz = static_mode ? BS : gsz;
        a.static_mode = static_mode; a.sym = sym; a.qmin = qmin; a.qmax = qmax;
        return a;
    }
    // W[:, c0:c1] -= Err[:, k rows] @ U[row0 : row0 + kd, c0:c1]
    SgemmArgs product(const float* A, int64_t row0, int kd, int64_t c0, int64_t c1, int phase_len) const {
        SgemmArgs g{};
        g.A = A; g.lda = err_ld; g.B = U + row0 * K + c0; g.ldb = K; g.C = W + c0; g.ldc = K;
        g.M = g.M_last = (int)R; g.N = g.N_last = (int)(c1 - c0); g.Kd = g.Kd_last = kd;
        g.epilogue = SG_SUB; g.batch = 1; g.phase_len = phase_len;
        return g;
    }
    // block i1's update of the rest of its group's columns. The GEMM wants 16-B aligned operands: a ragged n_quant (OWQ) starts
    // up to 3 columns early, on columns the loop has already visited — W is dead there (their values live in Wout)
    SgemmArgs near(int64_t i1) const {
        const int64_t g0 = i1 - i1 % GW, c0 = (i1 + count(i1)) & ~(int64_t)3;
        return product(err((int)(i1 / GW), i1 % GW), i1, count(i1), c0, near_end(g0), 0);
    }
    SgemmArgs far(int group, int64_t c0, int64_t c1, int k0, int k1) const {
        return product(err(group, k0), (int64_t)group * GW + k0, k1 - k0, c0, c1, BS);
    }
    RiderArgs riders(int group, const Piece& q, int nchain) const {
        RiderArgs ra{};
        wide::wide_operands<2>(far(group, q.c0, q.c1, q.k0, q.k1), ra.w);
        ra.nchain = nchain; ra.per = (nchain % 8 == 0 && ra.w.tm % 8 == 0) ? ra.w.tm / 8 : 0;
        return ra;
    }
};

// The launches of one call in issue order, for tests: with a recorder the loop launches nothing and touches no device. The records
// are laid out as include/llmc_hip_test.h says: PLAN_W int32 for the one-stream plan, one more (the lane) for the pipelined plan,
// which also has event rows (the event's id where a launch has its group).
enum { PLAN_BLOCK = 0, PLAN_NEAR = 1, PLAN_NEAR_FAR = 2, PLAN_FAR = 3, PLAN_FLUSH = 4, PLAN_W = 12 };
static const int32_t PLAN_BLANK[PLAN_W] = {0, 0, 0, 0, -1, -1, -1, 0, 0, -1, 0, 0};

// One place that either launches or, for a plan, writes down what WOULD be launched — read back from the very arguments the
// kernel gets (columns from C, k range from B's row, err buffer from A, lane from the stream), not from the loop's own bookkeeping.
struct Sink {
    const ColCall& o; const Lanes& ln; PlanRec* rec;
    void add(int lane, int kind, int group, int64_t w0, int64_t w1, int err_rd, int err_wr, int rgroup, int64_t r0, int64_t r1, int rerr,
             int k0, int k1) const {
        const int32_t v[PLAN_W] = {kind, group, (int32_t)w0, (int32_t)w1, err_rd, err_wr, rgroup, (int32_t)r0, (int32_t)r1, rerr, k0, k1};
        rec->row(v, lane);
    }
    int err_index(const float* pe) const { return (int)((size_t)(pe - o.ErrBuf[0]) / ((size_t)o.Rp * GW)); }
    void k_range(int group, const float* B, int64_t c0, int kd, int* k0, int* k1) const {
        *k0 = (int)((B - o.U - c0) / o.K - (int64_t)group * GW);
        *k1 = *k0 + kd;
        if (kd == GW) *k0 = *k1 = 0;      // all of the group's err columns
    }
    int product(int kind, int group, const SgemmArgs& g, hipStream_t st) const {
        if (!rec) return sgemm_launch(g, o.ekm, false, st);
        const int64_t c0 = g.C - o.W;
        int k0 = 0, k1 = 0;
        if (kind != PLAN_NEAR) k_range(group, g.B, c0, g.Kd, &k0, &k1);
        add(ln.lane_of(st), kind, group, c0, c0 + g.N, err_index(g.A), -1, -1, 0, 0, -1, k0, k1);
        return LLMC_OK;
    }
    // the in-block kernel of block a.i1 on the chain, with the rider tiles `ra` of group `rgroup` if any
    int in_block(int group, const GptqBlockArgs& a, int variant, int nt, int grid, const RiderArgs* ra, int rgroup) const {
        const hipStream_t st = ln.s[CHAIN];
        if (rec) {
            int64_t r0 = 0, r1 = 0;
            int rerr = -1, k0 = 0, k1 = 0;
            if (ra) {
                r0 = ra->w.C - o.W, r1 = r0 + (int64_t)ra->w.tn * 128, rerr = err_index(ra->w.A);
                k_range(rgroup, ra->w.B, r0, ra->w.nst * wide::W_K, &k0, &k1);
            }
            add(CHAIN, PLAN_BLOCK, group, a.i1, a.i1 + a.count, -1, err_index(a.Err), rgroup, r0, r1, rerr, k0, k1);
            return LLMC_OK;
        }
        // one translation unit per quantizer kind holds its kernels (gptq_block_kernels.h)
        return o.kind == QK_E4M3 ? gptq_launch_in_block_e4m3(a, variant, nt, grid, ra, st)
             : o.kind == QK_E5M2 ? gptq_launch_in_block_e5m2(a, variant, nt, grid, ra, st)
                                 : launch_in_block<QK_INT>(a, variant, nt, grid, ra, st);
    }
};

// Tile columns of a far update that one in-block launch carries as riders: one 128 x 128 tile per CU the chain role leaves free.
// 0: nothing rides — split schedule, shapes off whole tiles or with fewer than three groups, a chain role that fills the chip (R >=
// 8192 on 256 CUs; 1024-thread workgroups) or takes less than half of it (nearly the whole far update would ride: measured, lost).
static int rider_quota(const ColCall& o, bool merged, int nt, int grid) {
    if (!merged || opt(OPT_NO_RIDERS) || !o.ekm || nt != GBT || o.R % 128 || o.K % 128 || o.NQ <= GW || o.K <= 2 * (int64_t)GW) return 0;
    const int free_cus = device_cu_count() - grid;
    // the first group's far-far product: every later one has the same strides and alignment
    if (sgemm_route(o.far(0, 2 * GW, o.K, 0, GW), true, false).wide_form != 2 || free_cus <= 0 || 2 * grid < device_cu_count()) return 0;
    return (int)(free_cus / (o.R / 128));
}

static int gptq_cols_impl(float* W, const float* Hinv, int64_t R, int64_t K, int64_t n_quant, int sym, float qmin,
                          float qmax, int64_t group_size, int static_groups, const int32_t* col_group, float* scales,
                          float* zeros, float* Wout, float* losses, int blocksize, void* ws, llmc_stream_t stream,
                          const MseSearch* mse, PlanRec* rec = nullptr, int kind = QK_INT) {
    LLMC_REQUIRE(W && Hinv && Wout && scales && ws && R > 0 && K > 0, "gptq_quantize: null/empty argument");
    LLMC_REQUIRE(n_quant > 0 && n_quant <= K, "gptq_quantize: n_quant must be in (0, K]");
    LLMC_REQUIRE(blocksize == BS, "gptq_quantize: blocksize must be 128");
    LLMC_REQUIRE(K % 4 == 0 && K < (1 << 30), "gptq_quantize: K must be a multiple of 4");
    LLMC_REQUIRE(sym || zeros, "gptq_quantize: zeros required for asymmetric");
    const bool per_channel = group_size <= 0;
    const int static_mode = static_groups || per_channel || mse != nullptr;
    const int gsz = (int)group_size;
    if (!static_mode || mse) {
        if (!(gsz == 16 || gsz == 32 || gsz == 64 || gsz == 128)) {
            set_last_error_msg("gptq_quantize: dynamic group qparams need group_size in {16,32,64,128}");
            return LLMC_ENOTSUP;
        }
    } else if (!per_channel) {
        LLMC_REQUIRE(col_group != nullptr, "gptq_quantize: col_group required with static groups");
    }
    const bool ekm = !opt(OPT_K4_ERR_ROWMAJOR);
    const int64_t Rp = (R + 3) & ~(int64_t)3;
    const ColCall o{W, Hinv, Wout, losses, scales, zeros, per_channel ? nullptr : col_group, R, K, n_quant,
                    ekm, Rp, ekm ? Rp : GW, {(float*)ws, (float*)ws + (size_t)Rp * GW, (float*)ws + 2 * (size_t)Rp * GW},
                    per_channel ? 1 : (int)ceil_div64(K, group_size), gsz, static_mode, sym, qmin, qmax, mse, kind};
    Lanes ln((hipStream_t)stream, rec);
    const Sink sink{o, ln, rec};
    const bool merged = !ln.piped() && !opt(OPT_K4_SPLIT_FAR);
    // 64 KB of LDS per workgroup = 2 workgroups per CU: tall weights use 1024-thread workgroups so that the whole grid is resident
    // at once (R = 28672: 448 workgroups on 512 slots instead of 896)
    const int nt = R >= 16384 ? 1024 : GBT;
    const int grid = (int)ceil_div64(R, nt / 16);
    const int rider_cols = rider_quota(o, merged, nt, grid);
    const bool force_generic = opt(OPT_GPTQ_GENERIC) != 0;
    // The far update of group `fg` in pieces. pc[next .. np) is the rider queue: its RIDE pieces, worked off in order by the next
    // group's in-block launches; what is still queued when something else is about to write its columns goes out as plain launches.
    Piece pc[1 + CARRIERS];
    int np = 0, next = 0, fg = 0;
    auto flush = [&]() -> int {
        for (; next < np; ++next)
            LLMC_TRY(sink.product(PLAN_FLUSH, fg, o.far(fg, pc[next].c0, pc[next].c1, pc[next].k0, pc[next].k1), ln.s[CHAIN]));
        return LLMC_OK;
    };
    Ev reached_next{};     // bulk: the previous group's far update has reached the columns of the group after it
    Ev err_read[3] = {};   // bulk: the far update that read this err buffer is complete (the buffer may be rewritten)
    Ev bulk_tail{};        // bulk: behind its most recent launch
    LLMC_TRY(ln.fork());
    int g = 0;
    for (int64_t g0 = 0; g0 < o.NQ; g0 += GW, ++g) {
        const int64_t gend = o.group_end(g0), near_end = o.near_end(g0);
        if (near_end > gend) {
            // OWQ's last group: its per-block updates reach the never-visited columns [n_quant, K), which queued rider tiles and
            // the earlier groups' pieces on the bulk lane also write (nothing else orders the two when last_group_start + 512 < K)
            LLMC_TRY(flush());
            LLMC_TRY(ln.wait(CHAIN, bulk_tail));
        }
        // this group's err buffer was read three groups ago (implied today: the wait for reached_next one group back is behind
        // those pieces on the in-order bulk lane — stated all the same, it is the dependency)
        LLMC_TRY(ln.wait(CHAIN, err_read[g % 3]));
        for (int64_t i1 = g0; i1 < gend; i1 += BS) {
            const GptqBlockArgs a = o.block(i1);
            // group sizes 16/32/64 with qparams taken mid-block stay on the generic path (their fast variants spill: the qparams
            // change inside the unrolled loop)
            const int variant = (a.count != BS || force_generic) ? 0 : static_mode ? 1 : gsz == BS ? BS : 0;
            if (mse && !rec) {
                // every group starting in [i1, i1 + count) from the block-start panel (gsz divides 128, so groups start at
                // i1 + k * gsz; the last one is clipped at n_quant like the reference's min(i + g, columns - n_out))
                LLMC_TRY(llmc_mse_qparams_panel(W, R, K, i1, a.count, gsz, sym, mse->round_zp, qmin, qmax, mse->nsteps, mse->grid,
                                                mse->norm, scales, zeros, o.ng, i1 / gsz, (llmc_stream_t)ln.s[CHAIN]));
            }
            // riders write columns >= gend2 of the group before and read its err buffer; this group's launches write columns < gend2
            // and their own err buffer: a launch's two roles never meet
            const bool ride = next < np;
            const RiderArgs ra = ride ? o.riders(fg, pc[next++], grid) : RiderArgs{};
            LLMC_TRY(sink.in_block(g, a, variant, nt, grid, ride ? &ra : nullptr, ride ? fg : -1));
            if (i1 + a.count < near_end) LLMC_TRY(sink.product(PLAN_NEAR, g, o.near(i1), ln.s[CHAIN]));
        }
        if (near_end == K) continue;
        // the next group's columns were last written by the previous group's first piece on the bulk lane
        LLMC_TRY(ln.wait(CHAIN, reached_next));
        reached_next = Ev{};
        LLMC_TRY(flush());       // (nothing is left by now: four launches carry at most what was queued)
        np = far_pieces(gend, K, merged, rider_cols, pc);
        fg = g;
        int nbulk = 0;
        for (next = 0; next < np && pc[next].lane != RIDE; ++next) {      // RIDE pieces come last: they stay queued
            const Piece& p = pc[next];
            if (p.lane == BULK && nbulk == 0) LLMC_TRY(ln.order(CHAIN, BULK));      // this group's err columns are complete on the chain
            const int kind = (p.lane == CHAIN && !merged) ? PLAN_NEAR_FAR : PLAN_FAR;
            LLMC_TRY(sink.product(kind, g, o.far(g, p.c0, p.c1, p.k0, p.k1), ln.s[p.lane]));
            if (p.lane == BULK && nbulk++ == 0) LLMC_TRY(ln.record(BULK, &reached_next));
        }
        if (nbulk) {
            LLMC_TRY(ln.record(BULK, &err_read[g % 3]));
            bulk_tail = err_read[g % 3];
        }
    }
    LLMC_TRY(flush());
    return ln.join();
}

extern "C" int llmc_gptq_quantize_cols(float* W, const float* Hinv, int64_t R, int64_t K, int64_t n_quant, int sym,
                                       float qmin, float qmax, int64_t group_size, int static_groups,
                                       const int32_t* col_group, float* scales, float* zeros, float* Wout,
                                       float* losses, int blocksize, void* ws, llmc_stream_t stream) {
    return gptq_cols_impl(W, Hinv, R, K, n_quant, sym, qmin, qmax, group_size, static_groups, col_group, scales, zeros,
                          Wout, losses, blocksize, ws, stream, nullptr);
}

// The same loop on a FloatQuantizer grid (QK_E4M3 / QK_E5M2). The quantizer is symmetric without zero points; qmax is the
// format's largest value (finfo(float8_e4m3fn / float8_e5m2).max, quant.py:982-996) and only scales the dynamic groups' range,
// the float grid saturates by itself.
extern "C" int llmc_gptq_quantize_fp8_cols(float* W, const float* Hinv, int64_t R, int64_t K, int64_t n_quant, int fmt,
                                           int64_t group_size, int static_groups, const int32_t* col_group, float* scales,
                                           float* Wout, float* losses, int blocksize, void* ws, llmc_stream_t stream) {
    if (fmt != 0 && fmt != 1) {
        set_last_error_msg("gptq_quantize_fp8_cols: fmt must be 0 (e4m3) or 1 (e5m2)");
        return LLMC_ENOTSUP;
    }
    const float qmax = fmt ? 57344.0f : 448.0f;
    return gptq_cols_impl(W, Hinv, R, K, n_quant, 1, -qmax, qmax, group_size, static_groups, col_group, scales, nullptr, Wout,
                          losses, blocksize, ws, stream, nullptr, nullptr, fmt ? QK_E5M2 : QK_E4M3);
}

extern "C" size_t llmc_gptq_quantize_mse_ws_bytes(int64_t R, int64_t K) { return llmc_gptq_quantize_ws_bytes(R, K); }

extern "C" int llmc_gptq_quantize_mse(float* W, const float* Hinv, int64_t R, int64_t K, int64_t n_quant, int sym,
                                      float qmin, float qmax, int64_t group_size, int round_zp, int nsteps, int grid,
                                      float norm, float* scales, float* zeros, float* Wout, float* losses,
                                      int blocksize, void* ws, llmc_stream_t stream) {
    LLMC_REQUIRE(nsteps >= 1 && grid >= 1, "gptq_quantize_mse: nsteps and grid must be positive");
    if (!(group_size == 16 || group_size == 32 || group_size == 64 || group_size == 128)) {
        set_last_error_msg("gptq_quantize_mse: the searched group qparams need group_size in {16,32,64,128}");
        return LLMC_ENOTSUP;
    }
    const MseSearch m{round_zp, nsteps, grid, norm};
    return gptq_cols_impl(W, Hinv, R, K, n_quant, sym, qmin, qmax, group_size, 0, nullptr, scales, zeros, Wout, losses,
                          blocksize, ws, stream, &m);
}

// Test hooks (include/llmc_hip_test.h): the launch plan of the column loop for these shapes under the calling thread's options,
// without a device — on one stream (width PLAN_W) or with helper streams (PLAN_W + 1: lanes and events).
static int gptq_plan(int64_t R, int64_t K, int64_t n_quant, int64_t group_size, int static_groups, int32_t* out, int cap, bool lanes) {
    LLMC_REQUIRE(out && cap >= 0, "gptq plan: null output");
    PlanRec rec{out, cap, 0, PLAN_W, lanes, PLAN_BLANK};
    // addresses that are only ever offset and compared, never read: 256-B aligned like device allocations, far apart
    float* const base = (float*)(uintptr_t)((uint64_t)1 << 40);
    const size_t span = (size_t)1 << 36;
    int32_t* cg = (int32_t*)(base + 6 * span);
    int rc = gptq_cols_impl(base, base + span, R, K, n_quant, 0, 0.0f, 15.0f, group_size, static_groups, cg, base + 2 * span,
                            base + 3 * span, base + 4 * span, nullptr, BS, base + 5 * span, nullptr, nullptr, &rec);
    return rc ? rc : rec.n;
}
extern "C" int llmc_test_gptq_rider_plan(int64_t R, int64_t K, int64_t n_quant, int64_t group_size, int static_groups, int32_t* out, int cap) {
    return gptq_plan(R, K, n_quant, group_size, static_groups, out, cap, false);
}
extern "C" int llmc_test_gptq_pipe_plan(int64_t R, int64_t K, int64_t n_quant, int64_t group_size, int static_groups, int32_t* out, int cap) {
    return gptq_plan(R, K, n_quant, group_size, static_groups, out, cap, true);
}
