// gptq_block_body.h — the statement body of the in-block kernel, included INSIDE a kernel: k_gptq_block (static LDS) and the chain
// role of k_gptq_block_riders (the same arrays carved from dynamic LDS) in gptq_block_kernels.h. Text and not a function on purpose: as an
// inlined function the same statements compiled to other register counts (k_gptq_block<128, 1024>: 78 instead of 64 VGPRs, one
// workgroup per CU instead of two). The including scope provides: GptqBlockArgs a; constexpr int VARIANT, NT, KIND; LDS objects
// float Us[BS * BS] (16-B aligned), float dg[BS], float2 dtab[BS] (fast path: {d, refined 1/d}), int d_not_plain (some d of the
// block is outside the plain range: generic path for everyone). `return` leaves the kernel.
//   Us[i][p*8 + e] = U[i1+i][i1 + p + 16e] for p+16e > i, else 0 ; dg[i] = U[i1+i][i1+i]
    if (threadIdx.x == 0) d_not_plain = 0;
    __syncthreads();
    const int tid = threadIdx.x;
    {
        // all 8 float4 loads of a thread are issued before the first use (a per-element loop serialises 32
        // L2 round trips, which used to be most of this kernel's time)
        constexpr int NV = BS * BS / 4 / NT;
        float4 v[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int idx = tid + NT * j;
            const int i = idx >> 5, c4 = (idx & 31) * 4;   // count and i1 are multiples of 4
            v[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (i < a.count && c4 < a.count)
                v[j] = *reinterpret_cast<const float4*>(a.U + (int64_t)(a.i1 + i) * a.K + a.i1 + c4);
        }
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int idx = tid + NT * j;
            const int i = idx >> 5, c4 = (idx & 31) * 4;
            const float vv[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int c = c4 + t;   // column inside the block
                if (c == i && i < a.count) {
                    dg[i] = vv[t];
                    dtab[i] = make_float2(vv[t], rcp_refined(vv[t]));
                    if (!plain_pos(vv[t])) d_not_plain = 1;
                }
                Us[i * BS + (c & 15) * 8 + (c >> 4)] = c > i ? vv[t] : 0.0f;
            }
        }
    }
    __syncthreads();

    const int lane = tid & 63;
    const int p = lane & 15;
    const int64_t row = ((int64_t)blockIdx.x * (NT / 64) + (tid >> 6)) * 4 + (lane >> 4);
    const bool active = row < a.R;
    const int64_t rr = active ? row : a.R - 1;

    if (VARIANT != 0 && !d_not_plain) {
        const bool done = block_fast<VARIANT == 1, VARIANT == 1 ? BS : VARIANT, KIND>(a, Us, dtab, p, row, active);
        if (done) return;
    }

    float w[8], w0[8], er[8], ls[8], sc[8], zr[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int c = p + 16 * e;
        w[e] = (c < a.count) ? a.W[rr * a.K + a.i1 + c] : 0.0f;
        w0[e] = w[e];
        er[e] = 0.0f;
        ls[e] = 0.0f;
        sc[e] = 1.0f;
        zr[e] = 0.0f;
        if (a.static_mode && c < a.count) {
            const int g = a.col_group ? a.col_group[a.i1 + c] : (a.i1 + c) / a.col_gsz;
            sc[e] = a.scales[rr * a.ng + g];
            zr[e] = a.zeros ? a.zeros[rr * a.ng + g] : 0.0f;
        }
    }
    float s_cur = 1.0f, z_cur = 0.0f;
    float s_grp[8], z_grp[8];  // dynamic mode: qparams captured at each 16-column boundary (group starts)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        s_grp[e] = 0.0f;
        z_grp[e] = 0.0f;
    }
    const float* us = Us + p * 8;

#define LLMC_CHUNK(E)                                                             \
    gptq_steps16<16 * E, KIND>(w, w0, er, ls, sc, zr, us, dg, p, s_cur, z_cur, a);  \
    s_grp[E] = s_cur;                                                             \
    z_grp[E] = z_cur;
    LLMC_CHUNK(0) LLMC_CHUNK(1) LLMC_CHUNK(2) LLMC_CHUNK(3) LLMC_CHUNK(4) LLMC_CHUNK(5) LLMC_CHUNK(6) LLMC_CHUNK(7)
#undef LLMC_CHUNK

    if (!active) return;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int c = p + 16 * e;
        if (c < a.count) {
            a.Wout[row * a.K + a.i1 + c] = w[e];
            if (a.losses) a.losses[row * a.K + a.i1 + c] = ls[e];
        }
        a.Err[a.err_kmajor ? (int64_t)c * a.err_ld + row : (int64_t)row * a.err_ld + c] = (c < a.count) ? er[e] : 0.0f;
    }
    if (!a.static_mode && p == 0) {
        // qparams of the groups that start in this block (gsz divides 128, multiple of 16)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int i = 16 * e;
            if (i < a.count && (i % a.gsz) == 0) {
                const int g = (a.i1 + i) / a.gsz;
                a.scales[row * a.ng + g] = s_grp[e];
                if (a.zeros) a.zeros[row * a.ng + g] = z_grp[e];
            }
        }
    }
