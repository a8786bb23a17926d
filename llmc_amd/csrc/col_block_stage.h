// col_block_stage.h — the prologue of a block kernel of col_block.h's scaffold (the LDS image of U[i1:i2, i1:i2] and the thread's
// place), included INSIDE a kernel of CB_NT threads, first thing. Text and not a function, like gptq_block_body.h: a function gets Us and dg as generic pointers, and the same statements
// then compile to another LDS address arithmetic (profiles/col_block_refactor.txt). The including scope provides `a` with U, K,
// i1, count (K, i1 and count multiples of 4) and R, and gets, behind a barrier:
//   Us[i][p*8 + e] = U[i1+i][i1 + p + 16e] above the diagonal, else 0 ; dg[i] = U[i1+i][i1+i], 1.0 past count
// and the thread's place: lane p of the 16 that own `row`; a row past R (!active) takes part in every cross-lane step and stores nothing
    __shared__ __attribute__((aligned(16))) float Us[CB_BS * CB_BS];
    __shared__ float dg[CB_BS];
    {
        const int tid = threadIdx.x;
        constexpr int NV = CB_BS * CB_BS / 4 / CB_NT;
        float4 v[NV];          // all loads of a thread are issued before the first use
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int idx = tid + CB_NT * j;
            const int i = idx >> 5, c4 = (idx & 31) * 4;
            v[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (i < a.count && c4 < a.count) v[j] = *reinterpret_cast<const float4*>(a.U + (int64_t)(a.i1 + i) * a.K + a.i1 + c4);
        }
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int idx = tid + CB_NT * j;
            const int i = idx >> 5, c4 = (idx & 31) * 4;
            const float vv[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int c = c4 + t;
                if (c == i) dg[i] = i < a.count ? vv[t] : 1.0f;
                Us[i * CB_BS + (c & 15) * 8 + (c >> 4)] = c > i ? vv[t] : 0.0f;
            }
        }
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int p = lane & 15;
    const int64_t row = ((int64_t)blockIdx.x * (CB_NT / 64) + (threadIdx.x >> 6)) * 4 + (lane >> 4);
    const bool active = row < a.R;
