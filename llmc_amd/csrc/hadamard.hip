// hadamard.hip — Walsh-Hadamard transform along the middle axis of a contiguous [outer, n, inner] tensor (QuaRot's offline
// rotations and the online transform in front of down_proj / o_proj: llmc/compression/quantization/hadamard_utils.py:72-122,
// module_utils.py:460-503 of the reference, which needs the CUDA-only fast_hadamard_transform extension for it).
//
//   y[o, a*m + j, c] = scale * sum_{b, i} hadK[a][b] * S_m[j][i] * x[o, b*m + i, c]        n = K0 * m, m a power of two,
//
// S_m the Sylvester matrix in natural order, hadK a [K0, K0] matrix of +-1 (absent for K0 = 1). Butterflies are additions and
// subtractions only, accumulated in fp32 (F16 / BF16 / F32 tensors) or fp64 (F64); one multiplication by `scale` and one rounding
// at the end. A row is read from HBM once and written once:
//
//   k_had_rows (inner == 1): a workgroup owns a contiguous span of whole rows (several short rows share one). Phase A: every
//     lane loads a run of 8 elements and does index bits 0-2 in registers, bits 3-8 across the wave's lanes (DPP quad
//     permutes, ds_swizzle, v_permlane32_swap) — a wave finishes a 512-element tile without touching LDS. Rows with m <= 512 and
//     K0 == 1 are stored straight from the registers. Longer rows go through ONE exchange: the tile is written to LDS, and after
//     the barrier each lane gathers the 2^(L-9) elements that differ in the high bits only (stride 512: a wave reads 64
//     consecutive words) and finishes them in registers. The K0 mix is K0 signed adds per output, signs read from LDS.
//   k_had_cols (inner > 1): a workgroup owns one `outer` index and a chunk of C columns; the slab [n, C] lies in LDS as it lies
//     in memory (loads, stores and LDS accesses all run along `inner`), and each lane does radix-8 passes down its column.
#include "common.h"

namespace llmc {
namespace {

constexpr int HAD_LDS_MAX = 160 * 1024;      // gfx950: 160 KiB of LDS per workgroup
constexpr int HAD_TILE = 512;                // elements a wave transforms in registers + lanes: 8 per lane x 64 lanes
constexpr int HAD_MAX_K0 = 64;

// ---- value of lane (lane ^ M) ----------------------------------------------------------------------------------------------
template <int M> __device__ __forceinline__ uint32_t lane_xor_u32(uint32_t v) {
    if constexpr (M == 1) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, true);        // quad_perm [1,0,3,2]
    else if constexpr (M == 2) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, true);   // quad_perm [2,3,0,1]
    else if constexpr (M < 32) return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, (M << 10) | 0x1F);          // bit mode: and 0x1f, xor M
    else {
        // v_permlane32_swap: .x = {v[0..31], v[0..31]}, .y = {v[32..63], v[32..63]}
        const auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false);
        return (__lane_id() & 32) ? r[0] : r[1];
    }
}
template <int M> __device__ __forceinline__ float lane_xor(float v) { return __uint_as_float(lane_xor_u32<M>(__float_as_uint(v))); }
template <int M> __device__ __forceinline__ double lane_xor(double v) {
    const uint64_t u = (uint64_t)__double_as_longlong(v);
    const uint32_t lo = lane_xor_u32<M>((uint32_t)u), hi = lane_xor_u32<M>((uint32_t)(u >> 32));
    return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}

// ---- element access in the tensor's dtype ---------------------------------------------------------------------------------------
template <typename A> __device__ __forceinline__ A ld_elem(const void* p, int64_t i, int dt) {
    if constexpr (sizeof(A) == 8) return ((const double*)p)[i];
    else return load_as_f32(p, i, dt);
}
template <typename A> __device__ __forceinline__ void st_elem(void* p, int64_t i, int dt, A v) {
    if constexpr (sizeof(A) == 8) ((double*)p)[i] = v;
    else store_from_f32(p, i, dt, v);
}
template <typename A> __device__ __forceinline__ int elem_size(int dt) {
    if constexpr (sizeof(A) == 8) return 8;
    else return dt == LLMC_F32 ? 4 : 2;
}

// a run of 8 consecutive elements starting at element i (16-byte vectors when the address allows it); cnt = valid elements
template <typename A> __device__ __forceinline__ void ld_run8(const void* p, int64_t i, int dt, int cnt, A (&v)[8]) {
    const int es = elem_size<A>(dt);
    const uintptr_t addr = (uintptr_t)p + (uintptr_t)i * es;
    if (cnt >= 8 && (addr & 15) == 0) {
        if constexpr (sizeof(A) == 8) {
            const double2* q = (const double2*)addr;
#pragma unroll
            for (int r = 0; r < 4; ++r) { const double2 t = q[r]; v[2 * r] = t.x; v[2 * r + 1] = t.y; }
        } else if (es == 4) {
            const float4* q = (const float4*)addr;
            const float4 t0 = q[0], t1 = q[1];
            v[0] = t0.x; v[1] = t0.y; v[2] = t0.z; v[3] = t0.w; v[4] = t1.x; v[5] = t1.y; v[6] = t1.z; v[7] = t1.w;
        } else {
            const uint4 t = *(const uint4*)addr;
            const uint32_t w[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (dt == LLMC_F16) {
                    v[2 * r] = f16_bits_to_f32((uint16_t)(w[r] & 0xffff));
                    v[2 * r + 1] = f16_bits_to_f32((uint16_t)(w[r] >> 16));
                } else {
                    v[2 * r] = __uint_as_float(w[r] << 16);
                    v[2 * r + 1] = __uint_as_float(w[r] & 0xffff0000u);
                }
            }
        }
    } else {
#pragma unroll
        for (int r = 0; r < 8; ++r) v[r] = r < cnt ? ld_elem<A>(p, i + r, dt) : (A)0;
    }
}
template <typename A> __device__ __forceinline__ void st_run8(void* p, int64_t i, int dt, int cnt, const A (&v)[8]) {
    const int es = elem_size<A>(dt);
    const uintptr_t addr = (uintptr_t)p + (uintptr_t)i * es;
    if (cnt >= 8 && (addr & 15) == 0) {
        if constexpr (sizeof(A) == 8) {
            double2* q = (double2*)addr;
#pragma unroll
            for (int r = 0; r < 4; ++r) q[r] = make_double2(v[2 * r], v[2 * r + 1]);
        } else if (es == 4) {
            float4* q = (float4*)addr;
            q[0] = make_float4(v[0], v[1], v[2], v[3]);
            q[1] = make_float4(v[4], v[5], v[6], v[7]);
        } else {
            uint32_t w[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const uint32_t lo = dt == LLMC_F16 ? f32_to_f16_bits(v[2 * r]) : f32_to_bf16_bits(v[2 * r]);
                const uint32_t hi = dt == LLMC_F16 ? f32_to_f16_bits(v[2 * r + 1]) : f32_to_bf16_bits(v[2 * r + 1]);
                w[r] = lo | (hi << 16);
            }
            *(uint4*)addr = make_uint4(w[0], w[1], w[2], w[3]);
        }
    } else {
#pragma unroll
        for (int r = 0; r < 8; ++r)
            if (r < cnt) st_elem<A>(p, i + r, dt, v[r]);
    }
}

// a run of 8 in LDS at an index that is a multiple of 8: 16-byte accesses (scalar ones at a lane stride of 8 words would hit the
// same bank from every eighth lane)
__device__ __forceinline__ void lds_ld8(const float* p, float (&v)[8]) {
    const float4 t0 = ((const float4*)p)[0], t1 = ((const float4*)p)[1];
    v[0] = t0.x; v[1] = t0.y; v[2] = t0.z; v[3] = t0.w; v[4] = t1.x; v[5] = t1.y; v[6] = t1.z; v[7] = t1.w;
}
__device__ __forceinline__ void lds_ld8(const double* p, double (&v)[8]) {
#pragma unroll
    for (int r = 0; r < 4; ++r) { const double2 t = ((const double2*)p)[r]; v[2 * r] = t.x; v[2 * r + 1] = t.y; }
}
__device__ __forceinline__ void lds_st8(float* p, const float (&v)[8]) {
    ((float4*)p)[0] = make_float4(v[0], v[1], v[2], v[3]);
    ((float4*)p)[1] = make_float4(v[4], v[5], v[6], v[7]);
}
__device__ __forceinline__ void lds_st8(double* p, const double (&v)[8]) {
#pragma unroll
    for (int r = 0; r < 4; ++r) ((double2*)p)[r] = make_double2(v[2 * r], v[2 * r + 1]);
}

// ---- butterflies ----------------------------------------------------------------------------------------------------------
// 2^NB values whose indices differ in NB bits: NB stages in registers
template <int NB, typename A> __device__ __forceinline__ void bfly_regs(A* v, int nb) {
#pragma unroll
    for (int s = 0; s < NB; ++s) {
        if (s < nb) {
#pragma unroll
            for (int r = 0; r < (1 << NB); ++r) {
                if (!(r & (1 << s))) {
                    const A a = v[r], b = v[r | (1 << s)];
                    v[r] = a + b;
                    v[r | (1 << s)] = a - b;
                }
            }
        }
    }
}
// v or -v: the sign bit is flipped by `mask` (0 or 0x80000000), so that a signed add is one XOR and one addition. p + (-v) is
// the same fp operation as p - v.
__device__ __forceinline__ float flip(float v, uint32_t mask) { return __uint_as_float(__float_as_uint(v) ^ mask); }
__device__ __forceinline__ double flip(double v, uint32_t mask) {
    return __longlong_as_double(__double_as_longlong(v) ^ (long long)((uint64_t)mask << 32));
}
template <int M, typename A> __device__ __forceinline__ void bfly_lanes(A (&v)[8], int lane) {
    const uint32_t mask = (lane & M) ? 0x80000000u : 0u;        // the upper lane of a pair holds partner - own
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const A p = lane_xor<M>(v[r]);
        v[r] = p + flip(v[r], mask);
    }
}

struct HadArgs {
    const void* x;
    void* y;
    const float* hadK;
    int64_t outer, n, inner;
    double scale;
    int dt, K0, L;       // m = n / K0 = 1 << L
    int rpb;             // k_had_rows: rows per workgroup
    int C, logC;         // k_had_cols: columns per workgroup
    int64_t bx;          // k_had_cols: column chunks per `outer` index
};

// phase B of k_had_rows: index bits 9 .. 9+HB-1 of every length-m segment of the span, in registers
template <int HB, typename A> __device__ __forceinline__ void rows_high_bits(A* buf, int span, int L, int wave, int nwaves, int lane) {
    const int nseg = span >> L;
    const int items = nseg * (HAD_TILE / 64);
    for (int it = wave; it < items; it += nwaves) {
        const int seg = it >> 3, lo = ((it & 7) << 6) | lane;
        A* p = buf + ((size_t)seg << L) + lo;
        A v[1 << HB];
#pragma unroll
        for (int r = 0; r < (1 << HB); ++r) v[r] = p[r * HAD_TILE];
        bfly_regs<HB>(v, HB);
#pragma unroll
        for (int r = 0; r < (1 << HB); ++r) p[r * HAD_TILE] = v[r];
    }
}

template <typename A> __global__ void __launch_bounds__(1024) k_had_rows(const HadArgs a) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const int n = (int)a.n, L = a.L, K0 = a.K0, dt = a.dt;
    const int64_t row0 = (int64_t)blockIdx.x * a.rpb;
    const int nrows = (int)(a.outer - row0 < a.rpb ? a.outer - row0 : a.rpb);
    const int span = nrows * n;
    const int64_t base = row0 * n;
    A* buf = (A*)smem_raw;
    uint32_t* hk = (uint32_t*)(buf + (size_t)a.rpb * n);        // sign masks of the factor matrix
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = blockDim.x >> 6;
    const A scale = (A)a.scale;
    const bool direct = K0 == 1 && L <= 9;        // a tile holds whole rows: no exchange

    if (K0 > 1)
        for (int i = tid; i < K0 * K0; i += blockDim.x) hk[i] = a.hadK[i] < 0.f ? 0x80000000u : 0u;

    // phase A: index bits 0 .. min(L, 9) - 1. Partners differ in a bit below L, so they lie in the same tile and the same row.
    const int ntiles = (span + HAD_TILE - 1) / HAD_TILE;
    for (int t = wave; t < ntiles; t += nwaves) {
        const int g0 = t * HAD_TILE + lane * 8;
        const int cnt = span - g0;
        A v[8];
        ld_run8<A>(a.x, base + g0, dt, cnt, v);
        bfly_regs<3>(v, L);
        if (L > 3) bfly_lanes<1>(v, lane);
        if (L > 4) bfly_lanes<2>(v, lane);
        if (L > 5) bfly_lanes<4>(v, lane);
        if (L > 6) bfly_lanes<8>(v, lane);
        if (L > 7) bfly_lanes<16>(v, lane);
        if (L > 8) bfly_lanes<32>(v, lane);
        if (direct) {
#pragma unroll
            for (int r = 0; r < 8; ++r) v[r] = v[r] * scale;
            st_run8<A>(a.y, base + g0, dt, cnt, v);
        } else if (cnt >= 8) {
            lds_st8(buf + g0, v);
        } else {
#pragma unroll
            for (int r = 0; r < 8; ++r)
                if (r < cnt) buf[g0 + r] = v[r];
        }
    }
    if (direct) return;
    __syncthreads();

    if (L > 9) {
        switch (L - 9) {
        case 1: rows_high_bits<1>(buf, span, L, wave, nwaves, lane); break;
        case 2: rows_high_bits<2>(buf, span, L, wave, nwaves, lane); break;
        case 3: rows_high_bits<3>(buf, span, L, wave, nwaves, lane); break;
        case 4: rows_high_bits<4>(buf, span, L, wave, nwaves, lane); break;
        case 5: rows_high_bits<5>(buf, span, L, wave, nwaves, lane); break;
        default: rows_high_bits<6>(buf, span, L, wave, nwaves, lane); break;
        }
        __syncthreads();
    }

    // the K0 mix (K0 signed adds per output), the scale, one rounding, the store
    const int m = 1 << L;
    for (int g0 = tid * 8; g0 < span; g0 += blockDim.x * 8) {
        const int cnt = span - g0;
        A v[8];
        if (K0 == 1 && cnt >= 8) {
            lds_ld8(buf + g0, v);
        } else if (K0 == 1) {
#pragma unroll
            for (int r = 0; r < 8; ++r) v[r] = r < cnt ? buf[g0 + r] : (A)0;
        } else if (L >= 3) {            // the run lies in one segment: same row, same output factor index
            const int row = g0 / n, pos = g0 - row * n, oa = pos >> L, i = pos & (m - 1);
            const A* src = buf + row * n + i;
            const uint32_t* sg = hk + oa * K0;
#pragma unroll
            for (int r = 0; r < 8; ++r) v[r] = (A)0;
            for (int b = 0; b < K0; ++b) {
                const uint32_t mask = sg[b];
                A w[8];
                lds_ld8(src + b * m, w);
#pragma unroll
                for (int r = 0; r < 8; ++r) v[r] = v[r] + flip(w[r], mask);
            }
        } else {
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                v[r] = (A)0;
                if (r < cnt) {
                    const int g = g0 + r, row = g / n, pos = g - row * n, oa = pos >> L, i = pos & (m - 1);
                    for (int b = 0; b < K0; ++b) v[r] = v[r] + flip(buf[row * n + b * m + i], hk[oa * K0 + b]);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 8; ++r) v[r] = v[r] * scale;
        st_run8<A>(a.y, base + g0, dt, cnt, v);
    }
}

// one radix-2^NB pass of k_had_cols over index bits [s0, s0 + NB) of the slab buf[n][C]
template <int NB, typename A> __device__ __forceinline__ void cols_pass(A* buf, int n, int C, int logC, int s0, int tid, int nthreads) {
    const int items = (n >> NB) << logC;
    for (int it = tid; it < items; it += nthreads) {
        const int j = it & (C - 1), q = it >> logC;
        const int k = ((q >> s0) << (s0 + NB)) | (q & ((1 << s0) - 1));
        A* p = buf + ((size_t)k << logC) + j;
        const size_t st = (size_t)1 << (s0 + logC);
        A v[1 << NB];
#pragma unroll
        for (int r = 0; r < (1 << NB); ++r) v[r] = p[r * st];
        bfly_regs<NB>(v, NB);
#pragma unroll
        for (int r = 0; r < (1 << NB); ++r) p[r * st] = v[r];
    }
}

template <typename A> __global__ void __launch_bounds__(256) k_had_cols(const HadArgs a) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const int n = (int)a.n, L = a.L, K0 = a.K0, dt = a.dt, C = a.C, logC = a.logC;
    A* buf = (A*)smem_raw;
    uint32_t* hk = (uint32_t*)(buf + ((size_t)n << logC));
    const int tid = threadIdx.x, nth = blockDim.x;
    const int64_t o = (int64_t)blockIdx.x / a.bx;
    const int64_t c0 = ((int64_t)blockIdx.x - o * a.bx) << logC;
    const int64_t obase = o * a.n * a.inner;
    const A scale = (A)a.scale;
    const int total = n << logC;

    if (K0 > 1)
        for (int i = tid; i < K0 * K0; i += nth) hk[i] = a.hadK[i] < 0.f ? 0x80000000u : 0u;
    for (int e = tid; e < total; e += nth) {
        const int j = e & (C - 1), k = e >> logC;
        buf[e] = c0 + j < a.inner ? ld_elem<A>(a.x, obase + (int64_t)k * a.inner + c0 + j, dt) : (A)0;
    }
    __syncthreads();
    for (int s0 = 0; s0 < L; s0 += 3) {
        const int nb = L - s0;
        if (nb >= 3) cols_pass<3>(buf, n, C, logC, s0, tid, nth);
        else if (nb == 2) cols_pass<2>(buf, n, C, logC, s0, tid, nth);
        else cols_pass<1>(buf, n, C, logC, s0, tid, nth);
        __syncthreads();
    }
    const int m = 1 << L;
    for (int e = tid; e < total; e += nth) {
        const int j = e & (C - 1), k = e >> logC;
        if (c0 + j >= a.inner) continue;
        A v;
        if (K0 == 1) {
            v = buf[e];
        } else {
            const int oa = k >> L, i = k & (m - 1);
            v = (A)0;
            for (int b = 0; b < K0; ++b) v = v + flip(buf[((size_t)(b * m + i) << logC) + j], hk[oa * K0 + b]);
        }
        st_elem<A>(a.y, obase + (int64_t)k * a.inner + c0 + j, dt, v * scale);
    }
}

template <typename A> int launch_had(HadArgs& a, hipStream_t st) {
    const int64_t hk_bytes = a.K0 > 1 ? (int64_t)a.K0 * a.K0 * 4 : 0;
    const int64_t row_bytes = a.n * (int64_t)sizeof(A);
    if (row_bytes + hk_bytes > HAD_LDS_MAX) {
        set_last_error_msg("hadamard: the row is too long to stay resident in LDS (n * accumulator size + K0^2 * 4 > 160 KiB)");
        return LLMC_ENOTSUP;
    }
    if (a.inner == 1) {
        // several short rows share a workgroup: ~32 KiB of fp32 per workgroup keeps a few of them on a CU
        int64_t rpb = (8192 * 4 / (int64_t)sizeof(A)) / a.n;
        if (rpb < 1) rpb = 1;
        if (rpb > a.outer) rpb = a.outer;
        a.rpb = (int)rpb;
        const int64_t span = rpb * a.n;
        int threads = (int)(((span + 7) / 8 + 63) / 64 * 64);
        threads = threads < 64 ? 64 : threads > 1024 ? 1024 : threads;
        const int64_t blocks = ceil_div64(a.outer, rpb);
        LLMC_REQUIRE(blocks < ((int64_t)1 << 31), "hadamard: too many rows");
        if (int rc = ensure_dynamic_lds((const void*)k_had_rows<A>, HAD_LDS_MAX)) return rc;
        hipLaunchKernelGGL((k_had_rows<A>), dim3((unsigned)blocks), dim3(threads), (size_t)(span * sizeof(A) + hk_bytes), st, a);
    } else {
        int C = pow2_ceil(a.inner < 128 ? a.inner : 128);
        while (C > 1 && (int64_t)C * row_bytes + hk_bytes > 32 * 1024) C >>= 1;      // long columns: as many as fit
        a.C = C;
        a.logC = 0;
        while ((1 << a.logC) < C) ++a.logC;
        a.bx = ceil_div64(a.inner, C);
        LLMC_REQUIRE(a.bx < ((int64_t)1 << 31) && a.bx * a.outer < ((int64_t)1 << 31), "hadamard: outer * ceil(inner / C) must be below 2^31");
        if (int rc = ensure_dynamic_lds((const void*)k_had_cols<A>, HAD_LDS_MAX)) return rc;
        hipLaunchKernelGGL((k_had_cols<A>), dim3((unsigned)(a.bx * a.outer)), dim3(256), (size_t)(C * row_bytes + hk_bytes), st, a);
    }
    LLMC_LAUNCH_CHECK();
    return LLMC_OK;
}

}  // namespace
}  // namespace llmc

extern "C" int llmc_hadamard(const void* x, void* y, int dt, int64_t outer, int64_t n, int64_t inner, const float* hadK, int K0,
                             double scale, llmc_stream_t stream) {
    using namespace llmc;
    LLMC_REQUIRE(dt == LLMC_F16 || dt == LLMC_BF16 || dt == LLMC_F32 || dt == LLMC_F64, "hadamard: dtype must be f16, bf16, f32 or f64");
    LLMC_REQUIRE(outer >= 0 && n >= 1 && inner >= 1 && K0 >= 1, "hadamard: outer >= 0, n >= 1, inner >= 1, K0 >= 1");
    if (K0 > HAD_MAX_K0) {
        set_last_error_msg("hadamard: factor matrices larger than 64 x 64 (K0 > 64) are not supported");
        return LLMC_ENOTSUP;
    }
    if (n % K0 != 0 || ((n / K0) & (n / K0 - 1)) != 0) {
        set_last_error_msg("hadamard: n / K0 must be a power of two");
        return LLMC_ENOTSUP;
    }
    HadArgs a = {};
    a.L = 0;
    while (((int64_t)1 << a.L) < n / K0) ++a.L;
    if (a.L > 15) {
        set_last_error_msg("hadamard: the row is too long to stay resident in LDS (n / K0 > 32768)");
        return LLMC_ENOTSUP;
    }
    LLMC_REQUIRE(K0 == 1 || hadK, "hadamard: hadK is null with K0 > 1");
    if (outer == 0) return LLMC_OK;
    LLMC_REQUIRE(x && y, "hadamard: null tensor");
    a.x = x; a.y = y; a.hadK = hadK; a.outer = outer; a.n = n; a.inner = inner; a.scale = scale; a.dt = dt; a.K0 = K0;
    if (dt == LLMC_F64) return launch_had<double>(a, (hipStream_t)stream);
    return launch_had<float>(a, (hipStream_t)stream);
}
