// vec16.h — the N consecutive elements a lane holds, stated once: one 16-byte access where N * sizeof(T) == 16 (the caller checked
// the alignment), element by element otherwise. Every HBM-bound pass that reads or writes whole vectors takes it from here: the
// integer quantizer's kernels through quant_group.h, the column reductions (col_reduce.h), prune.hip, awq_kernels.hip,
// act_hist.hip, mixed_quant.hip; load_group (hqq.hip) takes the type alone (see there).
#pragma once
#include "common.h"

namespace llmc {

template <typename T, int N> struct Vec {
    T v[N];
};
template <typename T, int N> __device__ __forceinline__ Vec<T, N> load_vec(const T* p) {
    Vec<T, N> r;
    if constexpr (N * sizeof(T) == 16) {
        const uint4 raw = *reinterpret_cast<const uint4*>(p);
        __builtin_memcpy(&r, &raw, 16);
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) r.v[i] = p[i];
    }
    return r;
}
template <typename T, int N> __device__ __forceinline__ void store_vec(T* p, const Vec<T, N>& r) {
    if constexpr (N * sizeof(T) == 16) {
        uint4 raw;
        __builtin_memcpy(&raw, &r, 16);
        *reinterpret_cast<uint4*>(p) = raw;
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) p[i] = r.v[i];
    }
}
// the vector of a code container (N int32 / int8 / uint8 beside N elements of T) to a 16-byte aligned p: 32 / 16 / 8-byte stores
template <typename O, int N> __device__ __forceinline__ void store_vec_wide(O* p, const Vec<O, N>& o) {
    if constexpr (sizeof(O) * N == 32) {
        uint4 lo, hi;
        __builtin_memcpy(&lo, &o.v[0], 16);
        __builtin_memcpy(&hi, &o.v[N / 2], 16);
        reinterpret_cast<uint4*>(p)[0] = lo;
        reinterpret_cast<uint4*>(p)[1] = hi;
    } else if constexpr (sizeof(O) * N == 16) {
        uint4 lo;
        __builtin_memcpy(&lo, &o.v[0], 16);
        reinterpret_cast<uint4*>(p)[0] = lo;
    } else if constexpr (sizeof(O) * N == 8) {
        uint2 lo;
        __builtin_memcpy(&lo, &o.v[0], 8);
        reinterpret_cast<uint2*>(p)[0] = lo;
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k) p[k] = o.v[k];
    }
}
// N mask bytes beside N elements of T: stores of P = 8 or 4 bytes each where `aligned` says that p allows them, bytes otherwise
template <int P, int N> __device__ __forceinline__ void store_bytes(uint8_t* p, const Vec<uint8_t, N>& m, bool aligned) {
    static_assert(P == 8 || P == 4 || P == 1, "store_bytes: pieces of 8, 4 or 1 bytes");
    if (P > 1 && aligned) {
#pragma unroll
        for (int j = 0; j < N; j += P) {
            std::conditional_t<P == 8, uint2, uint32_t> q;
            __builtin_memcpy(&q, &m.v[j], P);
            *reinterpret_cast<decltype(q)*>(p + j) = q;
        }
    } else {
#pragma unroll
        for (int j = 0; j < N; ++j) p[j] = m.v[j];
    }
}

// +0 of a storage dtype
template <typename T> __device__ __forceinline__ T zero_of() {
    return T{};
}

}  // namespace llmc
