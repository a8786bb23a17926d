// vec_powf.h — fp32 pow of a positive finite base as ATen's vectorised CPU kernels evaluate it (Tensor.pow(python_float) on a CPU
// tensor: Vectorized<float>::pow = Sleef's 1.0-ulp powf). The published algorithm is restated here: expk(logk(x) * y) in
// double-float arithmetic with fused multiply-adds. It is NOT correctly rounded (about 2 % of results for y = 0.75 and over half
// for y = 0.3 are one ulp off), and goldens made by the reference on a CPU carry exactly these values: checked bit for bit
// against torch.pow on 16 M inputs on the host, and by tests/test_smooth_osplus_gpu.py on the device. (ATen's scalar tail — the
// last numel % 16 elements of a parallel chunk — calls glibc's correctly rounded powf instead; callers here take this routine
// for every element.)
#pragma once
#include <math.h>
#include <stdint.h>

namespace llmc {
#define SF_INLINE __host__ __device__ __forceinline__
struct sf2 { float x, y; };
SF_INLINE sf2 sf_add2_ff(float x, float y) { float s = x + y, v = s - x; return {s, (x - (s - v)) + (y - v)}; }
SF_INLINE sf2 sf_add2_df(sf2 x, float y) { float s = x.x + y, v = s - x.x; return {s, ((x.x - (s - v)) + (y - v)) + x.y}; }
SF_INLINE sf2 sf_add_dd(sf2 x, sf2 y) { float s = x.x + y.x; return {s, x.x - s + y.x + x.y + y.y}; }
SF_INLINE sf2 sf_add2_dd(sf2 x, sf2 y) { float s = x.x + y.x, v = s - x.x; return {s, ((x.x - (s - v)) + (y.x - v)) + (x.y + y.y)}; }
SF_INLINE sf2 sf_add_fd(float x, sf2 y) { float s = x + y.x; return {s, x - s + y.x + y.y}; }
SF_INLINE sf2 sf_mul_df(sf2 x, float y) { float s = x.x * y; return {s, fmaf(x.y, y, fmaf(x.x, y, -s))}; }
SF_INLINE sf2 sf_mul_dd(sf2 x, sf2 y) { float s = x.x * y.x; return {s, fmaf(x.x, y.y, fmaf(x.y, y.x, fmaf(x.x, y.x, -s)))}; }
SF_INLINE sf2 sf_squ(sf2 x) { float s = x.x * x.x; return {s, fmaf(x.x + x.x, x.y, fmaf(x.x, x.x, -s))}; }
SF_INLINE sf2 sf_div_dd(sf2 n, sf2 d) {
    float t = 1.0f / d.x, s = n.x * t, u = fmaf(t, n.x, -s);
    float v = fmaf(-d.y, t, fmaf(-d.x, t, 1.0f));
    return {s, fmaf(s, v, fmaf(n.y, t, u))};
}
SF_INLINE float sf_bits(int32_t i) { float f; __builtin_memcpy(&f, &i, 4); return f; }
SF_INLINE int32_t sf_ibits(float f) { int32_t i; __builtin_memcpy(&i, &f, 4); return i; }
SF_INLINE sf2 sf_logk(float d) {
    const int o = d < 1.17549435e-38f;
    if (o) d *= 4294967296.0f * 4294967296.0f;
    int32_t e = ((sf_ibits(d * (1.0f / 0.75f)) >> 23) & 0xff) - 0x7f;
    const float m = sf_bits(sf_ibits(d) + (int32_t)((uint32_t)(-e) << 23));
    if (o) e -= 64;
    const sf2 x = sf_div_dd(sf_add2_ff(-1.0f, m), sf_add2_ff(1.0f, m));
    const sf2 x2 = sf_squ(x);
    float t = 0.240320354700088500976562f;
    t = fmaf(t, x2.x, 0.285112679004669189453125f);
    t = fmaf(t, x2.x, 0.400007992982864379882812f);
    const sf2 c = {0.66666662693023681640625f, 3.69183861259614332084311e-09f};
    sf2 s = sf_mul_df(sf2{0.69314718246459960938f, -1.904654323148236017e-09f}, (float)e);
    s = sf_add_dd(s, sf2{x.x * 2.0f, x.y * 2.0f});
    s = sf_add_dd(s, sf_mul_dd(sf_mul_dd(x2, x), sf_add2_dd(sf_mul_df(x2, t), c)));
    return s;
}
SF_INLINE float sf_expk(sf2 d) {
    float u = (d.x + d.y) * 1.442695040888963407359924681001892137426645954152985934135449406931f;
    const int32_t q = (int32_t)rintf(u);
    sf2 s = sf_add2_df(d, (float)q * -0.693145751953125f);
    s = sf_add2_df(s, (float)q * -1.428606765330187045e-06f);
    { const float t0 = s.x + s.y; s = sf2{t0, s.x - t0 + s.y}; }
    u = 0.00136324646882712841033936f;
    u = fmaf(u, s.x, 0.00836596917361021041870117f);
    u = fmaf(u, s.x, 0.0416710823774337768554688f);
    u = fmaf(u, s.x, 0.166665524244308471679688f);
    u = fmaf(u, s.x, 0.499999850988388061523438f);
    sf2 t = sf_add_dd(s, sf_mul_df(sf_squ(s), u));
    t = sf_add_fd(1.0f, t);
    u = t.x + t.y;
    // ldexp2kf: two exact power-of-two factors
    u = u * sf_bits(((q >> 1) + 0x7f) << 23) * sf_bits(((q - (q >> 1)) + 0x7f) << 23);
    if (d.x < -104.0f) u = 0.0f;
    return u;
}
SF_INLINE float sf_powf_pos(float x, float y) { return sf_expk(sf_mul_df(sf_logk(x), y)); }
#undef SF_INLINE
}  // namespace llmc
