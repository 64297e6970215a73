// exact_math.h -- glibc 2.35 expf and powf restated for host and device (shared by the GPU sampler
// and the host self-test entry points rwkvtts_debug_expf / rwkvtts_debug_powf).
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

namespace rwkvtts {

__host__ __device__ inline uint64_t exp2_tab(int i) {
  constexpr uint64_t kExp2Tab[32] = {
    0x3ff0000000000000ull, 0x3fefd9b0d3158574ull, 0x3fefb5586cf9890full, 0x3fef9301d0125b51ull,
    0x3fef72b83c7d517bull, 0x3fef54873168b9aaull, 0x3fef387a6e756238ull, 0x3fef1e9df51fdee1ull,
    0x3fef06fe0a31b715ull, 0x3feef1a7373aa9cbull, 0x3feedea64c123422ull, 0x3feece086061892dull,
    0x3feebfdad5362a27ull, 0x3feeb42b569d4f82ull, 0x3feeab07dd485429ull, 0x3feea47eb03a5585ull,
    0x3feea09e667f3bcdull, 0x3fee9f75e8ec5f74ull, 0x3feea11473eb0187ull, 0x3feea589994cce13ull,
    0x3feeace5422aa0dbull, 0x3feeb737b0cdc5e5ull, 0x3feec49182a3f090ull, 0x3feed503b23e255dull,
    0x3feee89f995ad3adull, 0x3feeff76f2fb5e47ull, 0x3fef199bdd85529cull, 0x3fef3720dcef9069ull,
    0x3fef5818dcfba487ull, 0x3fef7c97337b9b5full, 0x3fefa4afa2a490daull, 0x3fefd0765b6e4540ull};
  return kExp2Tab[i];
}

// glibc expf for x <= 0 (and NaN / -inf). sysdeps/ieee754/flt-32/e_expf.c algorithm. `tab`:
// the 32-entry 2^(i/32) table (exp2_tab) -- on the device a copy in LDS, so that the per-element
// gather is a conflict-free LDS read instead of a dependent global load.
template <typename Tab>
__host__ __device__ inline float glibc_expf_t(float x, const Tab& tab) {
  if (x == -__builtin_inff()) return 0.0f;
  if (x != x) return x + x;
  if (x < -0x1.9fe368p6f) return 0.0f;  // underflow to +0
  const double xd = (double)x;
  const double InvLn2N = 0x1.71547652b82fep+0 * 32;
  const double SHIFT = 0x1.8p+52;
  const double C0 = 0x1.c6af84b912394p-5 / 32 / 32 / 32, C1 = 0x1.ebfce50fac4f3p-3 / 32 / 32,
               C2 = 0x1.62e42ff0c52d6p-1 / 32;
  const double z = InvLn2N * xd;
  double kd = z + SHIFT;
  const uint64_t ki = __builtin_bit_cast(uint64_t, kd);
  kd -= SHIFT;
  const double r = __builtin_fma(InvLn2N, xd, -kd);
  uint64_t t = tab((int)(ki % 32));
  t += ki << (52 - 5);
  const double s = __builtin_bit_cast(double, t);
  const double zz = __builtin_fma(C0, r, C1);
  double y = __builtin_fma(C2, r, 1.0);
  y = __builtin_fma(zz, r * r, y);
  y = y * s;
  return (float)y;
}
__host__ __device__ inline float glibc_expf(float x) {
  return glibc_expf_t(x, [](int i) { return exp2_tab(i); });
}

// glibc 2.35 powf (sysdeps/ieee754/flt-32/e_powf.c, x86_64 FMA variant) for the domain the
// sampler presents: x in (0, 1], subnormals included, and y = 1.0f / T with T in [0.1, 4.0]
// (y in [0.25, 10]). Only this domain is exact: x <= 0, x > 1, inf / NaN and y outside it take
// none of glibc's special cases (0 < x outside (0, 1] still goes through the same arithmetic).
// log2(x) from the 16-entry table (1/c, log2 c) and the degree-5 polynomial, y log2(x) in double,
// 2^(y log2 x) from exp2_tab and expf's polynomial, one double -> float rounding; the underflow
// exits return glibc's __math_uflowf / __math_may_uflowf values (+0 and 2^-149). The table
// constants are libm-2.35's __powf_log2_data; tools/powf_sweep.c checks every x of the domain
// against libm.
__host__ __device__ inline double powf_log2_tab(int i) {  // 2 i: invc, 2 i + 1: logc
  static constexpr double kTab[32] = {
    0x1.661ec79f8f3bep+0, -0x1.efec65b963019p-2, 0x1.571ed4aaf883dp+0, -0x1.b0b6832d4fca4p-2,
    0x1.49539f0f010b0p+0, -0x1.7418b0a1fb77bp-2, 0x1.3c995b0b80385p+0, -0x1.39de91a6dcf7bp-2,
    0x1.30d190c8864a5p+0, -0x1.01d9bf3f2b631p-2, 0x1.25e227b0b8ea0p+0, -0x1.97c1d1b3b7af0p-3,
    0x1.1bb4a4a1a343fp+0, -0x1.2f9e393af3c9fp-3, 0x1.12358f08ae5bap+0, -0x1.960cbbf788d5cp-4,
    0x1.0953f419900a7p+0, -0x1.a6f9db6475fcep-5, 0x1.0000000000000p+0, 0x0.0p+0,
    0x1.e608cfd9a47acp-1, 0x1.338ca9f24f53dp-4,  0x1.ca4b31f026aa0p-1, 0x1.476a9543891bap-3,
    0x1.b2036576afce6p-1, 0x1.e840b4ac4e4d2p-3,  0x1.9c2d163a1aa2dp-1, 0x1.40645f0c6651cp-2,
    0x1.886e6037841edp-1, 0x1.88e9c2c1b9ff8p-2,  0x1.767dcf5534862p-1, 0x1.ce0a44eb17bccp-2};
  return kTab[i];
}
// log2_inline of that powf: log2 of the positive normal number whose bits are ix (a subnormal is
// normalised by the caller first, as powf does), in double: the table entry (1/c, log2 c) of the
// interval that holds the mantissa and the degree-5 polynomial in r = z / c - 1 with the fused
// operations glibc's build has. glibc_powf_t and lg2f share this one copy, on host and device.
__host__ __device__ inline __attribute__((always_inline)) double powf_log2_inline(uint32_t ix) {
#pragma clang fp contract(off)  // only the fused operations glibc's build has, written as fma
  const uint32_t tmp = ix - 0x3f330000u;
  const int i = (int)((tmp >> (23 - 4)) % 16u);
  const uint32_t top = tmp & 0xff800000u;
  const uint32_t iz = ix - top;
  const int k = (int32_t)top >> 23;
  const double invc = powf_log2_tab(2 * i), logc = powf_log2_tab(2 * i + 1);
  const double z = (double)__builtin_bit_cast(float, iz);
  const double A0 = 0x1.27616c9496e0bp-2, A1 = -0x1.71969a075c67ap-2, A2 = 0x1.ec70a6ca7baddp-2,
               A3 = -0x1.7154748bef6c8p-1, A4 = 0x1.71547652ab82bp+0;
  const double r = __builtin_fma(z, invc, -1.0);
  const double y0 = logc + (double)k;
  const double r2 = r * r;
  double yl = __builtin_fma(A0, r, A1);
  const double p = __builtin_fma(A2, r, A3);
  const double r4 = r2 * r2;
  double q = __builtin_fma(A4, r, y0);
  q = __builtin_fma(p, r2, q);
  yl = __builtin_fma(yl, r4, q);
  return yl;
}
// powf's normalisation of a subnormal x, so that the exponent becomes negative
__host__ __device__ inline __attribute__((always_inline)) uint32_t powf_norm_bits(float x) {
  uint32_t ix = __builtin_bit_cast(uint32_t, x);
  if (ix < 0x00800000u) {
    ix = __builtin_bit_cast(uint32_t, x * 0x1p23f);
    ix &= 0x7fffffffu;
    ix -= 23u << 23;
  }
  return ix;
}
// lg(x) of the Mirostat contract (rwkvtts.h): log2 of a positive finite x, subnormals included, as
// the double above rounded once to f32. The same source on the host (rwkvtts_debug_lg2) and in
// the decode-step controller, so the two agree bit for bit by construction.
__host__ __device__ inline float lg2f(float x) { return (float)powf_log2_inline(powf_norm_bits(x)); }

template <typename Tab>
__host__ __device__ inline float glibc_powf_t(float x, float y, const Tab& tab) {  // tab: as glibc_expf_t's
#pragma clang fp contract(off)  // only the fused operations glibc's build has, written as fma
  const double yl = powf_log2_inline(powf_norm_bits(x));
  const double ylogx = (double)y * yl;
  if (((__builtin_bit_cast(uint64_t, ylogx) >> 47) & 0xffff) >= (__builtin_bit_cast(uint64_t, 126.0) >> 47)) {
    if (ylogx > 0x1.fffffffd1d571p+6) return __builtin_inff();  // overflow (outside the domain)
    if (ylogx <= -150.0) return 0.0f;                           // __math_uflowf
    if (ylogx < -149.0) return 0x1p-149f;                       // __math_may_uflowf: RN(0x1.4p-75f^2)
  }
  // exp2_inline
  const double SHIFT = 0x1.8p+52 / 32;
  const double C0 = 0x1.c6af84b912394p-5, C1 = 0x1.ebfce50fac4f3p-3, C2 = 0x1.62e42ff0c52d6p-1;
  double kd = ylogx + SHIFT;
  const uint64_t ki = __builtin_bit_cast(uint64_t, kd);
  kd -= SHIFT;
  const double rr = ylogx - kd;
  uint64_t t = tab((int)(ki % 32));
  t += ki << (52 - 5);
  const double s = __builtin_bit_cast(double, t);
  const double zz = __builtin_fma(C0, rr, C1);
  const double rr2 = rr * rr;
  double e = __builtin_fma(C2, rr, 1.0);
  e = __builtin_fma(zz, rr2, e);
  e = e * s;
  return (float)e;
}
__host__ __device__ inline float glibc_powf(float x, float y) {
  return glibc_powf_t(x, y, [](int i) { return exp2_tab(i); });
}


}  // namespace rwkvtts
