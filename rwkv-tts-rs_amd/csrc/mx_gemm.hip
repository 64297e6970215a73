// mx_gemm.hip -- OCP Microscaling weights (RWKVTTS_QUANT_MXFP8 / MXFP4 / MXFP6_E2M3 / MXFP6_E3M2 /
// MXINT8) for the LM projection GEMMs of a bf16 model: the pack kernel, the GEMM (k_gemm_mx) and the
// round-trip debug entry.
//
// Contract (include/rwkvtts.h): blocks of 32 along K share one power-of-two scale 2^e (E8M0 byte
// e + 127); elements are E4M3 (MXFP8), E2M1 (MXFP4), E2M3 / E3M2 (MXFP6) or a two's-complement byte
// in units of 2^-6 (MXINT8). With the header's clamps on e every
// dequantised weight element * 2^e is zero or a bf16 normal, so an MX layer is a bf16 layer with
// other weights: k_gemm_mx rebuilds the bf16 B fragment in registers and issues the MFMAs of the
// unquantised separate launch (k_gemm2 / k_gemm_wide) -- per output element the same K-slice, the
// 32-deep steps in order, the x_hi and x_lo chains apart, hi + lo at the end -- so its partial slabs
// are bit for bit those of the unquantised kernels on the dequantised matrix.
//
// Packed layout (launch_mx_pack). The matrix is cut into superblocks of 16 columns x 128 k = four
// MFMA 16x16x32 steps, ordered column-block-major (superblock (nb, kq) at (nb * K / 128 + kq) * SB):
//   bytes [0, CB)        codes: lane l = 16 g + li of a wave owns V = CB / 64 bytes (16 MXFP4, 32 MXFP8
//                        and MXINT8) at l * V: step s of the four at s * V / 4, holding
//                        k = 128 kq + 32 s + 8 g .. + 8 of column 16 nb + li (MXFP4: low nibble the even k)
//   bytes [CB, CB + 64)  scales: column li's four E8M0 bytes (steps 0..3) as one 32-bit word at 4 li
// MXFP6 (V = 24, CB = 1536) cuts its 6-bit codes into two planes, because a plain bit stream would
// straddle dwords and leave a lane's 24 bytes off the 16-byte grid:
//   bytes [0, 1024)      nibble plane: the low 4 bits of every code, lane l at 16 l, step s at 4 s,
//                        element i at bits 4 i -- MXFP4's addresses and shifts
//   bytes [1024, 1536)   2-bit plane: bits 4..5 of every code (the top exponent bit and the sign), lane l
//                        at 1024 + 8 l, step s the 16-bit word at 2 s, element i at bits 2 i
//   bytes [1536, 1600)   scales, as above
// A 16x16x32 MFMA step reads exactly one MX block per column, so a lane's whole weight feed for four
// steps is one 16-byte load (two for MXFP8 / MXINT8; one 16-byte and one 8-byte load for MXFP6) plus one
// 4-byte load of its column's scale word from the same superblock: all addresses come from the lane
// index alone (no load depends on another) and the four lanes that share a column read the same word
// (one request per wave).
//
// Work split: a workgroup = 4 waves = 64 columns (16 per wave) x one K-slice, as the unquantised
// launch it mirrors (the K-slices and their split-K slabs are fixed by the bitwise constraint). The
// codes are requested after the X slice, dequantised ONCE into the KSTEPS bf16 fragments while the
// X image settles in LDS, and then serve every row group the workgroup runs (prefill steps: the
// next group's X in flight behind the current group's MFMAs), which the Int8 / NF4 forms of
// k_gemm2 cannot do (their dequantisation sits inside the step loop and spills with the row loop).
// The rkv launch's 16-bit LoRA-down tiles (tile table, tinfo bit 31 clear) take the plain fragment
// stream in the same kernel.
#include "lm_kernels.h"

#include <algorithm>
#include <vector>

namespace rwkvtts {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

// ---- element formats ---------------------------------------------------------------------------
// bf16 bits of (E2M1 code n) * 2^(sb - 127). E2M1 magnitudes 0, .5, 1, 1.5, 2, 3, 4, 6: from code 2
// on the code is the bf16 exponent | top mantissa bit (<< 6); code 1 (0.5, the subnormal) has a clear
// mantissa. Zero keeps its sign.
__host__ __device__ inline uint32_t mx_e2m1_bf16(uint32_t n, int sb) {
  const uint32_t mag = n & 7u;
  uint32_t r = 0;
  if (mag) r = (uint32_t)((int)(0x3F00u + (mag << 6) - (mag == 1u ? 0x40u : 0u)) + ((sb - 127) << 7));
  return r | ((n & 8u) << 12);
}
// bf16 bits of (E4M3 byte b) * 2^(sb - 127): a normal is a shift and a rebias (7 -> 127); a subnormal
// (m * 2^-9, m = 1..7) is normalised by the integer -> f32 convert.
__host__ __device__ inline uint32_t mx_e4m3_bf16(uint32_t b, int sb) {
  const uint32_t mag = b & 0x7Fu;
  uint32_t r = 0;
  if (mag >= 8u) r = (uint32_t)((int)(mag << 4) + ((sb - 7) << 7));
  else if (mag) r = (uint32_t)((int)(as_u32((float)mag) >> 16) + ((sb - 136) << 7));
  return r | ((b & 0x80u) << 8);
}
// bf16 bits of (E2M3 code n, bits above 5 ignored) * 2^(sb - 127): bits 0..4 are exponent | mantissa. A
// normal (>= 8) is a shift and a rebias (1 -> 127); a subnormal (m * 2^-3, m = 1..7) goes through the
// integer -> f32 convert. Zero keeps its sign.
__host__ __device__ inline uint32_t mx_e2m3_bf16(uint32_t n, int sb) {
  const uint32_t mag = n & 31u;
  uint32_t r = 0;
  if (mag >= 8u) r = (uint32_t)((int)(mag << 4) + ((sb - 1) << 7));
  else if (mag) r = (uint32_t)((int)(as_u32((float)mag) >> 16) + ((sb - 130) << 7));
  return r | ((n & 32u) << 10);
}
// the same for E3M2: a normal (>= 4) is a shift and a rebias (3 -> 127); a subnormal is m * 2^-4, m = 1..3
__host__ __device__ inline uint32_t mx_e3m2_bf16(uint32_t n, int sb) {
  const uint32_t mag = n & 31u;
  uint32_t r = 0;
  if (mag >= 4u) r = (uint32_t)((int)(mag << 5) + ((sb - 3) << 7));
  else if (mag) r = (uint32_t)((int)(as_u32((float)mag) >> 16) + ((sb - 131) << 7));
  return r | ((n & 32u) << 10);
}
// bf16 bits of (MXINT8 byte b: i * 2^-6, two's complement) * 2^(sb - 127): the signed convert gives sign,
// exponent and the (at most 7-bit) mantissa at once, the exponent add rebias and scale. |i| = 0 (bytes
// 0x00 and 0x80) is a zero with the byte's sign: 0x80, never a value, is the pack's -0.
__host__ __device__ inline uint32_t mx_int8_bf16(uint32_t b, int sb) {
  const uint32_t f = as_u32((float)(int)(int8_t)b) >> 16;
  return (b & 0x7Fu) ? (uint32_t)((int)f + ((sb - 133) << 7)) : (f & 0x8000u);
}
// a lane's 8 weights of one step -> the bf16 B fragment. c0, c1: the step's code dwords (MXFP8 / MXINT8
// two, MXFP4 one; MXFP6: c0 the nibble plane's dword, c1 the 2-bit plane's 16 bits)
template <MxFmt FMT>
__device__ inline short8 mx_fragment(uint32_t c0, uint32_t c1, int sb) {
  uint32_t p[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if constexpr (FMT == kMxFp4) {
      p[e] = mx_e2m1_bf16(c0 >> (8 * e), sb) | (mx_e2m1_bf16(c0 >> (8 * e + 4), sb) << 16);
    } else if constexpr (FMT == kMxE2M3 || FMT == kMxE3M2) {
      const uint32_t n0 = ((c0 >> (8 * e)) & 15u) | ((c1 >> (4 * e)) << 4);
      const uint32_t n1 = ((c0 >> (8 * e + 4)) & 15u) | ((c1 >> (4 * e + 2)) << 4);
      if constexpr (FMT == kMxE2M3) p[e] = mx_e2m3_bf16(n0, sb) | (mx_e2m3_bf16(n1, sb) << 16);
      else p[e] = mx_e3m2_bf16(n0, sb) | (mx_e3m2_bf16(n1, sb) << 16);
    } else if constexpr (FMT == kMxInt8) {
      const uint32_t c = e < 2 ? c0 : c1;
      p[e] = mx_int8_bf16(c >> (16 * (e & 1)), sb) | (mx_int8_bf16(c >> (16 * (e & 1) + 8), sb) << 16);
    } else {
      const uint32_t c = e < 2 ? c0 : c1;
      p[e] = mx_e4m3_bf16(c >> (16 * (e & 1)), sb) | (mx_e4m3_bf16(c >> (16 * (e & 1) + 8), sb) << 16);
    }
  }
  return __builtin_bit_cast(short8, (u32x4_){p[0], p[1], p[2], p[3]});
}

// ---- pack ----------------------------------------------------------------------------------------
// |q| (finite) -> the nearest element magnitude, ties to even on the element's mantissa, saturated;
// returned as the code without its sign. MB mantissa bits, EMIN the smallest normal exponent.
template <int MB, int EMIN, int BIAS>
__host__ __device__ inline uint32_t mx_encode(double aq, double sat) {
  if (aq == 0.0) return 0u;
  const int ea = ilogb(aq), ex = ea > EMIN ? ea : EMIN;
  const double step = ldexp(1.0, ex - MB);
  const double v = fmin(rint(aq / step) * step, sat);  // rint: to nearest, ties to even
  if (v == 0.0) return 0u;
  const int ev = ilogb(v);
  if (ev < EMIN) return (uint32_t)ldexp(v, MB - EMIN);
  return ((uint32_t)(ev + BIAS) << MB) | (uint32_t)(ldexp(v, MB - ev) - (double)(1 << MB));
}
// step 2: the block's scale exponent from its maximum (finite)
template <MxFmt FMT>
__host__ __device__ inline int mx_block_exp(float amax) {
  constexpr int EMAX = FMT == kMxFp8 ? 8 : FMT == kMxE3M2 ? 4 : FMT == kMxInt8 ? 0 : 2;
  constexpr int E_MIN = FMT == kMxFp8 ? -117 : FMT == kMxFp4 ? -125 : FMT == kMxE2M3 ? -123 : FMT == kMxE3M2 ? -122 : -120;
  if (amax == 0.0f) return E_MIN;
  const int e = ilogb((double)amax) - EMAX;
  return e < E_MIN ? E_MIN : e > 127 ? 127 : e;
}
// step 3: the code (sign included) of bf16 weight h under scale exponent e
template <MxFmt FMT>
__host__ __device__ inline uint32_t mx_code(uint16_t h, int e) {
  const double aq = ldexp((double)bf16_to_f32((uint16_t)(h & 0x7FFFu)), -e);
  const uint32_t sign = h >> 15;
  if constexpr (FMT == kMxFp4) return mx_encode<1, 0, 1>(aq, 6.0) | (sign << 3);
  else if constexpr (FMT == kMxE2M3) return mx_encode<3, 0, 1>(aq, 7.5) | (sign << 5);
  else if constexpr (FMT == kMxE3M2) return mx_encode<2, -2, 3>(aq, 28.0) | (sign << 5);
  else if constexpr (FMT == kMxInt8) {
    // "6 mantissa bits, exponent 0 at bias 1" encodes |q| as the integer |i| = 0 .. 127; -0 is byte 0x80
    const uint32_t mag = mx_encode<6, 0, 1>(aq, 127.0 / 64.0);
    if (!sign) return mag;
    return mag ? 0x100u - mag : 0x80u;
  } else return mx_encode<3, -6, 7>(aq, 448.0) | (sign << 7);
}
// one thread per (column n, 32-block kb): steps 1-3 of the contract and the stores in the layout above
template <MxFmt FMT>
__global__ __launch_bounds__(256) void k_mx_pack(const uint16_t* W, int N, int K, uint8_t* out, int* nonfinite) {
  constexpr bool FP4 = FMT == kMxFp4, FP6 = FMT == kMxE2M3 || FMT == kMxE3M2;
  constexpr int V = mx_lane_bytes(FMT), CB = 64 * V, SB = CB + 64;
  const int nkb = K >> 5;
  const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (int64_t)N * nkb) return;
  const int n = (int)(id / nkb), kb = (int)(id % nkb);
  const uint16_t* row = W + (int64_t)n * K + kb * 32;
  float amax = 0.0f;
  bool bad = false;
  for (int i = 0; i < 32; ++i) {
    bad = bad || (row[i] & 0x7F80u) == 0x7F80u;
    amax = fmaxf(amax, fabsf(bf16_to_f32(row[i])));
  }
  if (bad) {  // step 5: the engine fails; the block is stored as zeros
    *nonfinite = 1;
    amax = 0.0f;
  }
  const int e = mx_block_exp<FMT>(amax);
  uint8_t* sb = out + ((int64_t)(n >> 4) * (K >> 7) + (kb >> 2)) * SB;
  const int li = n & 15, s = kb & 3;
  sb[CB + 4 * li + s] = (uint8_t)(e + 127);
  for (int g = 0; g < 4; ++g) {
    uint32_t c[2] = {0u, 0u};
    for (int i = 0; i < 8; ++i) {
      const uint32_t q = bad ? 0u : mx_code<FMT>(row[8 * g + i], e);
      if constexpr (FP4) c[0] |= q << (4 * i);
      else if constexpr (FP6) {
        c[0] |= (q & 15u) << (4 * i);
        c[1] |= (q >> 4) << (2 * i);
      } else c[i >> 2] |= q << (8 * (i & 3));
    }
    if constexpr (FP6) {  // the nibble plane as MXFP4's codes, the 2-bit plane behind it
      *(uint32_t*)(sb + (16 * g + li) * 16 + s * 4) = c[0];
      *(uint16_t*)(sb + 1024 + (16 * g + li) * 8 + s * 2) = (uint16_t)c[1];
    } else {
      uint8_t* dst = sb + (16 * g + li) * V + s * (V / 4);
      *(uint32_t*)dst = c[0];
      if constexpr (!FP4) *(uint32_t*)(dst + 4) = c[1];
    }
  }
}
// the one place a quant code becomes a template argument: CALL(format) for the format of qt
#define MX_FMT_SWITCH(qt, CALL)             \
  switch (qt) {                             \
    case kMxFp8: CALL(kMxFp8); break;       \
    case kMxFp4: CALL(kMxFp4); break;       \
    case kMxE2M3: CALL(kMxE2M3); break;     \
    case kMxE3M2: CALL(kMxE3M2); break;     \
    case kMxInt8: CALL(kMxInt8); break;     \
    default: break;                         \
  }
void launch_mx_pack(const uint16_t* W, int N, int K, int qt, uint8_t* out, int* nonfinite, hipStream_t st) {
  const int64_t n = (int64_t)N * (K / 32);
  const dim3 grid((unsigned)((n + 255) / 256));
#define MX_PACK(F) hipLaunchKernelGGL(k_mx_pack<F>, grid, dim3(256), 0, st, W, N, K, out, nonfinite)
  MX_FMT_SWITCH(qt, MX_PACK)
#undef MX_PACK
}

// the trivial unpack of the round-trip entry: the packed matrix back to row-major bf16 through the
// GEMM's own fragment dequantisation (mx_fragment). One thread per (column, step, g).
template <MxFmt FMT>
__global__ __launch_bounds__(256) void k_mx_unpack(const uint8_t* in, int N, int K, uint16_t* W) {
  constexpr bool FP4 = FMT == kMxFp4, FP6 = FMT == kMxE2M3 || FMT == kMxE3M2;
  constexpr int V = mx_lane_bytes(FMT), CB = 64 * V, SB = CB + 64;
  const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (int64_t)N * (K >> 3)) return;
  const int n = (int)(id / (K >> 3)), k8 = (int)(id % (K >> 3));
  const int kb = k8 >> 2, g = k8 & 3, li = n & 15, s = kb & 3;
  const uint8_t* sb = in + ((int64_t)(n >> 4) * (K >> 7) + (kb >> 2)) * SB;
  uint32_t c0, c1 = 0u;
  if constexpr (FP6) {
    c0 = *(const uint32_t*)(sb + (16 * g + li) * 16 + s * 4);
    c1 = *(const uint16_t*)(sb + 1024 + (16 * g + li) * 8 + s * 2);
  } else {
    const uint32_t* cp = (const uint32_t*)(sb + (16 * g + li) * V + s * (V / 4));
    c0 = cp[0];
    if constexpr (!FP4) c1 = cp[1];
  }
  const short8 f = mx_fragment<FMT>(c0, c1, (int)sb[CB + 4 * li + s]);
  *(short8*)(W + (int64_t)n * K + 8 * k8) = f;
}

// ---- GEMM ------------------------------------------------------------------------------------------
// out[split][row][col_off + n] = sum_{k in split} X[row][k] * W[n][k], W in the packed MX layout (MS 2:
// the tiles whose tinfo bit 31 is set; the others 16-bit fragments at a.tw). X as bf16 hi / lo planes
// (kXPlanes) or relu(sum of NX f32 slabs)^2 split on the fly (kXRelu2), staged as k_gemm2's plain role
// stages it (same sums, same split: the same X image). Grid (column tiles, K-splits, row groups).
template <int MT, int KSTEPS, int XMODE, int NX, int MS, MxFmt FMT>
__global__ __launch_bounds__(256) void k_gemm_mx(GemmArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int KS = KSTEPS * 32, LD = KS + 8, ROWS = MT * 16;
  constexpr bool FP6 = FMT == kMxE2M3 || FMT == kMxE3M2;
  constexpr int V = mx_lane_bytes(FMT), CB = 64 * V, SB = CB + 64, NSB = KSTEPS / 4;
  static_assert(KSTEPS % 4 == 0, "a K-slice is whole superblocks");
  tl_begin(a.tl);
  bf16_t* xh = (bf16_t*)smem;
  bf16_t* xl = xh + ROWS * LD;
  const int tile = blockIdx.x, split = blockIdx.y;
  const bf16_t* Wm = a.seg[0].W;
  const bf16_t* Xhi = a.seg[0].Xhi;
  const bf16_t* Xlo = a.seg[0].Xlo;
  const int ldx = a.seg[0].ldx;
  int Nn = a.seg[0].N, col_off = a.seg[0].col_off, tstart = a.seg[0].tile_start;
  bool mx = true;
  if constexpr (MS == 2) {
    const uint32_t ti = a.tinfo[tile];
    mx = (ti >> 31) != 0;
    const int mix = ti & 7;
    Wm = a.tw + (int64_t)tile * 64 * a.K;
    Xhi += mix * a.x_mix_stride;
    Xlo += mix * a.x_mix_stride;
    Nn = (ti >> 3) & 127;
    col_off = (int)((ti >> 10) & 0x1FFFFFu);
    tstart = tile;
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int g = lane >> 4, li = lane & 15;
  const int col0 = (tile - tstart) * 64 + wave * 16;
  const int kbeg = split * KS;
  const int nrg = (a.M + ROWS - 1) / ROWS;
  int rg = blockIdx.z;
  int xrow0 = rg * ROWS;
  constexpr int CH = KS / 8;
  constexpr int PERP = ROWS * CH / 256;      // kXPlanes: 16-byte chunks per thread per plane
  constexpr int PERR = ROWS * KS / 4 / 256;  // kXRelu2: float4 chunks per thread per slab
  short8 vh[XMODE == kXPlanes ? PERP : 1], vl[XMODE == kXPlanes ? PERP : 1];
  float4_ xr[XMODE == kXPlanes ? 1 : NX][XMODE == kXPlanes ? 1 : PERR];
  auto load_x = [&]() {  // rows past M: a copy of row M - 1 (never stored)
    if constexpr (XMODE == kXPlanes) {
#pragma unroll
      for (int u = 0; u < PERP; ++u) {
        const int c = threadIdx.x + u * 256;
        const int r = c / CH, k8 = (c % CH) * 8;
        const int64_t o = (int64_t)min(xrow0 + r, a.M - 1) * ldx + kbeg + k8;
        vh[u] = *(const short8*)(Xhi + o);
        vl[u] = *(const short8*)(Xlo + o);
      }
    } else {
#pragma unroll
      for (int p = 0; p < NX; ++p)
#pragma unroll
        for (int u = 0; u < PERR; ++u) {
          const int c = threadIdx.x + u * 256;
          const int r = c / (KS / 4), k4 = (c % (KS / 4)) * 4;
          xr[p][u] = *(const float4_*)(a.x_part + p * a.x_part_stride + (int64_t)min(xrow0 + r, a.M - 1) * a.x_ld + kbeg + k4);
        }
    }
  };
  load_x();
  // the weight feed: per superblock one 16-byte (MXFP4), two 16-byte (MXFP8 / MXINT8) or a 16-byte and an
  // 8-byte (MXFP6: nibble plane, 2-bit plane) code load and the column's scale word; a 16-bit tile streams
  // its fragments into b directly
  int nb = col0 >> 4;
  const int nblk = (Nn + 15) >> 4;
  if (nb >= nblk) nb = nblk - 1;
  short8 b[KSTEPS];
  u32x4_ cq[NSB][V == 32 ? 2 : 1];
  u32x2 hq[FP6 ? NSB : 1];  // MXFP6: the 2-bit plane, 16 bits per step
  uint32_t sq[NSB];
  if (mx) {
    const int nbq = MS == 2 ? tile * 4 + wave : nb;
    const uint8_t* sp = a.qw + ((int64_t)nbq * (a.K >> 7) + (kbeg >> 7)) * SB;
#pragma unroll
    for (int j = 0; j < NSB; ++j) {
      const u32x4_* cp = (const u32x4_*)(sp + (int64_t)j * SB + lane * (FP6 ? 16 : V));
      cq[j][0] = __builtin_nontemporal_load(cp);
      if constexpr (V == 32) cq[j][1] = __builtin_nontemporal_load(cp + 1);
      if constexpr (FP6) hq[j] = __builtin_nontemporal_load((const u32x2*)(sp + (int64_t)j * SB + 1024) + lane);
    }
#pragma unroll
    for (int j = 0; j < NSB; ++j) sq[j] = __builtin_nontemporal_load((const uint32_t*)(sp + (int64_t)j * SB + CB) + li);
  } else {
    const bf16_t* wp = Wm + (((int64_t)nb * (a.K >> 5) + (kbeg >> 5)) * 64 + lane) * 8;
#pragma unroll
    for (int t = 0; t < KSTEPS; ++t) b[t] = __builtin_nontemporal_load((const short8*)(wp + t * 512));
  }
  bool first = true;
  for (;;) {
    // X -> LDS
    if constexpr (XMODE == kXPlanes) {
#pragma unroll
      for (int u = 0; u < PERP; ++u) {
        const int c = threadIdx.x + u * 256;
        const int r = c / CH, k8 = (c % CH) * 8;
        *(short8*)(xh + r * LD + k8) = vh[u];
        *(short8*)(xl + r * LD + k8) = vl[u];
      }
    } else {
#pragma unroll
      for (int u = 0; u < PERR; ++u) {
        const int c = threadIdx.x + u * 256;
        const int r = c / (KS / 4), k4 = (c % (KS / 4)) * 4;
        float4_ x = xr[0][u];
#pragma unroll
        for (int p = 1; p < NX; ++p) x += xr[p][u];
        float y[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] = x[e] > 0.f ? x[e] * x[e] : 0.f;
        uint32_t h0, l0, h1, l1;
        split2<false>(y[0], y[1], h0, l0);
        split2<false>(y[2], y[3], h1, l1);
        *(uint2*)(xh + r * LD + k4) = make_uint2(h0, h1);
        *(uint2*)(xl + r * LD + k4) = make_uint2(l0, l1);
      }
    }
    if (first && mx) {  // the codes have landed behind X: the slice's bf16 fragments, once
#pragma unroll
      for (int t = 0; t < KSTEPS; ++t) {
        const int j = t >> 2, s = t & 3;
        const int sb = (int)((sq[j] >> (8 * s)) & 255u);
        if constexpr (FMT == kMxFp4) b[t] = mx_fragment<FMT>(cq[j][0][s], 0u, sb);
        else if constexpr (FP6) b[t] = mx_fragment<FMT>(cq[j][0][s], hq[j][s >> 1] >> (16 * (s & 1)), sb);
        else b[t] = mx_fragment<FMT>(cq[j][s >> 1][2 * (s & 1)], cq[j][s >> 1][2 * (s & 1) + 1], sb);
      }
    }
    first = false;
    __syncthreads();
    const int rg_next = rg + (int)gridDim.z;
    if (rg_next < nrg) {  // the next row group's X, in flight during this group's MFMAs and stores
      xrow0 = rg_next * ROWS;
      load_x();
    }
    // one MFMA per activation plane and step: the x_hi and x_lo chains apart, added at the end
    float4_ acc_h[MT], acc_l[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) acc_h[m] = acc_l[m] = (float4_){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < KSTEPS; ++t) {
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        const int o = (m * 16 + li) * LD + t * 32 + g * 8;
        const short8 ah = *(const short8*)(xh + o);
        const short8 al = *(const short8*)(xl + o);
        acc_h[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, ah), __builtin_bit_cast(bf16x8, b[t]),
                                                           acc_h[m], 0, 0, 0);
        acc_l[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, al), __builtin_bit_cast(bf16x8, b[t]),
                                                           acc_l[m], 0, 0, 0);
      }
    }
    // store (D layout: col = lane & 15, row = 4 (lane >> 4) + j)
    const int col = col0 + li;
    if (col < Nn) {
      float* out = a.out + split * a.split_stride + col_off + col;
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int row = rg * ROWS + m * 16 + 4 * g + j;
          if (row < a.M) out[(int64_t)row * a.ldo] = acc_h[m][j] + acc_l[m][j];
        }
    }
    if (rg_next >= nrg) break;
    rg = rg_next;
    __syncthreads();  // every wave is done with the LDS X image
  }
  tl_end(a.tl);
}

template <int MT, int KSTEPS, MxFmt FMT>
static bool launch_gemm_mx_t(const GemmArgs& a, dim3 grid, hipStream_t st) {
  const size_t lds = (size_t)MT * 16 * (KSTEPS * 32 + 8) * 2 * 2;
#define GMX(XM, NX_, MS_) RT_LAUNCH((k_gemm_mx<MT, KSTEPS, XM, NX_, MS_, FMT>), grid, dim3(256), lds, st, a)
  if (a.xmode == kXPlanes) {
    if (a.nseg > 1) GMX(kXPlanes, 1, 2);
    else GMX(kXPlanes, 1, 0);
  } else if (a.x_nsplit == 4) GMX(kXRelu2, 4, 0);
  else if (a.x_nsplit == 2) GMX(kXRelu2, 2, 0);
  else if (a.x_nsplit == 1) GMX(kXRelu2, 1, 0);
  else return false;
#undef GMX
  return true;
}

// the row tile and K-slice depth of one format (the quantised launches' K-slices are 128 or 256 deep:
// Engine::init's splits)
template <MxFmt FMT>
static bool launch_gemm_mx_f(const GemmArgs& a, int mt, dim3 grid, hipStream_t st) {
  if (a.kslice == 128) return mt == 1 ? launch_gemm_mx_t<1, 4, FMT>(a, grid, st) : launch_gemm_mx_t<2, 4, FMT>(a, grid, st);
  if (a.kslice == 256) return mt == 1 ? launch_gemm_mx_t<1, 8, FMT>(a, grid, st) : launch_gemm_mx_t<2, 8, FMT>(a, grid, st);
  return false;
}

int launch_gemm_mx(const GemmArgs& a, hipStream_t st) {
  // bf16 only; several segments only through the tile table; one segment starts at tile 0
  if (a.f16 || (a.nseg > 1 && a.n_tinfo <= 0) || (a.nseg == 1 && a.seg[0].tile_start != 0)) return -1;
  const int tiles = a.seg[a.nseg - 1].tile_start + (a.seg[a.nseg - 1].N + 63) / 64;
  const int mt = a.M <= 16 ? 1 : 2;  // the row tile of the unquantised launch
  const int mg = (a.M + mt * 16 - 1) / (mt * 16);
  dim3 grid(tiles, a.k_split, mg);
  // prefill steps: several row groups per workgroup (codes loaded and dequantised once), as many as keep
  // >= 4 workgroups per CU (launch_gemm's rule)
  if (grid.z > 1) {
    const int rpw = std::max(1, (int)grid.z * (int)(grid.x * grid.y) / 1024);
    grid.z = (grid.z + rpw - 1) / rpw;
  }
  bool ok = false;
#define GMX_FMT(F) ok = launch_gemm_mx_f<F>(a, mt, grid, st)
  MX_FMT_SWITCH(a.q_fmt, GMX_FMT)
#undef GMX_FMT
  return ok ? (int)(grid.x * grid.y * grid.z) : -1;
}

// rwkvtts_mx_roundtrip (include/rwkvtts.h): pack and unpack on the device
int mx_roundtrip(int qt, const uint16_t* w, int N, int K, uint16_t* out) {
  RT_CHECK(quant_is_mx(qt), RWKVTTS_EINVAL, "mx_roundtrip: type must be a Microscaling type (mxfp8 .. mxint8)");
  RT_CHECK(w && out && N > 0 && K > 0 && N % 16 == 0 && K % 128 == 0, RWKVTTS_EINVAL,
           "mx_roundtrip: N must be a multiple of 16 and K of 128");
  const size_t wb = (size_t)N * K * 2, pb = mx_pack_bytes(qt, N, K);
  uint8_t* d = nullptr;
  RT_HIP(hipMalloc(&d, 2 * wb + pb + 16));
  uint16_t* dw = (uint16_t*)d;
  uint16_t* dout = (uint16_t*)(d + wb);
  uint8_t* dp = d + 2 * wb;
  int* dflag = (int*)(dp + pb);
  int flag = 0;
  hipError_t e = hipMemcpy(dw, w, wb, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(dflag, &flag, sizeof(int), hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    launch_mx_pack(dw, N, K, qt, dp, dflag, nullptr);
    const dim3 grid((unsigned)(((int64_t)N * (K / 8) + 255) / 256));
#define MX_UNPACK(F) hipLaunchKernelGGL(k_mx_unpack<F>, grid, dim3(256), 0, nullptr, dp, N, K, dout)
    MX_FMT_SWITCH(qt, MX_UNPACK)
#undef MX_UNPACK
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(out, dout, wb, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(&flag, dflag, sizeof(int), hipMemcpyDeviceToHost);
  (void)hipFree(d);
  RT_HIP(e);
  RT_CHECK(flag == 0, RWKVTTS_EINVAL, "mx_roundtrip: non-finite weight");
  return RWKVTTS_OK;
}

}  // namespace rwkvtts
