// lora.hip -- per-request LoRA adapters (include/rwkvtts.h, "adapters"): the device repack of an
// adapter's matrices at load and k_lora, the gathered low-rank GEMM that adds a row's delta
//   y += B (s * (A x))
// into split-K slab 0 of the base GEMM launch it follows (Engine::launch_forward).
//
// Work split. A workgroup = 4 waves = one row tile x 256 output columns (64 per wave) of one
// target matrix; grid (column blocks, row tiles, targets of the launch). A row tile is up to 16
// row indices of the step that share an adapter (gathered: the rows need not be adjacent), read
// from the step's tile table at a fixed device address: [0] the tile count, then per tile
// kLoraTileInts ints {adapter, rows, -, -, row[16]}. Tiles past the count exit, so a captured
// grid only has to be large enough.
//
// Shrink, t [16][r] = X A^T. Wave w takes the w-th contiguous quarter of K in 32-deep MFMA steps.
// A lane's operands are 8 contiguous k of one row (X hi and lo planes, straight from global memory
// into registers; the value target forms relu(sum of the key slabs)^2 and its planes in registers,
// k_relu2_planes' arithmetic) and 8 contiguous k of one rank row (A in fragment order: every wave
// load is 1 KB contiguous). One v_mfma_f32_16x16x32_bf16 chain per plane and 16-wide rank block,
// hi + lo at the end. The four partial t go through LDS ([4][16][RP] f32, 16 KB at r = 64), are
// summed in wave order ((0 + 1) + 2) + 3, scaled by s (one rounded multiply), split into hi / lo
// bf16 planes and left in the same LDS.
//
// Expand, y [16][64 per wave] += t B^T with K = RP, the rank padded to the MFMA depth: ranks 16 and
// 48 are ZERO-PADDED to 32 / 64 when the adapter is packed (A's pad rows are zero, so t's pad columns
// are exact zeros; B's pad columns are zero). Two chains (t_hi, t_lo), added at the end, then a plain
// read-modify-write of slab 0 for the tile's valid rows: each output element belongs to one lane of
// one workgroup, so no atomics. Every column block recomputes the shrink (X and A come from L2): one
// launch per insertion point instead of two.
//
// Invariance. An MFMA output row depends on its own A-operand row only, the K order is fixed, and a
// tile's pad rows (copies of its first row) are never stored: a row's delta depends on the row and
// its adapter, not on the tile's other rows, its position, the step's row count or the route.
#include "lm_kernels.h"

#include <type_traits>

namespace rwkvtts {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// ---- pack ----------------------------------------------------------------------------------------
// W [N][K] row-major bf16 -> [Np][Kp] (zero-padded; Np % 16 == 0, Kp % 32 == 0) in MFMA fragment
// order: block (nb, kb) = 16 rows x 32 k at ((nb * Kp / 32 + kb) * 64 + lane) * 8, lane 16 g + li
// holding k = 32 kb + 8 g .. + 8 of row 16 nb + li. *nonfinite is set to 1 for an Inf or a NaN.
__global__ __launch_bounds__(256) void k_lora_pack(const uint16_t* W, int N, int K, int Np, int Kp, uint16_t* out,
                                                   int* nonfinite) {
  const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // one 8-element lane chunk each
  if (id >= (int64_t)Np * Kp / 8) return;
  const int lane = (int)(id & 63);
  const int64_t blk = id >> 6;
  const int kb = (int)(blk % (Kp >> 5)), nb = (int)(blk / (Kp >> 5));
  const int n = nb * 16 + (lane & 15), k0 = kb * 32 + (lane >> 4) * 8;
  short8 v = {0, 0, 0, 0, 0, 0, 0, 0};
  bool bad = false;
  if (n < N)
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (k0 + e < K) {
        const uint16_t h = W[(int64_t)n * K + k0 + e];
        bad = bad || (h & 0x7F80u) == 0x7F80u;
        v[e] = (short)h;
      }
  if (bad) *nonfinite = 1;
  *(short8*)(out + id * 8) = v;
}

void launch_lora_pack(const uint16_t* W, int N, int K, int Np, int Kp, uint16_t* out, int* nonfinite, hipStream_t st) {
  const int64_t n = (int64_t)Np * Kp / 8;
  hipLaunchKernelGGL(k_lora_pack, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, W, N, K, Np, Kp, out, nonfinite);
}

// ---- k_lora --------------------------------------------------------------------------------------
// a lane's 8 k of one row of the value target's input: relu(slab 0 + slab 1 + ...)^2, split
__device__ inline void relu2_operand(const LoraArgs& a, int64_t o, short8& hi, short8& lo) {
  float4_ x0 = *(const float4_*)(a.x_part + o), x1 = *(const float4_*)(a.x_part + o + 4);
  for (int p = 1; p < a.x_nsplit; ++p) {
    x0 += *(const float4_*)(a.x_part + p * a.x_part_stride + o);
    x1 += *(const float4_*)(a.x_part + p * a.x_part_stride + o + 4);
  }
  float y[8];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    y[e] = x0[e] > 0.f ? x0[e] * x0[e] : 0.f;
    y[4 + e] = x1[e] > 0.f ? x1[e] * x1[e] : 0.f;
  }
  uint32_t h[4], l[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) split2<false>(y[2 * e], y[2 * e + 1], h[e], l[e]);
  hi = __builtin_bit_cast(short8, (u32x4_){h[0], h[1], h[2], h[3]});
  lo = __builtin_bit_cast(short8, (u32x4_){l[0], l[1], l[2], l[3]});
}

// RB: 16-wide rank blocks of the padded rank (RP = 16 RB = 32 or 64)
template <int RB, bool RELU2>
__device__ inline void lora_tile(const LoraArgs& a, const int* tile, float s, const bf16_t* Ap, const bf16_t* Bp,
                                 const bf16_t* xhi, const bf16_t* xlo, int col_off, char* smem) {
  constexpr int RP = RB * 16, LDT = RP + 8;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int g = lane >> 4, li = lane & 15;
  const int nrows = tile[1];
  // ---- shrink: this wave's quarter of K
  const int xrow = tile[4 + min(li, nrows - 1)];  // pad rows: a copy of a valid row, never stored
  const int KQ = a.K >> 2, kbeg = wave * KQ, steps = KQ >> 5;
  float4_ acc_h[RB], acc_l[RB];
#pragma unroll
  for (int rb = 0; rb < RB; ++rb) acc_h[rb] = acc_l[rb] = (float4_){0.f, 0.f, 0.f, 0.f};
  const bf16_t* ap = Ap + ((int64_t)(kbeg >> 5) * 64 + lane) * 8;
  const int64_t ablk = (int64_t)(a.K >> 5) * 512;  // elements per rank block
  const int64_t xo = (int64_t)xrow * (RELU2 ? a.x_ld : a.ldx) + kbeg + g * 8;
  // U steps' operands are requested together and then consumed in ascending k (the chains' order is
  // that of a step-by-step loop): the loop is bound by load latency, not by the MFMAs
  constexpr int U = RELU2 ? 2 : 4;
  auto run = [&](int t0, auto un) {
    constexpr int N_ = decltype(un)::value;
    short8 xh[N_], xl[N_], af[N_][RB];
#pragma unroll
    for (int u = 0; u < N_; ++u) {
      if constexpr (RELU2) {
        relu2_operand(a, xo + (t0 + u) * 32, xh[u], xl[u]);
      } else {
        xh[u] = *(const short8*)(xhi + xo + (t0 + u) * 32);
        xl[u] = *(const short8*)(xlo + xo + (t0 + u) * 32);
      }
#pragma unroll
      for (int rb = 0; rb < RB; ++rb) af[u][rb] = *(const short8*)(ap + rb * ablk + (t0 + u) * 512);
    }
#pragma unroll
    for (int u = 0; u < N_; ++u)
#pragma unroll
      for (int rb = 0; rb < RB; ++rb) {
        acc_h[rb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, xh[u]),
                                                            __builtin_bit_cast(bf16x8, af[u][rb]), acc_h[rb], 0, 0, 0);
        acc_l[rb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, xl[u]),
                                                            __builtin_bit_cast(bf16x8, af[u][rb]), acc_l[rb], 0, 0, 0);
      }
  };
  int t = 0;
  for (; t + U <= steps; t += U) run(t, std::integral_constant<int, U>{});
  for (; t < steps; ++t) run(t, std::integral_constant<int, 1>{});
  // ---- the four partial t through LDS (D layout: col = lane & 15, row = 4 (lane >> 4) + j)
  float* part = (float*)smem;  // [4][16][RP]
#pragma unroll
  for (int rb = 0; rb < RB; ++rb)
#pragma unroll
    for (int j = 0; j < 4; ++j) part[(wave * 16 + 4 * g + j) * RP + rb * 16 + li] = acc_h[rb][j] + acc_l[rb][j];
  __syncthreads();
  constexpr int PAIRS = 8 * RP / 256;  // adjacent-element pairs per thread
  float tv[PAIRS][2];
#pragma unroll
  for (int u = 0; u < PAIRS; ++u) {
    const int p = threadIdx.x + u * 256;
    const int row = p / (RP / 2), c = 2 * (p % (RP / 2));
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int o = row * RP + c + e;
      tv[u][e] = (((part[o] + part[16 * RP + o]) + part[32 * RP + o]) + part[48 * RP + o]) * s;
    }
  }
  __syncthreads();  // every partial is read: the planes take the same LDS
  bf16_t* th = (bf16_t*)smem;  // [16][LDT] hi, then lo
  bf16_t* tlo = th + 16 * LDT;
#pragma unroll
  for (int u = 0; u < PAIRS; ++u) {
    const int p = threadIdx.x + u * 256;
    const int row = p / (RP / 2), c = 2 * (p % (RP / 2));
    uint32_t h, l;
    split2<false>(tv[u][0], tv[u][1], h, l);
    *(uint32_t*)(th + row * LDT + c) = h;
    *(uint32_t*)(tlo + row * LDT + c) = l;
  }
  __syncthreads();
  // ---- expand: this wave's 64 columns, 16 at a time
  short8 ah[RP / 32], al[RP / 32];
#pragma unroll
  for (int ks = 0; ks < RP / 32; ++ks) {
    ah[ks] = *(const short8*)(th + li * LDT + ks * 32 + g * 8);
    al[ks] = *(const short8*)(tlo + li * LDT + ks * 32 + g * 8);
  }
  int orow[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) orow[j] = 4 * g + j < nrows ? tile[4 + 4 * g + j] : -1;
#pragma unroll
  for (int cb = 0; cb < 4; ++cb) {
    const int col0 = blockIdx.x * 256 + wave * 64 + cb * 16;
    if (col0 >= a.N) continue;  // (N % 16 == 0: a 16-column block is whole or absent)
    const bf16_t* bp = Bp + ((int64_t)(col0 >> 4) * (RP / 32) * 64 + lane) * 8;
    float4_ dh = {0.f, 0.f, 0.f, 0.f}, dl = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < RP / 32; ++ks) {
      const short8 bf = *(const short8*)(bp + ks * 512);
      dh = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, ah[ks]), __builtin_bit_cast(bf16x8, bf), dh, 0,
                                                   0, 0);
      dl = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, al[ks]), __builtin_bit_cast(bf16x8, bf), dl, 0,
                                                   0, 0);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (orow[j] >= 0) {
        float* o = a.out + (int64_t)orow[j] * a.ldo + col_off + col0 + li;
        *o += dh[j] + dl[j];
      }
  }
}

template <bool RELU2>
__global__ __launch_bounds__(256) void k_lora(LoraArgs a) {
  __shared__ __attribute__((aligned(16))) char smem[4 * 16 * 64 * 4];
  tl_begin(a.tl);
  const int t = blockIdx.y;
  if (t < a.tiles[0]) {
    const int* tile = a.tiles + kLoraTileHead + t * kLoraTileInts;
    const LoraDev ad = a.adapters[tile[0]];
    const int target = a.target0 + blockIdx.z;
    const int64_t* offs = ad.offs + ((int64_t)a.layer * 6 + target) * 2;
    if (offs[0] >= 0) {  // (a target the adapter does not carry contributes nothing)
      const bf16_t* Ap = ad.base + offs[0];
      const bf16_t* Bp = ad.base + offs[1];
      const bf16_t* xhi = RELU2 ? nullptr : a.xhi + a.xmix[blockIdx.z] * a.x_mix_stride;
      const bf16_t* xlo = RELU2 ? nullptr : a.xlo + a.xmix[blockIdx.z] * a.x_mix_stride;
      const int col_off = blockIdx.z * a.col_stride;
      if (ad.rb == 2) lora_tile<2, RELU2>(a, tile, ad.s, Ap, Bp, xhi, xlo, col_off, smem);
      else lora_tile<4, RELU2>(a, tile, ad.s, Ap, Bp, xhi, xlo, col_off, smem);
    }
  }
  tl_end(a.tl);
}

int launch_lora(const LoraArgs& a, int n_tiles, int n_targets, hipStream_t st) {
  const dim3 grid((a.N + 255) / 256, n_tiles, n_targets);
  if (a.x_part) RT_LAUNCH(k_lora<true>, grid, dim3(256), 0, st, a);
  else RT_LAUNCH(k_lora<false>, grid, dim3(256), 0, st, a);
  return (int)(grid.x * grid.y * grid.z);
}

}  // namespace rwkvtts
