// wm.hip -- a provenance watermark on the MI355X, for the `watermark` keyword of the pipeline and the
// /api/watermark/detect route: a time-domain spread-spectrum mark embedded one-shot, batched (a key, a
// payload and a strength per signal) and over exact stream windows, and a brute-force detector over
// every alignment of the mark's period. No reference counterpart: the reference marks nothing.
//
// The contract is in include/rwkvtts.h. The embedder is arithmetic, pinned bitwise to
// its numpy restatement (tests/test_gpu_wm.py): chips from a counter-based hash, a carrier as a
// sequential f32 tap sum, a block gain from the leveller's energy sum with a correctly rounded divide
// and square root, a linear ramp per block. The detector is held to the float64 restatement within
// the forward-error bound of its f32 sums; its summation orders are fixed, so it is deterministic.
//
// Work: k_wm_embed gives a workgroup to a block -- the B + L - 1 chips it needs hashed into LDS, the
// block's and the previous block's energies by one wave each, a lane per sample for the tap sum and
// the apply. k_wm_whiten gives a workgroup to a block; k_wm_fold a lane to a phase m of the period
// (the clip staged through LDS a tile at a time); k_wm_search a lane to an offset tau: per bit slot
// the TB + 255 folded values a tile of 256 offsets reads are staged in LDS as (F, F^2) pairs with the
// slot's chips as packed bits, every lane walks the slot's phases (the chip word is uniform, the
// pairs are one conflict-free 8-byte read per lane) and flips F's sign bit by the chip; the tile's
// best offset goes to global memory and k_wm_pick reduces over tiles. All launches go to one stream;
// kernel order is the only hand-off.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <new>
#include <vector>

#include "common.h"
#include "stage.h"

// the table and the threshold are built in double, step by step: no contraction anywhere
#pragma clang fp contract(off)

namespace rwkvtts {

constexpr int kWmThreads = 256;
constexpr int64_t kWmMaxSamples = (int64_t)1 << 40;
constexpr int64_t kWmMaxClip = (int64_t)1 << 30;
constexpr float kWmEps = 7.62939453125e-06f;  // 2^-17

struct WmCfg {
  int B, L, NB, TB, NP;
  double lo, hi, sdb;
};

// One grid row of k_wm_embed: blocks [c, c + cnt) of one signal go out. The given samples are signal
// indices [in_first, in_end), stored at x[in_off ...]; every other index reads as zero (the host has
// checked that those are past the end of a final window). k2 = splitmix64(key).
struct WmJob {
  int64_t in_off, in_first, in_end;
  int64_t c, cnt, out_off, out_count;
  uint64_t k2;
  uint32_t payload;
  float s, a_prev;
};

// One clip of the detector: samples x[in_off, in_off + n), its folded pairs at fg[job * NP], its tile
// results at tiles[job * n_tiles]; dbg_off: the clip's slice of the debug arrays, or -1.
struct WmDetJob {
  int64_t in_off, n, dbg_off;
  uint64_t k2;
};

struct WmBest {
  float S;
  int32_t tau;
  uint32_t payload, seen;
  float min_z;
};

__host__ __device__ inline uint64_t wm_splitmix64(uint64_t x) {
  uint64_t z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__device__ inline float wm_x(const float* __restrict__ x, const WmJob& j, int64_t idx) {
  return (idx >= j.in_first && idx < j.in_end) ? x[j.in_off + (idx - j.in_first)] : 0.0f;
}

// Correctly rounded f32 divide and square root, through double (level.hip has the argument).
__device__ inline float wm_div(float a, float b) { return (float)((double)a / (double)b); }
__device__ inline float wm_sqrt(float a) { return (float)sqrt((double)a); }

// One wave: the block energy of xs[0, B) in the contract's order; every lane returns E in lane 0's place.
__device__ inline float wm_energy(const float* xs, int B, int lane) {
  float p = 0.0f;  // p[l]: the squares of i = l (mod 64), ascending
  for (int i = lane; i < B; i += 64) p = __fadd_rn(p, __fmul_rn(xs[i], xs[i]));
  for (int s = 32; s >= 1; s >>= 1) p = __fadd_rn(p, __shfl_down(p, s, 64));
  return __shfl(p, 0, 64);
}

// grid (blocks of the longest job, jobs). LDS: cs[B + L - 1], the chips of samples
// [kB - (L - 1), (k + 1)B) as +-1.0f; xs[B], the block; xp[B], the block before it.
__global__ __launch_bounds__(kWmThreads) void k_wm_embed(const float* __restrict__ x, const float* __restrict__ h,
                                                         const float* __restrict__ r,
                                                         const WmJob* __restrict__ jobs, float* __restrict__ y,
                                                         float* __restrict__ a_last, int B, int L, int TB, int NP) {
  extern __shared__ float s_mem[];
  __shared__ float s_a[2];
  const WmJob j = jobs[blockIdx.y];
  if ((int64_t)blockIdx.x >= j.cnt) return;  // (uniform over the workgroup)
  const int64_t k = j.c + blockIdx.x;
  const int tid = threadIdx.x;
  const int nc = B + L - 1;
  float* cs = s_mem;
  float* xs = s_mem + nc;
  float* xp = xs + B;
  const bool have_prev = blockIdx.x > 0;  // (the block before is this window's own: its samples are given)
  const int64_t base = k * B - (L - 1);
  for (int i = tid; i < nc; i += kWmThreads) {
    int64_t m = (base + i) % NP;
    if (m < 0) m += NP;
    const uint32_t chip = (uint32_t)(wm_splitmix64(j.k2 + (uint64_t)m) >> 63);
    const uint32_t bit = (j.payload >> (uint32_t)(m / TB)) & 1u;
    cs[i] = chip == bit ? 1.0f : -1.0f;
  }
  for (int i = tid; i < B; i += kWmThreads) {
    xs[i] = wm_x(x, j, k * B + i);
    xp[i] = have_prev ? wm_x(x, j, (k - 1) * B + i) : 0.0f;
  }
  __syncthreads();
  const int wave = tid >> 6, lane = tid & 63;
  if (wave == 0 || (wave == 1 && have_prev)) {
    const float E = wm_energy(wave == 0 ? xs : xp, B, lane);
    if (lane == 0) s_a[1 - wave] = __fmul_rn(j.s, wm_sqrt(wm_div(E, (float)B)));
  }
  __syncthreads();
  const float a1 = s_a[1];
  const float a0 = have_prev ? s_a[0] : (k == 0 ? a1 : j.a_prev);  // a_{-1} = a_0
  const float da = __fsub_rn(a1, a0);
  for (int i = tid; i < B; i += kWmThreads) {
    const int64_t o = (int64_t)blockIdx.x * B + i;
    if (o >= j.out_count) break;
    const float* cp = cs + (L - 1) + i;  // the chip of sample kB + i; tap t reads cp[-t]
    float u = 0.0f;
#pragma unroll 8
    for (int t = 0; t < L; ++t) u = __fadd_rn(u, __fmul_rn(h[t], cp[-t]));
    const float g = __fadd_rn(a0, __fmul_rn(da, r[i]));
    y[j.out_off + o] = __fadd_rn(xs[i], __fmul_rn(g, u));
  }
  if (blockIdx.x + 1 == j.cnt && tid == 0) a_last[blockIdx.y] = a1;
}

// ---- the detector --------------------------------------------------------------------------------
// grid (blocks of the longest clip, clips): w = x / (sqrt(E / B) + eps) for one block.
__global__ __launch_bounds__(kWmThreads) void k_wm_whiten(const float* __restrict__ x,
                                                          const WmDetJob* __restrict__ jobs, float* __restrict__ w,
                                                          int B) {
  extern __shared__ float s_mem[];
  __shared__ float s_q;
  const WmDetJob j = jobs[blockIdx.y];
  const int64_t n0 = (int64_t)blockIdx.x * B;
  if (n0 >= j.n) return;  // (uniform)
  const int tid = threadIdx.x;
  for (int i = tid; i < B; i += kWmThreads) s_mem[i] = n0 + i < j.n ? x[j.in_off + n0 + i] : 0.0f;
  __syncthreads();
  if (tid < 64) {
    const float E = wm_energy(s_mem, B, tid);
    if (tid == 0) s_q = sqrtf(E / (float)B) + kWmEps;
  }
  __syncthreads();
  const float q = s_q;
  for (int i = tid; i < B; i += kWmThreads)
    if (n0 + i < j.n) w[j.in_off + n0 + i] = s_mem[i] / q;
}

// grid (tiles of 256 phases, clips): lane m of a tile sums v[n] over n = m (mod NP) in ascending n,
// v[n] = sum_k h[k] w[n + k], and stores the pair (F, F^2). LDS: ws[256 + L - 1], the clip from the
// tile's fold on.
__global__ __launch_bounds__(kWmThreads) void k_wm_fold(const float* __restrict__ w, const float* __restrict__ h,
                                                        const WmDetJob* __restrict__ jobs, float2* __restrict__ fg,
                                                        int L, int NP) {
  extern __shared__ float s_mem[];
  const WmDetJob j = jobs[blockIdx.y];
  const int tid = threadIdx.x;
  const int m = blockIdx.x * kWmThreads + tid;
  const int nw = kWmThreads + L - 1;
  float F = 0.0f;
  for (int64_t n0 = (int64_t)blockIdx.x * kWmThreads; n0 < j.n; n0 += NP) {  // (uniform)
    __syncthreads();
    for (int i = tid; i < nw; i += kWmThreads) s_mem[i] = n0 + i < j.n ? w[j.in_off + n0 + i] : 0.0f;
    __syncthreads();
    if (m < NP && n0 + tid < j.n) {
      const float* wp = s_mem + tid;
      float v = 0.0f;
#pragma unroll 8
      for (int t = 0; t < L; ++t) v = fmaf(h[t], wp[t], v);
      F += v;
    }
  }
  if (m < NP) fg[(int64_t)blockIdx.y * NP + m] = make_float2(F, F * F);
}

// grid (tiles of 256 offsets, clips). LDS: pairs[TB + 255] then words[TB / 32]. Lane t holds offset
// tau = tile * 256 + t; pairs[q] is (F, F^2) at phase (b TB - tile * 256 - 255 + q) mod NP, so that
// phase m of slot b is pairs[(m - b TB) + 255 - t] for lane t.
__global__ __launch_bounds__(kWmThreads) void k_wm_search(const float2* __restrict__ fg,
                                                          const WmDetJob* __restrict__ jobs,
                                                          WmBest* __restrict__ tiles, float* __restrict__ dbg_r,
                                                          float* __restrict__ dbg_d, int NB, int TB, int NP) {
  extern __shared__ float2 s_pairs[];
  __shared__ float s_S[kWmThreads / 64];
  __shared__ int s_tau[kWmThreads / 64];
  const WmDetJob j = jobs[blockIdx.y];
  const int t = threadIdx.x;
  const int tau0 = blockIdx.x * kWmThreads;
  const int tau = tau0 + t;
  const int np = TB + kWmThreads - 1;
  uint32_t* words = (uint32_t*)(s_pairs + np);
  const float2* src = fg + (int64_t)blockIdx.y * NP;
  float S = 0.0f, min_z = 3.4028234e38f;
  uint32_t payload = 0, seen = 0;
  for (int b = 0; b < NB; ++b) {
    __syncthreads();
    for (int q = t; q < np; q += kWmThreads) {
      int ph = (b * TB - tau0 - (kWmThreads - 1) + q) % NP;
      if (ph < 0) ph += NP;
      s_pairs[q] = src[ph];
    }
    for (int wd = t; wd < TB / 32; wd += kWmThreads) {
      uint32_t word = 0;
      const uint64_t m0 = (uint64_t)(b * TB + wd * 32);
      for (int i = 0; i < 32; ++i) word |= (uint32_t)(wm_splitmix64(j.k2 + m0 + (uint64_t)i) >> 63) << i;
      words[wd] = ~word;  // a set bit: chip -1, the sign flips
    }
    __syncthreads();
    const float2* p = s_pairs + (kWmThreads - 1 - t);
    float r = 0.0f, d = 0.0f;
    for (int wd = 0; wd < TB / 32; ++wd) {
      const uint32_t flip = words[wd];  // (uniform: a broadcast)
#pragma unroll
      for (int i = 0; i < 32; ++i) {
        const float2 v = p[wd * 32 + i];
        r += __uint_as_float(__float_as_uint(v.x) ^ ((flip >> i) << 31));
        d += v.y;
      }
    }
    if (j.dbg_off >= 0 && tau < NP) {
      dbg_r[j.dbg_off + (int64_t)b * NP + tau] = r;
      dbg_d[j.dbg_off + (int64_t)b * NP + tau] = d;
    }
    if (d > 0.0f) {
      const float z = r / sqrtf(d);
      S = fmaf(z, z, S);
      seen |= 1u << b;
      if (z > 0.0f) payload |= 1u << b;
      min_z = fminf(min_z, fabsf(z));
    }
  }
  // the tile's best: the highest S, the lowest tau on a tie (offsets past the period never win)
  float bS = tau < NP ? S : -1.0f;
  int bt = tau;
  for (int off = 32; off >= 1; off >>= 1) {
    const float oS = __shfl_xor(bS, off, 64);
    const int ot = __shfl_xor(bt, off, 64);
    if (oS > bS || (oS == bS && ot < bt)) bS = oS, bt = ot;
  }
  if ((t & 63) == 0) s_S[t >> 6] = bS, s_tau[t >> 6] = bt;
  __syncthreads();
  bS = s_S[0], bt = s_tau[0];
  for (int w = 1; w < kWmThreads / 64; ++w)
    if (s_S[w] > bS || (s_S[w] == bS && s_tau[w] < bt)) bS = s_S[w], bt = s_tau[w];
  if (tau == bt) tiles[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = WmBest{S, tau, payload, seen, seen ? min_z : 0.0f};
}

// grid (clips), one wave each: the best tile (the lowest on a tie, so the lowest tau).
__global__ __launch_bounds__(64) void k_wm_pick(const WmBest* __restrict__ tiles, WmBest* __restrict__ out,
                                                int n_tiles) {
  const WmBest* row = tiles + (int64_t)blockIdx.x * n_tiles;
  float bS = -2.0f;
  int bi = 0x7fffffff;
  for (int i = threadIdx.x; i < n_tiles; i += 64)
    if (row[i].S > bS) bS = row[i].S, bi = i;  // (ascending i: the first of equals stays)
  for (int off = 32; off >= 1; off >>= 1) {
    const float oS = __shfl_xor(bS, off, 64);
    const int oi = __shfl_xor(bi, off, 64);
    if (oS > bS || (oS == bS && oi < bi)) bS = oS, bi = oi;
  }
  if (bi >= n_tiles) bi = 0;  // (every score a NaN: a non-finite clip)
  if (threadIdx.x == 0) out[blockIdx.x] = row[bi];
}

// ---- host: configuration, table, threshold, plan ---------------------------------------------
static int wm_config(const rwkvtts_wm_desc* d, WmCfg* c, const char* who) {
  RT_CHECK(d && d->struct_size >= sizeof(rwkvtts_wm_desc), RWKVTTS_EINVAL,
           std::string(who) + ": null desc or struct_size too small");
  c->B = d->block ? d->block : 320;
  c->L = d->taps ? d->taps : 129;
  c->NB = d->bits ? d->bits : 16;
  c->TB = d->bit_len ? d->bit_len : 1600;
  c->lo = d->band_lo != 0.0f ? (double)d->band_lo : 1000.0;
  c->hi = d->band_hi != 0.0f ? (double)d->band_hi : 3400.0;
  c->sdb = d->strength_db != 0.0f ? (double)d->strength_db : -26.0;
  RT_CHECK(c->B >= 64 && c->B <= 4800 && c->B % 64 == 0, RWKVTTS_EINVAL,
           std::string(who) + ": block must be a multiple of 64, 64 .. 4800 (0 = 320)");
  RT_CHECK(c->L >= 3 && c->L <= 1023 && c->L % 2 == 1, RWKVTTS_EINVAL,
           std::string(who) + ": taps must be odd, 3 .. 1023 (0 = 129)");
  RT_CHECK(c->NB >= 1 && c->NB <= 32, RWKVTTS_EINVAL, std::string(who) + ": bits must be 1 .. 32 (0 = 16)");
  RT_CHECK(c->TB >= c->B && c->TB <= 6400 && c->TB % c->B == 0, RWKVTTS_EINVAL,
           std::string(who) + ": bit_len must be a multiple of block, at most 6400 (0 = 1600)");
  RT_CHECK(c->lo > 0.0 && c->hi > c->lo && c->hi < 8000.0, RWKVTTS_EINVAL,
           std::string(who) + ": the band must satisfy 0 < band_lo < band_hi < 8000 Hz");  // (NaN fails)
  RT_CHECK(c->sdb >= -60.0 && c->sdb <= -6.0, RWKVTTS_EINVAL,
           std::string(who) + ": strength_db must be -60 .. -6 (0 = -26)");
  c->NP = c->NB * c->TB;
  return RWKVTTS_OK;
}

static double wm_sinc(double x) {
  const double pi = 3.141592653589793;
  const double y = pi * (x == 0.0 ? 1.0e-20 : x);
  return sin(y) / y;
}

static void wm_make_table(const WmCfg& c, float* out) {
  const double pi = 3.141592653589793;
  std::vector<double> g((size_t)c.L);
  const double fh = (2.0 * c.hi) / 16000.0, fl = (2.0 * c.lo) / 16000.0;
  double e = 0.0;
  for (int k = 0; k < c.L; ++k) {
    const double t = (double)k - (double)((c.L - 1) / 2);
    const double w = (0.42 - 0.5 * cos(((2.0 * pi) * (double)k) / (double)(c.L - 1))) +
                     0.08 * cos(((4.0 * pi) * (double)k) / (double)(c.L - 1));
    g[(size_t)k] = w * (fh * wm_sinc(fh * t) - fl * wm_sinc(fl * t));
    e = e + g[(size_t)k] * g[(size_t)k];
  }
  const double norm = sqrt(e);
  for (int k = 0; k < c.L; ++k) out[k] = (float)(g[(size_t)k] / norm);
  for (int i = 0; i < c.B; ++i) out[c.L + i] = (float)((double)(i + 1) / (double)c.B);
}

// Q(T; k): the chi-square upper tail, by its closed forms.
static double wm_chi2_sf(double T, int k) {
  const double x = 0.5 * T;
  double s = 0.0;
  if (k % 2 == 0) {
    double term = 1.0;
    for (int i = 0; i < k / 2; ++i) {
      s += term;
      term *= x / (double)(i + 1);
    }
    return exp(-x) * s;
  }
  double term = sqrt(x) / tgamma(1.5);  // x^(i + 1/2) / Gamma(i + 3/2)
  for (int i = 0; i < (k - 1) / 2; ++i) {
    s += term;
    term *= x / ((double)i + 1.5);
  }
  return erfc(sqrt(x)) + exp(-x) * s;
}

static double wm_threshold(const WmCfg& c) {
  double lo = 0.0, hi = 1.0;
  while ((double)c.NP * wm_chi2_sf(hi, c.NB) > 1e-6) hi *= 2.0;
  for (int i = 0; i < 200; ++i) {
    const double mid = 0.5 * (lo + hi);
    if ((double)c.NP * wm_chi2_sf(mid, c.NB) > 1e-6)
      lo = mid;
    else
      hi = mid;
  }
  return hi;
}

static inline int64_t wm_ready_end(const WmCfg& c, int64_t n_known, int final) {
  return final ? n_known : c.B * (n_known / c.B);
}

struct WmWin {
  const float* in;
  int64_t in_first, n_in;
  int final;
  float s;
  uint64_t key;
  uint32_t payload;
  float a_prev;
  int64_t block_first, out_count;
  float* out;
  float* a_last;
};

}  // namespace rwkvtts

using namespace rwkvtts;

struct rwkvtts_wm : Stage<WmJob> {  // d_table: h[L] then r[B]
  WmCfg cfg;
  DevBuf<float> d_a;  // a of each job's last block
  std::vector<float> last;
  // the detector's
  DevBuf<WmDetJob> d_det;
  DevBuf<float> d_w, d_dbg_r, d_dbg_d;
  DevBuf<float2> d_fg;
  DevBuf<WmBest> d_tiles, d_best;
  std::vector<WmDetJob> det;
  std::vector<WmBest> best;
};

// Checks every window against the plan, then runs them all in one launch. Nothing is launched and
// nothing written unless every window passes.
static int wm_run(rwkvtts_wm* v, const std::vector<WmWin>& ws, const char* who) {
  const WmCfg& c = v->cfg;
  int64_t tot_in = 0, tot_out = 0, max_blocks = 0;
  size_t n_jobs = 0;
  for (const WmWin& w : ws) {
    RT_CHECK(w.s > 0.0f && w.s <= 1.0f, RWKVTTS_EINVAL, std::string(who) + ": strength must be finite, in (0, 1]");
    RT_CHECK(c.NB == 32 || (w.payload >> c.NB) == 0, RWKVTTS_EINVAL, std::string(who) + ": payload has bits past `bits`");
    RT_CHECK(w.in_first >= 0 && w.n_in >= 0 && w.block_first >= 0 && w.out_count >= 0 &&
                 w.in_first + w.n_in <= kWmMaxSamples && w.block_first <= kWmMaxSamples / c.B &&
                 (w.in || w.n_in == 0) && (w.out || w.out_count == 0),
             RWKVTTS_EINVAL, std::string(who) + ": bad window (negative size, null buffer or too long)");
    RT_CHECK(w.block_first == 0 || (w.a_prev >= 0.0f && w.a_prev <= 3.4028234e38f), RWKVTTS_EINVAL,
             std::string(who) + ": a_prev must be finite and not negative");
    if (w.out_count == 0) continue;
    const int64_t n = w.in_first + w.n_in, end = w.block_first * c.B + w.out_count;
    RT_CHECK(end <= wm_ready_end(c, n, w.final), RWKVTTS_EINVAL,
             std::string(who) + ": a requested block needs samples past the given ones");
    RT_CHECK(w.out_count % c.B == 0 || (w.final && end == n), RWKVTTS_EINVAL,
             std::string(who) + ": out_count must end on a block or, with final, on the signal's end");
    RT_CHECK(w.in_first <= w.block_first * c.B, RWKVTTS_EINVAL,
             std::string(who) + ": a requested block reads before the given samples");
    tot_in += w.n_in;
    tot_out += w.out_count;
    max_blocks = std::max(max_blocks, (w.out_count + c.B - 1) / c.B);
    ++n_jobs;
  }
  if (n_jobs == 0) {
    for (const WmWin& w : ws)
      if (w.a_last) *w.a_last = w.a_prev;
    return RWKVTTS_OK;
  }
  RT_CHECK(n_jobs <= 65535 && max_blocks <= 0x7fffffff, RWKVTTS_EINVAL, std::string(who) + ": too much for one launch");
  std::lock_guard<std::mutex> lock(v->mu);
  v->desc.clear();
  v->last.assign(n_jobs, 0.0f);
  int64_t in_off = 0, out_off = 0;
  for (const WmWin& w : ws) {
    if (w.out_count == 0) continue;
    WmJob j;
    j.in_off = in_off;
    j.in_first = w.in_first;
    j.in_end = w.in_first + w.n_in;
    j.c = w.block_first;
    j.cnt = (w.out_count + c.B - 1) / c.B;
    j.out_off = out_off;
    j.out_count = w.out_count;
    j.k2 = wm_splitmix64(w.key);
    j.payload = w.payload;
    j.s = w.s;
    j.a_prev = w.block_first == 0 ? 0.0f : w.a_prev;
    v->desc.push_back(j);
    in_off += w.n_in;
    out_off += w.out_count;
  }
  int rc;
  if ((rc = stage_reserve(v, tot_in, tot_out)) || (rc = v->d_a.reserve(n_jobs)) || (rc = stage_upload(v, ws))) return rc;
  const size_t lds = (size_t)(3 * c.B + c.L - 1) * sizeof(float);  // 61.7 KB at the widest
  hipExtLaunchKernelGGL(k_wm_embed, dim3((unsigned)max_blocks, (unsigned)n_jobs), dim3(kWmThreads), lds, v->stream,
                        v->ev0, v->ev1, 0u, v->d_in.p, v->d_table, v->d_table + c.L, v->d_desc.p, v->d_out.p, v->d_a.p,
                        c.B, c.L, c.TB, c.NP);
  RT_HIP(hipGetLastError());
  RT_HIP(hipMemcpyAsync(v->last.data(), v->d_a.p, n_jobs * sizeof(float), hipMemcpyDeviceToHost, v->stream));
  if ((rc = stage_download(v, ws))) return rc;
  size_t k = 0;
  for (const WmWin& w : ws) {
    const float a = w.out_count == 0 ? w.a_prev : v->last[k++];
    if (w.a_last) *w.a_last = a;
  }
  return RWKVTTS_OK;
}

extern "C" int rwkvtts_wm_table(const rwkvtts_wm_desc* desc, float* out) {
  WmCfg c;
  int rc = wm_config(desc, &c, "wm_table");
  if (rc) return rc;
  RT_CHECK(out, RWKVTTS_EINVAL, "wm_table: null output");
  return guard_alloc("wm_table", [&] {
    wm_make_table(c, out);
    return RWKVTTS_OK;
  });
}

extern "C" float rwkvtts_wm_strength(double strength_db) {
  if (!(strength_db >= -60.0 && strength_db <= -6.0)) return nanf("");
  return (float)pow(10.0, strength_db / 20.0);
}

extern "C" int rwkvtts_wm_threshold(const rwkvtts_wm_desc* desc, double* out) {
  WmCfg c;
  int rc = wm_config(desc, &c, "wm_threshold");
  if (rc) return rc;
  RT_CHECK(out, RWKVTTS_EINVAL, "wm_threshold: null output");
  *out = wm_threshold(c);
  return RWKVTTS_OK;
}

extern "C" int rwkvtts_wm_plan(const rwkvtts_wm_desc* desc, int64_t n_known, int final, int64_t block_first,
                               int64_t* out_ready_end, int64_t* in_first_needed) {
  WmCfg c;
  int rc = wm_config(desc, &c, "wm_plan");
  if (rc) return rc;
  RT_CHECK(n_known >= 0 && n_known <= kWmMaxSamples && block_first >= 0 && block_first <= kWmMaxSamples / c.B,
           RWKVTTS_EINVAL, "wm_plan: n_known / block_first out of range");
  if (out_ready_end) *out_ready_end = wm_ready_end(c, n_known, final);
  if (in_first_needed) *in_first_needed = block_first * c.B;
  return RWKVTTS_OK;
}

extern "C" int rwkvtts_wm_create(int device, const rwkvtts_wm_desc* desc, const float* table, rwkvtts_wm** out) {
  RT_CHECK(out, RWKVTTS_EINVAL, "wm_create: null output");
  *out = nullptr;
  WmCfg c;
  int rc = wm_config(desc, &c, "wm_create");
  if (rc) return rc;
  rwkvtts_wm* v = nullptr;
  rc = stage_create("wm_create", device, table, (size_t)(c.L + c.B), [&](float* t) { wm_make_table(c, t); }, &v);
  if (rc) return rc;
  v->cfg = c;
  *out = v;
  return RWKVTTS_OK;
}

extern "C" int rwkvtts_wm_destroy(rwkvtts_wm* v) {
  if (!v) return RWKVTTS_OK;
  (void)hipSetDevice(v->device);
  stage_free(v, {v->d_a.p, v->d_det.p, v->d_w.p, v->d_dbg_r.p, v->d_dbg_d.p, v->d_fg.p, v->d_tiles.p, v->d_best.p});
  return RWKVTTS_OK;
}

extern "C" int rwkvtts_wm_embed_batch(rwkvtts_wm* v, const float* const* in, const int64_t* n_in, const uint64_t* key,
                                      const uint32_t* payload, const float* strength, int n, float* const* out) {
  RT_CHECK(v && n >= 0 && (n == 0 || (in && n_in && key && payload && out)), RWKVTTS_EINVAL,
           "wm_embed_batch: bad arguments");
  return guard_alloc("wm_embed_batch", [&] {
    const float s0 = (float)pow(10.0, v->cfg.sdb / 20.0);
    std::vector<WmWin> ws((size_t)n);
    for (int i = 0; i < n; ++i) {
      RT_CHECK(n_in[i] >= 0 && n_in[i] <= kWmMaxSamples, RWKVTTS_EINVAL, "wm_embed_batch: n_in out of range");
      ws[(size_t)i] = WmWin{in[i], 0, n_in[i], 1, strength ? strength[i] : s0, key[i], payload[i], 0.0f, 0, n_in[i], out[i],
                            nullptr};
    }
    return wm_run(v, ws, "wm_embed_batch");
  });
}

extern "C" int rwkvtts_wm_embed_windows(rwkvtts_wm* v, rwkvtts_wm_window* w, int n) {
  RT_CHECK(v && n >= 0 && (n == 0 || w), RWKVTTS_EINVAL, "wm_embed_windows: bad arguments");
  if (n == 0) return RWKVTTS_OK;
  return guard_alloc("wm_embed_windows", [&] {
    std::vector<WmWin> ws;
    int rc = read_windows("wm_embed_windows", w, n, ws, [](rwkvtts_wm_window* wi) {
      return WmWin{wi->in, wi->in_first, wi->n_in, wi->final ? 1 : 0, wi->strength, wi->key, wi->payload, wi->a_prev,
                   wi->block_first, wi->out_count, wi->out, &wi->a_last};
    });
    return rc ? rc : wm_run(v, ws, "wm_embed_windows");
  });
}

extern "C" int rwkvtts_wm_detect_batch(rwkvtts_wm* v, const float* const* in, const int64_t* n_in, const uint64_t* key,
                                       int n, rwkvtts_wm_result* results) {
  RT_CHECK(v && n >= 0 && (n == 0 || (in && n_in && key && results)), RWKVTTS_EINVAL, "wm_detect_batch: bad arguments");
  if (n == 0) return RWKVTTS_OK;
  return guard_alloc("wm_detect_batch", [&] {
    const WmCfg& c = v->cfg;
    const size_t stride = results->struct_size;
    RT_CHECK(stride >= sizeof(rwkvtts_wm_result), RWKVTTS_EINVAL, "wm_detect_batch: struct_size too small");
    auto res = [&](int i) { return (rwkvtts_wm_result*)((char*)results + (size_t)i * stride); };
    const double T = wm_threshold(c);
    const int64_t per_dbg = (int64_t)c.NB * c.NP;
    int64_t tot_in = 0, tot_dbg = 0, max_n = 0;
    std::lock_guard<std::mutex> lock(v->mu);
    v->det.clear();
    for (int i = 0; i < n; ++i) {
      rwkvtts_wm_result* r = res(i);
      RT_CHECK(r->struct_size == stride, RWKVTTS_EINVAL, "wm_detect_batch: struct_size differs between results");
      RT_CHECK(n_in[i] >= 0 && n_in[i] <= kWmMaxClip && (in[i] || n_in[i] == 0), RWKVTTS_EINVAL,
               "wm_detect_batch: n_in out of range or null clip");
      RT_CHECK((r->dbg_r == nullptr) == (r->dbg_d == nullptr), RWKVTTS_EINVAL,
               "wm_detect_batch: dbg_r and dbg_d go together");
      if (n_in[i] == 0) continue;
      WmDetJob j;
      j.in_off = tot_in;
      j.n = n_in[i];
      j.dbg_off = r->dbg_r ? tot_dbg : -1;
      j.k2 = wm_splitmix64(key[i]);
      v->det.push_back(j);
      tot_in += n_in[i];
      if (r->dbg_r) tot_dbg += per_dbg;
      max_n = std::max(max_n, n_in[i]);
    }
    for (int i = 0; i < n; ++i) {
      rwkvtts_wm_result* r = res(i);
      r->detected = 0, r->score = 0.0f, r->offset = 0, r->payload = 0, r->seen = 0, r->min_z = 0.0f;
    }
    const size_t n_jobs = v->det.size();
    if (n_jobs == 0) return RWKVTTS_OK;
    RT_CHECK(n_jobs <= 65535, RWKVTTS_EINVAL, "wm_detect_batch: too many clips for one launch");
    const int n_tiles = (c.NP + kWmThreads - 1) / kWmThreads;
    int rc;
    RT_HIP(hipSetDevice(v->device));
    if ((rc = v->d_in.reserve((size_t)tot_in)) || (rc = v->d_w.reserve((size_t)tot_in)) ||
        (rc = v->d_det.reserve(n_jobs)) || (rc = v->d_fg.reserve(n_jobs * (size_t)c.NP)) ||
        (rc = v->d_tiles.reserve(n_jobs * (size_t)n_tiles)) || (rc = v->d_best.reserve(n_jobs)) ||
        (rc = v->d_dbg_r.reserve((size_t)std::max<int64_t>(tot_dbg, 1))) ||
        (rc = v->d_dbg_d.reserve((size_t)std::max<int64_t>(tot_dbg, 1))))
      return rc;
    size_t k = 0;
    for (int i = 0; i < n; ++i) {
      if (n_in[i] == 0) continue;
      RT_HIP(hipMemcpyAsync(v->d_in.p + v->det[k].in_off, in[i], (size_t)n_in[i] * sizeof(float), hipMemcpyHostToDevice,
                            v->stream));
      ++k;
    }
    RT_HIP(hipMemcpyAsync(v->d_det.p, v->det.data(), n_jobs * sizeof(WmDetJob), hipMemcpyHostToDevice, v->stream));
    // the event pair brackets all four kernels: start of the whitening, end of the pick
    const unsigned max_blocks = (unsigned)((max_n + c.B - 1) / c.B);
    hipExtLaunchKernelGGL(k_wm_whiten, dim3(max_blocks, (unsigned)n_jobs), dim3(kWmThreads), (size_t)c.B * sizeof(float),
                          v->stream, v->ev0, nullptr, 0u, v->d_in.p, v->d_det.p, v->d_w.p, c.B);
    RT_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_wm_fold, dim3((unsigned)n_tiles, (unsigned)n_jobs), dim3(kWmThreads),
                       (size_t)(kWmThreads + c.L - 1) * sizeof(float), v->stream, v->d_w.p, v->d_table, v->d_det.p,
                       v->d_fg.p, c.L, c.NP);
    RT_HIP(hipGetLastError());
    const size_t lds = (size_t)(c.TB + kWmThreads - 1) * sizeof(float2) + (size_t)(c.TB / 32) * sizeof(uint32_t);  // 54 KB at the widest
    hipLaunchKernelGGL(k_wm_search, dim3((unsigned)n_tiles, (unsigned)n_jobs), dim3(kWmThreads), lds, v->stream,
                       v->d_fg.p, v->d_det.p, v->d_tiles.p, v->d_dbg_r.p, v->d_dbg_d.p, c.NB, c.TB, c.NP);
    RT_HIP(hipGetLastError());
    hipExtLaunchKernelGGL(k_wm_pick, dim3((unsigned)n_jobs), dim3(64), 0, v->stream, nullptr, v->ev1, 0u, v->d_tiles.p,
                          v->d_best.p, n_tiles);
    RT_HIP(hipGetLastError());
    v->best.assign(n_jobs, WmBest{0.0f, 0, 0, 0, 0.0f});
    RT_HIP(hipMemcpyAsync(v->best.data(), v->d_best.p, n_jobs * sizeof(WmBest), hipMemcpyDeviceToHost, v->stream));
    k = 0;
    for (int i = 0; i < n; ++i) {
      if (n_in[i] == 0) continue;
      rwkvtts_wm_result* r = res(i);
      if (r->dbg_r) {
        RT_HIP(hipMemcpyAsync(r->dbg_r, v->d_dbg_r.p + v->det[k].dbg_off, (size_t)per_dbg * sizeof(float),
                              hipMemcpyDeviceToHost, v->stream));
        RT_HIP(hipMemcpyAsync(r->dbg_d, v->d_dbg_d.p + v->det[k].dbg_off, (size_t)per_dbg * sizeof(float),
                              hipMemcpyDeviceToHost, v->stream));
      }
      ++k;
    }
    RT_HIP(hipStreamSynchronize(v->stream));
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, v->ev0, v->ev1) == hipSuccess) v->kernel_ms = (double)ms;
    k = 0;
    for (int i = 0; i < n; ++i) {
      if (n_in[i] == 0) continue;
      const WmBest& b = v->best[k++];
      rwkvtts_wm_result* r = res(i);
      r->detected = (double)b.S >= T ? 1 : 0;
      r->score = b.S;
      r->offset = b.tau >= 0 && b.tau < c.NP ? b.tau : 0;  // (a non-finite clip can leave any lane's)
      r->payload = b.payload;
      r->seen = b.seen;
      r->min_z = b.min_z;
    }
    return RWKVTTS_OK;
  });
}

extern "C" int rwkvtts_wm_kernel_ms(rwkvtts_wm* v, double* ms) { return stage_kernel_ms("wm_kernel_ms", v, ms); }
