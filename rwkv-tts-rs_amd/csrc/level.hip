// level.hip -- a look-ahead loudness leveller with a peak ceiling on the MI355X, for the `loudness`
// keyword of the pipeline: one-shot, batched (a target per signal) and over exact stream windows. No
// reference counterpart: the reference peak-normalises a finished WAV to 0.8, which sets no loudness
// and cannot be streamed.
//
// The arithmetic contract is in include/rwkvtts.h: a K-weighting FIR as a sequential
// f32 sum per sample, block energies from 64 ordered partials and a fixed tree, a serial gain scan
// over blocks with correctly rounded divides and square roots, a linear gain ramp per block. The
// kernels are pinned bitwise to a numpy restatement of exactly that (tests/test_gpu_level.py).
//
// Work: k_level_measure gives a workgroup to a block: the block's samples and their L - 1 samples of
// history in LDS, a lane runs the whole L-step chain of each sample it owns (four chains side by side,
// the taps uniform over the lanes and so in scalar registers), one wave then sums the squares in the
// contract's order. k_level_gain gives one wave to a job: its lanes form the momentary powers, lane 0
// runs the scan. k_level_apply gives a lane to every output sample. All three go to one stream; kernel
// order is the only hand-off.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <new>
#include <vector>

#include "common.h"
#include "stage.h"

// the table is built in double, step by step as the header states it: no contraction anywhere
#pragma clang fp contract(off)

namespace rwkvtts {

constexpr int kLevelThreads = 256;
constexpr int kLevelWaves = kLevelThreads / 64;
constexpr int kLevelChains = 4;  // chains a lane runs side by side
constexpr int64_t kLevelMaxSamples = (int64_t)1 << 40;

struct LevelCfg {
  int B, L, A, H;
  float gate, C, g_min, g_max;
};

// One grid row of each kernel: blocks [c, c + cnt) of one signal go out. The given samples are signal
// indices [in_first, in_end), stored at x[in_off ...]; every other index reads as zero (the host has
// checked that those are below 0 or past the end of a final window). Blocks [m0, m0 + m_cnt) are
// measured, block k at index mb_off + (k - m0) of E, pk and P; E from block e0 on (earlier ones give
// their peak only), and blocks from p0 on enter the estimate in this call. `last` is the last block
// that exists as far as this call knows. g[g_off + b] is the gain of block c - 1 + b.
struct LevelJob {
  int64_t in_off, in_first, in_end;
  int64_t c, cnt, m0, m_cnt, e0, p0, last;
  int64_t mb_off, g_off, out_off, out_count;
  int64_t n_prev;
  float t2, s_prev, g_prev;
};

struct LevelState {
  int64_t N;
  float S, g;
};

__device__ inline float level_x(const float* __restrict__ x, const LevelJob& j, int64_t idx) {
  return (idx >= j.in_first && idx < j.in_end) ? x[j.in_off + (idx - j.in_first)] : 0.0f;
}

// grid (measured blocks of the longest job, jobs). LDS: xs[B + L - 1] = x[kB - (L - 1), (k + 1)B),
// then zs[B].
__global__ __launch_bounds__(kLevelThreads) void k_level_measure(const float* __restrict__ x,
                                                                 const float* __restrict__ h,
                                                                 const LevelJob* __restrict__ jobs,
                                                                 float* __restrict__ E, float* __restrict__ pk, int B,
                                                                 int L) {
  extern __shared__ float s_mem[];
  __shared__ float s_pk[kLevelWaves];
  const LevelJob j = jobs[blockIdx.y];
  if ((int64_t)blockIdx.x >= j.m_cnt) return;  // (uniform over the workgroup)
  const int64_t k = j.m0 + blockIdx.x;
  const int tid = threadIdx.x;
  const int nx = B + L - 1;
  float* xs = s_mem;
  float* zs = s_mem + nx;
  const int64_t base = k * B - (L - 1);
  for (int i = tid; i < nx; i += kLevelThreads) xs[i] = level_x(x, j, base + i);
  __syncthreads();
  // the peak: a maximum has no order
  float m = 0.0f;
  for (int i = tid; i < B; i += kLevelThreads) m = fmaxf(m, fabsf(xs[L - 1 + i]));
  for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
  if ((tid & 63) == 0) s_pk[tid >> 6] = m;
  if (k >= j.e0) {  // (uniform) the chains: z[n] = sum_k h[k] x[n - k], ascending k from +0
    for (int q = 0; q * kLevelThreads < B; q += kLevelChains) {
      const float* xp[kLevelChains];
      float z[kLevelChains];
#pragma unroll
      for (int r = 0; r < kLevelChains; ++r) {
        const int i = tid + (q + r) * kLevelThreads;
        xp[r] = xs + (L - 1) + (i < B ? i : B - 1);  // (a chain past the block reruns the last sample's; not stored)
        z[r] = 0.0f;
      }
      // the LDS reads of eight steps are issued together ahead of the dependent adds; h[t] is uniform
      for (int t0 = 0; t0 < L; t0 += 8) {
        float hv[8], xv[kLevelChains][8];
#pragma unroll
        for (int t = 0; t < 8; ++t) hv[t] = h[t0 + t];
#pragma unroll
        for (int r = 0; r < kLevelChains; ++r)
#pragma unroll
          for (int t = 0; t < 8; ++t) xv[r][t] = xp[r][-(t0 + t)];
#pragma unroll
        for (int t = 0; t < 8; ++t)
#pragma unroll
          for (int r = 0; r < kLevelChains; ++r) z[r] = __fadd_rn(z[r], __fmul_rn(hv[t], xv[r][t]));
      }
#pragma unroll
      for (int r = 0; r < kLevelChains; ++r) {
        const int i = tid + (q + r) * kLevelThreads;
        if (i < B) zs[i] = (k * B + i < j.in_end) ? z[r] : 0.0f;
      }
    }
  }
  __syncthreads();
  if (tid >= 64) return;
  if (tid == 0) {
    float p = s_pk[0];
    for (int w = 1; w < kLevelWaves; ++w) p = fmaxf(p, s_pk[w]);
    pk[j.mb_off + blockIdx.x] = p;
  }
  if (k < j.e0) return;
  float p = 0.0f;  // p[l]: the squares of i = l (mod 64), ascending
  for (int i = tid; i < B; i += 64) p = __fadd_rn(p, __fmul_rn(zs[i], zs[i]));
  // p[l] += p[l + s] for l < s: lanes at or above s hold values nothing reads again
  for (int s = 32; s >= 1; s >>= 1) p = __fadd_rn(p, __shfl_down(p, s, 64));
  if (tid == 0) E[j.mb_off + blockIdx.x] = p;
}

// Correctly rounded f32 divide and square root, through double: the double quotient (root) of f32
// operands, rounded once more to f32, is the correctly rounded f32 result (53 >= 2 * 24 + 2 bits), and
// the device's double divide and square root are correctly rounded. The device's __fsqrt_rn is not:
// it is the native approximation, an ulp off numpy's sqrt on the first signal tried.
__device__ inline float level_div(float a, float b) { return (float)((double)a / (double)b); }
__device__ inline float level_sqrt(float a) { return (float)sqrt((double)a); }

// grid (jobs), one wave each.
__global__ __launch_bounds__(64) void k_level_gain(const LevelJob* __restrict__ jobs, const float* __restrict__ E,
                                                   const float* __restrict__ pk, float* __restrict__ P,
                                                   float* __restrict__ g, LevelState* __restrict__ state, LevelCfg c) {
  const LevelJob j = jobs[blockIdx.x];
  const int64_t m1 = j.m0 + j.m_cnt - 1;
  const float den = (float)(4 * c.B);
  for (int64_t k = j.p0 + threadIdx.x; k <= m1; k += 64) {
    float s = 0.0f;
#pragma unroll
    for (int d = 3; d >= 0; --d) s = __fadd_rn(s, k - d >= 0 ? E[j.mb_off + (k - d - j.m0)] : 0.0f);
    P[j.mb_off + (k - j.m0)] = level_div(s, den);
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  float S = j.s_prev, gj = j.g_prev;
  int64_t N = j.n_prev, next = j.p0;
  if (j.c > 0) g[j.g_off] = j.g_prev;
  for (int64_t b = 0; b < j.cnt; ++b) {
    const int64_t blk = j.c + b;
    const int64_t lim = blk + c.A < j.last ? blk + c.A : j.last;
    for (; next <= lim; ++next) {
      const float Pk = P[j.mb_off + (next - j.m0)];
      if (Pk >= c.gate) {
        if (c.H == 0 || N < c.H) {
          S = __fadd_rn(S, Pk);
          N += 1;
        } else {
          S = __fadd_rn(__fsub_rn(S, level_div(S, (float)c.H)), Pk);
        }
      }
    }
    gj = N == 0 ? 1.0f : level_sqrt(level_div(j.t2, level_div(S, (float)N)));
    if (gj < c.g_min) gj = c.g_min;
    if (gj > c.g_max) gj = c.g_max;
    const float pa = pk[j.mb_off + (blk - j.m0)];
    const float pb = blk + 1 <= j.last ? pk[j.mb_off + (blk + 1 - j.m0)] : 0.0f;
    const float p = pa > pb ? pa : pb;
    if (__fmul_rn(gj, p) > c.C) gj = level_div(c.C, p);
    if (blk == 0) g[j.g_off] = gj;  // g_-1 = g_0
    g[j.g_off + 1 + b] = gj;
  }
  state[blockIdx.x] = LevelState{N, S, gj};
}

// grid (blocks of the longest job, jobs): block b of job y, a lane per output sample.
__global__ __launch_bounds__(kLevelThreads) void k_level_apply(const float* __restrict__ x,
                                                               const float* __restrict__ r,
                                                               const LevelJob* __restrict__ jobs,
                                                               const float* __restrict__ g, float* __restrict__ y,
                                                               int B) {
  const LevelJob j = jobs[blockIdx.y];
  const int64_t b = blockIdx.x;
  if (b >= j.cnt) return;
  const float ga = g[j.g_off + b], gb = g[j.g_off + b + 1];
  const float dg = __fsub_rn(gb, ga);
  for (int i = threadIdx.x; i < B; i += kLevelThreads) {
    const int64_t o = b * B + i;
    if (o >= j.out_count) return;
    const float gi = __fadd_rn(ga, __fmul_rn(dg, r[i]));
    y[j.out_off + o] = __fmul_rn(level_x(x, j, (j.c + b) * B + i), gi);
  }
}

// ---- host: configuration, table, plan --------------------------------------------------------
static int level_config(const rwkvtts_level_desc* d, LevelCfg* c, const char* who) {
  RT_CHECK(d && d->struct_size >= sizeof(rwkvtts_level_desc), RWKVTTS_EINVAL,
           std::string(who) + ": null desc or struct_size too small");
  c->B = d->block ? d->block : 1600;
  c->L = d->taps ? d->taps : 1024;
  c->A = d->lookahead ? d->lookahead : 4;
  c->H = d->horizon;
  c->gate = d->gate != 0.0f ? d->gate : 1e-5f;
  c->C = d->ceiling != 0.0f ? d->ceiling : 0.891f;
  c->g_min = d->g_min != 0.0f ? d->g_min : 0.1f;
  c->g_max = d->g_max != 0.0f ? d->g_max : 10.0f;
  RT_CHECK(c->B >= 64 && c->B <= 4800 && c->B % 64 == 0, RWKVTTS_EINVAL,
           std::string(who) + ": block must be a multiple of 64, 64 .. 4800 (0 = 1600)");
  RT_CHECK(c->L >= 64 && c->L <= 2048 && c->L % 64 == 0, RWKVTTS_EINVAL,
           std::string(who) + ": taps must be a multiple of 64, 64 .. 2048 (0 = 1024)");
  RT_CHECK(c->A >= 1 && c->A <= 16, RWKVTTS_EINVAL, std::string(who) + ": lookahead must be 1 .. 16 (0 = 4)");
  RT_CHECK(c->H >= 0 && c->H <= (1 << 24), RWKVTTS_EINVAL, std::string(who) + ": horizon must be 0 .. 2^24");
  auto pos = [](float v) { return v > 0.0f && v <= 3.4028234e38f; };  // (NaN fails)
  RT_CHECK(pos(c->gate) && pos(c->C) && pos(c->g_min) && pos(c->g_max) && c->g_max >= c->g_min, RWKVTTS_EINVAL,
           std::string(who) + ": gate, ceiling, g_min and g_max must be finite and positive, g_max >= g_min");
  return RWKVTTS_OK;
}

static int level_t2_ok(float t2, const char* who) {
  RT_CHECK(t2 > 0.0f && t2 <= 3.4028234e38f, RWKVTTS_EINVAL, std::string(who) + ": t2 must be finite and positive");
  return RWKVTTS_OK;
}

struct LevelBiquad {
  double b0, b1, b2, a1, a2;
  double x1 = 0.0, x2 = 0.0, y1 = 0.0, y2 = 0.0;
  double step(double x) {  // direct form I, one operation at a time, left to right
    double y = b0 * x;
    y = y + b1 * x1;
    y = y + b2 * x2;
    y = y - a1 * y1;
    y = y - a2 * y2;
    x2 = x1;
    x1 = x;
    y2 = y1;
    y1 = y;
    return y;
  }
};

// the two K-weighting biquads at rate fs (the header's formulas, in its order of operations)
static void level_biquads(double fs, LevelBiquad* shelf, LevelBiquad* hp) {
  const double pi = 3.141592653589793;
  {
    const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
    const double K = tan(pi * f0 / fs);
    const double Vh = pow(10.0, G / 20.0);
    const double Vb = pow(Vh, 0.4996667741545416);
    const double KQ = K / Q, KK = K * K;
    const double a0 = (1.0 + KQ) + KK;
    shelf->b0 = ((Vh + Vb * KQ) + KK) / a0;
    shelf->b1 = (2.0 * (KK - Vh)) / a0;
    shelf->b2 = ((Vh - Vb * KQ) + KK) / a0;
    shelf->a1 = (2.0 * (KK - 1.0)) / a0;
    shelf->a2 = ((1.0 - KQ) + KK) / a0;
  }
  {
    const double f0 = 38.13547087602444, Q = 0.5003270373238773;
    const double K = tan(pi * f0 / fs);
    const double KQ = K / Q, KK = K * K;
    const double a0 = (1.0 + KQ) + KK;
    hp->b0 = 1.0;
    hp->b1 = -2.0;
    hp->b2 = 1.0;
    hp->a1 = (2.0 * (KK - 1.0)) / a0;
    hp->a2 = ((1.0 - KQ) + KK) / a0;
  }
}

static void level_make_table(const LevelCfg& c, float* out) {
  LevelBiquad shelf, hp;
  level_biquads(16000.0, &shelf, &hp);
  for (int n = 0; n < c.L; ++n) out[n] = (float)hp.step(shelf.step(n == 0 ? 1.0 : 0.0));
  for (int i = 0; i < c.B; ++i) out[c.L + i] = (float)((double)(i + 1) / (double)c.B);
}

static inline int64_t level_ready_end(const LevelCfg& c, int64_t n_known, int final) {
  return final ? n_known : c.B * std::max<int64_t>(0, n_known / c.B - c.A);
}
static inline int64_t level_in_first_needed(const LevelCfg& c, int64_t bf) {
  return std::max<int64_t>(0, std::min<int64_t>(bf * c.B, (bf + c.A - 3) * c.B - (c.L - 1)));
}

struct LevelWin {
  const float* in;
  int64_t in_first, n_in;
  int final;
  float t2;
  int64_t block_first;
  float s_prev;
  int64_t n_prev;
  float g_prev;
  int64_t out_count;
  float* out;
  float* s_last;
  int64_t* n_last;
  float* g_last;
};

}  // namespace rwkvtts

using namespace rwkvtts;

struct rwkvtts_level : Stage<LevelJob> {  // d_table: h[L] then r[B]
  LevelCfg cfg;
  DevBuf<float> d_E, d_pk, d_P, d_g;
  DevBuf<LevelState> d_state;
  std::vector<LevelState> last;
};

// Checks every window against the plan, then runs them all: one launch each of measure, gain and
// apply. Nothing is launched and nothing written unless every window passes.
static int level_run(rwkvtts_level* v, const std::vector<LevelWin>& ws, const char* who) {
  const LevelCfg& c = v->cfg;
  int64_t tot_in = 0, tot_out = 0, tot_mb = 0, tot_g = 0, max_mb = 0, max_blocks = 0;
  size_t n_jobs = 0;
  int rc;
  for (const LevelWin& w : ws) {
    if ((rc = level_t2_ok(w.t2, who))) return rc;
    RT_CHECK(w.in_first >= 0 && w.n_in >= 0 && w.block_first >= 0 && w.out_count >= 0 &&
                 w.in_first + w.n_in <= kLevelMaxSamples && w.block_first <= kLevelMaxSamples / c.B &&
                 (w.in || w.n_in == 0) && (w.out || w.out_count == 0),
             RWKVTTS_EINVAL, std::string(who) + ": bad window (negative size, null buffer or too long)");
    const bool state_ok =
        w.block_first == 0
            ? (w.n_prev == 0 && w.s_prev == 0.0f)
            : (w.n_prev >= 0 && w.n_prev <= w.block_first + c.A && (c.H == 0 || w.n_prev <= c.H) &&
               w.s_prev >= 0.0f && w.s_prev <= 3.4028234e38f && (w.n_prev == 0) == (w.s_prev == 0.0f) &&
               w.g_prev > 0.0f && w.g_prev <= c.g_max);
    RT_CHECK(state_ok, RWKVTTS_EINVAL, std::string(who) + ": (s_prev, n_prev, g_prev) is no state a scan can have left");
    if (w.out_count == 0) continue;
    const int64_t n = w.in_first + w.n_in, end = w.block_first * c.B + w.out_count;
    RT_CHECK(end <= level_ready_end(c, n, w.final), RWKVTTS_EINVAL,
             std::string(who) + ": a requested block needs samples past the given ones");
    RT_CHECK(w.out_count % c.B == 0 || (w.final && end == n), RWKVTTS_EINVAL,
             std::string(who) + ": out_count must end on a block or, with final, on the signal's end");
    RT_CHECK(w.in_first <= level_in_first_needed(c, w.block_first), RWKVTTS_EINVAL,
             std::string(who) + ": a requested block reads before the given samples");
    const int64_t cnt = (w.out_count + c.B - 1) / c.B;
    const int64_t last = w.final ? (n + c.B - 1) / c.B - 1 : n / c.B - 1;
    const int64_t e0 = w.block_first == 0 ? 0 : std::max<int64_t>(0, w.block_first + c.A - 3);
    const int64_t m0 = std::min(w.block_first, e0);
    const int64_t m1 = std::min(w.block_first + cnt - 1 + c.A, last);
    tot_in += w.n_in;
    tot_out += w.out_count;
    tot_mb += m1 - m0 + 1;
    tot_g += cnt + 1;
    max_mb = std::max(max_mb, m1 - m0 + 1);
    max_blocks = std::max(max_blocks, cnt);
    ++n_jobs;
  }
  auto pass_state = [&](const LevelWin& w) {
    if (w.s_last) *w.s_last = w.s_prev;
    if (w.n_last) *w.n_last = w.n_prev;
    if (w.g_last) *w.g_last = w.g_prev;
  };
  if (n_jobs == 0) {
    for (const LevelWin& w : ws) pass_state(w);
    return RWKVTTS_OK;
  }
  RT_CHECK(n_jobs <= 65535 && max_mb <= 0x7fffffff, RWKVTTS_EINVAL, std::string(who) + ": too much for one launch");
  std::lock_guard<std::mutex> lock(v->mu);
  v->desc.clear();
  v->last.assign(n_jobs, LevelState{0, 0.0f, 0.0f});
  int64_t in_off = 0, out_off = 0, mb_off = 0, g_off = 0;
  for (const LevelWin& w : ws) {
    if (w.out_count == 0) continue;
    const int64_t n = w.in_first + w.n_in;
    LevelJob j;
    j.in_off = in_off;
    j.in_first = w.in_first;
    j.in_end = n;
    j.c = w.block_first;
    j.cnt = (w.out_count + c.B - 1) / c.B;
    j.last = w.final ? (n + c.B - 1) / c.B - 1 : n / c.B - 1;
    j.e0 = j.c == 0 ? 0 : std::max<int64_t>(0, j.c + c.A - 3);
    j.p0 = j.c == 0 ? 0 : j.c + c.A;
    j.m0 = std::min(j.c, j.e0);
    j.m_cnt = std::min(j.c + j.cnt - 1 + c.A, j.last) - j.m0 + 1;
    j.mb_off = mb_off;
    j.g_off = g_off;
    j.out_off = out_off;
    j.out_count = w.out_count;
    j.n_prev = j.c == 0 ? 0 : w.n_prev;
    j.t2 = w.t2;
    j.s_prev = j.c == 0 ? 0.0f : w.s_prev;
    j.g_prev = j.c == 0 ? 1.0f : w.g_prev;
    v->desc.push_back(j);
    in_off += w.n_in;
    out_off += w.out_count;
    mb_off += j.m_cnt;
    g_off += j.cnt + 1;
  }
  if ((rc = stage_reserve(v, tot_in, tot_out)) || (rc = v->d_E.reserve((size_t)tot_mb)) ||
      (rc = v->d_pk.reserve((size_t)tot_mb)) || (rc = v->d_P.reserve((size_t)tot_mb)) ||
      (rc = v->d_g.reserve((size_t)tot_g)) || (rc = v->d_state.reserve(n_jobs)) || (rc = stage_upload(v, ws)))
    return rc;
  // the event pair brackets all three kernels: start of the measure, end of the apply
  const size_t lds = (size_t)(2 * c.B + c.L - 1) * sizeof(float);  // 46.6 KB at the widest
  hipExtLaunchKernelGGL(k_level_measure, dim3((unsigned)max_mb, (unsigned)n_jobs), dim3(kLevelThreads), lds, v->stream,
                        v->ev0, nullptr, 0u, v->d_in.p, v->d_table, v->d_desc.p, v->d_E.p, v->d_pk.p, c.B, c.L);
  RT_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_level_gain, dim3((unsigned)n_jobs), dim3(64), 0, v->stream, v->d_desc.p, v->d_E.p, v->d_pk.p,
                     v->d_P.p, v->d_g.p, v->d_state.p, c);
  RT_HIP(hipGetLastError());
  hipExtLaunchKernelGGL(k_level_apply, dim3((unsigned)max_blocks, (unsigned)n_jobs), dim3(kLevelThreads), 0, v->stream,
                        nullptr, v->ev1, 0u, v->d_in.p, v->d_table + c.L, v->d_desc.p, v->d_g.p, v->d_out.p, c.B);
  RT_HIP(hipGetLastError());
  RT_HIP(hipMemcpyAsync(v->last.data(), v->d_state.p, n_jobs * sizeof(LevelState), hipMemcpyDeviceToHost, v->stream));
  if ((rc = stage_download(v, ws))) return rc;
  size_t k = 0;
  for (const LevelWin& w : ws) {
    if (w.out_count == 0) {
      pass_state(w);
      continue;
    }
    const LevelState& s = v->last[k++];
    if (w.s_last) *w.s_last = s.S;
    if (w.n_last) *w.n_last = s.N;
    if (w.g_last) *w.g_last = s.g;
  }
  return RWKVTTS_OK;
}

extern "C" int rwkvtts_level_table(const rwkvtts_level_desc* desc, float* out) {
  LevelCfg c;
  int rc = level_config(desc, &c, "level_table");
  if (rc) return rc;
  RT_CHECK(out, RWKVTTS_EINVAL, "level_table: null output");
  level_make_table(c, out);
  return RWKVTTS_OK;
}

extern "C" float rwkvtts_level_target(double loudness_db) { return (float)pow(10.0, (loudness_db + 0.691) / 10.0); }

extern "C" int rwkvtts_level_plan(const rwkvtts_level_desc* desc, int64_t n_known, int final, int64_t block_first,
                                  int64_t* out_ready_end, int64_t* in_first_needed) {
  LevelCfg c;
  int rc = level_config(desc, &c, "level_plan");
  if (rc) return rc;
  RT_CHECK(n_known >= 0 && n_known <= kLevelMaxSamples && block_first >= 0 && block_first <= kLevelMaxSamples / c.B,
           RWKVTTS_EINVAL, "level_plan: n_known / block_first out of range");
  if (out_ready_end) *out_ready_end = level_ready_end(c, n_known, final);
  if (in_first_needed) *in_first_needed = level_in_first_needed(c, block_first);
  return RWKVTTS_OK;
}

extern "C" int rwkvtts_level_create(int device, const rwkvtts_level_desc* desc, const float* table,
                                    rwkvtts_level** out) {
  RT_CHECK(out, RWKVTTS_EINVAL, "level_create: null output");
  *out = nullptr;
  LevelCfg c;
  int rc = level_config(desc, &c, "level_create");
  if (rc) return rc;
  rwkvtts_level* v = nullptr;
  rc = stage_create("level_create", device, table, (size_t)(c.L + c.B), [&](float* t) { level_make_table(c, t); }, &v);
  if (rc) return rc;
  v->cfg = c;
  *out = v;
  return RWKVTTS_OK;
}

extern "C" int rwkvtts_level_destroy(rwkvtts_level* v) {
  if (!v) return RWKVTTS_OK;
  (void)hipSetDevice(v->device);
  stage_free(v, {v->d_E.p, v->d_pk.p, v->d_P.p, v->d_g.p, v->d_state.p});
  return RWKVTTS_OK;
}

extern "C" int rwkvtts_level_batch(rwkvtts_level* v, const float* const* in, const int64_t* n_in, const float* t2,
                                   int n, float* const* out) {
  RT_CHECK(v && n >= 0 && (n == 0 || (in && n_in && t2 && out)), RWKVTTS_EINVAL, "level_batch: bad arguments");
  return guard_alloc("level_batch", [&] {
    std::vector<LevelWin> ws((size_t)n);
    for (int i = 0; i < n; ++i) {
      RT_CHECK(n_in[i] >= 0 && n_in[i] <= kLevelMaxSamples, RWKVTTS_EINVAL, "level_batch: n_in out of range");
      ws[(size_t)i] = LevelWin{in[i], 0, n_in[i], 1, t2[i], 0, 0.0f, 0, 1.0f, n_in[i], out[i], nullptr, nullptr, nullptr};
    }
    return level_run(v, ws, "level_batch");
  });
}

extern "C" int rwkvtts_level_windows(rwkvtts_level* v, rwkvtts_level_window* w, int n) {
  RT_CHECK(v && n >= 0 && (n == 0 || w), RWKVTTS_EINVAL, "level_windows: bad arguments");
  if (n == 0) return RWKVTTS_OK;
  return guard_alloc("level_windows", [&] {
    std::vector<LevelWin> ws;
    int rc = read_windows("level_windows", w, n, ws, [](rwkvtts_level_window* wi) {
      return LevelWin{wi->in, wi->in_first, wi->n_in, wi->final ? 1 : 0, wi->t2, wi->block_first, wi->s_prev,
                      wi->n_prev, wi->g_prev, wi->out_count, wi->out, &wi->s_last, &wi->n_last, &wi->g_last};
    });
    return rc ? rc : level_run(v, ws, "level_windows");
  });
}

extern "C" int rwkvtts_level_kernel_ms(rwkvtts_level* v, double* ms) { return stage_kernel_ms("level_kernel_ms", v, ms); }
