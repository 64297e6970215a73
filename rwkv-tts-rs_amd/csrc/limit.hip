// limit.hip -- a look-ahead true-peak limiter on the MI355X, for the `limit` keyword of the pipeline:
// PCM at the output rate in, the same number of samples out, none above the ceiling and the inter-sample
// peaks of a 4x reconstruction held under it too; one-shot, batched (a ceiling per signal) and over exact
// stream windows. No reference counterpart: the reference peak-normalises a finished WAV.
//
// The arithmetic contract is in include/rwkvtts.h: three 12-tap fractional-delay FIRs as
// sequential f32 sums, the required gain r = c / p by one correctly rounded divide where the estimate p
// passes the ceiling c, the minimum of r over 65 samples, the sum of 65 minima in ascending order and one
// correctly rounded divide by 65, a multiply and a clamp. The kernel is pinned bitwise to a numpy
// restatement of exactly that (tests/test_gpu_limit.py).
//
// Work: k_limit gives a workgroup of 256 lanes a piece of 1024 consecutive outputs of one window. The
// piece's samples with the stage's whole reach (69 before, 70 after: 1163 floats) go to LDS once. Then,
// all in LDS and nowhere else: r over the piece +-64 (1152 values, a lane runs the three 12-step chains of
// the positions it owns at unit stride; the 36 taps arrive by scalar loads); if no r of the piece is below
// 1 the workgroup copies its samples out and is done -- the common case, at the cost of the estimate
// alone. Otherwise the minimum runs in two levels of radix 8: t[n] = min r[n .. n + 7] (7 compares), then
// m[n] = min(t[n - 32], t[n - 24], .., t[n + 24], t[n + 25]) (8 compares; the last two spans overlap by
// seven, which a minimum does not see), 15 compares for 65 values, and m overwrites r, which nothing reads
// again. A lane then owns four consecutive outputs: it reads the 68 minima they share as 17 128-bit LDS
// loads and adds each output's 65 in ascending order out of registers -- the order is the contract's, so
// no running sum -- divides, multiplies, clamps, and parks the four results in t's array, from where the
// workgroup stores them at unit stride. Three arrays, 13.9 KB. Signal and window ends are the padding rule
// (x = 0, r = 1), not other kernels. No matrix instruction: there is no GEMM here.
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

constexpr int kLimTaps = 12, kLimPhases = 3, kLimTable = kLimTaps * kLimPhases;
constexpr int kLimHalf = 32;                  // the minimum and the box reach 32 either side
constexpr int kLimWin = 2 * kLimHalf + 1;     // 65
constexpr int kLimBack = 5, kLimAhead = 6;    // the estimate reads x[n - 5 .. n + 6]
constexpr int kLimPiece = 1024, kLimLanes = 256;
constexpr int kLimRs = kLimPiece + 4 * kLimHalf;            // r over [a0 - 64, a0 + 1088)
constexpr int kLimMs = kLimPiece + 2 * kLimHalf;            // m over [a0 - 32, a0 + 1056)
constexpr int kLimXs = kLimRs + kLimBack + kLimAhead;       // x over [a0 - 69, a0 + 1094)
constexpr int kLimPre = 2 * kLimHalf + kLimBack;            // 69 samples before an output
constexpr int kLimPost = 2 * kLimHalf + kLimAhead;          // 70 after it
constexpr int64_t kLimMaxSamples = (int64_t)1 << 40;
static_assert(kLimTable == RWKVTTS_LIMIT_TABLE_LEN, "table length");
static_assert(kLimPiece == 4 * kLimLanes && kLimWin == 8 * 8 + 1, "the kernel's split of the work");

// One window: its given samples are signal indices [in_first, in_end), stored at x[in_off ...]; every
// other index reads as zero (the host has checked that those are below 0, past the end of a final window,
// or out of every wanted output's reach). r = 1 below 0 and from in_end on.
struct LimWin {
  int64_t in_off, in_first, in_end;
  float c, pad;
};

// One workgroup: outputs [a0, a0 + count) of window `win`, count <= 1024, the first at y[out_off].
struct LimPiece {
  int64_t a0, out_off;
  int32_t count, win;
};

// Correctly rounded f32 divide through double (53 >= 2 * 24 + 2 bits), as level.hip's.
__device__ inline float lim_div(float a, float b) { return (float)((double)a / (double)b); }

// grid (pieces), 256 lanes each. LDS: xs = x[a0 - 69, a0 + 1094), rs = r[a0 - 64, a0 + 1088) and later
// m[a0 - 32, a0 + 1056), ts = t[a0 - 64, a0 + 1081) and later y[a0, a0 + 1024).
__global__ __launch_bounds__(kLimLanes) void k_limit(const float* __restrict__ x, const float* __restrict__ tab,
                                                     const LimWin* __restrict__ wins,
                                                     const LimPiece* __restrict__ pieces, float* __restrict__ y) {
  __shared__ float xs[kLimXs];
  __shared__ __attribute__((aligned(16))) float rs[kLimRs];
  __shared__ float ts[kLimRs];
  const LimPiece p = pieces[blockIdx.x];
  const LimWin w = wins[p.win];
  const int t = threadIdx.x;
  const float c = w.c;
  for (int i = t; i < kLimXs; i += kLimLanes) {
    const int64_t idx = p.a0 - kLimPre + i;
    xs[i] = (idx >= w.in_first && idx < w.in_end) ? x[w.in_off + (idx - w.in_first)] : 0.0f;
  }
  __syncthreads();
  // r[n]: v_q[n] = sum_k h_q[k] * x[n + k - 5], ascending k from +0, one rounded multiply and one rounded add
  int bound = 0;
  for (int i = t; i < kLimRs; i += kLimLanes) {
    const int64_t n = p.a0 - 2 * kLimHalf + i;
    const float* s = xs + i;  // x[n - 5]
    float pk = fabsf(s[kLimBack]);
#pragma unroll
    for (int q = 0; q < kLimPhases; ++q) {
      float acc = 0.0f;
#pragma unroll
      for (int k = 0; k < kLimTaps; ++k) acc = __fadd_rn(acc, __fmul_rn(tab[q * kLimTaps + k], s[k]));
      pk = fmaxf(pk, fabsf(acc));
    }
    const float r = (n >= 0 && n < w.in_end && pk > c) ? lim_div(c, pk) : 1.0f;
    bound |= r != 1.0f;
    rs[i] = r;
  }
  if (!__syncthreads_or(bound)) {  // (uniform) nothing within reach passes the ceiling: g = 1, y = x bit for bit
    for (int i = t; i < p.count; i += kLimLanes) y[p.out_off + i] = xs[kLimPre + i];
    return;
  }
  // t[n] = min r[n .. n + 7], over the n that m reads
  for (int i = t; i < kLimRs - 7; i += kLimLanes) {
    float v = rs[i];
#pragma unroll
    for (int k = 1; k < 8; ++k) v = fminf(v, rs[i + k]);
    ts[i] = v;
  }
  __syncthreads();
  // m[n] = min r[n - 32 .. n + 32] = min(t[n - 32 + 8 k], k = 0 .. 7, t[n + 25]); m index i is t index i + 32
  for (int i = t; i < kLimMs; i += kLimLanes) {
    float v = ts[i + 2 * kLimHalf - 7];
#pragma unroll
    for (int k = 0; k < 8; ++k) v = fminf(v, ts[i + 8 * k]);
    rs[i] = v;
  }
  __syncthreads();
  // g[n] = (sum_{j = -32 .. 32} m[n + j]) / 65 for the lane's four outputs, from the 68 minima they share
  float mv[kLimWin + 3];
  const float4* m4 = reinterpret_cast<const float4*>(rs) + t;
#pragma unroll
  for (int k = 0; k < (kLimWin + 3) / 4; ++k) {
    const float4 v = m4[k];
    mv[4 * k] = v.x, mv[4 * k + 1] = v.y, mv[4 * k + 2] = v.z, mv[4 * k + 3] = v.w;
  }
#pragma unroll
  for (int o = 0; o < 4; ++o) {
    float acc = 0.0f;
#pragma unroll
    for (int j = 0; j < kLimWin; ++j) acc = __fadd_rn(acc, mv[o + j]);
    const float g = lim_div(acc, (float)kLimWin);
    ts[4 * t + o] = fminf(fmaxf(__fmul_rn(xs[kLimPre + 4 * t + o], g), -c), c);
  }
  __syncthreads();
  for (int i = t; i < p.count; i += kLimLanes) y[p.out_off + i] = ts[i];
}

// ---- host: configuration, table, plan --------------------------------------------------------
static int lim_config(const rwkvtts_limit_desc* d, const char* who) {
  RT_CHECK(d && d->struct_size >= sizeof(rwkvtts_limit_desc), RWKVTTS_EINVAL,
           std::string(who) + ": null desc or struct_size too small");
  RT_CHECK(d->reserved == 0, RWKVTTS_EINVAL, std::string(who) + ": reserved must be 0");
  return RWKVTTS_OK;
}

static int lim_ceiling_ok(float c, const char* who) {
  RT_CHECK(c > 0.0f && c <= 1.0f, RWKVTTS_EINVAL, std::string(who) + ": a ceiling must be in (0, 1]");  // (NaN fails)
  return RWKVTTS_OK;
}

static void lim_make_table(float* out) {
  const double pi = 3.141592653589793;
  for (int q = 1; q <= kLimPhases; ++q) {
    double h[kLimTaps], s = 0.0;
    for (int k = 0; k < kLimTaps; ++k) {
      const double t = (double)(k - kLimBack) - (double)q / 4.0;
      h[k] = sin(pi * t) / (pi * t) * (0.5 + 0.5 * cos(pi * t / 6.0));
      s = s + h[k];
    }
    for (int k = 0; k < kLimTaps; ++k) out[(q - 1) * kLimTaps + k] = (float)(h[k] / s);
  }
}

static inline int64_t lim_ready_end(int64_t n_known, int final) {
  return final ? n_known : std::max<int64_t>(0, n_known - kLimPost);
}
static inline int64_t lim_in_first_needed(int64_t out_first) { return std::max<int64_t>(0, out_first - kLimPre); }

struct LimWindow {
  const float* in;
  int64_t in_first, n_in;
  int final;
  float c;
  int64_t out_first, out_count;
  float* out;
};

}  // namespace rwkvtts

using namespace rwkvtts;

struct rwkvtts_limit : Stage<LimPiece> {  // d_table: h_1[12], h_2[12], h_3[12]
  DevBuf<LimWin> d_wins;
  std::vector<LimWin> wins;
};

// Checks every window against the plan, then runs them all in one launch. Nothing is launched and
// nothing written unless every window passes.
static int lim_run(rwkvtts_limit* v, const std::vector<LimWindow>& ws, const char* who) {
  int64_t tot_in = 0, tot_out = 0;
  size_t n_wins = 0;
  int rc;
  for (const LimWindow& w : ws) {
    if ((rc = lim_ceiling_ok(w.c, who))) return rc;
    RT_CHECK(w.in_first >= 0 && w.n_in >= 0 && w.out_first >= 0 && w.out_count >= 0 &&
                 w.in_first + w.n_in <= kLimMaxSamples && w.out_first <= kLimMaxSamples &&
                 w.out_count <= kLimMaxSamples && (w.in || w.n_in == 0) && (w.out || w.out_count == 0),
             RWKVTTS_EINVAL, std::string(who) + ": bad window (negative size, null buffer or too long)");
    if (w.out_count == 0) continue;
    RT_CHECK(w.out_first + w.out_count <= lim_ready_end(w.in_first + w.n_in, w.final), RWKVTTS_EINVAL,
             std::string(who) + ": a requested output needs a sample past the given samples");
    RT_CHECK(w.in_first <= lim_in_first_needed(w.out_first), RWKVTTS_EINVAL,
             std::string(who) + ": a requested output reads before the given samples");
    tot_in += w.n_in;
    tot_out += w.out_count;
    ++n_wins;
  }
  if (n_wins == 0) return RWKVTTS_OK;
  RT_CHECK(n_wins <= (size_t)0x7fffffff, RWKVTTS_EINVAL, std::string(who) + ": too many windows for one launch");
  std::lock_guard<std::mutex> lock(v->mu);
  v->desc.clear();
  v->wins.clear();
  int64_t in_off = 0, out_off = 0;
  for (const LimWindow& w : ws) {
    if (w.out_count == 0) continue;
    LimWin j;
    j.in_off = in_off;
    j.in_first = w.in_first;
    j.in_end = w.in_first + w.n_in;
    j.c = w.c;
    j.pad = 0.0f;
    for (int64_t o = 0; o < w.out_count; o += kLimPiece) {
      LimPiece p;
      p.a0 = w.out_first + o;
      p.out_off = out_off + o;
      p.count = (int32_t)std::min<int64_t>(kLimPiece, w.out_count - o);
      p.win = (int32_t)v->wins.size();
      v->desc.push_back(p);
    }
    v->wins.push_back(j);
    in_off += w.n_in;
    out_off += w.out_count;
  }
  RT_CHECK(v->desc.size() <= (size_t)0x7fffffff, RWKVTTS_EINVAL, std::string(who) + ": too many outputs for one launch");
  if ((rc = stage_reserve(v, tot_in, tot_out)) || (rc = v->d_wins.reserve(n_wins)) || (rc = stage_upload(v, ws)))
    return rc;
  RT_HIP(hipMemcpyAsync(v->d_wins.p, v->wins.data(), n_wins * sizeof(LimWin), hipMemcpyHostToDevice, v->stream));
  hipExtLaunchKernelGGL(k_limit, dim3((unsigned)v->desc.size()), dim3(kLimLanes), 0, v->stream, v->ev0, v->ev1, 0u,
                        v->d_in.p, v->d_table, v->d_wins.p, v->d_desc.p, v->d_out.p);
  RT_HIP(hipGetLastError());
  return stage_download(v, ws);
}

extern "C" int rwkvtts_limit_table(const rwkvtts_limit_desc* desc, float* out) {
  int rc = lim_config(desc, "limit_table");
  if (rc) return rc;
  RT_CHECK(out, RWKVTTS_EINVAL, "limit_table: null output");
  lim_make_table(out);
  return RWKVTTS_OK;
}

extern "C" int rwkvtts_limit_ceiling(double limit_db, float* c) {
  RT_CHECK(c && limit_db >= -12.0 && limit_db <= 0.0, RWKVTTS_EINVAL,
           "limit_ceiling: null output or limit outside -12 .. 0 dB");  // (NaN fails)
  *c = (float)pow(10.0, limit_db / 20.0);
  return RWKVTTS_OK;
}

extern "C" int rwkvtts_limit_plan(int64_t n_known, int final, int64_t out_first, int64_t* out_ready_end,
                                  int64_t* in_first_needed) {
  RT_CHECK(n_known >= 0 && n_known <= kLimMaxSamples && out_first >= 0 && out_first <= kLimMaxSamples, RWKVTTS_EINVAL,
           "limit_plan: n_known / out_first out of range");
  if (out_ready_end) *out_ready_end = lim_ready_end(n_known, final);
  if (in_first_needed) *in_first_needed = lim_in_first_needed(out_first);
  return RWKVTTS_OK;
}

extern "C" int rwkvtts_limit_create(int device, const rwkvtts_limit_desc* desc, const float* table,
                                    rwkvtts_limit** out) {
  RT_CHECK(out, RWKVTTS_EINVAL, "limit_create: null output");
  *out = nullptr;
  int rc = lim_config(desc, "limit_create");
  if (rc) return rc;
  rwkvtts_limit* v = nullptr;
  rc = stage_create("limit_create", device, table, (size_t)kLimTable, [&](float* t) { lim_make_table(t); }, &v);
  if (rc) return rc;
  *out = v;
  return RWKVTTS_OK;
}

extern "C" int rwkvtts_limit_destroy(rwkvtts_limit* v) {
  if (!v) return RWKVTTS_OK;
  (void)hipSetDevice(v->device);
  stage_free(v, {v->d_wins.p});
  return RWKVTTS_OK;
}

extern "C" int rwkvtts_limit_batch(rwkvtts_limit* v, const float* const* in, const int64_t* n_in, const float* c, int n,
                                   float* const* out) {
  RT_CHECK(v && n >= 0 && (n == 0 || (in && n_in && c && out)), RWKVTTS_EINVAL, "limit_batch: bad arguments");
  return guard_alloc("limit_batch", [&] {
    std::vector<LimWindow> ws((size_t)n);
    for (int i = 0; i < n; ++i) {
      RT_CHECK(n_in[i] >= 0 && n_in[i] <= kLimMaxSamples, RWKVTTS_EINVAL, "limit_batch: n_in out of range");
      ws[(size_t)i] = LimWindow{in[i], 0, n_in[i], 1, c[i], 0, n_in[i], out[i]};
    }
    return lim_run(v, ws, "limit_batch");
  });
}

extern "C" int rwkvtts_limit_windows(rwkvtts_limit* v, const rwkvtts_limit_window* w, int n) {
  RT_CHECK(v && n >= 0 && (n == 0 || w), RWKVTTS_EINVAL, "limit_windows: bad arguments");
  if (n == 0) return RWKVTTS_OK;
  return guard_alloc("limit_windows", [&] {
    std::vector<LimWindow> ws;
    int rc = read_windows("limit_windows", w, n, ws, [](const rwkvtts_limit_window* wi) {
      return LimWindow{wi->in, wi->in_first, wi->n_in, wi->final ? 1 : 0, wi->c, wi->out_first, wi->out_count, wi->out};
    });
    return rc ? rc : lim_run(v, ws, "limit_windows");
  });
}

extern "C" int rwkvtts_limit_kernel_ms(rwkvtts_limit* v, double* ms) { return stage_kernel_ms("limit_kernel_ms", v, ms); }
