// pitch.hip -- a formant-preserving pitch shift (period estimation and pitch-synchronous overlap-add)
// on the MI355X, for the `pitch_shift` keyword of the pipeline: one-shot, batched (a factor per
// signal) and over exact stream windows. No reference counterpart: the reference's only pitch control
// is the `pitch` property token, which a cloned voice does not get.
//
// The arithmetic contract is in include/rwkvtts.h: per frame and lag two sequential
// f32 sums over Wc samples, the period as the lowest lag that passes four comparisons, two integer
// walks over the periods, grains summed in ascending order and one correctly rounded divide. The
// kernels are pinned bitwise to a numpy restatement of exactly that (tests/test_gpu_pitch.py).
//
// Work: k_pitch_period gives a workgroup to a frame: the frame's Wc + Lmax + 1 samples in LDS, a lane
// owns a lag and runs its two chains (x[i] is a broadcast read, x[i + lag] a read of consecutive
// words), the lags' sums go back to LDS and the lowest qualifying lag is an integer minimum.
// k_pitch_marks gives one wave to a job: the periods pass through LDS in chunks, lane 0 runs both
// walks, then every lane pairs synthesis marks with their nearest analysis marks. k_pitch_synth gives
// a lane to every output sample: a binary search for the first grain that can reach it, then the sum.
// All three go to one stream; kernel order is the only hand-off.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <new>
#include <vector>

#include "common.h"
#include "pitch_plan.h"
#include "stage.h"

namespace rwkvtts {

constexpr int kPitchThreads = 320;  // five waves: the 291 lags of the default range in one pass
constexpr int kPitchWaves = kPitchThreads / 64;
constexpr int kPitchChunk = 4096;  // periods in LDS at a time in the walk
constexpr int kPitchNone = 0x7fffffff;

// One grid row of each kernel: outputs [out_first, out_first + out_count) of one signal. The given
// samples are signal indices [in_first, in_end), stored at x[in_off ...]; every other index reads as
// zero (the host has checked that those are below 0 or past the end of a final window). Frames
// [j0, j0 + nf) are measured, frame j at per[per_off + j - j0]. The walks start at a_prev and s_prev;
// analysis marks go to am[am_off ...] (at most am_cap), grains to gr[sm_off ...] (at most sm_cap).
struct PitchJob {
  int64_t in_off, out_off, per_off, am_off, sm_off;
  int32_t in_first, in_end, out_first, out_count;
  int32_t j0, nf, a_prev, s_prev, am_cap, sm_cap;
  double factor;
};

struct PitchGrain {  // synthesis mark, its analysis mark and that mark's period
  int32_t s, a, p, pad;
};

struct PitchState {
  int32_t ns, a_last, s_last, pad;
};

__device__ inline float pitch_x(const float* __restrict__ x, const PitchJob& j, int64_t idx) {
  return (idx >= j.in_first && idx < j.in_end) ? x[j.in_off + (idx - j.in_first)] : 0.0f;
}

// one step of a lag's two chains
#define PITCH_STEP(a, b)                                           \
  {                                                                \
    const float t_ = __fsub_rn(a, b);                              \
    d = __fadd_rn(d, __fmul_rn(t_, t_));                           \
    m = __fadd_rn(m, __fadd_rn(__fmul_rn(a, a), __fmul_rn(b, b))); \
  }

// grid (frames of the longest job, jobs). LDS: xs[Wc + Lmax + 1] = x[c, c + Wc + Lmax], then dd and mm
// of the Lmax - Lmin + 3 lags Lmin - 1 .. Lmax + 1.
__global__ __launch_bounds__(kPitchThreads) void k_pitch_period(const float* __restrict__ x,
                                                                const PitchJob* __restrict__ jobs,
                                                                int32_t* __restrict__ per, PitchCfg c) {
  extern __shared__ float s_mem[];
  __shared__ int s_key[kPitchWaves];
  const PitchJob j = jobs[blockIdx.y];
  if ((int)blockIdx.x >= j.nf) return;  // (uniform over the workgroup)
  const int tid = threadIdx.x;
  const int nx = c.Wc + c.Lmax + 1, nl = c.Lmax - c.Lmin + 3;
  float* xs = s_mem;
  float* dd = xs + nx;
  float* mm = dd + nl;
  const int64_t base = (int64_t)(j.j0 + (int)blockIdx.x) * c.Ha;
  for (int i = tid; i < nx; i += kPitchThreads) xs[i] = pitch_x(x, j, base + i);
  __syncthreads();
  for (int l = tid; l < nl; l += kPitchThreads) {
    const float* pb = xs + (c.Lmin - 1 + l);
    float d = 0.0f, m = 0.0f;
    int i = 0;
    // the LDS reads of eight steps are issued together ahead of the dependent adds
    for (; i + 8 <= c.Wc; i += 8) {
      float av[8], bv[8];
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        av[t] = xs[i + t];
        bv[t] = pb[i + t];
      }
#pragma unroll
      for (int t = 0; t < 8; ++t) PITCH_STEP(av[t], bv[t]);
    }
    for (; i < c.Wc; ++i) PITCH_STEP(xs[i], pb[i]);
    dd[l] = d;
    mm[l] = m;
  }
  __syncthreads();
  int key = kPitchNone;  // the lowest qualifying lag: a minimum of integers has no order
  for (int l = 1 + tid; l < nl - 1; l += kPitchThreads) {
    const float d = dd[l], m = mm[l];
    if (d <= dd[l - 1] && d <= dd[l + 1] && d <= __fmul_rn(c.theta, m) && m > c.floor) key = min(key, c.Lmin - 1 + l);
  }
  for (int off = 32; off >= 1; off >>= 1) key = min(key, __shfl_xor(key, off, 64));
  if ((tid & 63) == 0) s_key[tid >> 6] = key;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kPitchWaves; ++w) key = min(key, s_key[w]);
    per[j.per_off + blockIdx.x] = key == kPitchNone ? 0 : key;
  }
}

// grid (jobs), one wave each.
__global__ __launch_bounds__(64) void k_pitch_marks(const PitchJob* __restrict__ jobs, const int32_t* __restrict__ per,
                                                    int32_t* __restrict__ am, PitchGrain* __restrict__ gr,
                                                    PitchState* __restrict__ state, PitchCfg c) {
  __shared__ int32_t s_per[kPitchChunk];
  __shared__ int s_cnt[2];
  const PitchJob j = jobs[blockIdx.x];
  const int lane = threadIdx.x;
  const int end = j.out_first + j.out_count;
  const int lim = end + c.Lmax;  // both walks stop at their first mark at or past it
  const int s_keep = max(0, end - c.Lmax);
  int a = j.a_prev, s = j.s_prev, na = 1, ns = 1, s_last = j.s_prev;
  if (lane == 0) {
    am[j.am_off] = a;
    gr[j.sm_off].s = s;
  }
  for (int c0 = 0; c0 < j.nf; c0 += kPitchChunk) {  // (uniform)
    const int cn = min(kPitchChunk, j.nf - c0);
    __syncthreads();
    for (int i = lane; i < cn; i += 64) s_per[i] = per[j.per_off + c0 + i];
    __syncthreads();
    if (lane == 0) {
      const int f0 = j.j0 + c0;
      const int64_t t_end = (int64_t)(f0 + cn) * c.Ha;  // the first sample past the chunk's frames
      while (a < lim && a < t_end && na < j.am_cap) {
        const int p = s_per[a / c.Ha - f0];
        a += p ? p : c.P0;
        am[j.am_off + na++] = a;
      }
      while (s < lim && s < t_end && ns < j.sm_cap) {
        const int p = s_per[s / c.Ha - f0];
        int step = c.P0;
        if (p) {
          step = (int)floor((double)p / j.factor + 0.5);
          if (step < 1) step = 1;
        }
        s += step;
        if (s <= s_keep) s_last = s;
        gr[j.sm_off + ns++].s = s;
      }
    }
  }
  if (lane == 0) {
    // (the host sizes nf so that every mark below lim has its frame; a mark past the frames is unvoiced)
    while (a < lim && na < j.am_cap) {
      a += c.P0;
      am[j.am_off + na++] = a;
    }
    while (s < lim && ns < j.sm_cap) {
      s += c.P0;
      if (s <= s_keep) s_last = s;
      gr[j.sm_off + ns++].s = s;
    }
    s_cnt[0] = na;
    s_cnt[1] = ns;
  }
  __threadfence();
  __syncthreads();
  na = s_cnt[0];
  ns = s_cnt[1];
  const int32_t* A = am + j.am_off;
  for (int q = lane; q < ns; q += 64) {
    const int sq = gr[j.sm_off + q].s;
    int lo = 0, hi = na;  // the first analysis mark at or past sq
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (A[mid] >= sq) hi = mid; else lo = mid + 1;
    }
    int k = lo;
    if (k == na) k = na - 1;
    else if (k > 0 && sq - A[k - 1] <= A[k] - sq) k = k - 1;  // the lower mark wins a tie
    const int ak = A[k];
    const int f = ak / c.Ha - j.j0;
    const int p = f < j.nf ? per[j.per_off + f] : 0;
    gr[j.sm_off + q] = PitchGrain{sq, ak, p ? p : c.P0, 0};
  }
  if (lane == 0) {
    const int a_keep = max(0, s_last - c.Lmax);
    int lo = 0, hi = na;  // the first analysis mark past a_keep; A[0] = a_prev is not past it
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (A[mid] > a_keep) hi = mid; else lo = mid + 1;
    }
    state[blockIdx.x] = PitchState{ns, A[lo > 0 ? lo - 1 : 0], s_last, 0};
  }
}

// Correctly rounded f32 divide through double (53 >= 2 * 24 + 2 bits; the device's double divide is
// correctly rounded).
__device__ inline float pitch_div(float a, float b) { return (float)((double)a / (double)b); }

// grid (320-sample pieces of the longest job, jobs): a lane per output sample.
__global__ __launch_bounds__(kPitchThreads) void k_pitch_synth(const float* __restrict__ x,
                                                               const float* __restrict__ tab,
                                                               const PitchJob* __restrict__ jobs,
                                                               const PitchGrain* __restrict__ gr,
                                                               const PitchState* __restrict__ state,
                                                               float* __restrict__ y, PitchCfg c) {
  const PitchJob j = jobs[blockIdx.y];
  const int i = blockIdx.x * kPitchThreads + threadIdx.x;
  if (i >= j.out_count) return;
  const int o = j.out_first + i;
  const int ns = state[blockIdx.y].ns;
  const PitchGrain* G = gr + j.sm_off;
  int lo = 0, hi = ns;  // the first synthesis mark whose grain can reach o: s + Lmax > o
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (G[mid].s > o - c.Lmax) hi = mid; else lo = mid + 1;
  }
  float num = 0.0f, den = 0.0f;
  for (int q = lo; q < ns; ++q) {
    const PitchGrain g = G[q];
    if (g.s - c.Lmax > o) break;  // no later grain starts at or before o
    const int r = o - (g.s - g.p);
    if (r >= 0 && r < 2 * g.p) {
      const float w = tab[(g.p - c.Lmin) * (g.p + c.Lmin - 1) + r];  // (pitch_row_offset)
      num = __fadd_rn(num, __fmul_rn(w, pitch_x(x, j, (int64_t)g.a - g.p + r)));
      den = __fadd_rn(den, w);
    }
  }
  y[j.out_off + i] = den == 0.0f ? 0.0f : pitch_div(num, den);
}

// ---- host: the configuration, the table and the plan are pitch_plan.h's ------------------------
static int pitch_config(const rwkvtts_pitch_desc* d, PitchCfg* c, const char* who) {
  const char* bad = pitch_config_of(d, c);
  RT_CHECK(!bad, RWKVTTS_EINVAL, std::string(who) + ": " + bad);
  return RWKVTTS_OK;
}

struct PitchWin {
  const float* in;
  int64_t in_first, n_in;
  int final;
  double factor;
  int64_t out_first, a_prev, s_prev, out_count;
  float* out;
  int64_t* a_last;
  int64_t* s_last;
};

}  // namespace rwkvtts

using namespace rwkvtts;

struct rwkvtts_pitch : Stage<PitchJob> {  // d_table: the rows Lmin .. Lmax
  PitchCfg cfg;
  DevBuf<int32_t> d_per, d_am;
  DevBuf<PitchGrain> d_gr;
  DevBuf<PitchState> d_state;
  std::vector<PitchState> last;
  hipEvent_t ev2 = nullptr, ev3 = nullptr;  // bracket the marks kernel
  double walk_ms = 0.0;
};

// Checks every window against the plan, then runs them all: one launch each of period, marks and
// synth. Nothing is launched and nothing written unless every window passes.
static int pitch_run(rwkvtts_pitch* v, const std::vector<PitchWin>& ws, const char* who) {
  const PitchCfg& c = v->cfg;
  int64_t tot_in = 0, tot_out = 0, tot_per = 0, tot_am = 0, tot_sm = 0, max_nf = 0, max_out = 0;
  size_t n_jobs = 0;
  int rc;
  for (const PitchWin& w : ws) {
    const char* bad = pitch_window_check(c, w.in_first, w.n_in, w.final, w.factor, w.out_first, w.a_prev, w.s_prev,
                                         w.out_count, w.in != nullptr, w.out != nullptr);
    RT_CHECK(!bad, RWKVTTS_EINVAL, std::string(who) + ": " + bad);
    if (w.out_count == 0) continue;
    const PitchGeom g = pitch_geometry(c, w.out_first, w.out_count, w.a_prev, w.s_prev);
    tot_in += w.n_in;
    tot_out += w.out_count;
    tot_per += g.nf;
    tot_am += g.am_cap;
    tot_sm += g.sm_cap;
    max_nf = std::max(max_nf, g.nf);
    max_out = std::max(max_out, w.out_count);
    ++n_jobs;
  }
  auto pass_state = [&](const PitchWin& w) {
    if (w.a_last) *w.a_last = w.a_prev;
    if (w.s_last) *w.s_last = w.s_prev;
  };
  if (n_jobs == 0) {
    for (const PitchWin& w : ws) pass_state(w);
    return RWKVTTS_OK;
  }
  RT_CHECK(n_jobs <= 65535, RWKVTTS_EINVAL, std::string(who) + ": too much for one launch");
  std::lock_guard<std::mutex> lock(v->mu);
  v->desc.clear();
  v->last.assign(n_jobs, PitchState{0, 0, 0, 0});
  int64_t in_off = 0, out_off = 0, per_off = 0, am_off = 0, sm_off = 0;
  for (const PitchWin& w : ws) {
    if (w.out_count == 0) continue;
    const PitchGeom g = pitch_geometry(c, w.out_first, w.out_count, w.a_prev, w.s_prev);
    PitchJob j;
    j.nf = (int32_t)g.nf;
    j.j0 = (int32_t)g.j0;
    j.in_off = in_off;
    j.out_off = out_off;
    j.per_off = per_off;
    j.am_off = am_off;
    j.sm_off = sm_off;
    j.in_first = (int32_t)w.in_first;
    j.in_end = (int32_t)(w.in_first + w.n_in);
    j.out_first = (int32_t)w.out_first;
    j.out_count = (int32_t)w.out_count;
    j.a_prev = (int32_t)w.a_prev;
    j.s_prev = (int32_t)w.s_prev;
    j.am_cap = (int32_t)g.am_cap;
    j.sm_cap = (int32_t)g.sm_cap;
    j.factor = w.factor;
    v->desc.push_back(j);
    in_off += w.n_in;
    out_off += w.out_count;
    per_off += j.nf;
    am_off += j.am_cap;
    sm_off += j.sm_cap;
  }
  if ((rc = stage_reserve(v, tot_in, tot_out)) || (rc = v->d_per.reserve((size_t)tot_per)) ||
      (rc = v->d_am.reserve((size_t)tot_am)) || (rc = v->d_gr.reserve((size_t)tot_sm)) ||
      (rc = v->d_state.reserve(n_jobs)) || (rc = stage_upload(v, ws)))
    return rc;
  // the event pair brackets all three kernels: start of the period kernel, end of the synthesis
  const size_t lds = (size_t)(c.Wc + c.Lmax + 1 + 2 * (c.Lmax - c.Lmin + 3)) * sizeof(float);  // 28.7 KB at the widest
  hipExtLaunchKernelGGL(k_pitch_period, dim3((unsigned)max_nf, (unsigned)n_jobs), dim3(kPitchThreads), lds, v->stream,
                        v->ev0, nullptr, 0u, v->d_in.p, v->d_desc.p, v->d_per.p, c);
  RT_HIP(hipGetLastError());
  hipExtLaunchKernelGGL(k_pitch_marks, dim3((unsigned)n_jobs), dim3(64), 0, v->stream, v->ev2, v->ev3, 0u, v->d_desc.p,
                        v->d_per.p, v->d_am.p, v->d_gr.p, v->d_state.p, c);
  RT_HIP(hipGetLastError());
  hipExtLaunchKernelGGL(k_pitch_synth, dim3((unsigned)((max_out + kPitchThreads - 1) / kPitchThreads), (unsigned)n_jobs),
                        dim3(kPitchThreads), 0, v->stream, nullptr, v->ev1, 0u, v->d_in.p, v->d_table, v->d_desc.p,
                        v->d_gr.p, v->d_state.p, v->d_out.p, c);
  RT_HIP(hipGetLastError());
  RT_HIP(hipMemcpyAsync(v->last.data(), v->d_state.p, n_jobs * sizeof(PitchState), hipMemcpyDeviceToHost, v->stream));
  if ((rc = stage_download(v, ws))) return rc;
  float ms = 0.0f;
  if (hipEventElapsedTime(&ms, v->ev2, v->ev3) == hipSuccess) v->walk_ms = (double)ms;
  size_t k = 0;
  for (const PitchWin& w : ws) {
    if (w.out_count == 0) {
      pass_state(w);
      continue;
    }
    const PitchState& s = v->last[k++];
    if (w.a_last) *w.a_last = s.a_last;
    if (w.s_last) *w.s_last = s.s_last;
  }
  return RWKVTTS_OK;
}

extern "C" int rwkvtts_pitch_table(const rwkvtts_pitch_desc* desc, float* out) {
  PitchCfg c;
  int rc = pitch_config(desc, &c, "pitch_table");
  if (rc) return rc;
  RT_CHECK(out, RWKVTTS_EINVAL, "pitch_table: null output");
  pitch_make_table(c, out);
  return RWKVTTS_OK;
}

extern "C" int rwkvtts_pitch_plan(const rwkvtts_pitch_desc* desc, int64_t n_known, int final, int64_t out_first,
                                  int64_t a_prev, int64_t s_prev, int64_t* out_ready_end, int64_t* in_first_needed) {
  PitchCfg c;
  int rc = pitch_config(desc, &c, "pitch_plan");
  if (rc) return rc;
  RT_CHECK(n_known >= 0 && n_known <= kPitchMaxSamples && out_first >= 0 && out_first <= kPitchMaxSamples,
           RWKVTTS_EINVAL, "pitch_plan: n_known / out_first out of range");
  RT_CHECK(pitch_state_ok(c, out_first, a_prev, s_prev), RWKVTTS_EINVAL,
           "pitch_plan: (a_prev, s_prev) is no state a walk can have left");
  if (out_ready_end) *out_ready_end = pitch_ready_end(c, n_known, final);
  if (in_first_needed) *in_first_needed = pitch_in_first_needed(c, a_prev);
  return RWKVTTS_OK;
}

extern "C" int rwkvtts_pitch_create(int device, const rwkvtts_pitch_desc* desc, const float* table,
                                    rwkvtts_pitch** out) {
  RT_CHECK(out, RWKVTTS_EINVAL, "pitch_create: null output");
  *out = nullptr;
  PitchCfg c;
  int rc = pitch_config(desc, &c, "pitch_create");
  if (rc) return rc;
  rwkvtts_pitch* v = nullptr;
  rc = stage_create("pitch_create", device, table, pitch_table_len(c), [&](float* t) { pitch_make_table(c, t); }, &v);
  if (rc) return rc;
  v->cfg = c;
  hipError_t e;
  if ((e = hipEventCreate(&v->ev2)) != hipSuccess || (e = hipEventCreate(&v->ev3)) != hipSuccess) {
    set_error(std::string("pitch_create: hipEventCreate: ") + hipGetErrorString(e));
    rwkvtts_pitch_destroy(v);
    return RWKVTTS_EHIP;
  }
  *out = v;
  return RWKVTTS_OK;
}

extern "C" int rwkvtts_pitch_destroy(rwkvtts_pitch* v) {
  if (!v) return RWKVTTS_OK;
  (void)hipSetDevice(v->device);
  if (v->ev2) (void)hipEventDestroy(v->ev2);
  if (v->ev3) (void)hipEventDestroy(v->ev3);
  stage_free(v, {v->d_per.p, v->d_am.p, v->d_gr.p, v->d_state.p});
  return RWKVTTS_OK;
}

extern "C" int rwkvtts_pitch_batch(rwkvtts_pitch* v, const float* const* in, const int64_t* n_in, const double* factor,
                                   int n, float* const* out) {
  RT_CHECK(v && n >= 0 && (n == 0 || (in && n_in && factor && out)), RWKVTTS_EINVAL, "pitch_batch: bad arguments");
  return guard_alloc("pitch_batch", [&] {
    std::vector<PitchWin> ws((size_t)n);
    for (int i = 0; i < n; ++i) {
      RT_CHECK(n_in[i] >= 0 && n_in[i] <= kPitchMaxSamples, RWKVTTS_EINVAL, "pitch_batch: n_in out of range");
      ws[(size_t)i] = PitchWin{in[i], 0, n_in[i], 1, factor[i], 0, 0, 0, n_in[i], out[i], nullptr, nullptr};
    }
    return pitch_run(v, ws, "pitch_batch");
  });
}

extern "C" int rwkvtts_pitch_windows(rwkvtts_pitch* v, rwkvtts_pitch_window* w, int n) {
  RT_CHECK(v && n >= 0 && (n == 0 || w), RWKVTTS_EINVAL, "pitch_windows: bad arguments");
  if (n == 0) return RWKVTTS_OK;
  return guard_alloc("pitch_windows", [&] {
    std::vector<PitchWin> ws;
    int rc = read_windows("pitch_windows", w, n, ws, [](rwkvtts_pitch_window* wi) {
      return PitchWin{wi->in, wi->in_first, wi->n_in, wi->final ? 1 : 0, wi->factor, wi->out_first, wi->a_prev,
                      wi->s_prev, wi->out_count, wi->out, &wi->a_last, &wi->s_last};
    });
    return rc ? rc : pitch_run(v, ws, "pitch_windows");
  });
}

extern "C" int rwkvtts_pitch_kernel_ms(rwkvtts_pitch* v, double* ms) { return stage_kernel_ms("pitch_kernel_ms", v, ms); }

extern "C" int rwkvtts_pitch_walk_ms(rwkvtts_pitch* v, double* ms) {
  RT_CHECK(v && ms, RWKVTTS_EINVAL, "pitch_walk_ms: null argument");
  std::lock_guard<std::mutex> lock(v->mu);
  *ms = v->walk_ms;
  return RWKVTTS_OK;
}
