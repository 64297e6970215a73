// resample.hip -- windowed-sinc resampling on the MI355X: rubato 0.15 SincFixedIn with linear
// interpolation between sinc tables, as src/ref_audio_utilities.rs:532-576 configures it (sinc_len
// 256, oversampling 256, f_cutoff 0.95, Blackman-Harris^2) and rwkvtts/audio.py restates it, for the
// reference-audio front end (rubato alignment) and for output rates other than 16 kHz (zero
// alignment), one-shot, batched and over exact stream windows.
//
// The arithmetic contract is in include/rwkvtts.h: positions in IEEE double (one operation per
// step, never fused), two sequential f32 sums per output in ascending tap order starting from +0
// (one rounded multiply, one rounded add per tap), three rounded f32 operations for the
// interpolation. The kernel is pinned bitwise to a numpy restatement of exactly that
// (tests/test_gpu_resample.py), not to rubato itself.
//
// Work: a lane owns one output sample and runs its two independent chains a (table p0) and b (table
// p0 + 1); a workgroup of 256 lanes owns a tile of up to 256 consecutive outputs of one signal and
// stages the tile's input span (about W * t_ratio + L samples, zeros outside the signal) in LDS
// once. The tables (256 KB at the defaults) stay in device memory and are read through L2 / L1 as
// 16-byte row pieces. The tile is narrowed at small ratios so that the span fits 32 KB of LDS.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <new>
#include <vector>

#include "common.h"
#include "stage.h"

// the position arithmetic below is shared by the host plan and the kernel: no contraction anywhere
#pragma clang fp contract(off)

namespace rwkvtts {

constexpr int kRsThreads = 256;     // lanes = outputs per tile at most
constexpr int kRsLdsFloats = 8192;  // input span of a tile: 32 KB, 5 workgroups per CU at the widest

struct RsCfg {
  int sr_in, sr_out, L, O, align;
  double cutoff;  // the table's: f_cutoff, times ratio when downsampling
  double ratio, t_ratio, delay;
};

struct RsPos {
  int64_t start;
  int p0;
  float w1;
};

// idx = o * t_ratio - delay; start = floor(idx); pos = (idx - start) * O; p0 = floor(pos);
// w1 = (float)(pos - p0): each step one correctly rounded double operation, on both sides.
__host__ __device__ inline RsPos rs_position(int64_t o, double t_ratio, double delay, int O) {
  RsPos p;
#ifdef __HIP_DEVICE_COMPILE__
  const double idx = __dsub_rn(__dmul_rn((double)o, t_ratio), delay);
  const double st = floor(idx);
  const double pos = __dmul_rn(__dsub_rn(idx, st), (double)O);
  const double p0 = floor(pos);
  p.w1 = (float)__dsub_rn(pos, p0);
#else
  const double prod = (double)o * t_ratio;
  const double idx = prod - delay;
  const double st = floor(idx);
  const double frac = idx - st;
  const double pos = frac * (double)O;
  const double p0 = floor(pos);
  p.w1 = (float)(pos - p0);
#endif
  p.start = (int64_t)st;
  p.p0 = (int)p0;
  return p;
}

// One tile: outputs [o0, o0 + count) of one window. The window's given samples are signal indices
// [in_first, in_end), stored at x[in_off ...]; every other index a tap names reads as zero (the host
// has checked that those are below 0 or, for a final window, past the end).
struct RsTile {
  int64_t in_off, in_first, in_end;
  int64_t o0, out_off;
  int32_t count, pad;
};

__global__ __launch_bounds__(kRsThreads) void k_resample(const float* __restrict__ x, const float* __restrict__ sincs,
                                                         const RsTile* __restrict__ tiles, float* __restrict__ y,
                                                         double t_ratio, double delay, int L, int O, int lds_floats) {
  extern __shared__ float s_x[];
  const RsTile t = tiles[blockIdx.x];
  const int half = L / 2;
  const int64_t lo = rs_position(t.o0, t_ratio, delay, O).start - half + 1;               // lowest tap of the tile
  const int64_t hi = rs_position(t.o0 + t.count - 1, t_ratio, delay, O).start + half;      // highest
  int64_t span = hi - lo + 1;
  if (span > lds_floats) span = lds_floats;  // (never: the host sizes the tile so that the span fits)
  for (int i = threadIdx.x; i < (int)span; i += kRsThreads) {
    const int64_t j = lo + i;
    s_x[i] = (j >= t.in_first && j < t.in_end) ? x[t.in_off + (j - t.in_first)] : 0.0f;
  }
  __syncthreads();
  if ((int)threadIdx.x >= t.count) return;
  const RsPos p = rs_position(t.o0 + threadIdx.x, t_ratio, delay, O);
  const float* xs = s_x + (int)(p.start - half + 1 - lo);
  const float4* s0 = (const float4*)(sincs + (size_t)(p.p0 % O) * L);
  const float4* s1 = (const float4*)(sincs + (size_t)((p.p0 + 1) % O) * L);
  float a = 0.0f, b = 0.0f;
  for (int k = 0; k < L; k += 8) {  // L is a multiple of 8: rows are 32-byte aligned
    const float4 c0 = s0[k / 4], c1 = s0[k / 4 + 1], d0 = s1[k / 4], d1 = s1[k / 4 + 1];
    const float x0 = xs[k], x1 = xs[k + 1], x2 = xs[k + 2], x3 = xs[k + 3];
    const float x4 = xs[k + 4], x5 = xs[k + 5], x6 = xs[k + 6], x7 = xs[k + 7];
    a = __fadd_rn(a, __fmul_rn(x0, c0.x)); b = __fadd_rn(b, __fmul_rn(x0, d0.x));
    a = __fadd_rn(a, __fmul_rn(x1, c0.y)); b = __fadd_rn(b, __fmul_rn(x1, d0.y));
    a = __fadd_rn(a, __fmul_rn(x2, c0.z)); b = __fadd_rn(b, __fmul_rn(x2, d0.z));
    a = __fadd_rn(a, __fmul_rn(x3, c0.w)); b = __fadd_rn(b, __fmul_rn(x3, d0.w));
    a = __fadd_rn(a, __fmul_rn(x4, c1.x)); b = __fadd_rn(b, __fmul_rn(x4, d1.x));
    a = __fadd_rn(a, __fmul_rn(x5, c1.y)); b = __fadd_rn(b, __fmul_rn(x5, d1.y));
    a = __fadd_rn(a, __fmul_rn(x6, c1.z)); b = __fadd_rn(b, __fmul_rn(x6, d1.z));
    a = __fadd_rn(a, __fmul_rn(x7, c1.w)); b = __fadd_rn(b, __fmul_rn(x7, d1.w));
  }
  y[t.out_off + threadIdx.x] = __fadd_rn(a, __fmul_rn(__fsub_rn(b, a), p.w1));
}

// ---- host: configuration, table, plan --------------------------------------------------------
static int rs_config(const rwkvtts_resample_desc* d, RsCfg* c, const char* who) {
  RT_CHECK(d && d->struct_size >= sizeof(rwkvtts_resample_desc), RWKVTTS_EINVAL,
           std::string(who) + ": null desc or struct_size too small");
  c->sr_in = d->sr_in;
  c->sr_out = d->sr_out;
  c->L = d->sinc_len ? d->sinc_len : 256;
  c->O = d->oversampling ? d->oversampling : 256;
  const double fc = d->f_cutoff != 0.0 ? d->f_cutoff : 0.95;
  c->align = d->align;
  RT_CHECK(c->sr_in >= 1 && c->sr_in <= 192000 && c->sr_out >= 1 && c->sr_out <= 192000, RWKVTTS_EINVAL,
           std::string(who) + ": sample rates must be 1 .. 192000");
  RT_CHECK(c->L >= 8 && c->L <= 1024 && c->L % 8 == 0, RWKVTTS_EINVAL,
           std::string(who) + ": sinc_len must be a multiple of 8, 8 .. 1024");
  RT_CHECK(c->O >= 1 && c->O <= 1024, RWKVTTS_EINVAL, std::string(who) + ": oversampling must be 1 .. 1024");
  RT_CHECK(fc > 0.0 && fc <= 1.0, RWKVTTS_EINVAL, std::string(who) + ": f_cutoff must be in (0, 1]");
  RT_CHECK(c->align == RWKVTTS_RESAMPLE_ALIGN_RUBATO || c->align == RWKVTTS_RESAMPLE_ALIGN_ZERO, RWKVTTS_EINVAL,
           std::string(who) + ": unknown align");
  c->ratio = (double)c->sr_out / (double)c->sr_in;
  c->t_ratio = 1.0 / c->ratio;
  c->cutoff = c->ratio >= 1.0 ? fc : fc * c->ratio;
  c->delay = c->align == RWKVTTS_RESAMPLE_ALIGN_RUBATO ? (double)(c->L / 2) : 0.0;
  return RWKVTTS_OK;
}

// rubato make_sincs in the order rwkvtts/audio.py::_make_sincs evaluates it; the normalising sum in
// double (numpy's is a pairwise f32 sum: the two tables differ by that sum's rounding alone).
static void rs_make_sincs(const RsCfg& c, float* out) {
  const int64_t tot = (int64_t)c.L * c.O;
  const double n = (double)tot, pi = 3.141592653589793;
  std::vector<float> y((size_t)tot);
  double sum = 0.0;
  for (int64_t i = 0; i < tot; ++i) {
    const double k = (double)i;
    const double w = 0.35875 - 0.48829 * cos(2.0 * pi * k / n) + 0.14128 * cos(4.0 * pi * k / n) -
                     0.01168 * cos(6.0 * pi * k / n);
    const float win = (float)(w * w);
    const double xv = (double)(i - tot / 2) * c.cutoff / (double)c.O;
    const double py = pi * (xv == 0.0 ? 1.0e-20 : xv);
    y[(size_t)i] = (float)((double)win * (sin(py) / py));
    sum += (double)y[(size_t)i];
  }
  const float s = (float)(sum / (double)c.O);
  for (int r = 0; r < c.O; ++r)
    for (int m = 0; m < c.L; ++m) out[(size_t)(c.O - r - 1) * c.L + m] = y[(size_t)r + (size_t)m * c.O] / s;
}

static inline int64_t rs_out_len(const RsCfg& c, int64_t n) { return (int64_t)ceil((double)n * c.ratio); }
static inline int64_t rs_start(const RsCfg& c, int64_t o) { return rs_position(o, c.t_ratio, c.delay, c.O).start; }

// The first output whose highest tap (start + L/2) is sample n_known or later, at most out_len(n_known):
// start is monotone in o (every step of rs_position is a monotone rounded operation), so bisect.
static int64_t rs_ready_end(const RsCfg& c, int64_t n_known, int final) {
  const int64_t cap = rs_out_len(c, n_known);
  if (final) return cap;
  int64_t lo = 0, hi = cap;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (rs_start(c, mid) + c.L / 2 >= n_known) hi = mid; else lo = mid + 1;
  }
  return lo;
}
static inline int64_t rs_in_first_needed(const RsCfg& c, int64_t out_first) {
  return std::max<int64_t>(0, rs_start(c, out_first) - c.L / 2 + 1);
}

constexpr int64_t kRsMaxSamples = (int64_t)1 << 40;  // positions stay far inside double's exact integers

struct RsWin {
  const float* in;
  int64_t in_first, n_in;
  int final;
  int64_t out_first, out_count;
  float* out;
};

}  // namespace rwkvtts

using namespace rwkvtts;

struct rwkvtts_resampler : Stage<RsTile> {  // d_table: the sinc tables
  RsCfg cfg;
  int tile = kRsThreads;   // outputs per tile
  int lds_floats = 0;      // the widest tile's input span
};

// Checks every window against the plan, then runs them all in one launch. Nothing is launched and
// nothing written unless every window passes.
static int rs_run(rwkvtts_resampler* r, const std::vector<RsWin>& ws, const char* who) {
  const RsCfg& c = r->cfg;
  int64_t tot_in = 0, tot_out = 0;
  for (const RsWin& w : ws) {
    RT_CHECK(w.in_first >= 0 && w.n_in >= 0 && w.out_first >= 0 && w.out_count >= 0 &&
                 w.in_first + w.n_in <= kRsMaxSamples && (w.in || w.n_in == 0) && (w.out || w.out_count == 0),
             RWKVTTS_EINVAL, std::string(who) + ": bad window (negative size, null buffer or too long)");
    if (w.out_count == 0) continue;
    RT_CHECK(w.out_first + w.out_count <= rs_ready_end(c, w.in_first + w.n_in, w.final), RWKVTTS_EINVAL,
             std::string(who) + ": a requested output reads past the given samples");
    RT_CHECK(w.in_first <= rs_in_first_needed(c, w.out_first), RWKVTTS_EINVAL,
             std::string(who) + ": a requested output reads before the given samples");
    tot_in += w.n_in;
    tot_out += w.out_count;
  }
  if (tot_out == 0) return RWKVTTS_OK;
  std::lock_guard<std::mutex> lock(r->mu);
  r->desc.clear();
  int64_t in_off = 0, out_off = 0;
  for (const RsWin& w : ws) {
    if (w.out_count == 0) continue;
    for (int64_t o = 0; o < w.out_count; o += r->tile) {
      RsTile t;
      t.in_off = in_off;
      t.in_first = w.in_first;
      t.in_end = w.in_first + w.n_in;
      t.o0 = w.out_first + o;
      t.out_off = out_off + o;
      t.count = (int32_t)std::min<int64_t>(r->tile, w.out_count - o);
      t.pad = 0;
      r->desc.push_back(t);
    }
    in_off += w.n_in;
    out_off += w.out_count;
  }
  RT_CHECK(r->desc.size() <= (size_t)0x7fffffff, RWKVTTS_EINVAL, std::string(who) + ": too many outputs for one launch");
  int rc;
  if ((rc = stage_reserve(r, tot_in, tot_out)) || (rc = stage_upload(r, ws))) return rc;
  hipExtLaunchKernelGGL(k_resample, dim3((unsigned)r->desc.size()), dim3(kRsThreads),
                        (size_t)r->lds_floats * sizeof(float), r->stream, r->ev0, r->ev1, 0u, r->d_in.p, r->d_table,
                        r->d_desc.p, r->d_out.p, c.t_ratio, c.delay, c.L, c.O, r->lds_floats);
  RT_HIP(hipGetLastError());
  return stage_download(r, ws);
}

extern "C" int rwkvtts_resample_sincs(const rwkvtts_resample_desc* desc, float* out) {
  RsCfg c;
  int rc = rs_config(desc, &c, "resample_sincs");
  if (rc) return rc;
  RT_CHECK(out, RWKVTTS_EINVAL, "resample_sincs: null output");
  return guard_alloc("resample_sincs", [&] {
    rs_make_sincs(c, out);
    return RWKVTTS_OK;
  });
}

extern "C" int64_t rwkvtts_resample_out_len(const rwkvtts_resample_desc* desc, int64_t n_in) {
  RsCfg c;
  if (rs_config(desc, &c, "resample_out_len")) return -1;
  if (n_in < 0 || n_in > kRsMaxSamples) {
    set_error("resample_out_len: n_in out of range");
    return -1;
  }
  return rs_out_len(c, n_in);
}

extern "C" int rwkvtts_resample_plan(const rwkvtts_resample_desc* desc, int64_t n_known, int final, int64_t out_first,
                                     int64_t* out_ready_end, int64_t* in_first_needed) {
  RsCfg c;
  int rc = rs_config(desc, &c, "resample_plan");
  if (rc) return rc;
  RT_CHECK(n_known >= 0 && n_known <= kRsMaxSamples && out_first >= 0 && out_first <= kRsMaxSamples, RWKVTTS_EINVAL,
           "resample_plan: n_known / out_first out of range");
  if (out_ready_end) *out_ready_end = rs_ready_end(c, n_known, final);
  if (in_first_needed) *in_first_needed = rs_in_first_needed(c, out_first);
  return RWKVTTS_OK;
}

extern "C" int rwkvtts_resampler_create(int device, const rwkvtts_resample_desc* desc, const float* table,
                                        rwkvtts_resampler** out) {
  RT_CHECK(out, RWKVTTS_EINVAL, "resampler_create: null output");
  *out = nullptr;
  RsCfg c;
  int rc = rs_config(desc, &c, "resampler_create");
  if (rc) return rc;
  rwkvtts_resampler* r = nullptr;
  rc = stage_create("resampler_create", device, table, (size_t)c.L * c.O, [&](float* t) { rs_make_sincs(c, t); }, &r);
  if (rc) return rc;
  r->cfg = c;
  // the widest tile whose input span, (W - 1) * t_ratio + L + 2 samples at most, fits the LDS budget
  const double room = (double)(kRsLdsFloats - c.L - 2) / c.t_ratio;
  r->tile = (int)std::max(1.0, std::min((double)kRsThreads, floor(room) + 1.0));
  r->lds_floats = (int)std::min<int64_t>(kRsLdsFloats, (int64_t)ceil((double)(r->tile - 1) * c.t_ratio) + c.L + 2);
  *out = r;
  return RWKVTTS_OK;
}

extern "C" int rwkvtts_resampler_destroy(rwkvtts_resampler* r) {
  if (!r) return RWKVTTS_OK;
  (void)hipSetDevice(r->device);
  stage_free(r);
  return RWKVTTS_OK;
}

extern "C" int rwkvtts_resample_batch(rwkvtts_resampler* r, const float* const* in, const int64_t* n_in, int n,
                                      float* const* out) {
  RT_CHECK(r && n >= 0 && (n == 0 || (in && n_in && out)), RWKVTTS_EINVAL, "resample_batch: bad arguments");
  return guard_alloc("resample_batch", [&] {
    std::vector<RsWin> ws((size_t)n);
    for (int i = 0; i < n; ++i) {
      RT_CHECK(n_in[i] >= 0 && n_in[i] <= kRsMaxSamples, RWKVTTS_EINVAL, "resample_batch: n_in out of range");
      ws[(size_t)i] = RsWin{in[i], 0, n_in[i], 1, 0, rs_out_len(r->cfg, n_in[i]), out[i]};
    }
    return rs_run(r, ws, "resample_batch");
  });
}

extern "C" int rwkvtts_resample_windows(rwkvtts_resampler* r, const rwkvtts_resample_window* w, int n) {
  RT_CHECK(r && n >= 0 && (n == 0 || w), RWKVTTS_EINVAL, "resample_windows: bad arguments");
  if (n == 0) return RWKVTTS_OK;
  return guard_alloc("resample_windows", [&] {
    std::vector<RsWin> ws;
    int rc = read_windows("resample_windows", w, n, ws, [](const rwkvtts_resample_window* wi) {
      return RsWin{wi->in, wi->in_first, wi->n_in, wi->final ? 1 : 0, wi->out_first, wi->out_count, wi->out};
    });
    return rc ? rc : rs_run(r, ws, "resample_windows");
  });
}

extern "C" int rwkvtts_resampler_kernel_ms(rwkvtts_resampler* r, double* ms) {
  return stage_kernel_ms("resampler_kernel_ms", r, ms);
}
