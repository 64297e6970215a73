// eq.hip -- an equaliser on the MI355X, for the `eq` keyword of the pipeline: 16 kHz PCM in, the same
// number of samples out, filtered by a FIR of 64 .. 4096 taps that the caller shapes as 1 .. 8 cookbook
// biquads (or names as a device profile); one-shot, batched (a tap set per signal) and over exact stream
// windows. No reference counterpart: the reference has no tone control.
//
// The arithmetic contract is in include/rwkvtts.h: the taps are the biquad cascade's
// impulse response in double, cut where its tail falls under 2^-24 of its sum and rounded to f32; an
// output is the sequential f32 sum of h[k] * x[n - k] in ascending k from +0, one rounded multiply and
// one rounded add per tap. The kernel is pinned bitwise to a numpy restatement of exactly that
// (tests/test_gpu_eq.py).
//
// Work: k_eq gives a workgroup of 256 lanes a piece of 2048 consecutive outputs of one window. The
// window's N taps and the piece's input span x[a0 - N + 1, a0 + 2048) go to LDS once, zeros where the
// signal has not begun. A lane owns 8 consecutive outputs as four pairs of accumulators, eight chains
// that do not wait for each other, and walks k upward in blocks of 8: two 128-bit LDS reads bring the 8
// samples that enter the 15-sample window the block's 64 products draw on, two more (one address for
// the whole wave, a broadcast) the block's 8 taps, and the window slides by the unrolled body's two
// halves trading names, not by moves. The lanes' reads are 32 bytes apart, so lanes t and t + 8 would meet in
// the same banks; four floats of padding after every 64 of the image move them half a stride apart
// (eq_pad). Products and sums are written on pairs of outputs (float2), which gfx950 runs as v_pk_mul_f32
// and v_pk_add_f32; the k order is each chain's own, so the result depends neither on where a piece is
// cut nor on how a batch is grouped. No matrix instruction, deliberately: an MFMA's internal order of
// summation would give up the bitwise contract. LDS: N + (2048 + N) * 17 / 16 floats, 9 KB at N = 64 and
// 41.5 KB at N = 4096 (three workgroups a CU).
#include <math.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <new>
#include <vector>

#include "common.h"
#include "stage.h"

// the kernel's sums and the design in double are step by step as the header states them: no contraction
#pragma clang fp contract(off)

namespace rwkvtts {

constexpr int kEqPiece = 2048, kEqLanes = 256, kEqPer = 8;  // outputs a workgroup, lanes, outputs a lane
constexpr int kEqStep = RWKVTTS_EQ_TAP_STEP, kEqMaxTaps = RWKVTTS_EQ_MAX_TAPS, kEqMaxBands = RWKVTTS_EQ_MAX_BANDS;
constexpr int kEqImpulse = 8192;  // samples of the cascade's impulse response the design looks at
constexpr double kEqFs = 16000.0;
constexpr int64_t kEqMaxSamples = (int64_t)1 << 40;
static_assert(kEqPiece == kEqPer * kEqLanes && kEqStep % (2 * kEqPer) == 0, "the kernel's split of the work");

// One window: its given samples are signal indices [in_first, in_end), stored at x[in_off ...]; every
// other index a wanted output reads is below 0 (the host has checked) and reads as zero. Its taps are
// taps[tap_off, tap_off + n_taps).
struct EqWin {
  int64_t in_off, in_first, in_end;
  int32_t tap_off, n_taps;
};

// One workgroup: outputs [a0, a0 + count) of window `win`, count <= 2048, the first at y[out_off].
struct EqPiece {
  int64_t a0, out_off;
  int32_t count, win;
};

typedef float eq_f2 __attribute__((ext_vector_type(2)));

// Where float i of the input image lies: four floats of padding after every 64, which keeps 16-byte
// alignment and puts the 128-bit reads of lanes t and t + 8 (256 bytes apart in the image) 16 bytes further apart.
__host__ __device__ inline int eq_pad(int i) { return i + ((i >> 6) << 2); }
static inline size_t eq_lds_bytes(int n_taps) { return (size_t)(n_taps + eq_pad(kEqPiece + n_taps)) * sizeof(float); }

__device__ inline void eq_read8(const float* p, float (&v)[8]) {
  const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
  v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
}

// Taps h[0 .. 7] of one block on the lane's 8 chains. With d0 the signal index of the lane's first output less
// the block's first tap index, lo holds x[d0 - 7 .. d0] and hi x[d0 + 1 .. d0 + 8]; output j at tap r reads
// x[d0 + j - r]. Each chain takes its taps in ascending r.
__device__ inline void eq_block(eq_f2 (&acc)[4], const float (&lo)[8], const float (&hi)[8], const float (&h)[8]) {
#pragma unroll
  for (int r = 0; r < 8; ++r)
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int e = 2 * p - r + 7;  // output 2 p reads element e of (lo, hi), output 2 p + 1 element e + 1
      eq_f2 xv;
      xv.x = e < 8 ? lo[e & 7] : hi[e & 7];
      xv.y = e + 1 < 8 ? lo[(e + 1) & 7] : hi[(e + 1) & 7];
      acc[p] = acc[p] + h[r] * xv;  // a rounded multiply, then a rounded add
    }
}

// grid (pieces), 256 lanes each. Dynamic LDS: hs = the window's taps [0, N), then xs = the image of
// x[a0 - N + 1, a0 + 2049) at eq_pad(i), i = 0 .. 2048 + N - 1; sized by the host for the call's largest N.
__global__ __launch_bounds__(kEqLanes) void k_eq(const float* __restrict__ x, const float* __restrict__ taps,
                                                 const EqWin* __restrict__ wins, const EqPiece* __restrict__ pieces,
                                                 float* __restrict__ y) {
  extern __shared__ float4 eq_lds[];
  const EqPiece p = pieces[blockIdx.x];
  const EqWin w = wins[p.win];
  const int t = threadIdx.x, N = w.n_taps;
  float* hs = reinterpret_cast<float*>(eq_lds);
  float* xs = hs + N;
  for (int i = t; i < N; i += kEqLanes) hs[i] = taps[w.tap_off + i];
  for (int i = t; i < kEqPiece + N; i += kEqLanes) {
    const int64_t idx = p.a0 - (N - 1) + i;
    xs[eq_pad(i)] = (idx >= w.in_first && idx < w.in_end) ? x[w.in_off + (idx - w.in_first)] : 0.0f;
  }
  __syncthreads();
  if (kEqPer * t >= p.count) return;  // (no barrier follows)
  // image group g = floats [8 g, 8 g + 8) = x[a0 - N + 1 + 8 g ...]; the lane's outputs start at a0 + 8 t, so
  // x[a0 + 8 t + 1 ...] is group t + N / 8 and block m of the taps brings group t + N / 8 - 1 - m >= t
  eq_f2 acc[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) acc[q] = eq_f2{0.0f, 0.0f};
  float wa[8], wb[8], h[8];
  int g = t + N / kEqPer;
  eq_read8(xs + eq_pad(kEqPer * g), wa);
  for (int k = 0; k < N; k += 2 * kEqPer) {
    eq_read8(xs + eq_pad(kEqPer * (g - 1)), wb);
    eq_read8(hs + k, h);
    eq_block(acc, wb, wa, h);
    g -= 2;
    eq_read8(xs + eq_pad(kEqPer * g), wa);
    eq_read8(hs + k + kEqPer, h);
    eq_block(acc, wa, wb, h);
  }
  float* out = y + p.out_off + kEqPer * t;
  const int left = p.count - kEqPer * t;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (2 * q < left) out[2 * q] = acc[q].x;
    if (2 * q + 1 < left) out[2 * q + 1] = acc[q].y;
  }
}

// ---- host: the design and the plan ------------------------------------------------------------
static const char* const kEqKinds[] = {"peak", "lowshelf", "highshelf", "highpass", "lowpass"};

// c = (b0, b1, b2, a1, a2) / a0 of one band, in the header's order of operations.
static int eq_biquad(const rwkvtts_eq_band& b, double* c) {
  RT_CHECK(b.kind >= RWKVTTS_EQ_PEAK && b.kind <= RWKVTTS_EQ_LOWPASS && b.reserved == 0, RWKVTTS_EINVAL,
           "eq_design: unknown band kind");
  const bool pass = b.kind == RWKVTTS_EQ_HIGHPASS || b.kind == RWKVTTS_EQ_LOWPASS;
  RT_CHECK(b.freq_hz >= 50.0 && b.freq_hz <= 7600.0 && b.q >= 0.3 && b.q <= 4.0 &&
               (pass || (b.gain_db >= -18.0 && b.gain_db <= 18.0)),
           RWKVTTS_EINVAL, "eq_design: a band needs freq_hz in [50, 7600], gain_db in [-18, 18] and q in [0.3, 4]");  // (NaN fails)
  const double pi = 3.141592653589793;
  const double w = 2.0 * pi * b.freq_hz / kEqFs;
  const double cs = cos(w), al = sin(w) / (2.0 * b.q);
  double b0, b1, b2, a0, a1, a2;
  if (pass) {
    const double u = b.kind == RWKVTTS_EQ_LOWPASS ? 1.0 - cs : 1.0 + cs;
    b0 = u / 2.0, b1 = b.kind == RWKVTTS_EQ_LOWPASS ? u : -u, b2 = u / 2.0;
    a0 = 1.0 + al, a1 = -2.0 * cs, a2 = 1.0 - al;
  } else {
    const double A = pow(10.0, b.gain_db / 40.0);
    if (b.kind == RWKVTTS_EQ_PEAK) {
      b0 = 1.0 + al * A, b1 = -2.0 * cs, b2 = 1.0 - al * A;
      a0 = 1.0 + al / A, a1 = -2.0 * cs, a2 = 1.0 - al / A;
    } else {
      const double be = 2.0 * sqrt(A) * al;
      const double lo = (A + 1.0) - (A - 1.0) * cs, hi = (A + 1.0) + (A - 1.0) * cs;
      if (b.kind == RWKVTTS_EQ_LOWSHELF) {
        b0 = A * (lo + be), b1 = 2.0 * A * ((A - 1.0) - (A + 1.0) * cs), b2 = A * (lo - be);
        a0 = hi + be, a1 = -2.0 * ((A - 1.0) + (A + 1.0) * cs), a2 = hi - be;
      } else {
        b0 = A * (hi + be), b1 = -2.0 * A * ((A - 1.0) + (A + 1.0) * cs), b2 = A * (hi - be);
        a0 = lo + be, a1 = 2.0 * ((A - 1.0) - (A + 1.0) * cs), a2 = lo - be;
      }
    }
  }
  c[0] = b0 / a0, c[1] = b1 / a0, c[2] = b2 / a0, c[3] = a1 / a0, c[4] = a2 / a0;
  return RWKVTTS_OK;
}

// h64 and N of a band list; RWKVTTS_EINVAL for a bad band or a filter that rings past 4096 taps.
static int eq_make(const rwkvtts_eq_band* bands, int n_bands, std::vector<double>& v, int* n_taps, double* sum_abs) {
  RT_CHECK(bands && n_bands >= 1 && n_bands <= kEqMaxBands, RWKVTTS_EINVAL, "eq_design: an equaliser is 1 .. 8 bands");
  v.assign((size_t)kEqImpulse, 0.0);
  v[0] = 1.0;
  int ringer = 0;
  for (int i = 0; i < n_bands; ++i) {
    double c[5];
    int rc = eq_biquad(bands[i], c);
    if (rc) return rc;
    if (bands[i].freq_hz / bands[i].q < bands[ringer].freq_hz / bands[ringer].q) ringer = i;
    double x1 = 0.0, x2 = 0.0, y1 = 0.0, y2 = 0.0;
    for (double& s : v) {
      const double x0 = s;
      double t = c[0] * x0;
      t = t + c[1] * x1;
      t = t + c[2] * x2;
      t = t - c[3] * y1;
      t = t - c[4] * y2;
      x2 = x1, x1 = x0, y2 = y1, y1 = t;
      s = t;
    }
  }
  std::vector<double> tail((size_t)kEqImpulse + 1, 0.0);
  for (int k = kEqImpulse - 1; k >= 0; --k) tail[(size_t)k] = fabs(v[(size_t)k]) + tail[(size_t)k + 1];
  const double bound = ldexp(tail[0], -24);
  int N = kEqStep;
  while (N <= kEqMaxTaps && !(tail[(size_t)N] <= bound)) N += kEqStep;  // (a NaN response is refused too)
  const rwkvtts_eq_band& r = bands[ringer];
  RT_CHECK(N <= kEqMaxTaps, RWKVTTS_EINVAL,
           "eq_design: the filter rings past " + std::to_string(kEqMaxTaps) + " taps; band " + std::to_string(ringer) +
               " (" + kEqKinds[r.kind] + ", " + std::to_string(r.freq_hz) + " Hz, q " + std::to_string(r.q) +
               ") has the lowest freq_hz / q");
  *n_taps = N;
  if (sum_abs) *sum_abs = tail[0];
  return RWKVTTS_OK;
}

static inline int64_t eq_in_first_needed(int n_taps, int64_t out_first) {
  return std::max<int64_t>(0, out_first - (n_taps - 1));
}

struct EqWindow {
  const float* in;
  int64_t in_first, n_in;
  int set;
  int64_t out_first, out_count;
  float* out;
};

}  // namespace rwkvtts

using namespace rwkvtts;

struct rwkvtts_eq : Stage<EqPiece> {  // (d_table stays empty: the tap sets come with each call)
  DevBuf<EqWin> d_wins;
  DevBuf<float> d_taps;
  std::vector<EqWin> wins;
  std::vector<int32_t> tap_off;
};

// Checks the tap sets and every window against the plan, then runs them all in one launch. Nothing is
// launched and nothing written unless everything passes.
static int eq_run(rwkvtts_eq* v, const std::vector<EqWindow>& ws, const float* table, const int32_t* set_taps, int n_sets,
                  const char* who) {
  RT_CHECK(n_sets >= 0 && n_sets <= 0x7fffffff / kEqMaxTaps && (n_sets == 0 || (table && set_taps)), RWKVTTS_EINVAL,
           std::string(who) + ": bad tap table");
  for (int s = 0; s < n_sets; ++s)
    RT_CHECK(set_taps[s] >= kEqStep && set_taps[s] <= kEqMaxTaps && set_taps[s] % kEqStep == 0, RWKVTTS_EINVAL,
             std::string(who) + ": a tap set is a multiple of 64 taps in [64, 4096]");
  int64_t tot_in = 0, tot_out = 0;
  size_t n_wins = 0;
  int max_taps = 0;
  for (const EqWindow& w : ws) {
    RT_CHECK(w.set >= 0 && w.set < n_sets, RWKVTTS_EINVAL, std::string(who) + ": a window names a tap set that is not given");
    RT_CHECK(w.in_first >= 0 && w.n_in >= 0 && w.out_first >= 0 && w.out_count >= 0 &&
                 w.in_first + w.n_in <= kEqMaxSamples && w.out_first <= kEqMaxSamples && w.out_count <= kEqMaxSamples &&
                 (w.in || w.n_in == 0) && (w.out || w.out_count == 0),
             RWKVTTS_EINVAL, std::string(who) + ": bad window (negative size, null buffer or too long)");
    if (w.out_count == 0) continue;
    RT_CHECK(w.out_first + w.out_count <= w.in_first + w.n_in, RWKVTTS_EINVAL,
             std::string(who) + ": a requested output needs a sample past the given samples");
    RT_CHECK(w.in_first <= eq_in_first_needed(set_taps[w.set], w.out_first), RWKVTTS_EINVAL,
             std::string(who) + ": a requested output reads before the given samples");
    tot_in += w.n_in;
    tot_out += w.out_count;
    max_taps = std::max(max_taps, (int)set_taps[w.set]);
    ++n_wins;
  }
  if (n_wins == 0) return RWKVTTS_OK;
  RT_CHECK(n_wins <= (size_t)0x7fffffff, RWKVTTS_EINVAL, std::string(who) + ": too many windows for one launch");
  std::lock_guard<std::mutex> lock(v->mu);
  v->tap_off.assign((size_t)n_sets, 0);
  int32_t n_table = 0;
  for (int s = 0; s < n_sets; ++s) v->tap_off[(size_t)s] = n_table, n_table += set_taps[s];
  v->desc.clear();
  v->wins.clear();
  int64_t in_off = 0, out_off = 0;
  for (const EqWindow& w : ws) {
    if (w.out_count == 0) continue;
    EqWin j;
    j.in_off = in_off;
    j.in_first = w.in_first;
    j.in_end = w.in_first + w.n_in;
    j.tap_off = v->tap_off[(size_t)w.set];
    j.n_taps = set_taps[w.set];
    for (int64_t o = 0; o < w.out_count; o += kEqPiece) {
      EqPiece p;
      p.a0 = w.out_first + o;
      p.out_off = out_off + o;
      p.count = (int32_t)std::min<int64_t>(kEqPiece, w.out_count - o);
      p.win = (int32_t)v->wins.size();
      v->desc.push_back(p);
    }
    v->wins.push_back(j);
    in_off += w.n_in;
    out_off += w.out_count;
  }
  RT_CHECK(v->desc.size() <= (size_t)0x7fffffff, RWKVTTS_EINVAL, std::string(who) + ": too many outputs for one launch");
  int rc;
  if ((rc = stage_reserve(v, tot_in, tot_out)) || (rc = v->d_wins.reserve(n_wins)) ||
      (rc = v->d_taps.reserve((size_t)n_table)) || (rc = stage_upload(v, ws)))
    return rc;
  RT_HIP(hipMemcpyAsync(v->d_wins.p, v->wins.data(), n_wins * sizeof(EqWin), hipMemcpyHostToDevice, v->stream));
  RT_HIP(hipMemcpyAsync(v->d_taps.p, table, (size_t)n_table * sizeof(float), hipMemcpyHostToDevice, v->stream));
  hipExtLaunchKernelGGL(k_eq, dim3((unsigned)v->desc.size()), dim3(kEqLanes), eq_lds_bytes(max_taps), v->stream, v->ev0,
                        v->ev1, 0u, v->d_in.p, v->d_taps.p, v->d_wins.p, v->d_desc.p, v->d_out.p);
  RT_HIP(hipGetLastError());
  return stage_download(v, ws);
}

extern "C" int rwkvtts_eq_design(const rwkvtts_eq_band* bands, int n_bands, float* taps, int32_t* n_taps,
                                 double* sum_abs) {
  RT_CHECK(n_taps, RWKVTTS_EINVAL, "eq_design: null output");
  return guard_alloc("eq_design", [&] {
    std::vector<double> h;
    int N = 0;
    int rc = eq_make(bands, n_bands, h, &N, sum_abs);
    if (rc) return rc;
    *n_taps = N;
    if (taps)
      for (int k = 0; k < N; ++k) taps[k] = (float)h[(size_t)k];
    return RWKVTTS_OK;
  });
}

extern "C" int rwkvtts_eq_plan(int32_t n_taps, int64_t n_known, int final, int64_t out_first, int64_t* out_ready_end,
                               int64_t* in_first_needed) {
  RT_CHECK(n_taps >= kEqStep && n_taps <= kEqMaxTaps && n_taps % kEqStep == 0 && n_known >= 0 &&
               n_known <= kEqMaxSamples && out_first >= 0 && out_first <= kEqMaxSamples,
           RWKVTTS_EINVAL, "eq_plan: n_taps / n_known / out_first out of range");
  (void)final;  // an output never waits for a later sample
  if (out_ready_end) *out_ready_end = n_known;
  if (in_first_needed) *in_first_needed = eq_in_first_needed(n_taps, out_first);
  return RWKVTTS_OK;
}

extern "C" int rwkvtts_eq_create(int device, const rwkvtts_eq_desc* desc, rwkvtts_eq** out) {
  RT_CHECK(out, RWKVTTS_EINVAL, "eq_create: null output");
  *out = nullptr;
  RT_CHECK(desc && desc->struct_size >= sizeof(rwkvtts_eq_desc) && desc->reserved == 0, RWKVTTS_EINVAL,
           "eq_create: null desc, struct_size too small or reserved not 0");
  // (no table of its own: stage_create's d_table is left out, the rest is what it does)
  rwkvtts_eq* v = nullptr;
  int rc = guard_alloc("eq_create", [&] {
    v = new rwkvtts_eq();
    return RWKVTTS_OK;
  });
  if (rc) return rc;
  v->device = device;
  auto fail = [&](hipError_t e, const char* what) {
    set_error(std::string("eq_create: ") + what + ": " + hipGetErrorString(e));
    stage_free(v);
    return RWKVTTS_EHIP;
  };
  hipError_t e;
  if ((e = hipSetDevice(device)) != hipSuccess) return fail(e, "hipSetDevice");
  if ((e = hipStreamCreate(&v->stream)) != hipSuccess) return fail(e, "hipStreamCreate");
  if ((e = hipEventCreate(&v->ev0)) != hipSuccess) return fail(e, "hipEventCreate");
  if ((e = hipEventCreate(&v->ev1)) != hipSuccess) return fail(e, "hipEventCreate");
  *out = v;
  return RWKVTTS_OK;
}

extern "C" int rwkvtts_eq_destroy(rwkvtts_eq* v) {
  if (!v) return RWKVTTS_OK;
  (void)hipSetDevice(v->device);
  stage_free(v, {v->d_wins.p, v->d_taps.p});
  return RWKVTTS_OK;
}

extern "C" int rwkvtts_eq_batch(rwkvtts_eq* v, const float* const* in, const int64_t* n_in, const int32_t* set, int n,
                                const float* table, const int32_t* set_taps, int n_sets, float* const* out) {
  RT_CHECK(v && n >= 0 && (n == 0 || (in && n_in && set && out)), RWKVTTS_EINVAL, "eq_batch: bad arguments");
  return guard_alloc("eq_batch", [&] {
    std::vector<EqWindow> ws((size_t)n);
    for (int i = 0; i < n; ++i) {
      RT_CHECK(n_in[i] >= 0 && n_in[i] <= kEqMaxSamples, RWKVTTS_EINVAL, "eq_batch: n_in out of range");
      ws[(size_t)i] = EqWindow{in[i], 0, n_in[i], set[i], 0, n_in[i], out[i]};
    }
    return eq_run(v, ws, table, set_taps, n_sets, "eq_batch");
  });
}

extern "C" int rwkvtts_eq_windows(rwkvtts_eq* v, const rwkvtts_eq_window* w, int n, const float* table,
                                  const int32_t* set_taps, int n_sets) {
  RT_CHECK(v && n >= 0 && (n == 0 || w), RWKVTTS_EINVAL, "eq_windows: bad arguments");
  if (n == 0) return RWKVTTS_OK;
  return guard_alloc("eq_windows", [&] {
    std::vector<EqWindow> ws;
    int rc = read_windows("eq_windows", w, n, ws, [](const rwkvtts_eq_window* wi) {
      return EqWindow{wi->in, wi->in_first, wi->n_in, wi->set, wi->out_first, wi->out_count, wi->out};
    });
    return rc ? rc : eq_run(v, ws, table, set_taps, n_sets, "eq_windows");
  });
}

extern "C" int rwkvtts_eq_kernel_ms(rwkvtts_eq* v, double* ms) { return stage_kernel_ms("eq_kernel_ms", v, ms); }
