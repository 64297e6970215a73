// highband.hip -- blind bandwidth extension by spectral folding on the MI355X, for the `highband`
// keyword of the pipeline: 16 kHz PCM in, 32 kHz PCM out whose 8-12 kHz band is synthesised from the
// input's own 4-8 kHz band, one-shot, batched (a gain per signal) and over exact stream windows. No
// reference counterpart: the reference emits 16 kHz only.
//
// The arithmetic contract is in include/rwkvtts.h: three FIRs as sequential f32 sums
// (a 31-tap high-pass at 16 kHz, a 32-tap half-band interpolator, a 63-tap shaping filter at 32 kHz
// over the sign-alternated high band), block energies from 64 ordered partials and a fixed tree, a
// smoothstep of their ratio as the block gain, a linear gain ramp per block. The kernels are pinned
// bitwise to a numpy restatement of exactly that (tests/test_gpu_highband.py).
//
// Work: k_hb_gain gives a wave to a block: the block's 160 samples and HP4's 15 either side in LDS,
// a lane runs the 31-step chain of the two or three samples it owns, the wave sums both energies in
// the contract's order and lane 0 writes the gain. k_hb_synth gives a workgroup of 320 lanes to a piece
// of 320 input positions, 640 outputs (two blocks): the input span with the three filters' summed halo
// (412 floats) goes to LDS once; the lanes form b over the span (382 values), then the negated odd
// phase of its interpolation (351 values), both in LDS; then each lane runs the chains of its own input
// position -- the odd phase of u over x, and the even and the odd output of SH, each of which reads b
// at its odd (even) taps and the interpolated phase at the others, so the 32 kHz signal v never exists
// -- and stores its two outputs. Nothing intermediate goes to device memory but the block gains. The
// taps are uniform over the lanes at compile-time offsets: scalar loads from the table, no LDS. A piece
// whose three gains are all zero forms neither b nor w. Both kernels go to one stream; kernel order is
// the only hand-off. No matrix instruction: the contract is the sequential sums.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <new>
#include <vector>

#include "common.h"
#include "stage.h"

// the tables are built in double, step by step as the header states them: no contraction anywhere
#pragma clang fp contract(off)

namespace rwkvtts {

constexpr int kHbHp = 31, kHbIp = 32, kHbSh = 63;  // taps
constexpr int kHbB = 160;                          // input samples per block
constexpr int kHbPiece = 2 * kHbB;                 // input positions per workgroup of k_hb_synth
constexpr int kHbOffIp = kHbHp, kHbOffSh = kHbHp + kHbIp, kHbOffR = kHbHp + kHbIp + kHbSh;
constexpr int kHbTable = kHbOffR + 2 * kHbB;
constexpr int kHbXs = kHbPiece + 92, kHbBs = kHbPiece + 62, kHbVs = kHbPiece + 31;  // LDS spans of a piece
constexpr int kHbLook = 46;  // input samples an output's filters reach ahead of (and behind) its position
constexpr int64_t kHbMaxSamples = (int64_t)1 << 40;
static_assert(kHbTable == RWKVTTS_HIGHBAND_TABLE_LEN, "table length");

struct HbCfg {
  double level_db;
  float r_lo, r_hi, floor;
};

// One window: its given samples are signal indices [in_first, in_end), stored at x[in_off ...]; every
// other index reads as zero (the host has checked that those are below 0 or past the end of a final
// window). The gains of blocks [gb0, gb0 + g_cnt) lie at g[g_off ...].
struct HbWin {
  int64_t in_off, in_first, in_end;
  int64_t gb0, g_cnt, g_off;
  float G, pad;
};

// One workgroup of k_hb_synth: input positions [a0, a0 + 320) of window `win`, a0 a multiple of 320;
// of its outputs [2 a0, 2 a0 + 640) those in [o_lo, o_hi) are wanted, o_lo at y[out_off].
struct HbPiece {
  int64_t a0, o_lo, o_hi, out_off;
  int32_t win, pad;
};

__device__ inline float hb_x(const float* __restrict__ x, const HbWin& w, int64_t idx) {
  return (idx >= w.in_first && idx < w.in_end) ? x[w.in_off + (idx - w.in_first)] : 0.0f;
}

// Correctly rounded f32 divide through double (53 >= 2 * 24 + 2 bits), as level.hip's.
__device__ inline float hb_div(float a, float b) { return (float)((double)a / (double)b); }

// sum_k h[k] * s[top - k], k = 0 .. T - 1, ascending from +0: one rounded multiply, one rounded add.
template <int T>
__device__ inline float hb_chain(const float* __restrict__ h, const float* s_top) {
  float acc = 0.0f;
#pragma unroll
  for (int k = 0; k < T; ++k) acc = __fadd_rn(acc, __fmul_rn(h[k], s_top[-k]));
  return acc;
}

// grid (gain blocks of the longest window, windows), one wave each.
__global__ __launch_bounds__(64) void k_hb_gain(const float* __restrict__ x, const float* __restrict__ tab,
                                                const HbWin* __restrict__ wins, float* __restrict__ g, float r_lo,
                                                float r_hi, float floor_) {
  __shared__ float xs[kHbB + kHbHp - 1];  // x[160 k - 15, 160 k + 175)
  const HbWin w = wins[blockIdx.y];
  if ((int64_t)blockIdx.x >= w.g_cnt) return;  // (uniform over the wave)
  const int64_t k = w.gb0 + blockIdx.x;
  const int lane = threadIdx.x;
  const int64_t base = k * kHbB - (kHbHp / 2);
  for (int i = lane; i < kHbB + kHbHp - 1; i += 64) xs[i] = hb_x(x, w, base + i);
  __syncthreads();
  float pb = 0.0f, px = 0.0f;  // p[l]: the squares of i = l (mod 64), ascending
  for (int i = lane; i < kHbB; i += 64) {
    const float acc = hb_chain<kHbHp>(tab, xs + i + kHbHp - 1);
    const float b = (k * kHbB + i < w.in_end) ? acc : 0.0f;
    const float xv = xs[i + kHbHp / 2];
    pb = __fadd_rn(pb, __fmul_rn(b, b));
    px = __fadd_rn(px, __fmul_rn(xv, xv));
  }
  // p[l] += p[l + s] for l < s: lanes at or above s hold values nothing reads again
  for (int s = 32; s >= 1; s >>= 1) {
    pb = __fadd_rn(pb, __shfl_down(pb, s, 64));
    px = __fadd_rn(px, __shfl_down(px, s, 64));
  }
  if (lane != 0) return;
  const float r = px < floor_ ? 0.0f : hb_div(pb, px);
  float s;
  if (r <= r_lo) {
    s = 0.0f;
  } else if (r >= r_hi) {
    s = 1.0f;
  } else {
    const float t = hb_div(__fsub_rn(r, r_lo), __fsub_rn(r_hi, r_lo));
    s = __fmul_rn(__fmul_rn(t, t), __fsub_rn(3.0f, __fmul_rn(2.0f, t)));
  }
  g[w.g_off + blockIdx.x] = __fmul_rn(w.G, s);
}

// grid (pieces), 320 lanes each. LDS: xs = x[a0 - 46, a0 + 366), bs = b[a0 - 31, a0 + 351),
// vs = -ub[2n + 1] for n in [a0 - 16, a0 + 335).
__global__ __launch_bounds__(kHbPiece) void k_hb_synth(const float* __restrict__ x, const float* __restrict__ tab,
                                                       const HbWin* __restrict__ wins,
                                                       const HbPiece* __restrict__ pieces, const float* __restrict__ g,
                                                       float* __restrict__ y) {
  __shared__ float xs[kHbXs];
  __shared__ float bs[kHbBs];
  __shared__ float vs[kHbVs];
  const HbPiece p = pieces[blockIdx.x];
  const HbWin w = wins[p.win];
  const int t = threadIdx.x;
  for (int i = t; i < kHbXs; i += kHbPiece) xs[i] = hb_x(x, w, p.a0 - kHbLook + i);
  // the gains of blocks j0 - 1, j0, j0 + 1; an index outside the window's gains is one no wanted output uses
  // (g_{-1} = g_0 is the clamp at block 0)
  const int64_t j0 = p.a0 / kHbB, g_hi = w.gb0 + w.g_cnt - 1;
  float gs[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    int64_t j = j0 - 1 + d;
    j = j < w.gb0 ? w.gb0 : (j > g_hi ? g_hi : j);
    gs[d] = g[w.g_off + (j - w.gb0)];
  }
  const bool live = gs[0] != 0.0f || gs[1] != 0.0f || gs[2] != 0.0f;  // (uniform over the workgroup)
  __syncthreads();
  if (live) {
    for (int i = t; i < kHbBs; i += kHbPiece) {  // b[n] = sum_k hp[k] x[n + 15 - k]
      const int64_t n = p.a0 - 31 + i;
      const float acc = hb_chain<kHbHp>(tab, xs + i + 30);
      bs[i] = (n >= 0 && n < w.in_end) ? acc : 0.0f;
    }
    __syncthreads();
    for (int i = t; i < kHbVs; i += kHbPiece) {  // -ub[2n + 1] = -(sum_k ip[k] b[n + 16 - k])
      const int64_t n = p.a0 - 16 + i;
      const float acc = hb_chain<kHbIp>(tab + kHbOffIp, bs + i + 31);
      vs[i] = (n >= 0 && n < w.in_end) ? -acc : 0.0f;
    }
    __syncthreads();
  }
  const float xe = xs[t + kHbLook];                                   // u[2a] = x[a]
  const float uo = hb_chain<kHbIp>(tab + kHbOffIp, xs + t + 62);      // u[2a + 1] = sum_k ip[k] x[a + 16 - k]
  float ye = xe, yo = uo;
  if (live) {
    // w[2a] = sum_k sh[k] v[2a + 31 - k]: odd k reads b[a + (31 - k) / 2], even k the other phase at
    // a + (30 - k) / 2; w[2a + 1] = sum_k sh[k] v[2a + 32 - k]: even k reads b[a + (32 - k) / 2], odd k
    // the other phase at a + (31 - k) / 2. Both in ascending k.
    const float* sh = tab + kHbOffSh;
    const float* bp = bs + t + 31;
    const float* vp = vs + t + 16;
    float w0 = 0.0f, w1 = 0.0f;
#pragma unroll
    for (int k = 0; k < kHbSh; ++k) {
      const float h = sh[k];
      const float s0 = (k & 1) ? bp[(31 - k) / 2] : vp[(30 - k) / 2];
      const float s1 = (k & 1) ? vp[(31 - k) / 2] : bp[(32 - k) / 2];
      w0 = __fadd_rn(w0, __fmul_rn(h, s0));
      w1 = __fadd_rn(w1, __fmul_rn(h, s1));
    }
    const int hi = t >= kHbB ? 1 : 0;
    const float ga = gs[hi], dg = __fsub_rn(gs[hi + 1], gs[hi]);
    const float* r = tab + kHbOffR + 2 * (t - hi * kHbB);
    const float ge = __fadd_rn(ga, __fmul_rn(dg, r[0]));
    const float go = __fadd_rn(ga, __fmul_rn(dg, r[1]));
    if (ge != 0.0f) ye = __fadd_rn(xe, __fmul_rn(ge, w0));
    if (go != 0.0f) yo = __fadd_rn(uo, __fmul_rn(go, w1));
  }
  const int64_t o = 2 * (p.a0 + t);
  if (o >= p.o_lo && o < p.o_hi) y[p.out_off + (o - p.o_lo)] = ye;
  if (o + 1 >= p.o_lo && o + 1 < p.o_hi) y[p.out_off + (o + 1 - p.o_lo)] = yo;
}

// ---- host: configuration, table, plan --------------------------------------------------------
static int hb_config(const rwkvtts_highband_desc* d, HbCfg* c, const char* who) {
  RT_CHECK(d && d->struct_size >= sizeof(rwkvtts_highband_desc), RWKVTTS_EINVAL,
           std::string(who) + ": null desc or struct_size too small");
  c->level_db = d->level_db != 0.0f ? (double)d->level_db : -6.0;
  c->r_lo = d->r_lo != 0.0f ? d->r_lo : 0.02f;
  c->r_hi = d->r_hi != 0.0f ? d->r_hi : 0.2f;
  c->floor = d->floor != 0.0f ? d->floor : 1e-6f;
  auto pos = [](float v) { return v > 0.0f && v <= 3.4028234e38f; };  // (NaN fails)
  RT_CHECK(c->level_db >= -40.0 && c->level_db <= 20.0, RWKVTTS_EINVAL,
           std::string(who) + ": level_db must be -40 .. 20 (0 = -6)");
  RT_CHECK(pos(c->r_lo) && pos(c->r_hi) && c->r_hi > c->r_lo && pos(c->floor), RWKVTTS_EINVAL,
           std::string(who) + ": r_lo, r_hi and floor must be finite and positive, r_hi > r_lo");
  return RWKVTTS_OK;
}

static int hb_gain_ok(float G, const char* who) {
  RT_CHECK(G >= 0.0f && G <= 1.0e4f, RWKVTTS_EINVAL, std::string(who) + ": G must be finite, 0 .. 1e4");
  return RWKVTTS_OK;
}

static void hb_make_table(float* out) {
  const double pi = 3.141592653589793;
  double lp[kHbHp], q[kHbIp];
  double s = 0.0;
  for (int k = 0; k < kHbHp; ++k) {
    const double t = (double)(k - 15);
    const double w = 0.54 + 0.46 * cos(pi * t / 15.0);
    lp[k] = (k == 15 ? 0.5 : sin(pi * t / 2.0) / (pi * t)) * w;
    s = s + lp[k];
  }
  for (int k = 0; k < kHbHp; ++k) out[k] = (float)((k == 15 ? 1.0 : 0.0) - lp[k] / s);
  s = 0.0;
  for (int k = 0; k < kHbIp; ++k) {
    const double t = 15.5 - (double)k;
    const double w = 0.54 + 0.46 * cos(pi * t / 16.0);
    q[k] = sin(pi * t) / (pi * t) * w;
    s = s + q[k];
  }
  for (int k = 0; k < kHbIp; ++k) out[kHbOffIp + k] = (float)(q[k] / s);
  const double edge_f[3] = {8500.0, 12000.0, 13000.0}, edge_a[3] = {1.0, 0.35, 0.0};
  for (int k = 0; k < kHbSh; ++k) {
    const double t = (double)(k - 31);
    double acc = 0.0;
    for (int e = 0; e < 2; ++e) {
      const double w1 = 2.0 * pi * edge_f[e] / 32000.0, w2 = 2.0 * pi * edge_f[e + 1] / 32000.0;
      const double a1 = edge_a[e], a2 = edge_a[e + 1];
      const double beta = (a2 - a1) / (w2 - w1);
      double seg;
      if (k == 31)
        seg = a1 * (w2 - w1) + beta * (w2 - w1) * (w2 - w1) / 2.0;
      else
        seg = (a2 * sin(w2 * t) - a1 * sin(w1 * t)) / t + beta * (cos(w2 * t) - cos(w1 * t)) / (t * t);
      acc = acc + seg;
    }
    out[kHbOffSh + k] = (float)(acc / pi * (0.54 + 0.46 * cos(pi * t / 31.0)));
  }
  for (int i = 0; i < 2 * kHbB; ++i) out[kHbOffR + i] = (float)((double)(i + 1) / (double)(2 * kHbB));
}

static inline int64_t hb_ready_end(int64_t n_known, int final) {
  if (final) return 2 * n_known;
  const int64_t by_gain = 2 * kHbB * std::max<int64_t>(0, (n_known - kHbHp / 2) / kHbB);
  return std::min(by_gain, 2 * std::max<int64_t>(0, n_known - kHbLook));
}
static inline int64_t hb_in_first_needed(int64_t out_first) {
  return std::max<int64_t>(0, kHbB * (out_first / (2 * kHbB) - 1) - kHbHp / 2);
}

struct HbWindow {
  const float* in;
  int64_t in_first, n_in;
  int final;
  float G;
  int64_t out_first, out_count;
  float* out;
};

}  // namespace rwkvtts

using namespace rwkvtts;

struct rwkvtts_highband : Stage<HbPiece> {  // d_table: hp, ip, sh, r
  HbCfg cfg;
  DevBuf<HbWin> d_wins;
  DevBuf<float> d_g;
  std::vector<HbWin> wins;
};

// Checks every window against the plan, then runs them all: one launch each of gain and synth. Nothing
// is launched and nothing written unless every window passes.
static int hb_run(rwkvtts_highband* v, const std::vector<HbWindow>& ws, const char* who) {
  int64_t tot_in = 0, tot_out = 0, tot_g = 0, max_g = 0;
  size_t n_wins = 0;
  int rc;
  for (const HbWindow& w : ws) {
    if ((rc = hb_gain_ok(w.G, who))) return rc;
    RT_CHECK(w.in_first >= 0 && w.n_in >= 0 && w.out_first >= 0 && w.out_count >= 0 &&
                 w.in_first + w.n_in <= kHbMaxSamples && w.out_first <= 2 * kHbMaxSamples &&
                 w.out_count <= 2 * kHbMaxSamples && (w.in || w.n_in == 0) && (w.out || w.out_count == 0),
             RWKVTTS_EINVAL, std::string(who) + ": bad window (negative size, null buffer or too long)");
    if (w.out_count == 0) continue;
    RT_CHECK(w.out_first + w.out_count <= hb_ready_end(w.in_first + w.n_in, w.final), RWKVTTS_EINVAL,
             std::string(who) + ": a requested output needs a sample or a block gain past the given samples");
    RT_CHECK(w.in_first <= hb_in_first_needed(w.out_first), RWKVTTS_EINVAL,
             std::string(who) + ": a requested output reads before the given samples");
    const int64_t gb0 = std::max<int64_t>(0, w.out_first / (2 * kHbB) - 1);
    const int64_t g_cnt = (w.out_first + w.out_count - 1) / (2 * kHbB) - gb0 + 1;
    tot_in += w.n_in;
    tot_out += w.out_count;
    tot_g += g_cnt;
    max_g = std::max(max_g, g_cnt);
    ++n_wins;
  }
  if (n_wins == 0) return RWKVTTS_OK;
  RT_CHECK(n_wins <= 65535 && max_g <= 0x7fffffff, RWKVTTS_EINVAL, std::string(who) + ": too much for one launch");
  std::lock_guard<std::mutex> lock(v->mu);
  v->desc.clear();
  v->wins.clear();
  int64_t in_off = 0, out_off = 0, g_off = 0;
  for (const HbWindow& w : ws) {
    if (w.out_count == 0) continue;
    const int64_t o_end = w.out_first + w.out_count;
    HbWin j;
    j.in_off = in_off;
    j.in_first = w.in_first;
    j.in_end = w.in_first + w.n_in;
    j.gb0 = std::max<int64_t>(0, w.out_first / (2 * kHbB) - 1);
    j.g_cnt = (o_end - 1) / (2 * kHbB) - j.gb0 + 1;
    j.g_off = g_off;
    j.G = w.G;
    j.pad = 0.0f;
    for (int64_t q = w.out_first / (2 * kHbPiece); q <= (o_end - 1) / (2 * kHbPiece); ++q) {
      HbPiece p;
      p.a0 = q * kHbPiece;
      p.o_lo = std::max(w.out_first, 2 * p.a0);
      p.o_hi = std::min(o_end, 2 * (p.a0 + kHbPiece));
      p.out_off = out_off + (p.o_lo - w.out_first);
      p.win = (int32_t)v->wins.size();
      p.pad = 0;
      v->desc.push_back(p);
    }
    v->wins.push_back(j);
    in_off += w.n_in;
    out_off += w.out_count;
    g_off += j.g_cnt;
  }
  RT_CHECK(v->desc.size() <= (size_t)0x7fffffff, RWKVTTS_EINVAL, std::string(who) + ": too many outputs for one launch");
  if ((rc = stage_reserve(v, tot_in, tot_out)) || (rc = v->d_wins.reserve(n_wins)) ||
      (rc = v->d_g.reserve((size_t)tot_g)) || (rc = stage_upload(v, ws)))
    return rc;
  RT_HIP(hipMemcpyAsync(v->d_wins.p, v->wins.data(), n_wins * sizeof(HbWin), hipMemcpyHostToDevice, v->stream));
  // the event pair brackets both kernels: start of the gain, end of the synth
  const HbCfg& c = v->cfg;
  hipExtLaunchKernelGGL(k_hb_gain, dim3((unsigned)max_g, (unsigned)n_wins), dim3(64), 0, v->stream, v->ev0, nullptr, 0u,
                        v->d_in.p, v->d_table, v->d_wins.p, v->d_g.p, c.r_lo, c.r_hi, c.floor);
  RT_HIP(hipGetLastError());
  hipExtLaunchKernelGGL(k_hb_synth, dim3((unsigned)v->desc.size()), dim3(kHbPiece), 0, v->stream, nullptr, v->ev1, 0u,
                        v->d_in.p, v->d_table, v->d_wins.p, v->d_desc.p, v->d_g.p, v->d_out.p);
  RT_HIP(hipGetLastError());
  return stage_download(v, ws);
}

extern "C" int rwkvtts_highband_table(const rwkvtts_highband_desc* desc, float* out) {
  HbCfg c;
  int rc = hb_config(desc, &c, "highband_table");
  if (rc) return rc;
  RT_CHECK(out, RWKVTTS_EINVAL, "highband_table: null output");
  hb_make_table(out);
  return RWKVTTS_OK;
}

extern "C" int rwkvtts_highband_gain(const rwkvtts_highband_desc* desc, double highband_db, float* out) {
  HbCfg c;
  int rc = hb_config(desc, &c, "highband_gain");
  if (rc) return rc;
  RT_CHECK(out && highband_db >= -12.0 && highband_db <= 12.0, RWKVTTS_EINVAL,
           "highband_gain: null output or highband outside -12 .. 12 dB");
  *out = (float)pow(10.0, (c.level_db + highband_db) / 20.0);
  return RWKVTTS_OK;
}

extern "C" int rwkvtts_highband_plan(const rwkvtts_highband_desc* desc, int64_t n_known, int final, int64_t out_first,
                                     int64_t* out_ready_end, int64_t* in_first_needed) {
  HbCfg c;
  int rc = hb_config(desc, &c, "highband_plan");
  if (rc) return rc;
  RT_CHECK(n_known >= 0 && n_known <= kHbMaxSamples && out_first >= 0 && out_first <= 2 * kHbMaxSamples,
           RWKVTTS_EINVAL, "highband_plan: n_known / out_first out of range");
  if (out_ready_end) *out_ready_end = hb_ready_end(n_known, final);
  if (in_first_needed) *in_first_needed = hb_in_first_needed(out_first);
  return RWKVTTS_OK;
}

extern "C" int rwkvtts_highband_create(int device, const rwkvtts_highband_desc* desc, const float* table,
                                       rwkvtts_highband** out) {
  RT_CHECK(out, RWKVTTS_EINVAL, "highband_create: null output");
  *out = nullptr;
  HbCfg c;
  int rc = hb_config(desc, &c, "highband_create");
  if (rc) return rc;
  rwkvtts_highband* v = nullptr;
  rc = stage_create("highband_create", device, table, (size_t)kHbTable, [&](float* t) { hb_make_table(t); }, &v);
  if (rc) return rc;
  v->cfg = c;
  *out = v;
  return RWKVTTS_OK;
}

extern "C" int rwkvtts_highband_destroy(rwkvtts_highband* v) {
  if (!v) return RWKVTTS_OK;
  (void)hipSetDevice(v->device);
  stage_free(v, {v->d_wins.p, v->d_g.p});
  return RWKVTTS_OK;
}

extern "C" int rwkvtts_highband_batch(rwkvtts_highband* v, const float* const* in, const int64_t* n_in, const float* G,
                                      int n, float* const* out) {
  RT_CHECK(v && n >= 0 && (n == 0 || (in && n_in && G && out)), RWKVTTS_EINVAL, "highband_batch: bad arguments");
  return guard_alloc("highband_batch", [&] {
    std::vector<HbWindow> ws((size_t)n);
    for (int i = 0; i < n; ++i) {
      RT_CHECK(n_in[i] >= 0 && n_in[i] <= kHbMaxSamples, RWKVTTS_EINVAL, "highband_batch: n_in out of range");
      ws[(size_t)i] = HbWindow{in[i], 0, n_in[i], 1, G[i], 0, 2 * n_in[i], out[i]};
    }
    return hb_run(v, ws, "highband_batch");
  });
}

extern "C" int rwkvtts_highband_windows(rwkvtts_highband* v, const rwkvtts_highband_window* w, int n) {
  RT_CHECK(v && n >= 0 && (n == 0 || w), RWKVTTS_EINVAL, "highband_windows: bad arguments");
  if (n == 0) return RWKVTTS_OK;
  return guard_alloc("highband_windows", [&] {
    std::vector<HbWindow> ws;
    int rc = read_windows("highband_windows", w, n, ws, [](const rwkvtts_highband_window* wi) {
      return HbWindow{wi->in, wi->in_first, wi->n_in, wi->final ? 1 : 0, wi->G, wi->out_first, wi->out_count, wi->out};
    });
    return rc ? rc : hb_run(v, ws, "highband_windows");
  });
}

extern "C" int rwkvtts_highband_kernel_ms(rwkvtts_highband* v, double* ms) {
  return stage_kernel_ms("highband_kernel_ms", v, ms);
}
