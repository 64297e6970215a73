// denoise.hip -- an STFT spectral gate on the MI355X, for the `denoise` keyword of the pipeline: 16 kHz
// PCM in, the same number of samples out, the noise floor between harmonics and in pauses taken down by
// at most `denoise` dB; one-shot, batched (a depth per signal) and over exact stream windows. No
// reference counterpart: the reference ships the vocoder's PCM as it is.
//
// The arithmetic contract is in include/rwkvtts.h: frames of 512 at hop 128 under a
// root-Hann window, frames 2 m and 2 m + 1 packed as the real and imaginary part of one 512-point
// complex transform of nine radix-2 decimation-in-frequency stages, a split into the two spectra, the
// power's mean over five frames, its minimum over 125, a gain by one correctly rounded divide, its
// smoothing over three bins, the same butterflies backwards, the window and an overlap-add of four frames
// in ascending order. The kernels are pinned bitwise to a numpy restatement of exactly that
// (tests/test_gpu_denoise.py).
//
// Work, one launch triple per call:
//   k_dn_analyse  a wave per pair of frames, four waves a workgroup. A lane holds 8 complex points and
//                 runs three radix-8 register passes, each three of the contract's radix-2 stages in the
//                 contract's order; between passes the points cross lanes through a padded LDS tile (576
//                 floats a plane; both the stores and the loads of both exchanges touch 64 different banks).
//                 The input is windowed on its way from global memory into registers, at unit stride. The
//                 split reads Z[k] and Z[512 - k] out of LDS and stores X and P = |X|^2, which stay on the
//                 device.
//   k_dn_gain     a wave per (64 output frames, 62 bins + one halo bin either side), a lane per bin, so
//                 every global access is a row of consecutive bins. The lane walks its bin along the
//                 frames: S from a five-frame register window into its own LDS column (188 values), then
//                 the 125-frame minimum as three levels of five in place (4 + 4 + 4 compares an output,
//                 never a rescan), the gain, and the smoothing over bins by two lane shuffles.
//   k_dn_synth    a workgroup per 512 outputs: its four waves inverse-transform the four pairs whose
//                 frames the piece's four hops draw on (G * X packed as it is loaded, the forward
//                 butterflies on swapped parts), window them into LDS, and the 256 lanes add each sample's
//                 four frames in ascending order and store at unit stride.
// LDS: analyse 20.0 KB, gain 47.0 KB (three waves a CU: the kernel moves little and waits on nothing but
// its own loads), synth 36.0 KB (four workgroups a CU). No matrix instruction, deliberately: an MFMA's
// internal order of summation is not the contract's.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <new>
#include <vector>

#include "common.h"
#include "stage.h"

// every sum and product is one rounded operation, as the header states them: no contraction anywhere
#pragma clang fp contract(off)

namespace rwkvtts {

constexpr int kDnN = 512, kDnHop = 128, kDnBins = 257, kDnRow = 264;  // a spectrum's row stride in floats
constexpr int kDnBack = 94, kDnAhead = 30, kDnSmooth = 2;             // the floor's and the mean's reach in frames
constexpr int kDnTile = kDnN + 64;                                    // a padded plane of the exchange tile
constexpr int kDnLanes = 256, kDnWaves = 4;
constexpr int kDnChunk = 64, kDnCol = kDnChunk + kDnBack + kDnAhead, kDnOwn = 62, kDnBinTiles = 5;
constexpr int kDnReach = kDnBack + kDnSmooth;           // 96 frames behind a frame whose gain is wanted
constexpr int kDnLead = kDnAhead + kDnSmooth;           // 32 ahead of it
constexpr int64_t kDnMaxSamples = (int64_t)1 << 36;
static_assert(kDnBack + kDnAhead + 1 == 125 && kDnOwn * kDnBinTiles >= kDnBins, "the gain kernel's split of the work");
static_assert(2 * kDnN == RWKVTTS_DENOISE_TABLE_LEN, "table length");

// One window: its given samples are signal indices [in_first, in_end), stored at x[in_off ...]; every
// other index a frame reads is zero. Its frames are [pa, pb), whole pairs, row `row + f - pa` of the
// spectra; [pa, hi) exist in the signal (hi < pb: the last pair's second frame lies past the end).
struct DnWin {
  int64_t in_off, in_first, in_end, row, pa, pb, hi;
  float g_min, pad;
};

// One workgroup of one of the three kernels, of window `win`.
//   analyse: pairs of frames a, a + 2, .. (n of them, <= 4)
//   gain:    output frames [a, a + n), n <= 64, bin tile b
//   synth:   outputs [a, a + n) inside one 512-aligned block, the first at y[b]
struct DnPiece {
  int64_t a, b;
  int32_t win, n;
};

// Correctly rounded f32 divide through double (53 >= 2 * 24 + 2 bits), as limit.hip's.
__device__ inline float dn_div(float a, float b) { return (float)((double)a / (double)b); }

// d * W^t, W = e^(-2 pi i / 512), tw = cos[256] then -sin[256]; t = 0 and t = 128 are moves.
__device__ inline void dn_twiddle(float dr, float di, int t, const float* tw, float& pr, float& pi) {
  const float c = tw[t], s = tw[256 + t];
  const float r = dr * c - di * s, i = dr * s + di * c;
  pr = t == 0 ? dr : (t == 128 ? di : r);
  pi = t == 0 ? di : (t == 128 ? -dr : i);
}

// Stages 3 P, 3 P + 1, 3 P + 2 of the nine on the lane's 8 points: element j is z[base + (j << (6 - 3 P))].
template <int P>
__device__ inline void dn_radix8(float (&re)[8], float (&im)[8], int base, const float* tw) {
  constexpr int sh = 6 - 3 * P;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const int s = 3 * P + r, h = 256 >> s, step = 4 >> r;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (j & step) continue;
      const int t = ((base + (j << sh)) & (h - 1)) << s;
      const float ur = re[j], ui = im[j], vr = re[j + step], vi = im[j + step];
      re[j] = ur + vr;
      im[j] = ui + vi;
      dn_twiddle(ur - vr, ui - vi, t, tw, re[j + step], im[j + step]);
    }
  }
}

// The 512-point transform of one wave. In: element j is z[lane + 64 j]. Out: element j is Z[dn_out_index(lane, j)].
// tr / ti: the wave's two planes of kDnTile floats. Every wave of the workgroup must call it (barriers).
__device__ inline void dn_fft512(float (&re)[8], float (&im)[8], float* tr, float* ti, const float* tw, int lane) {
  dn_radix8<0>(re, im, lane, tw);
  // exchange 1: point i at i + 8 (i >> 6)
#pragma unroll
  for (int j = 0; j < 8; ++j) tr[lane + 72 * j] = re[j], ti[lane + 72 * j] = im[j];
  __syncthreads();
  const int hi = lane >> 3, lo = lane & 7;
#pragma unroll
  for (int j = 0; j < 8; ++j) re[j] = tr[72 * hi + 8 * j + lo], im[j] = ti[72 * hi + 8 * j + lo];
  dn_radix8<1>(re, im, 64 * hi + lo, tw);
  __syncthreads();
  // exchange 2: point i at i + (i >> 3)
#pragma unroll
  for (int j = 0; j < 8; ++j) tr[72 * hi + 9 * j + lo] = re[j], ti[72 * hi + 9 * j + lo] = im[j];
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 8; ++j) re[j] = tr[9 * lane + j], im[j] = ti[9 * lane + j];
  dn_radix8<2>(re, im, 8 * lane, tw);
  __syncthreads();
}

// k of element j after dn_fft512: the 9-bit reversal of 8 lane + j.
__device__ inline int dn_out_index(int lane, int j) {
  return ((((j & 1) << 2) | (j & 2) | ((j >> 2) & 1)) << 6) | (int)(__brev((unsigned)lane) >> 26);
}

__device__ inline void dn_load_twiddles(float* tw, const float* __restrict__ tab) {
  for (int i = threadIdx.x; i < kDnN; i += kDnLanes) tw[i] = tab[kDnN + i];
  __syncthreads();
}

// grid (pieces), 256 lanes. Wave v takes frames f = a + 2 v and f + 1 (v < n; the others run on zeros and store nothing).
__global__ __launch_bounds__(kDnLanes) void k_dn_analyse(const float* __restrict__ x, const float* __restrict__ tab,
                                                         const DnWin* __restrict__ wins,
                                                         const DnPiece* __restrict__ pieces, float2* __restrict__ X,
                                                         float* __restrict__ Pw) {
  __shared__ float tw[kDnN];
  __shared__ float tile[kDnWaves][2][kDnTile];
  const DnPiece p = pieces[blockIdx.x];
  const DnWin w = wins[p.win];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool live = wave < p.n;
  const int64_t f = p.a + 2 * wave;
  dn_load_twiddles(tw, tab);
  float re[8], im[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int i = lane + 64 * j;
    const int64_t ia = kDnHop * f - 3 * kDnHop + i, ib = ia + kDnHop;
    const float wi = tab[i];
    const float xa = (live && ia >= w.in_first && ia < w.in_end) ? x[w.in_off + (ia - w.in_first)] : 0.0f;
    const float xb = (live && ib >= w.in_first && ib < w.in_end) ? x[w.in_off + (ib - w.in_first)] : 0.0f;
    re[j] = xa * wi;
    im[j] = xb * wi;
  }
  float* tr = tile[wave][0];
  float* ti = tile[wave][1];
  dn_fft512(re, im, tr, ti, tw, lane);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int k = dn_out_index(lane, j);
    tr[k] = re[j], ti[k] = im[j];
  }
  __syncthreads();
  if (!live) return;  // (no barrier follows)
  const int64_t ra = (w.row + (f - w.pa)) * kDnRow, rb = ra + kDnRow;
#pragma unroll
  for (int q = 0; q < 5; ++q) {
    const int k = lane + 64 * q;
    if (k >= kDnBins) break;
    const int m = (kDnN - k) & (kDnN - 1);
    const float zr = tr[k], zi = ti[k], mr = tr[m], mi = ti[m];
    const float ar = (zr + mr) * 0.5f, ai = (zi - mi) * 0.5f, br = (zi + mi) * 0.5f, bi = (mr - zr) * 0.5f;
    X[ra + k] = make_float2(ar, ai);
    X[rb + k] = make_float2(br, bi);
    Pw[ra + k] = ar * ar + ai * ai;
    Pw[rb + k] = br * br + bi * bi;
  }
}

// The mean of the frames that exist among five (an absent one is marked by a negative value), summed in
// ascending order from +0 and multiplied by the rounded reciprocal of their number; +inf where the
// middle one is absent, so that a minimum passes over it.
__device__ inline float dn_mean5(float p0, float p1, float p2, float p3, float p4) {
  if (!(p2 >= 0.0f)) return INFINITY;
  float acc = 0.0f;
  int cnt = 0;
  if (p0 >= 0.0f) acc = acc + p0, ++cnt;
  if (p1 >= 0.0f) acc = acc + p1, ++cnt;
  acc = acc + p2, ++cnt;
  if (p3 >= 0.0f) acc = acc + p3, ++cnt;
  if (p4 >= 0.0f) acc = acc + p4, ++cnt;
  const float rc = cnt == 5 ? (float)(1.0 / 5.0) : cnt == 4 ? 0.25f : cnt == 3 ? (float)(1.0 / 3.0) : cnt == 2 ? 0.5f : 1.0f;
  return acc * rc;
}

// grid (pieces), 64 lanes. Lane l holds bin 62 b - 1 + l, clamped to [0, 256] (the clamp is the
// replicated edge), and writes it if 1 <= l <= 62. LDS: col[i][l] = S, then the block minima, of frame a - 94 + i.
__global__ __launch_bounds__(64) void k_dn_gain(const float* __restrict__ Pw, const DnWin* __restrict__ wins,
                                                const DnPiece* __restrict__ pieces, float alpha, float* __restrict__ G) {
  __shared__ float col[kDnCol * 64];
  const DnPiece p = pieces[blockIdx.x];
  const DnWin w = wins[p.win];
  const int lane = threadIdx.x;
  const int raw = kDnOwn * (int)p.b - 1 + lane, bin = min(max(raw, 0), kDnBins - 1);
  const float* Pb = Pw + w.row * kDnRow + bin;
  auto ld = [&](int64_t f) { return (f >= w.pa && f < w.hi) ? Pb[(f - w.pa) * kDnRow] : -1.0f; };
  const int64_t f0 = p.a - kDnBack;
  float p0 = ld(f0 - 2), p1 = ld(f0 - 1), p2 = ld(f0), p3 = ld(f0 + 1);
  for (int i = 0; i < kDnCol; ++i) {
    const float p4 = ld(f0 + i + 2);
    col[i * 64 + lane] = dn_mean5(p0, p1, p2, p3, p4);
    p0 = p1, p1 = p2, p2 = p3, p3 = p4;
  }
  // three levels of five, each in place in the lane's own column: min over 5, 25, 125 frames from i on
  for (int i = 0; i < kDnCol - 4; ++i) {
    float v = col[i * 64 + lane];
#pragma unroll
    for (int k = 1; k < 5; ++k) v = fminf(v, col[(i + k) * 64 + lane]);
    col[i * 64 + lane] = v;
  }
  for (int i = 0; i < kDnCol - 24; ++i) {
    float v = col[i * 64 + lane];
#pragma unroll
    for (int k = 1; k < 5; ++k) v = fminf(v, col[(i + 5 * k) * 64 + lane]);
    col[i * 64 + lane] = v;
  }
  for (int o = 0; o < p.n; ++o) {
    const int64_t f = p.a + o;
    float g = 1.0f;  // a frame past the signal's end
    if (f < w.hi) {
      float nf = col[o * 64 + lane];
#pragma unroll
      for (int k = 1; k < 5; ++k) nf = fminf(nf, col[(o + 25 * k) * 64 + lane]);
      const float s = dn_mean5(ld(f - 2), ld(f - 1), ld(f), ld(f + 1), ld(f + 2));
      if (s != 0.0f) g = fmaxf(w.g_min, 1.0f - alpha * dn_div(nf, s));
    }
    const float gl = __shfl_up(g, 1), gr = __shfl_down(g, 1);
    if (lane >= 1 && lane <= kDnOwn && raw < kDnBins)
      G[(w.row + (f - w.pa)) * kDnRow + raw] = ((gl + 2.0f * g) + gr) * 0.25f;
  }
}

// grid (pieces), 256 lanes. The piece lies in the 512-aligned block that starts at frame hop 4 q, q = a >> 9;
// wave v inverse-transforms frames 4 q + 2 v and 4 q + 2 v + 1 if a wanted output draws on either.
__global__ __launch_bounds__(kDnLanes) void k_dn_synth(const float2* __restrict__ X, const float* __restrict__ G,
                                                       const float* __restrict__ tab, const DnWin* __restrict__ wins,
                                                       const DnPiece* __restrict__ pieces, float* __restrict__ y) {
  __shared__ float tw[kDnN];
  __shared__ float tile[kDnWaves][2][kDnTile];
  __shared__ float fr[2 * kDnWaves][kDnN];
  const DnPiece p = pieces[blockIdx.x];
  const DnWin w = wins[p.win];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t block0 = (p.a >> 9) << 9, f = 4 * (p.a >> 9) + 2 * wave;
  const int64_t f_lo = p.a >> 7, f_hi = ((p.a + p.n - 1) >> 7) + 3;
  const bool live = f + 1 >= f_lo && f <= f_hi;  // (then both frames are in [pa, pb): the host has checked)
  dn_load_twiddles(tw, tab);
  float re[8], im[8];
  const int64_t ra = live ? (w.row + (f - w.pa)) * kDnRow : 0, rb = ra + kDnRow;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int k = lane + 64 * j, kk = k < kDnBins ? k : kDnN - k;
    float yr = 0.0f, yi = 0.0f;
    if (live) {
      const float2 xa = X[ra + kk], xb = X[rb + kk];
      const float ga = G[ra + kk], gb = G[rb + kk];
      const float ar = ga * xa.x, ai = ga * xa.y, br = gb * xb.x, bi = gb * xb.y;
      yr = k < kDnBins ? ar - bi : ar + bi;  // Y = Ya + i Yb at k, conj(Ya) + i conj(Yb) at 512 - k
      yi = k < kDnBins ? ai + br : br - ai;
    }
    re[j] = yi;  // swapped parts in, swapped parts out: the forward butterflies run the inverse transform
    im[j] = yr;
  }
  dn_fft512(re, im, tile[wave][0], tile[wave][1], tw, lane);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int n = dn_out_index(lane, j);
    const float wn = tab[n];
    fr[2 * wave][n] = (im[j] * (1.0f / kDnN)) * wn;
    fr[2 * wave + 1][n] = (re[j] * (1.0f / kDnN)) * wn;
  }
  __syncthreads();
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    const int s = threadIdx.x + kDnLanes * half;
    const int64_t i = block0 + s;
    if (i < p.a || i >= p.a + p.n) continue;
    float acc = 0.0f;
#pragma unroll
    for (int q = 0; q < 4; ++q) acc = acc + fr[(s >> 7) + q][(s & 127) + (3 - q) * kDnHop];
    y[p.b + (i - p.a)] = acc * 0.5f;
  }
}

// ---- host: configuration, table, plan --------------------------------------------------------
static int dn_config(const rwkvtts_denoise_desc* d, const char* who) {
  RT_CHECK(d && d->struct_size >= sizeof(rwkvtts_denoise_desc), RWKVTTS_EINVAL,
           std::string(who) + ": null desc or struct_size too small");
  RT_CHECK(d->alpha >= 0.0f && d->alpha <= 16.0f, RWKVTTS_EINVAL, std::string(who) + ": alpha must be in [0, 16]");  // (NaN fails)
  return RWKVTTS_OK;
}

static void dn_make_table(float* out) {
  const double pi = 3.141592653589793;
  for (int j = 0; j < kDnN; ++j) out[j] = (float)sqrt(0.5 - 0.5 * cos(2.0 * pi * (double)j / (double)kDnN));
  for (int t = 0; t < kDnN / 2; ++t) {
    out[kDnN + t] = (float)cos(2.0 * pi * (double)t / (double)kDnN);
    out[kDnN + kDnN / 2 + t] = (float)-sin(2.0 * pi * (double)t / (double)kDnN);
  }
}

// The first frame of the pair that holds a sample's first frame.
static inline int64_t dn_pair_of(int64_t sample) { return (sample >> 7) & ~(int64_t)1; }

static inline int64_t dn_ready_end(int64_t n_known, int final) {
  return final ? n_known : std::max<int64_t>(0, kDnHop * (dn_pair_of(n_known) - (kDnLead + 3)));
}
static inline int64_t dn_in_first_needed(int64_t out_first) {
  return std::max<int64_t>(0, kDnHop * (std::max<int64_t>(0, dn_pair_of(out_first) - kDnReach) - 3));
}

struct DnWindow {
  const float* in;
  int64_t in_first, n_in;
  int final;
  float g_min;
  int64_t out_first, out_count;
  float* out;
};

}  // namespace rwkvtts

using namespace rwkvtts;

struct rwkvtts_denoise : Stage<DnPiece> {  // d_table: w[512], cos[256], -sin[256]
  float alpha = 2.0f;
  DevBuf<DnWin> d_wins;
  DevBuf<float2> d_X;
  DevBuf<float> d_P, d_G;
  std::vector<DnWin> wins;
};

// Checks every window against the plan, then runs them all in one launch triple. Nothing is launched and
// nothing written unless every window passes.
static int dn_run(rwkvtts_denoise* v, const std::vector<DnWindow>& ws, const char* who) {
  int64_t tot_in = 0, tot_out = 0;
  size_t n_wins = 0;
  for (const DnWindow& w : ws) {
    RT_CHECK(w.g_min > 0.0f && w.g_min <= 1.0f, RWKVTTS_EINVAL, std::string(who) + ": g_min must be in (0, 1]");  // (NaN fails)
    RT_CHECK(w.in_first >= 0 && w.n_in >= 0 && w.out_first >= 0 && w.out_count >= 0 &&
                 w.in_first + w.n_in <= kDnMaxSamples && w.out_first <= kDnMaxSamples && w.out_count <= kDnMaxSamples &&
                 (w.in || w.n_in == 0) && (w.out || w.out_count == 0),
             RWKVTTS_EINVAL, std::string(who) + ": bad window (negative size, null buffer or too long)");
    if (w.out_count == 0) continue;
    RT_CHECK(w.out_first + w.out_count <= dn_ready_end(w.in_first + w.n_in, w.final), RWKVTTS_EINVAL,
             std::string(who) + ": a requested output needs a sample past the given samples");
    RT_CHECK(w.in_first <= dn_in_first_needed(w.out_first), RWKVTTS_EINVAL,
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
  std::vector<DnPiece> gain, synth;  // the analyse pieces go to v->desc first, these two behind them
  int64_t in_off = 0, out_off = 0, rows = 0;
  for (const DnWindow& w : ws) {
    if (w.out_count == 0) continue;
    DnWin j;
    j.in_off = in_off;
    j.in_first = w.in_first;
    j.in_end = w.in_first + w.n_in;
    j.row = rows;
    j.pa = w.in_first == 0 ? 0 : (w.in_first + 3 * kDnHop + kDnHop - 1) / kDnHop;
    j.pa += j.pa & 1;
    if (w.final) {
      j.hi = (j.in_end - 1) / kDnHop + 4;
      j.pb = j.hi + (j.hi & 1);
    } else {
      j.pb = j.hi = dn_pair_of(j.in_end);
    }
    j.g_min = w.g_min;
    j.pad = 0.0f;
    // the frames whose gains the outputs draw on, whole pairs, and what those reach
    const int64_t ga = dn_pair_of(w.out_first), gb = ((((w.out_first + w.out_count - 1) >> 7) + 3) | 1) + 1;
    RT_CHECK(j.pa <= std::max<int64_t>(0, ga - kDnReach) && gb <= j.pb && (w.final || gb + kDnLead <= j.pb), RWKVTTS_EINVAL,
             std::string(who) + ": internal: the plan and the frame ranges disagree");
    const int32_t win = (int32_t)v->wins.size();
    for (int64_t f = j.pa; f < j.pb; f += 2 * kDnWaves)
      v->desc.push_back(DnPiece{f, 0, win, (int32_t)std::min<int64_t>(kDnWaves, (j.pb - f) / 2)});
    for (int64_t f = ga; f < gb; f += kDnChunk)
      for (int b = 0; b < kDnBinTiles; ++b)
        gain.push_back(DnPiece{f, b, win, (int32_t)std::min<int64_t>(kDnChunk, gb - f)});
    for (int64_t a = w.out_first, end = w.out_first + w.out_count; a < end;) {
      const int64_t stop = std::min<int64_t>(end, ((a >> 9) + 1) << 9);
      synth.push_back(DnPiece{a, out_off + (a - w.out_first), win, (int32_t)(stop - a)});
      a = stop;
    }
    v->wins.push_back(j);
    rows += j.pb - j.pa;
    in_off += w.n_in;
    out_off += w.out_count;
  }
  const size_t n_an = v->desc.size(), n_gain = gain.size(), n_synth = synth.size();
  RT_CHECK(n_an <= (size_t)0x7fffffff && n_gain <= (size_t)0x7fffffff && n_synth <= (size_t)0x7fffffff, RWKVTTS_EINVAL,
           std::string(who) + ": too many frames for one launch");
  v->desc.insert(v->desc.end(), gain.begin(), gain.end());
  v->desc.insert(v->desc.end(), synth.begin(), synth.end());
  const size_t cells = (size_t)rows * kDnRow;
  int rc;
  if ((rc = stage_reserve(v, tot_in, tot_out)) || (rc = v->d_wins.reserve(n_wins)) || (rc = v->d_X.reserve(cells)) ||
      (rc = v->d_P.reserve(cells)) || (rc = v->d_G.reserve(cells)) || (rc = stage_upload(v, ws)))
    return rc;
  RT_HIP(hipMemcpyAsync(v->d_wins.p, v->wins.data(), n_wins * sizeof(DnWin), hipMemcpyHostToDevice, v->stream));
  hipExtLaunchKernelGGL(k_dn_analyse, dim3((unsigned)n_an), dim3(kDnLanes), 0, v->stream, v->ev0, nullptr, 0u, v->d_in.p,
                        v->d_table, v->d_wins.p, v->d_desc.p, v->d_X.p, v->d_P.p);
  RT_HIP(hipGetLastError());
  hipExtLaunchKernelGGL(k_dn_gain, dim3((unsigned)n_gain), dim3(64), 0, v->stream, nullptr, nullptr, 0u, v->d_P.p,
                        v->d_wins.p, v->d_desc.p + n_an, v->alpha, v->d_G.p);
  RT_HIP(hipGetLastError());
  hipExtLaunchKernelGGL(k_dn_synth, dim3((unsigned)n_synth), dim3(kDnLanes), 0, v->stream, nullptr, v->ev1, 0u, v->d_X.p,
                        v->d_G.p, v->d_table, v->d_wins.p, v->d_desc.p + n_an + n_gain, v->d_out.p);
  RT_HIP(hipGetLastError());
  return stage_download(v, ws);
}

extern "C" int rwkvtts_denoise_table(const rwkvtts_denoise_desc* desc, float* out) {
  int rc = dn_config(desc, "denoise_table");
  if (rc) return rc;
  RT_CHECK(out, RWKVTTS_EINVAL, "denoise_table: null output");
  dn_make_table(out);
  return RWKVTTS_OK;
}

extern "C" int rwkvtts_denoise_plan(int64_t n_known, int final, int64_t out_first, int64_t* out_ready_end,
                                    int64_t* in_first_needed) {
  RT_CHECK(n_known >= 0 && n_known <= kDnMaxSamples && out_first >= 0 && out_first <= kDnMaxSamples, RWKVTTS_EINVAL,
           "denoise_plan: n_known / out_first out of range");
  if (out_ready_end) *out_ready_end = dn_ready_end(n_known, final);
  if (in_first_needed) *in_first_needed = dn_in_first_needed(out_first);
  return RWKVTTS_OK;
}

extern "C" int rwkvtts_denoise_create(int device, const rwkvtts_denoise_desc* desc, const float* table,
                                      rwkvtts_denoise** out) {
  RT_CHECK(out, RWKVTTS_EINVAL, "denoise_create: null output");
  *out = nullptr;
  int rc = dn_config(desc, "denoise_create");
  if (rc) return rc;
  rwkvtts_denoise* v = nullptr;
  rc = stage_create("denoise_create", device, table, (size_t)(2 * kDnN), [&](float* t) { dn_make_table(t); }, &v);
  if (rc) return rc;
  v->alpha = desc->alpha;
  *out = v;
  return RWKVTTS_OK;
}

extern "C" int rwkvtts_denoise_destroy(rwkvtts_denoise* v) {
  if (!v) return RWKVTTS_OK;
  (void)hipSetDevice(v->device);
  stage_free(v, {v->d_wins.p, v->d_X.p, v->d_P.p, v->d_G.p});
  return RWKVTTS_OK;
}

extern "C" int rwkvtts_denoise_batch(rwkvtts_denoise* v, const float* const* in, const int64_t* n_in, const float* g_min,
                                     int n, float* const* out) {
  RT_CHECK(v && n >= 0 && (n == 0 || (in && n_in && g_min && out)), RWKVTTS_EINVAL, "denoise_batch: bad arguments");
  return guard_alloc("denoise_batch", [&] {
    std::vector<DnWindow> ws((size_t)n);
    for (int i = 0; i < n; ++i) {
      RT_CHECK(n_in[i] >= 0 && n_in[i] <= kDnMaxSamples, RWKVTTS_EINVAL, "denoise_batch: n_in out of range");
      ws[(size_t)i] = DnWindow{in[i], 0, n_in[i], 1, g_min[i], 0, n_in[i], out[i]};
    }
    return dn_run(v, ws, "denoise_batch");
  });
}

extern "C" int rwkvtts_denoise_windows(rwkvtts_denoise* v, const rwkvtts_denoise_window* w, int n) {
  RT_CHECK(v && n >= 0 && (n == 0 || w), RWKVTTS_EINVAL, "denoise_windows: bad arguments");
  if (n == 0) return RWKVTTS_OK;
  return guard_alloc("denoise_windows", [&] {
    std::vector<DnWindow> ws;
    int rc = read_windows("denoise_windows", w, n, ws, [](const rwkvtts_denoise_window* wi) {
      return DnWindow{wi->in, wi->in_first, wi->n_in, wi->final ? 1 : 0, wi->g_min, wi->out_first, wi->out_count, wi->out};
    });
    return rc ? rc : dn_run(v, ws, "denoise_windows");
  });
}

extern "C" int rwkvtts_denoise_kernel_ms(rwkvtts_denoise* v, double* ms) {
  return stage_kernel_ms("denoise_kernel_ms", v, ms);
}
