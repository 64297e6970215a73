// pause.hip -- silences capped on the MI355X, for the `max_pause` keyword of the pipeline: no silence
// inside the result longer than M samples, none at either end longer than half of it. One-shot,
// batched (an M per signal) and over exact stream windows. The first stage whose output length depends
// on the data. No reference counterpart: the reference sends whatever silence the semantic model chose.
//
// The arithmetic contract is in include/rwkvtts.h: a block is loud if a sample of it
// passes the threshold, active if a block within H of it is loud; a run of non-active blocks longer
// than the rule allows is cut to a head and a tail, each faded over F samples by one rounded f32
// multiply per sample; every other sample is copied. Comparisons and integers only, so nothing depends
// on an order. The kernels are pinned bitwise to a numpy restatement of exactly that
// (tests/test_gpu_pause.py).
//
// Work: k_pause_flags gives a wave 64 blocks of a signal -- 16-byte loads, a compare per sample, a
// ballot per 64 vectors -- and packs their loud bits into one 64-bit word. k_pause_plan gives a
// workgroup to a signal: it dilates the words by H, finds where runs start (bit operations on the
// words), has the lane that owns a word follow each of its runs to its end and apply the rule, and scans
// what the cuts remove; it writes a table of cuts (where a cut lands in the output, what has been
// removed up to and including it, its source range, its fades), n_out, the number of cuts and the
// stream state. k_pause_gather gives a workgroup to 1024 outputs: one search of the table per
// workgroup, then each lane copies, or multiplies by the ramp. All three go to one stream; kernel order
// is the only hand-off. The host learns n_out only after the plan, so the counts come back first, with
// a synchronisation of their own, and then n_out samples of each output.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <new>
#include <vector>

#include "common.h"
#include "stage.h"

#pragma clang fp contract(off)

namespace rwkvtts {

constexpr int kPauseThreads = 256;
constexpr int kPauseWaves = kPauseThreads / 64;
constexpr int kPauseTile = 4 * kPauseThreads;             // outputs per gather workgroup
constexpr int kPauseMaxHang = 32;                          // a dilated word reads its two neighbours only
constexpr int kPauseMaxFade = 4096;
constexpr int64_t kPauseMaxSamples = (int64_t)1 << 30;
constexpr int64_t kPauseFadeIn = 1, kPauseFadeOut = 2, kPauseCounted = 4;

struct PauseCfg {
  int B, H, F;
  float threshold;
};

// One signal or window. The given samples are signal indices [in_first, n_end), sample idx at
// x[in_off + (idx - in_first)] with in_off = in_first (mod 4), so a block starts on 16 bytes. Loud bits
// exist for blocks [fb, nbk), bit l of the job's words is block fb + l; blocks [c, kd) are decided in
// this call, from the state (c, seen, q). Output 0 is source sample p0; `end` is where the decided
// samples end.
struct PauseJob {
  int64_t in_off, in_first, n_end;
  int64_t fb, nbk, c, kd;
  int64_t q, M, p0, end;
  int64_t w_off, cut_off, cut_cap, out_off, out_cap;
  int32_t seen, final;
};

// Source samples [a, b) are removed. d: the output index of the first sample behind the cut; r: the
// samples removed up to and including it.
struct PauseCut {
  int64_t d, r, a, b, flags;
};

struct PauseRes {
  int64_t n_out, n_cuts, n_rec, c, q, seen;
};

template <typename T>
__device__ inline T pmin(T a, T b) { return b < a ? b : a; }

__device__ inline uint64_t pause_bits_from(int64_t l) {  // bits l .. 63 of a word; l <= 0: all, l >= 64: none
  return l <= 0 ? ~0ull : l >= 64 ? 0ull : ~0ull << l;
}
// the bits of word w whose block index lies in [lo, hi)
__device__ inline uint64_t pause_range(int64_t w, int64_t lo, int64_t hi) {
  return pause_bits_from(lo - w * 64) & ~pause_bits_from(hi - w * 64);
}

// grid (words of the longest job / 4, jobs): wave v of a workgroup packs word blockIdx.x * 4 + v.
__global__ __launch_bounds__(kPauseThreads) void k_pause_flags(const float* __restrict__ x,
                                                               const PauseJob* __restrict__ jobs,
                                                               uint64_t* __restrict__ loud, int B, float threshold) {
  const PauseJob j = jobs[blockIdx.y];
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * kPauseWaves + (threadIdx.x >> 6);
  const int64_t L = j.nbk - j.fb;
  if (w * 64 >= L) return;  // (uniform over the wave; the kernel has no barrier)
  const int64_t k0 = j.fb + w * 64;
  const int64_t s0 = k0 * B;
  const int64_t s1 = pmin<int64_t>((k0 + pmin<int64_t>(64, L - w * 64)) * B, j.n_end);
  const int64_t len = s1 - s0;           // > 0: block k0 exists
  const int64_t nvec = (len + 3) >> 2;   // the last vector may pass `len` by up to 3 samples: masked below,
                                         // and the host pads the input array so the load stays inside it
  const float4* __restrict__ xv = reinterpret_cast<const float4*>(x + j.in_off + (s0 - j.in_first));
  const int lpb = B >> 2;                // vectors per block: a vector never straddles two blocks
  uint64_t word = 0;
  for (int64_t v0 = 0; v0 < nvec; v0 += 4 * 64) {
    float4 f[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {  // four loads in flight ahead of the compares
      const int64_t v = v0 + u * 64 + lane;
      f[u] = v < nvec ? xv[v] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t vb = v0 + u * 64;
      if (vb >= nvec) break;  // (uniform)
      const int64_t i = (vb + lane) * 4;
      const bool ld = (i < len && fabsf(f[u].x) > threshold) || (i + 1 < len && fabsf(f[u].y) > threshold) ||
                      (i + 2 < len && fabsf(f[u].z) > threshold) || (i + 3 < len && fabsf(f[u].w) > threshold);
      const uint64_t m = __ballot(ld);  // (false for NaN and for a lane past the span)
      if (m == 0) continue;
      const int64_t b_first = vb / lpb, b_last = pmin<int64_t>(vb + 63, nvec - 1) / lpb;
      for (int64_t b = b_first; b <= b_last; ++b)  // the lanes of block b among these 64 vectors
        if (m & pause_range(0, b * lpb - vb, (b + 1) * lpb - vb)) word |= 1ull << b;
    }
  }
  if (lane == 0) loud[j.w_off + w] = word;
}

// What the rule makes of the run that starts at local block l (carried: the run of the state, which
// started q samples before block c). Returns false if nothing is removed.
struct PauseRun {
  int64_t a, b, flags;
  bool open;
  int64_t R;
};
__device__ inline bool pause_eval(const PauseJob& j, const uint64_t* __restrict__ ac, int64_t Wn, int B, int F,
                                  int64_t l, bool carried, PauseRun* out) {
  const int64_t l1 = j.kd - j.fb;
  int64_t ww = l >> 6;
  uint64_t m = ac[ww] & pause_bits_from(l & 63);
  while (m == 0 && ++ww < Wn) m = ac[ww];
  const int64_t le = m ? ww * 64 + __builtin_ctzll(m) : l1;  // (no active bit at or above l1: masked off)
  const bool after = le < l1;
  const int64_t s = carried ? j.c * B - j.q : (j.fb + l) * B;
  const bool before = carried ? j.seen != 0 : true;
  const int64_t e = pmin<int64_t>((j.fb + le) * B, j.n_end);
  const int64_t R = e - s, hd = j.M - j.M / 2, tl = j.M / 2;
  out->open = false;
  out->R = R;
  if (after) {
    if (before) {
      if (R <= j.M) return false;
      out->a = s + hd, out->b = e - tl, out->flags = kPauseFadeIn | kPauseFadeOut | kPauseCounted;
    } else {
      if (R <= tl) return false;
      out->a = s, out->b = e - tl, out->flags = kPauseFadeIn | kPauseCounted;
    }
    return true;
  }
  if (j.final) {
    if (before) {
      if (R <= hd) return false;
      out->a = s + hd, out->b = e, out->flags = kPauseFadeOut | kPauseCounted;
    } else {  // no active block in the whole signal
      out->a = s, out->b = e, out->flags = kPauseCounted;
    }
    return out->b > out->a;
  }
  // the run goes on behind what is decided: what may go out now is out, the rest waits
  out->open = true;
  if (before) {
    const bool cut = R > j.M;  // certain, whatever follows
    out->a = s + (cut ? hd : pmin<int64_t>(R, hd - F)), out->b = e, out->flags = cut ? kPauseFadeOut : 0;
  } else {
    out->a = s, out->b = e, out->flags = 0;
  }
  if (out->a < j.p0) out->a = j.p0;  // (a carried head that went out earlier)
  return out->b > out->a;
}

// grid (jobs), one workgroup each.
__global__ __launch_bounds__(kPauseThreads) void k_pause_plan(const PauseJob* __restrict__ jobs,
                                                              const uint64_t* __restrict__ loud,
                                                              uint64_t* __restrict__ act, PauseCut* __restrict__ cuts,
                                                              PauseRes* __restrict__ res, int B, int H, int F) {
  __shared__ int64_t s_cnt[kPauseThreads], s_rem[kPauseThreads], s_cc[kPauseThreads];
  const PauseJob j = jobs[blockIdx.x];
  const int tid = threadIdx.x;
  const int64_t L = j.nbk - j.fb, Wn = (L + 63) >> 6;
  const int64_t l0 = j.c - j.fb, l1 = j.kd - j.fb;
  const uint64_t* __restrict__ ld = loud + j.w_off;
  uint64_t* __restrict__ ac = act + j.w_off;
  // active = loud dilated by H, kept for the blocks this call decides
  int any = 0;
  for (int64_t w = tid; w < Wn; w += kPauseThreads) {
    const uint64_t cur = ld[w], prev = w ? ld[w - 1] : 0, next = w + 1 < Wn ? ld[w + 1] : 0;
    uint64_t a = cur;
    for (int d = 1; d <= H; ++d) a |= (cur << d) | (prev >> (64 - d)) | (cur >> d) | (next << (64 - d));
    a &= pause_range(w, l0, l1);
    ac[w] = a;
    any |= a != 0;
  }
  if (tid == 0) {  // (the lane that finds the open run writes q after the barrier)
    res[blockIdx.x].c = j.kd;
    res[blockIdx.x].q = 0;
  }
  any = __syncthreads_or(any);  // (also makes the words visible to the workgroup)
  PauseCut* __restrict__ ct = cuts + j.cut_off;
  int64_t c_cnt = 0, c_rem = 0, c_cc = 0;  // carried over the passes
  for (int64_t base = 0; base < Wn; base += kPauseThreads) {
    const int64_t w = base + tid;
    uint64_t starts = 0;
    bool first = false;
    if (w < Wn) {
      const uint64_t a = ac[w];
      starts = ~a & ((a << 1) | (w ? ac[w - 1] >> 63 : 0)) & pause_range(w, l0 + 1, l1);
      // block c opens the walk: the run of the state, or a run that starts there
      first = w == (l0 >> 6) && (j.q > 0 || (l0 < l1 && !((a >> (l0 & 63)) & 1)));
    }
    // pass 1 counts, pass 2 writes: a run is followed twice, and nothing is kept in between
    int64_t cnt = 0, rem = 0, cc = 0;
    PauseRun r;
    if (first && pause_eval(j, ac, Wn, B, F, l0, true, &r)) cnt += 1, rem += r.b - r.a, cc += (r.flags & kPauseCounted) != 0;
    for (uint64_t m = starts; m; m &= m - 1)
      if (pause_eval(j, ac, Wn, B, F, w * 64 + __builtin_ctzll(m), false, &r))
        cnt += 1, rem += r.b - r.a, cc += (r.flags & kPauseCounted) != 0;
    s_cnt[tid] = cnt, s_rem[tid] = rem, s_cc[tid] = cc;
    __syncthreads();
    for (int d = 1; d < kPauseThreads; d <<= 1) {  // inclusive scan of the lanes' sums
      const int64_t v0 = tid >= d ? s_cnt[tid - d] : 0, v1 = tid >= d ? s_rem[tid - d] : 0,
                    v2 = tid >= d ? s_cc[tid - d] : 0;
      __syncthreads();
      s_cnt[tid] += v0, s_rem[tid] += v1, s_cc[tid] += v2;
      __syncthreads();
    }
    int64_t at = c_cnt + s_cnt[tid] - cnt, gone = c_rem + s_rem[tid] - rem;
    auto put = [&](const PauseRun& r) {
      if (at < j.cut_cap) ct[at] = PauseCut{r.a - j.p0 - gone, gone + (r.b - r.a), r.a, r.b, r.flags};
      at += 1;
      gone += r.b - r.a;
    };
    if (first) {
      const bool cut = pause_eval(j, ac, Wn, B, F, l0, true, &r);
      if (cut) put(r);
      if (r.open) res[blockIdx.x].q = r.R;
    }
    for (uint64_t m = starts; m; m &= m - 1) {
      const bool cut = pause_eval(j, ac, Wn, B, F, w * 64 + __builtin_ctzll(m), false, &r);
      if (cut) put(r);
      if (r.open) res[blockIdx.x].q = r.R;
    }
    c_cnt += s_cnt[kPauseThreads - 1], c_rem += s_rem[kPauseThreads - 1], c_cc += s_cc[kPauseThreads - 1];
    __syncthreads();  // the scan arrays are written again
  }
  if (tid == 0) {
    res[blockIdx.x].n_out = j.end - j.p0 - c_rem;
    res[blockIdx.x].n_cuts = c_cc;
    res[blockIdx.x].n_rec = pmin<int64_t>(c_cnt, j.cut_cap);
    res[blockIdx.x].seen = (j.seen || any) ? 1 : 0;
  }
}

// grid (tiles of the largest capacity bound, jobs): outputs [blockIdx.x * 1024, + 1024) of a job.
__global__ __launch_bounds__(kPauseThreads) void k_pause_gather(const float* __restrict__ x,
                                                                const float* __restrict__ ramp,
                                                                const PauseJob* __restrict__ jobs,
                                                                const PauseCut* __restrict__ cuts,
                                                                const PauseRes* __restrict__ res,
                                                                float* __restrict__ y, int F) {
  const PauseJob j = jobs[blockIdx.y];
  const int64_t n_out = pmin<int64_t>(res[blockIdx.y].n_out, j.out_cap), n_rec = res[blockIdx.y].n_rec;
  const int64_t o0 = (int64_t)blockIdx.x * kPauseTile;
  if (o0 >= n_out) return;
  const PauseCut* __restrict__ ct = cuts + j.cut_off;
  int64_t lo = 0, hi = n_rec;  // the cuts that land at or before o0 (uniform over the workgroup)
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (ct[mid].d <= o0) lo = mid + 1;
    else hi = mid;
  }
  int64_t jj = lo;
  for (int k = 0; k < kPauseTile / kPauseThreads; ++k) {
    const int64_t o = o0 + k * kPauseThreads + threadIdx.x;
    if (o >= n_out) break;
    while (jj < n_rec && ct[jj].d <= o) ++jj;
    const int64_t idx = j.p0 + o + (jj ? ct[jj - 1].r : 0);
    float v = (idx >= j.in_first && idx < j.n_end) ? x[j.in_off + (idx - j.in_first)] : 0.0f;
    if (jj && (ct[jj - 1].flags & kPauseFadeIn) && (uint64_t)(idx - ct[jj - 1].b) < (uint64_t)F) v = __fmul_rn(v, ramp[idx - ct[jj - 1].b]);
    else if (jj < n_rec && (ct[jj].flags & kPauseFadeOut) && (uint64_t)(ct[jj].a - 1 - idx) < (uint64_t)F)
      v = __fmul_rn(v, ramp[ct[jj].a - 1 - idx]);
    y[j.out_off + o] = v;
  }
}

// ---- host: configuration, ramp, the stream plan ------------------------------------------------
static int pause_config(const rwkvtts_pause_desc* d, PauseCfg* c, const char* who) {
  RT_CHECK(d && d->struct_size >= sizeof(rwkvtts_pause_desc), RWKVTTS_EINVAL,
           std::string(who) + ": null desc or struct_size too small");
  c->B = d->block ? d->block : 160;
  c->H = d->hang ? d->hang : 5;
  c->F = d->fade ? d->fade : 80;
  RT_CHECK(d->threshold >= 0.0f && d->threshold <= 3.0e38f, RWKVTTS_EINVAL,  // (NaN and inf fail)
           std::string(who) + ": threshold must be finite and >= 0 (0 = 0.01)");
  c->threshold = d->threshold == 0.0f ? 0.01f : d->threshold;
  RT_CHECK(c->B >= 4 && c->B <= 4096 && c->B % 4 == 0, RWKVTTS_EINVAL,
           std::string(who) + ": block must be a multiple of 4, 4 .. 4096 (0 = 160)");
  RT_CHECK(c->H >= 1 && c->H <= kPauseMaxHang, RWKVTTS_EINVAL, std::string(who) + ": hang must be 1 .. 32 (0 = 5)");
  RT_CHECK(c->F >= 1 && c->F <= kPauseMaxFade, RWKVTTS_EINVAL, std::string(who) + ": fade must be 1 .. 4096 (0 = 80)");
  return RWKVTTS_OK;
}

static void pause_make_ramp(const PauseCfg& c, float* out) {
  for (int k = 0; k < c.F; ++k) out[k] = (float)(((double)k + 0.5) / (double)c.F);
}

// p of the header: the first sample a window in state (c, seen, q) may still send
static int64_t pause_pending(const PauseCfg& c, int64_t M, int64_t blk, int seen, int64_t q) {
  const int64_t hd = M - M / 2, tl = M / 2, at = blk * c.B;
  if (q == 0) return at;
  if (seen) return q > M ? at - tl : at - q + std::min<int64_t>(q, hd - c.F);
  return q > tl ? at - tl : at - q;
}
static int64_t pause_first_needed(const PauseCfg& c, int64_t M, int64_t blk, int seen, int64_t q) {
  return std::max<int64_t>(0, std::min(pause_pending(c, M, blk, seen, q), (blk - c.H) * c.B));
}

struct PauseWin {
  const float* in;
  int64_t in_first, n_in;
  int final;
  int64_t M, c, q;
  int seen;
  float* out;
  int64_t out_cap;
  int64_t *out_count, *n_cuts, *c_last, *q_last, *first_needed;
  int32_t* seen_last;
  bool work;
};

}  // namespace rwkvtts

using namespace rwkvtts;

struct rwkvtts_pause : Stage<PauseJob> {  // d_table: the ramp
  PauseCfg cfg;
  DevBuf<uint64_t> d_words;  // loud[words], then act[words]
  DevBuf<PauseCut> d_cuts;
  DevBuf<PauseRes> d_res;
  std::vector<PauseRes> res;
};

// Checks every window, then runs those that decide something: one launch each of flags, plan and
// gather. Nothing is launched and nothing written unless every window passes.
static int pause_run(rwkvtts_pause* p, std::vector<PauseWin>& ws, const char* who) {
  const PauseCfg& c = p->cfg;
  for (PauseWin& w : ws) {
    RT_CHECK(w.M >= 2 * (int64_t)c.F && w.M <= kPauseMaxSamples, RWKVTTS_EINVAL,
             std::string(who) + ": max_pause_samples must be 2 * fade .. 2^30");
    RT_CHECK(w.in_first >= 0 && w.n_in >= 0 && w.in_first + w.n_in <= kPauseMaxSamples && w.out_cap >= 0 &&
                 (w.in || w.n_in == 0) && (w.out || w.out_cap == 0),
             RWKVTTS_EINVAL, std::string(who) + ": bad window (negative size, null buffer or too long)");
    const bool state_ok = w.c >= 0 && (w.seen == 0 || w.seen == 1) && w.q >= 0 && w.q % c.B == 0 &&
                          (w.seen ? (w.c >= 1 && w.q <= (w.c - 1) * c.B) : w.q == w.c * c.B);
    RT_CHECK(state_ok, RWKVTTS_EINVAL, std::string(who) + ": (block_next, seen, quiet) is no state a scan can have left");
    const int64_t n = w.in_first + w.n_in;
    RT_CHECK(w.c * c.B <= n, RWKVTTS_EINVAL, std::string(who) + ": the samples end before block_next");
    RT_CHECK(w.in_first <= pause_first_needed(c, w.M, w.c, w.seen, w.q), RWKVTTS_EINVAL,
             std::string(who) + ": the samples start after in_first_needed");
    const int64_t nbk = w.final ? (n + c.B - 1) / c.B : n / c.B;
    const int64_t kd = w.final ? nbk : std::max(w.c, nbk - c.H);
    w.work = kd > w.c || (w.final && w.q > 0);
    if (!w.work) continue;
    const int64_t end = w.final ? n : kd * c.B;
    RT_CHECK(w.out_cap >= end - pause_pending(c, w.M, w.c, w.seen, w.q), RWKVTTS_EINVAL,
             std::string(who) + ": out_cap below what the window can decide");
  }
  auto finish = [&](const PauseWin& w, int64_t count, int64_t cuts, int64_t blk, int seen, int64_t q) {
    if (w.out_count) *w.out_count = count;
    if (w.n_cuts) *w.n_cuts = cuts;
    if (w.c_last) *w.c_last = blk;
    if (w.seen_last) *w.seen_last = seen;
    if (w.q_last) *w.q_last = q;
    if (w.first_needed) *w.first_needed = pause_first_needed(c, w.M, blk, seen, q);
  };
  std::lock_guard<std::mutex> lock(p->mu);
  p->desc.clear();
  int64_t in_cur = 0, out_off = 0, w_off = 0, cut_off = 0, max_words = 0, max_bound = 0;
  for (const PauseWin& w : ws) {
    if (!w.work) continue;
    const int64_t n = w.in_first + w.n_in;
    PauseJob j;
    j.in_off = ((in_cur + 3) & ~(int64_t)3) + (w.in_first & 3);
    j.in_first = w.in_first;
    j.n_end = n;
    j.fb = std::max<int64_t>(0, w.c - c.H);
    j.nbk = w.final ? (n + c.B - 1) / c.B : n / c.B;
    j.c = w.c;
    j.kd = w.final ? j.nbk : std::max(w.c, j.nbk - c.H);
    j.q = w.q;
    j.M = w.M;
    const int64_t hd = w.M - w.M / 2;
    j.p0 = w.c * c.B - w.q + (w.seen && w.q > 0 ? (w.q > w.M ? hd : std::min<int64_t>(w.q, hd - c.F)) : 0);
    j.end = w.final ? n : j.kd * c.B;
    const int64_t L = j.nbk - j.fb, words = (L + 63) / 64;
    j.w_off = w_off;
    j.cut_off = cut_off;
    j.cut_cap = L / 2 + 3;  // a cut per run at most, runs lie between active blocks, and the state's run
    j.out_off = out_off;
    j.out_cap = j.end - pause_pending(c, w.M, w.c, w.seen, w.q);  // <= the caller's, checked above
    j.seen = w.seen;
    j.final = w.final;
    p->desc.push_back(j);
    in_cur = j.in_off + w.n_in;
    const int64_t bound = j.end - pause_pending(c, w.M, w.c, w.seen, w.q);
    out_off += bound;
    w_off += words;
    cut_off += j.cut_cap;
    max_words = std::max(max_words, words);
    max_bound = std::max(max_bound, bound);
  }
  const size_t n_jobs = p->desc.size();
  if (n_jobs == 0) {
    for (const PauseWin& w : ws) finish(w, 0, 0, w.c, w.seen, w.q);
    return RWKVTTS_OK;
  }
  const int64_t tiles = (max_bound + kPauseTile - 1) / kPauseTile;
  RT_CHECK(n_jobs <= 65535 && tiles <= 0x7fffffff, RWKVTTS_EINVAL, std::string(who) + ": too much for one launch");
  int rc;
  // (+ 8: the last 16-byte load of a signal may pass its end, and stays inside the array)
  if ((rc = stage_reserve(p, in_cur + 8, std::max<int64_t>(out_off, 1))) || (rc = p->d_words.reserve((size_t)(2 * w_off))) ||
      (rc = p->d_cuts.reserve((size_t)cut_off)) || (rc = p->d_res.reserve(n_jobs)))
    return rc;
  {
    size_t k = 0;
    for (const PauseWin& w : ws) {
      if (!w.work) continue;
      if (w.n_in > 0)
        RT_HIP(hipMemcpyAsync(p->d_in.p + p->desc[k].in_off, w.in, (size_t)w.n_in * sizeof(float), hipMemcpyHostToDevice,
                              p->stream));
      ++k;
    }
  }
  RT_HIP(hipMemcpyAsync(p->d_desc.p, p->desc.data(), n_jobs * sizeof(PauseJob), hipMemcpyHostToDevice, p->stream));
  uint64_t* d_loud = p->d_words.p;
  uint64_t* d_act = p->d_words.p + w_off;
  // the event pair brackets all three kernels: start of the flags, end of the gather
  hipExtLaunchKernelGGL(k_pause_flags, dim3((unsigned)((max_words + kPauseWaves - 1) / kPauseWaves), (unsigned)n_jobs),
                        dim3(kPauseThreads), 0, p->stream, p->ev0, nullptr, 0u, p->d_in.p, p->d_desc.p, d_loud, c.B,
                        c.threshold);
  RT_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_pause_plan, dim3((unsigned)n_jobs), dim3(kPauseThreads), 0, p->stream, p->d_desc.p, d_loud, d_act,
                     p->d_cuts.p, p->d_res.p, c.B, c.H, c.F);
  RT_HIP(hipGetLastError());
  hipExtLaunchKernelGGL(k_pause_gather, dim3((unsigned)std::max<int64_t>(tiles, 1), (unsigned)n_jobs), dim3(kPauseThreads), 0,
                        p->stream, nullptr, p->ev1, 0u, p->d_in.p, p->d_table, p->d_desc.p, p->d_cuts.p, p->d_res.p,
                        p->d_out.p, c.F);
  RT_HIP(hipGetLastError());
  // the counts first: the host cannot know n_out before the plan has run
  p->res.assign(n_jobs, PauseRes{0, 0, 0, 0, 0, 0});
  RT_HIP(hipMemcpyAsync(p->res.data(), p->d_res.p, n_jobs * sizeof(PauseRes), hipMemcpyDeviceToHost, p->stream));
  RT_HIP(hipStreamSynchronize(p->stream));
  for (size_t k = 0; k < n_jobs; ++k)
    RT_CHECK(p->res[k].n_out >= 0 && p->res[k].n_out <= p->desc[k].out_cap, RWKVTTS_EHIP,
             std::string(who) + ": the plan kernel left an impossible count");
  {
    size_t k = 0;
    for (const PauseWin& w : ws) {
      if (!w.work) continue;
      if (p->res[k].n_out > 0)
        RT_HIP(hipMemcpyAsync(w.out, p->d_out.p + p->desc[k].out_off, (size_t)p->res[k].n_out * sizeof(float),
                              hipMemcpyDeviceToHost, p->stream));
      ++k;
    }
  }
  RT_HIP(hipStreamSynchronize(p->stream));
  float ms = 0.0f;
  if (hipEventElapsedTime(&ms, p->ev0, p->ev1) == hipSuccess) p->kernel_ms = (double)ms;
  size_t k = 0;
  for (const PauseWin& w : ws) {
    if (!w.work) {
      finish(w, 0, 0, w.c, w.seen, w.q);
      continue;
    }
    const PauseRes& r = p->res[k++];
    finish(w, r.n_out, r.n_cuts, r.c, (int)r.seen, r.q);
  }
  return RWKVTTS_OK;
}

extern "C" int rwkvtts_pause_ramp(const rwkvtts_pause_desc* desc, float* out) {
  PauseCfg c;
  int rc = pause_config(desc, &c, "pause_ramp");
  if (rc) return rc;
  RT_CHECK(out, RWKVTTS_EINVAL, "pause_ramp: null output");
  pause_make_ramp(c, out);
  return RWKVTTS_OK;
}

extern "C" int rwkvtts_pause_create(int device, const rwkvtts_pause_desc* desc, const float* table, rwkvtts_pause** out) {
  RT_CHECK(out, RWKVTTS_EINVAL, "pause_create: null output");
  *out = nullptr;
  PauseCfg c;
  int rc = pause_config(desc, &c, "pause_create");
  if (rc) return rc;
  rwkvtts_pause* p = nullptr;
  rc = stage_create("pause_create", device, table, (size_t)c.F, [&](float* r) { pause_make_ramp(c, r); }, &p);
  if (rc) return rc;
  p->cfg = c;
  *out = p;
  return RWKVTTS_OK;
}

extern "C" int rwkvtts_pause_destroy(rwkvtts_pause* p) {
  if (!p) return RWKVTTS_OK;
  (void)hipSetDevice(p->device);
  stage_free(p, {p->d_words.p, p->d_cuts.p, p->d_res.p});
  return RWKVTTS_OK;
}

extern "C" int rwkvtts_pause_batch(rwkvtts_pause* p, const float* const* in, const int64_t* n_in,
                                   const int64_t* max_pause_samples, int n, float* const* out, int64_t* n_out,
                                   int64_t* n_cuts) {
  RT_CHECK(p && n >= 0 && (n == 0 || (in && n_in && max_pause_samples && out && n_out)), RWKVTTS_EINVAL,
           "pause_batch: bad arguments");
  return guard_alloc("pause_batch", [&] {
    std::vector<PauseWin> ws((size_t)n);
    for (int i = 0; i < n; ++i) {
      RT_CHECK(n_in[i] >= 0 && n_in[i] <= kPauseMaxSamples, RWKVTTS_EINVAL, "pause_batch: n_in out of range");
      ws[(size_t)i] = PauseWin{in[i], 0, n_in[i], 1, max_pause_samples[i], 0, 0, 0, out[i], n_in[i], n_out + i,
                               n_cuts ? n_cuts + i : nullptr, nullptr, nullptr, nullptr, nullptr, false};
    }
    return pause_run(p, ws, "pause_batch");
  });
}

extern "C" int rwkvtts_pause_windows(rwkvtts_pause* p, rwkvtts_pause_window* w, int n) {
  RT_CHECK(p && n >= 0 && (n == 0 || w), RWKVTTS_EINVAL, "pause_windows: bad arguments");
  if (n == 0) return RWKVTTS_OK;
  return guard_alloc("pause_windows", [&] {
    std::vector<PauseWin> ws;
    int rc = read_windows("pause_windows", w, n, ws, [](rwkvtts_pause_window* wi) {
      return PauseWin{wi->in, wi->in_first, wi->n_in, wi->final ? 1 : 0, wi->max_pause_samples, wi->block_next, wi->quiet,
                      wi->seen, wi->out, wi->out_cap, &wi->out_count, &wi->n_cuts, &wi->block_last, &wi->quiet_last,
                      &wi->in_first_needed, &wi->seen_last, false};
    });
    return rc ? rc : pause_run(p, ws, "pause_windows");
  });
}

extern "C" int rwkvtts_pause_kernel_ms(rwkvtts_pause* p, double* ms) { return stage_kernel_ms("pause_kernel_ms", p, ms); }
