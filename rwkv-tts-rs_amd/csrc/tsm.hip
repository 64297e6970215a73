// tsm.hip -- pitch-preserving time-scale modification (WSOLA: waveform-similarity overlap-add) on
// the MI355X, for the `tempo` keyword of the pipeline: one-shot, batched (a tempo per signal) and
// over exact stream windows. No reference counterpart: the reference's only rate control is the
// five-bucket `speed` property token, which a cloned voice does not get.
//
// The arithmetic contract is in include/rwkvtts.h: frame positions from one IEEE
// double multiply, the similarity measure a sequential f32 sum of squared differences in ascending
// order from +0 (one rounded subtract, multiply and add per term, never fused, no division, no
// square root), the winner the unsigned 64-bit minimum of (f32 bits of d, rank), the output two
// rounded multiplies and one rounded add. The kernels are pinned bitwise to a numpy restatement of
// exactly that (tests/test_gpu_tsm.py).
//
// Work: k_tsm_search gives one workgroup to a signal (or stream window) and walks its frames in
// order -- frame m's template is cut from where frame m-1 landed, so the chain over m is inherent.
// Per frame the workgroup holds the template and the candidates' span (zeros outside the signal)
// in LDS, a lane runs the Hs-step chain of each candidate it owns (lanes stride over the 2D
// candidates), and a shuffle + LDS reduction of the 64-bit keys picks the shift. Starts go to a
// device array; k_tsm_ola then gives a lane to every output sample.
// Parallelism across utterances comes from the batch alone: that cost is accepted.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <new>
#include <vector>

#include "common.h"
#include "stage.h"

// frame positions are shared by the host plan and the kernels: no contraction anywhere
#pragma clang fp contract(off)

namespace rwkvtts {

constexpr int kTsmThreads = 256;
constexpr int kTsmWaves = kTsmThreads / 64;
constexpr int kTsmPre = 16;  // samples of a frame's buffer per lane at the widest: (2 * 1024 + 2048) / 256
constexpr int64_t kTsmMaxSamples = (int64_t)1 << 40;  // m * Hs * tempo stays far inside double's exact integers

struct TsmCfg {
  int W, Hs, D;
};

// a_m = floor((double)(m * Hs) * tempo): one rounded double multiply, on both sides
__host__ __device__ inline int64_t tsm_anchor(int64_t m, int Hs, double tempo) {
#ifdef __HIP_DEVICE_COMPILE__
  return (int64_t)floor(__dmul_rn((double)(m * Hs), tempo));
#else
  const double p = (double)(m * Hs) * tempo;
  return (int64_t)floor(p);
#endif
}

// One workgroup of k_tsm_search, one grid row of k_tsm_ola: blocks [m_first, m_first + m_count) of
// one signal. The given samples are signal indices [in_first, in_end), stored at x[in_off ...];
// every other index reads as zero (the host has checked that those are below 0 or, for a final
// window, past the end). starts[st_off + b] is the start of frame m_first - 1 + b.
struct TsmJob {
  int64_t in_off, in_first, in_end;
  int64_t m_first, m_count, s_prev;
  int64_t st_off, out_off, out_count;
  double tempo;
};

__device__ inline float tsm_x(const float* __restrict__ x, const TsmJob& j, int64_t idx) {
  return (idx >= j.in_first && idx < j.in_end) ? x[j.in_off + (idx - j.in_first)] : 0.0f;
}

// One candidate's chain: d = sum_i (t[i] - c[i])^2 in ascending i from +0. The LDS reads of eight
// steps are issued together (their latency would otherwise sit on every step); the arithmetic is
// the same three rounded operations per step, in the same order.
__device__ inline float tsm_chain(const float* __restrict__ t, const float* __restrict__ c, int Hs) {
  float d = 0.0f;
  int i = 0;
  for (; i + 8 <= Hs; i += 8) {
    float tv[8], cv[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      tv[k] = t[i + k];
      cv[k] = c[i + k];
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float e = __fsub_rn(tv[k], cv[k]);
      d = __fadd_rn(d, __fmul_rn(e, e));
    }
  }
  for (; i < Hs; ++i) {
    const float e = __fsub_rn(t[i], c[i]);
    d = __fadd_rn(d, __fmul_rn(e, e));
  }
  return d;
}

// LDS: two buffers of E = 2D + 2Hs samples. The buffer of frame m holds x[a_m - D, a_m + D + 2Hs):
// its first 2D + Hs samples are frame m's candidates, and frame m+1's template, Hs samples from
// s_m + Hs with s_m in [a_m - D, a_m + D), lies inside it wherever the search lands. So the next
// frame's buffer depends on no search result: it is fetched into registers before the chains run
// and stored after them, and no global load waits on the chain over m.
__global__ __launch_bounds__(kTsmThreads) void k_tsm_search(const float* __restrict__ x,
                                                            const TsmJob* __restrict__ jobs,
                                                            int64_t* __restrict__ starts, int Hs, int D) {
  extern __shared__ float s_mem[];
  __shared__ unsigned long long s_red[kTsmWaves];
  const TsmJob j = jobs[blockIdx.x];
  const int tid = threadIdx.x;
  const int E = 2 * D + 2 * Hs;  // at most kTsmPre * kTsmThreads
  int64_t s_prev = j.s_prev;
  if (tid == 0) starts[j.st_off] = s_prev;
  int64_t m = j.m_first;
  const int64_t m_end = j.m_first + j.m_count;
  if (m == 0 && m < m_end) {  // frame 0 starts at 0: nothing to search
    s_prev = 0;
    if (tid == 0) starts[j.st_off + 1] = 0;
    m = 1;
  }
  if (m >= m_end) return;  // (uniform over the workgroup)
  float* b_prev = s_mem;      // frame m-1's buffer; before the first search, x[s_prev - D ...)
  float* b_cur = s_mem + E;   // frame m's
  int64_t base_prev = s_prev - D;
  int64_t a = tsm_anchor(m, Hs, j.tempo);
  for (int i = tid; i < E; i += kTsmThreads) {
    b_prev[i] = tsm_x(x, j, base_prev + i);
    b_cur[i] = tsm_x(x, j, a - D + i);
  }
  __syncthreads();
  for (; m < m_end; ++m) {
    const int64_t a_next = tsm_anchor(m + 1, Hs, j.tempo);
    float pre[kTsmPre];
    if (m + 1 < m_end) {
#pragma unroll
      for (int k = 0; k < kTsmPre; ++k) {
        const int i = k * kTsmThreads + tid;
        pre[k] = i < E ? tsm_x(x, j, a_next - D + i) : 0.0f;
      }
    }
    const float* tp = b_prev + (int)(s_prev + Hs - base_prev);
    unsigned long long best = ~0ull;
    for (int c = tid; c < 2 * D; c += kTsmThreads) {  // candidate c: shift c - D
      const float d = tsm_chain(tp, b_cur + c, Hs);
      const int delta = c - D;
      const unsigned rank = delta < 0 ? (unsigned)(-2 * delta - 1) : (unsigned)(2 * delta);
      const unsigned bits = (d != d) ? 0x7f800000u : __float_as_uint(d);  // NaN counts as +inf
      const unsigned long long key = ((unsigned long long)bits << 32) | rank;
      best = key < best ? key : best;
    }
    for (int off = 32; off >= 1; off >>= 1) {
      const unsigned lo = __shfl_xor((unsigned)best, off, 64);
      const unsigned hi = __shfl_xor((unsigned)(best >> 32), off, 64);
      const unsigned long long o = ((unsigned long long)hi << 32) | lo;
      best = o < best ? o : best;
    }
    if ((tid & 63) == 0) s_red[tid >> 6] = best;
    __syncthreads();  // every chain has left both buffers
    best = s_red[0];
    for (int w = 1; w < kTsmWaves; ++w) best = s_red[w] < best ? s_red[w] : best;
    const unsigned rank = (unsigned)best;
    const int delta = (rank & 1u) ? -(int)((rank + 1u) >> 1) : (int)(rank >> 1);
    s_prev = a + delta;
    if (tid == 0) starts[j.st_off + (m - j.m_first) + 1] = s_prev;
    if (m + 1 < m_end) {
#pragma unroll
      for (int k = 0; k < kTsmPre; ++k) {
        const int i = k * kTsmThreads + tid;
        if (i < E) b_prev[i] = pre[k];
      }
    }
    __syncthreads();  // the next frame's buffer is in place; s_red may be written again
    float* sw = b_prev;
    b_prev = b_cur;
    b_cur = sw;
    base_prev = a - D;
    a = a_next;
  }
}

// grid (blocks of the longest job, jobs): block b of job y, a lane per output sample.
__global__ __launch_bounds__(kTsmThreads) void k_tsm_ola(const float* __restrict__ x, const float* __restrict__ win,
                                                         const TsmJob* __restrict__ jobs,
                                                         const int64_t* __restrict__ starts, float* __restrict__ y,
                                                         int Hs) {
  const TsmJob j = jobs[blockIdx.y];
  const int64_t b = blockIdx.x;
  if (b >= j.m_count) return;
  const int64_t s_a = starts[j.st_off + b], s_b = starts[j.st_off + b + 1];
  for (int i = threadIdx.x; i < Hs; i += kTsmThreads) {
    const int64_t o = b * Hs + i;
    if (o >= j.out_count) return;
    const float p = __fmul_rn(win[Hs + i], tsm_x(x, j, s_a + Hs + i));
    const float q = __fmul_rn(win[i], tsm_x(x, j, s_b + i));
    y[j.out_off + o] = __fadd_rn(p, q);
  }
}

// ---- host: configuration, window, plan -------------------------------------------------------
static int tsm_config(const rwkvtts_tsm_desc* d, TsmCfg* c, const char* who) {
  RT_CHECK(d && d->struct_size >= sizeof(rwkvtts_tsm_desc), RWKVTTS_EINVAL,
           std::string(who) + ": null desc or struct_size too small");
  c->W = d->window ? d->window : 512;
  c->D = d->search ? d->search : 128;
  RT_CHECK(c->W >= 32 && c->W <= 2048 && c->W % 2 == 0, RWKVTTS_EINVAL,
           std::string(who) + ": window must be even, 32 .. 2048 (0 = 512)");
  RT_CHECK(c->D >= 1 && c->D <= 1024, RWKVTTS_EINVAL, std::string(who) + ": search must be 1 .. 1024 (0 = 128)");
  c->Hs = c->W / 2;
  return RWKVTTS_OK;
}

static int tsm_tempo_ok(double tempo, const char* who) {
  RT_CHECK(tempo >= 0.25 && tempo <= 4.0, RWKVTTS_EINVAL, std::string(who) + ": tempo must be 0.25 .. 4.0");  // (NaN fails)
  return RWKVTTS_OK;
}

static void tsm_make_window(const TsmCfg& c, float* out) {
  const double pi = 3.141592653589793;
  for (int i = 0; i < c.W; ++i) out[i] = (float)(0.5 - 0.5 * cos(2.0 * pi * (double)i / (double)c.W));
}

static inline int64_t tsm_out_len(double tempo, int64_t n) { return n <= 0 ? 0 : (int64_t)ceil((double)n / tempo); }

// s_{m} lies in [a_m - D, a_m + D) for m >= 1; s_0 = 0, s_-1 = -Hs
static bool tsm_start_possible(const TsmCfg& c, double tempo, int64_t m, int64_t s) {
  if (m == -1) return s == -c.Hs;
  if (m == 0) return s == 0;
  const int64_t a = tsm_anchor(m, c.Hs, tempo);
  return s >= a - c.D && s < a + c.D;
}

// One past the highest sample that block j can read, frame j-1 having started at s_before (its
// template and its earlier frame's products end at s_before + 2 Hs; its candidates and its own
// frame's products end below a_j + D + Hs - 1).
static inline int64_t tsm_need(const TsmCfg& c, double tempo, int64_t j, int64_t s_before) {
  if (j == 0) return c.Hs;
  return std::max<int64_t>(s_before + 2 * c.Hs, tsm_anchor(j, c.Hs, tempo) + c.D + c.Hs - 1);
}
// the same with frame j-1's start unknown: its highest possible value
static inline int64_t tsm_need_worst(const TsmCfg& c, double tempo, int64_t j) {
  if (j <= 1) return tsm_need(c, tempo, j, j == 1 ? 0 : -c.Hs);
  return tsm_need(c, tempo, j, tsm_anchor(j - 1, c.Hs, tempo) + c.D - 1);
}

// The end of the ready blocks from block_first on (a sample index): blocks ready are those whose
// reads lie below n_known and that lie wholly below out_len(n_known). Both conditions are monotone
// in the block index, so bisect.
static int64_t tsm_ready_end(const TsmCfg& c, double tempo, int64_t n_known, int final, int64_t bf, int64_t s_prev) {
  const int64_t cap = tsm_out_len(tempo, n_known);
  if (final) return cap;
  const int64_t jmax = cap / c.Hs;  // blocks [0, jmax) lie wholly below cap
  if (bf >= jmax || tsm_need(c, tempo, bf, s_prev) > n_known) return bf * c.Hs;
  int64_t lo = bf + 1, hi = jmax;  // the first block in (bf, jmax) that is not ready, or jmax
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (tsm_need_worst(c, tempo, mid) > n_known) hi = mid; else lo = mid + 1;
  }
  return lo * c.Hs;
}
static inline int64_t tsm_in_first_needed(const TsmCfg& c, double tempo, int64_t bf, int64_t s_prev) {
  return std::max<int64_t>(0, std::min<int64_t>(s_prev + c.Hs, tsm_anchor(bf, c.Hs, tempo) - c.D));
}

struct TsmWin {
  const float* in;
  int64_t in_first, n_in;
  int final;
  double tempo;
  int64_t block_first, s_prev, out_count;
  float* out;
  int64_t* s_last;
};

}  // namespace rwkvtts

using namespace rwkvtts;

struct rwkvtts_tsm : Stage<TsmJob> {  // d_table: the Hann window
  TsmCfg cfg;
  DevBuf<int64_t> d_starts;
  std::vector<int64_t> last;
};

// Checks every window against the plan, then runs them all: one search launch, one overlap-add
// launch. Nothing is launched and nothing written unless every window passes.
static int tsm_run(rwkvtts_tsm* t, const std::vector<TsmWin>& ws, const char* who) {
  const TsmCfg& c = t->cfg;
  int64_t tot_in = 0, tot_out = 0, tot_starts = 0, max_blocks = 0;
  size_t n_jobs = 0;
  int rc;
  for (const TsmWin& w : ws) {
    if ((rc = tsm_tempo_ok(w.tempo, who))) return rc;
    RT_CHECK(w.in_first >= 0 && w.n_in >= 0 && w.block_first >= 0 && w.out_count >= 0 &&
                 w.in_first + w.n_in <= kTsmMaxSamples && w.block_first <= kTsmMaxSamples / c.Hs &&
                 (w.in || w.n_in == 0) && (w.out || w.out_count == 0),
             RWKVTTS_EINVAL, std::string(who) + ": bad window (negative size, null buffer or too long)");
    RT_CHECK(tsm_start_possible(c, w.tempo, w.block_first - 1, w.s_prev), RWKVTTS_EINVAL,
             std::string(who) + ": s_prev is no possible start of frame block_first - 1 (-Hs for block 0)");
    if (w.out_count == 0) continue;
    RT_CHECK(w.block_first * c.Hs + w.out_count <=
                 tsm_ready_end(c, w.tempo, w.in_first + w.n_in, w.final, w.block_first, w.s_prev),
             RWKVTTS_EINVAL, std::string(who) + ": a requested block reads past the given samples");
    RT_CHECK(w.in_first <= tsm_in_first_needed(c, w.tempo, w.block_first, w.s_prev), RWKVTTS_EINVAL,
             std::string(who) + ": a requested block reads before the given samples");
    const int64_t blocks = (w.out_count + c.Hs - 1) / c.Hs;
    tot_in += w.n_in;
    tot_out += w.out_count;
    tot_starts += blocks + 1;
    max_blocks = std::max(max_blocks, blocks);
    ++n_jobs;
  }
  if (n_jobs == 0) {
    for (const TsmWin& w : ws)
      if (w.s_last) *w.s_last = w.s_prev;
    return RWKVTTS_OK;
  }
  RT_CHECK(n_jobs <= 65535 && max_blocks <= 0x7fffffff, RWKVTTS_EINVAL, std::string(who) + ": too much for one launch");
  std::lock_guard<std::mutex> lock(t->mu);
  t->desc.clear();
  t->last.assign(n_jobs, 0);
  int64_t in_off = 0, out_off = 0, st_off = 0;
  for (const TsmWin& w : ws) {
    if (w.out_count == 0) continue;
    TsmJob j;
    j.in_off = in_off;
    j.in_first = w.in_first;
    j.in_end = w.in_first + w.n_in;
    j.m_first = w.block_first;
    j.m_count = (w.out_count + c.Hs - 1) / c.Hs;
    j.s_prev = w.s_prev;
    j.st_off = st_off;
    j.out_off = out_off;
    j.out_count = w.out_count;
    j.tempo = w.tempo;
    t->desc.push_back(j);
    in_off += w.n_in;
    out_off += w.out_count;
    st_off += j.m_count + 1;
  }
  if ((rc = stage_reserve(t, tot_in, tot_out)) || (rc = t->d_starts.reserve((size_t)tot_starts)) ||
      (rc = stage_upload(t, ws)))
    return rc;
  // the event pair brackets both kernels: start of the search, end of the overlap-add
  const size_t lds = (size_t)2 * (size_t)(2 * c.D + 2 * c.Hs) * sizeof(float);  // 32 KB at the widest
  hipExtLaunchKernelGGL(k_tsm_search, dim3((unsigned)n_jobs), dim3(kTsmThreads), lds, t->stream, t->ev0, nullptr, 0u,
                        t->d_in.p, t->d_desc.p, t->d_starts.p, c.Hs, c.D);
  RT_HIP(hipGetLastError());
  hipExtLaunchKernelGGL(k_tsm_ola, dim3((unsigned)max_blocks, (unsigned)n_jobs), dim3(kTsmThreads), 0, t->stream,
                        nullptr, t->ev1, 0u, t->d_in.p, t->d_table, t->d_desc.p, t->d_starts.p, t->d_out.p, c.Hs);
  RT_HIP(hipGetLastError());
  for (size_t k = 0; k < n_jobs; ++k) {  // the start of each job's last frame
    const TsmJob& j = t->desc[k];
    RT_HIP(hipMemcpyAsync(&t->last[k], t->d_starts.p + j.st_off + j.m_count, sizeof(int64_t), hipMemcpyDeviceToHost,
                          t->stream));
  }
  if ((rc = stage_download(t, ws))) return rc;
  size_t k = 0;
  for (const TsmWin& w : ws) {
    if (w.s_last) *w.s_last = w.out_count == 0 ? w.s_prev : t->last[k];
    if (w.out_count != 0) ++k;
  }
  return RWKVTTS_OK;
}

extern "C" int rwkvtts_tsm_window(const rwkvtts_tsm_desc* desc, float* out) {
  TsmCfg c;
  int rc = tsm_config(desc, &c, "tsm_window");
  if (rc) return rc;
  RT_CHECK(out, RWKVTTS_EINVAL, "tsm_window: null output");
  tsm_make_window(c, out);
  return RWKVTTS_OK;
}

extern "C" int64_t rwkvtts_tsm_out_len(const rwkvtts_tsm_desc* desc, double tempo, int64_t n_in) {
  TsmCfg c;
  if (tsm_config(desc, &c, "tsm_out_len") || tsm_tempo_ok(tempo, "tsm_out_len")) return -1;
  if (n_in < 0 || n_in > kTsmMaxSamples) {
    set_error("tsm_out_len: n_in out of range");
    return -1;
  }
  return tsm_out_len(tempo, n_in);
}

extern "C" int rwkvtts_tsm_plan(const rwkvtts_tsm_desc* desc, double tempo, int64_t n_known, int final,
                                int64_t block_first, int64_t s_prev, int64_t* out_ready_end,
                                int64_t* in_first_needed) {
  TsmCfg c;
  int rc = tsm_config(desc, &c, "tsm_plan");
  if (rc || (rc = tsm_tempo_ok(tempo, "tsm_plan"))) return rc;
  RT_CHECK(n_known >= 0 && n_known <= kTsmMaxSamples && block_first >= 0 && block_first <= kTsmMaxSamples / c.Hs,
           RWKVTTS_EINVAL, "tsm_plan: n_known / block_first out of range");
  RT_CHECK(tsm_start_possible(c, tempo, block_first - 1, s_prev), RWKVTTS_EINVAL,
           "tsm_plan: s_prev is no possible start of frame block_first - 1 (-Hs for block 0)");
  if (out_ready_end) *out_ready_end = tsm_ready_end(c, tempo, n_known, final, block_first, s_prev);
  if (in_first_needed) *in_first_needed = tsm_in_first_needed(c, tempo, block_first, s_prev);
  return RWKVTTS_OK;
}

extern "C" int rwkvtts_tsm_create(int device, const rwkvtts_tsm_desc* desc, const float* table, rwkvtts_tsm** out) {
  RT_CHECK(out, RWKVTTS_EINVAL, "tsm_create: null output");
  *out = nullptr;
  TsmCfg c;
  int rc = tsm_config(desc, &c, "tsm_create");
  if (rc) return rc;
  rwkvtts_tsm* t = nullptr;
  rc = stage_create("tsm_create", device, table, (size_t)c.W, [&](float* w) { tsm_make_window(c, w); }, &t);
  if (rc) return rc;
  t->cfg = c;
  *out = t;
  return RWKVTTS_OK;
}

extern "C" int rwkvtts_tsm_destroy(rwkvtts_tsm* t) {
  if (!t) return RWKVTTS_OK;
  (void)hipSetDevice(t->device);
  stage_free(t, {t->d_starts.p});
  return RWKVTTS_OK;
}

extern "C" int rwkvtts_tsm_batch(rwkvtts_tsm* t, const float* const* in, const int64_t* n_in, const double* tempo,
                                 int n, float* const* out) {
  RT_CHECK(t && n >= 0 && (n == 0 || (in && n_in && tempo && out)), RWKVTTS_EINVAL, "tsm_batch: bad arguments");
  return guard_alloc("tsm_batch", [&] {
    std::vector<TsmWin> ws((size_t)n);
    for (int i = 0; i < n; ++i) {
      int rc = tsm_tempo_ok(tempo[i], "tsm_batch");
      if (rc) return rc;
      RT_CHECK(n_in[i] >= 0 && n_in[i] <= kTsmMaxSamples, RWKVTTS_EINVAL, "tsm_batch: n_in out of range");
      ws[(size_t)i] = TsmWin{in[i], 0, n_in[i], 1, tempo[i], 0, -(int64_t)t->cfg.Hs, tsm_out_len(tempo[i], n_in[i]),
                             out[i], nullptr};
    }
    return tsm_run(t, ws, "tsm_batch");
  });
}

extern "C" int rwkvtts_tsm_windows(rwkvtts_tsm* t, rwkvtts_tsm_window_t* w, int n) {
  RT_CHECK(t && n >= 0 && (n == 0 || w), RWKVTTS_EINVAL, "tsm_windows: bad arguments");
  if (n == 0) return RWKVTTS_OK;
  return guard_alloc("tsm_windows", [&] {
    std::vector<TsmWin> ws;
    int rc = read_windows("tsm_windows", w, n, ws, [](rwkvtts_tsm_window_t* wi) {
      return TsmWin{wi->in, wi->in_first, wi->n_in, wi->final ? 1 : 0, wi->tempo, wi->block_first,
                    wi->s_prev, wi->out_count, wi->out, &wi->s_last};
    });
    return rc ? rc : tsm_run(t, ws, "tsm_windows");
  });
}

extern "C" int rwkvtts_tsm_kernel_ms(rwkvtts_tsm* t, double* ms) { return stage_kernel_ms("tsm_kernel_ms", t, ms); }
