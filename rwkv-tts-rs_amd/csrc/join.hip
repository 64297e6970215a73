// join.hip -- the PCM of a long text's segments joined into one signal on the MI355X: each
// segment's silent edges cut back to a kept margin and faded, a controlled pause after it. The
// last stage of generate_long_speech before the stretch and the resampler. No reference
// counterpart: the reference synthesises one request per text and stops at 2048 semantic tokens.
//
// The arithmetic contract is in include/rwkvtts.h: the cut bounds are integers
// (the first and last sample above the threshold, widened by `keep` and clamped to the segment),
// a faded sample is one rounded f32 multiply by a table entry, every other sample is copied, gaps
// are +0. The kernels are pinned bitwise to a numpy restatement of exactly that
// (tests/test_gpu_join.py).
//
// Work: k_join_bounds gives a workgroup 4096 samples of a segment and reduces the loud indices to
// a (min, max) pair per segment with integer atomics (order-free); k_join_layout gives a workgroup
// to a job and takes the prefix over its segments' piece and gap lengths; k_join_write gives a
// lane to every sample of a job's capacity: a piece sample (copied or faded), a gap zero, or a
// zero of the unused tail behind n_out. Every read of a segment is guarded by its own [0, n_s).
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

constexpr int kJoinThreads = 256;
constexpr int kJoinWaves = kJoinThreads / 64;
constexpr int kJoinPer = 16;                             // samples per lane of a bounds workgroup
constexpr int kJoinChunk = kJoinThreads * kJoinPer;      // samples per workgroup pass
constexpr int kJoinMaxSeg = 4096;                        // segments per job: kJoinThreads * kJoinPer
constexpr int kJoinMaxJobs = 1024;
constexpr int kJoinMaxFade = 4096;
constexpr int64_t kJoinMaxSamples = (int64_t)1 << 30;    // per segment: its indices fit the 32-bit atomics
constexpr int64_t kJoinMaxGap = (int64_t)1 << 40;
constexpr unsigned kJoinMaxGridY = 1024;                 // passes beyond it are walked by the same workgroups
constexpr int kJoinNone = 0x7f7f7f7f;                    // "no loud sample" of the minimum (a memset pattern)

struct JoinCfg {
  float threshold;
  int keep, fade, trim;
};

template <typename T>
__device__ inline T jmin(T a, T b) { return b < a ? b : a; }
template <typename T>
__device__ inline T jmax(T a, T b) { return a < b ? b : a; }

// One segment. cap_off: the samples and gaps of the job's earlier segments (where this segment's
// output would start if nothing were cut).
struct JoinSeg {
  int64_t in_off, n, gap, cap_off;
  int32_t job, pad;
};
struct JoinJob {
  int64_t seg0, n_seg, out_base;
};

// grid (segments, passes): the loud samples of a segment's [pass * 4096, + 4096)
__global__ __launch_bounds__(kJoinThreads) void k_join_bounds(const float* __restrict__ x,
                                                              const JoinSeg* __restrict__ segs,
                                                              int* __restrict__ lo, int* __restrict__ hi,
                                                              float threshold) {
  __shared__ int s_lo[kJoinWaves], s_hi[kJoinWaves];
  const JoinSeg sg = segs[blockIdx.x];
  const int tid = threadIdx.x;
  for (int64_t c0 = (int64_t)blockIdx.y * kJoinChunk; c0 < sg.n; c0 += (int64_t)gridDim.y * kJoinChunk) {
    int mn = kJoinNone, mx = -1;
#pragma unroll
    for (int k = 0; k < kJoinPer; ++k) {
      const int64_t i = c0 + (int64_t)k * kJoinThreads + tid;
      if (i < sg.n && fabsf(x[sg.in_off + i]) > threshold) {  // (false for NaN)
        mn = jmin(mn, (int)i);
        mx = jmax(mx, (int)i);
      }
    }
    for (int off = 32; off >= 1; off >>= 1) {
      mn = jmin(mn, __shfl_xor(mn, off, 64));
      mx = jmax(mx, __shfl_xor(mx, off, 64));
    }
    if ((tid & 63) == 0) {
      s_lo[tid >> 6] = mn;
      s_hi[tid >> 6] = mx;
    }
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < kJoinWaves; ++w) {
        mn = jmin(mn, s_lo[w]);
        mx = jmax(mx, s_hi[w]);
      }
      if (mx >= 0) {
        atomicMin(lo + blockIdx.x, mn);
        atomicMax(hi + blockIdx.x, mx);
      }
    }
    __syncthreads();  // s_lo / s_hi may be written again
  }
}

// grid (jobs): a_s, b_s of every segment and off_s, the exclusive prefix of len_s + gap_s; n_out.
// A lane owns kJoinPer consecutive segments; the lanes' sums are scanned in LDS.
__global__ __launch_bounds__(kJoinThreads) void k_join_layout(const JoinSeg* __restrict__ segs,
                                                              const JoinJob* __restrict__ jobs,
                                                              const int* __restrict__ lo, const int* __restrict__ hi,
                                                              int64_t* __restrict__ a_out, int64_t* __restrict__ b_out,
                                                              int64_t* __restrict__ off_out,
                                                              int64_t* __restrict__ n_out, int keep, int trim) {
  __shared__ int64_t s_scan[kJoinThreads];
  const JoinJob j = jobs[blockIdx.x];
  const int tid = threadIdx.x;
  int64_t span[kJoinPer];
  int64_t sum = 0;
#pragma unroll
  for (int k = 0; k < kJoinPer; ++k) {
    const int64_t s = (int64_t)tid * kJoinPer + k;
    span[k] = 0;
    if (s >= j.n_seg) continue;
    const JoinSeg sg = segs[j.seg0 + s];
    int64_t a = 0, b = sg.n;
    if (trim) {
      const int l = lo[j.seg0 + s], h = hi[j.seg0 + s];
      if (h < 0) {
        a = b = 0;
      } else {
        a = jmax<int64_t>(0, (int64_t)l - keep);
        b = jmin<int64_t>(sg.n, (int64_t)h + 1 + keep);
      }
    }
    a_out[j.seg0 + s] = a;
    b_out[j.seg0 + s] = b;
    span[k] = (b - a) + sg.gap;
    sum += span[k];
  }
  s_scan[tid] = sum;
  __syncthreads();
  for (int d = 1; d < kJoinThreads; d <<= 1) {  // inclusive scan of the lanes' sums
    const int64_t v = tid >= d ? s_scan[tid - d] : 0;
    __syncthreads();
    s_scan[tid] += v;
    __syncthreads();
  }
  int64_t off = s_scan[tid] - sum;
#pragma unroll
  for (int k = 0; k < kJoinPer; ++k) {
    const int64_t s = (int64_t)tid * kJoinPer + k;
    if (s >= j.n_seg) continue;
    off_out[j.seg0 + s] = off;
    off += span[k];
  }
  if (tid == kJoinThreads - 1) n_out[blockIdx.x] = s_scan[tid];
}

// grid (segments, passes): lane i of a segment's n_s + gap_s. i below len_s is a piece sample, the
// next gap_s lanes are the pause, and the n_s - len_s lanes left over (what the cut removed) zero
// their share of the job's unused tail behind n_out -- so the lanes of a job write each sample of
// its capacity exactly once.
__global__ __launch_bounds__(kJoinThreads) void k_join_write(const float* __restrict__ x, const float* __restrict__ ramp,
                                                             const JoinSeg* __restrict__ segs,
                                                             const JoinJob* __restrict__ jobs,
                                                             const int64_t* __restrict__ a_in,
                                                             const int64_t* __restrict__ b_in,
                                                             const int64_t* __restrict__ off_in,
                                                             const int64_t* __restrict__ n_out, float* __restrict__ y,
                                                             int fade, int trim) {
  const JoinSeg sg = segs[blockIdx.x];
  const int64_t a = a_in[blockIdx.x], len = b_in[blockIdx.x] - a, off = off_in[blockIdx.x];
  const int64_t span = sg.n + sg.gap;
  const int64_t f = trim ? jmin<int64_t>(fade, len / 2) : 0;
  float* __restrict__ yj = y + jobs[sg.job].out_base;
  const int64_t tail = n_out[sg.job] + (sg.cap_off - off) - (len + sg.gap);  // + i: the lane's tail sample
  const float* __restrict__ xs = x + sg.in_off + a;
  const int tid = threadIdx.x;
  for (int64_t c0 = (int64_t)blockIdx.y * kJoinChunk; c0 < span; c0 += (int64_t)gridDim.y * kJoinChunk) {
#pragma unroll 4
    for (int k = 0; k < kJoinPer; ++k) {
      const int64_t i = c0 + (int64_t)k * kJoinThreads + tid;
      if (i >= span) break;
      if (i < len) {  // a + i < b_s <= n_s
        float v = xs[i];
        if (i < f) v = __fmul_rn(v, ramp[i]);
        else if (i >= len - f) v = __fmul_rn(v, ramp[len - 1 - i]);
        yj[off + i] = v;
      } else if (i < len + sg.gap) {
        yj[off + i] = 0.0f;
      } else {
        yj[tail + i] = 0.0f;
      }
    }
  }
}

// ---- host: configuration, ramp -----------------------------------------------------------------
static int join_config(const rwkvtts_join_desc* d, JoinCfg* c, const char* who) {
  RT_CHECK(d && d->struct_size >= sizeof(rwkvtts_join_desc), RWKVTTS_EINVAL,
           std::string(who) + ": null desc or struct_size too small");
  RT_CHECK(d->threshold >= 0.0f && d->threshold <= 3.0e38f, RWKVTTS_EINVAL,  // (NaN and inf fail)
           std::string(who) + ": threshold must be finite and >= 0 (0 = 0.01)");
  RT_CHECK(d->keep >= 0, RWKVTTS_EINVAL, std::string(who) + ": keep must be >= 0");
  RT_CHECK(d->fade >= 0 && d->fade <= kJoinMaxFade, RWKVTTS_EINVAL, std::string(who) + ": fade must be 0 .. 4096");
  RT_CHECK(d->trim == 0 || d->trim == 1, RWKVTTS_EINVAL, std::string(who) + ": trim must be 0 or 1");
  c->threshold = d->threshold == 0.0f ? 0.01f : d->threshold;
  c->keep = d->keep;
  c->fade = d->fade;
  c->trim = d->trim;
  return RWKVTTS_OK;
}

static void join_make_ramp(const JoinCfg& c, float* out) {
  for (int k = 0; k < c.fade; ++k) out[k] = (float)(((double)k + 0.5) / (double)c.fade);
}

static int64_t join_capacity(const int64_t* n, const int64_t* gap, int32_t n_seg) {
  if (n_seg < 0 || n_seg > kJoinMaxSeg || (n_seg > 0 && (!n || !gap))) return -1;
  int64_t cap = 0;
  for (int s = 0; s < n_seg; ++s) {
    if (n[s] < 0 || n[s] > kJoinMaxSamples || gap[s] < 0 || gap[s] > kJoinMaxGap) return -1;
    cap += n[s] + gap[s];
  }
  return cap;
}

// the two copies of a call in the shape stage_upload / stage_download take
struct JoinXfer {
  const float* in;
  int64_t n_in;
  float* out;
  int64_t out_count;
};

}  // namespace rwkvtts

using namespace rwkvtts;

struct rwkvtts_join : Stage<JoinSeg> {  // d_table: the ramp (one entry at least)
  JoinCfg cfg;
  DevBuf<JoinJob> d_jobs;
  DevBuf<int> d_lohi;       // lo[segments], hi[segments]
  DevBuf<int64_t> d_res;    // a[segments], b[segments], off[segments], n_out[jobs]
  std::vector<JoinJob> jobs;
  std::vector<int64_t> res;  // a, b of every segment and n_out of every job, read back
};

static int join_run(rwkvtts_join* j, rwkvtts_join_job* const* jp, int n, const char* who) {
  const JoinCfg& c = j->cfg;
  int64_t tot_in = 0, tot_out = 0, tot_seg = 0, max_n = 0, max_span = 0;
  for (int k = 0; k < n; ++k) {
    const rwkvtts_join_job& q = *jp[k];
    const int64_t cap = join_capacity(q.n, q.gap, q.n_seg);
    RT_CHECK(cap >= 0, RWKVTTS_EINVAL,
             std::string(who) + ": bad job (n_seg outside 0 .. 4096, null array, negative or too long segment / gap)");
    RT_CHECK(q.out || cap == 0, RWKVTTS_EINVAL, std::string(who) + ": null output");
    RT_CHECK(q.seg || q.n_seg == 0, RWKVTTS_EINVAL, std::string(who) + ": null segment array");
    for (int s = 0; s < q.n_seg; ++s) {
      RT_CHECK(q.seg[s] || q.n[s] == 0, RWKVTTS_EINVAL, std::string(who) + ": null segment");
      tot_in += q.n[s];
      max_n = std::max(max_n, q.n[s]);
      max_span = std::max(max_span, q.n[s] + q.gap[s]);
    }
    tot_out += cap;
    tot_seg += q.n_seg;
  }
  if (tot_seg == 0) {
    for (int k = 0; k < n; ++k) jp[k]->n_out = 0;
    return RWKVTTS_OK;
  }
  RT_CHECK(tot_seg <= 0x7fffffff, RWKVTTS_EINVAL, std::string(who) + ": too much for one launch");
  std::lock_guard<std::mutex> lock(j->mu);
  j->desc.clear();
  j->jobs.clear();
  std::vector<JoinXfer> up, down;
  int64_t in_off = 0, out_base = 0;
  for (int k = 0; k < n; ++k) {
    const rwkvtts_join_job& q = *jp[k];
    JoinJob jb{(int64_t)j->desc.size(), q.n_seg, out_base};
    int64_t cap_off = 0;
    for (int s = 0; s < q.n_seg; ++s) {
      j->desc.push_back(JoinSeg{in_off, q.n[s], q.gap[s], cap_off, k, 0});
      up.push_back(JoinXfer{q.seg[s], q.n[s], nullptr, 1});
      in_off += q.n[s];
      cap_off += q.n[s] + q.gap[s];
    }
    j->jobs.push_back(jb);
    down.push_back(JoinXfer{nullptr, 0, q.out, cap_off});
    out_base += cap_off;
  }
  const size_t S = (size_t)tot_seg, J = (size_t)n;
  int rc;
  if ((rc = stage_reserve(j, tot_in, std::max<int64_t>(tot_out, 1))) || (rc = j->d_jobs.reserve(J)) ||
      (rc = j->d_lohi.reserve(2 * S)) || (rc = j->d_res.reserve(3 * S + J)) || (rc = stage_upload(j, up)))
    return rc;
  RT_HIP(hipMemcpyAsync(j->d_jobs.p, j->jobs.data(), J * sizeof(JoinJob), hipMemcpyHostToDevice, j->stream));
  int* d_lo = j->d_lohi.p;
  int* d_hi = j->d_lohi.p + S;
  int64_t *d_a = j->d_res.p, *d_b = d_a + S, *d_off = d_b + S, *d_nout = d_off + S;
  auto passes = [](int64_t len) { return (unsigned)std::min<int64_t>(std::max<int64_t>((len + kJoinChunk - 1) / kJoinChunk, 1), kJoinMaxGridY); };
  // the event pair brackets the kernels: the start of the first launched, the end of the write
  if (c.trim) {
    RT_HIP(hipMemsetAsync(d_lo, 0x7f, S * sizeof(int), j->stream));  // kJoinNone
    RT_HIP(hipMemsetAsync(d_hi, 0xff, S * sizeof(int), j->stream));  // -1
    hipExtLaunchKernelGGL(k_join_bounds, dim3((unsigned)S, passes(max_n)), dim3(kJoinThreads), 0, j->stream, j->ev0,
                          nullptr, 0u, j->d_in.p, j->d_desc.p, d_lo, d_hi, c.threshold);
    RT_HIP(hipGetLastError());
  }
  hipExtLaunchKernelGGL(k_join_layout, dim3((unsigned)J), dim3(kJoinThreads), 0, j->stream, c.trim ? nullptr : j->ev0,
                        nullptr, 0u, j->d_desc.p, j->d_jobs.p, d_lo, d_hi, d_a, d_b, d_off, d_nout, c.keep, c.trim);
  RT_HIP(hipGetLastError());
  hipExtLaunchKernelGGL(k_join_write, dim3((unsigned)S, passes(max_span)), dim3(kJoinThreads), 0, j->stream, nullptr,
                        j->ev1, 0u, j->d_in.p, j->d_table, j->d_desc.p, j->d_jobs.p, d_a, d_b, d_off, d_nout, j->d_out.p,
                        c.fade, c.trim);
  RT_HIP(hipGetLastError());
  // the bounds and the lengths come back with the samples, before the one synchronisation
  j->res.assign(2 * S + J, 0);
  RT_HIP(hipMemcpyAsync(j->res.data(), d_a, 2 * S * sizeof(int64_t), hipMemcpyDeviceToHost, j->stream));
  RT_HIP(hipMemcpyAsync(j->res.data() + 2 * S, d_nout, J * sizeof(int64_t), hipMemcpyDeviceToHost, j->stream));
  if ((rc = stage_download(j, down))) return rc;
  for (int k = 0; k < n; ++k) {
    rwkvtts_join_job& q = *jp[k];
    const size_t s0 = (size_t)j->jobs[(size_t)k].seg0;
    q.n_out = j->res[2 * S + (size_t)k];
    for (int s = 0; s < q.n_seg; ++s) {
      if (q.a) q.a[s] = j->res[s0 + (size_t)s];
      if (q.b) q.b[s] = j->res[S + s0 + (size_t)s];
    }
  }
  return RWKVTTS_OK;
}

extern "C" int rwkvtts_join_ramp(const rwkvtts_join_desc* desc, float* out) {
  JoinCfg c;
  int rc = join_config(desc, &c, "join_ramp");
  if (rc) return rc;
  RT_CHECK(out || c.fade == 0, RWKVTTS_EINVAL, "join_ramp: null output");
  join_make_ramp(c, out);
  return RWKVTTS_OK;
}

extern "C" int64_t rwkvtts_join_capacity(const int64_t* n, const int64_t* gap, int32_t n_seg) {
  const int64_t cap = join_capacity(n, gap, n_seg);
  if (cap < 0) set_error("join_capacity: n_seg outside 0 .. 4096, null array, negative or too long segment / gap");
  return cap;
}

extern "C" int rwkvtts_join_create(int device, const rwkvtts_join_desc* desc, const float* table, rwkvtts_join** out) {
  RT_CHECK(out, RWKVTTS_EINVAL, "join_create: null output");
  *out = nullptr;
  JoinCfg c;
  int rc = join_config(desc, &c, "join_create");
  if (rc) return rc;
  rwkvtts_join* j = nullptr;
  // (one entry at least, so the table exists for fade 0 too: it is never read then)
  rc = stage_create("join_create", device, c.fade ? table : nullptr, (size_t)std::max(c.fade, 1),
                    [&](float* r) { join_make_ramp(c, r); }, &j);
  if (rc) return rc;
  j->cfg = c;
  *out = j;
  return RWKVTTS_OK;
}

extern "C" int rwkvtts_join_destroy(rwkvtts_join* j) {
  if (!j) return RWKVTTS_OK;
  (void)hipSetDevice(j->device);
  stage_free(j, {j->d_jobs.p, j->d_lohi.p, j->d_res.p});
  return RWKVTTS_OK;
}

extern "C" int rwkvtts_join_jobs(rwkvtts_join* j, rwkvtts_join_job* jobs, int n) {
  RT_CHECK(j && jobs && n >= 1 && n <= kJoinMaxJobs, RWKVTTS_EINVAL, "join_jobs: bad arguments (1 .. 1024 jobs)");
  return guard_alloc("join_jobs", [&] {
    std::vector<rwkvtts_join_job*> jp;
    int rc = read_windows("join_jobs", jobs, n, jp, [](rwkvtts_join_job* q) { return q; });
    return rc ? rc : join_run(j, jp.data(), n, "join_jobs");
  });
}

extern "C" int rwkvtts_join_kernel_ms(rwkvtts_join* j, double* ms) { return stage_kernel_ms("join_kernel_ms", j, ms); }
