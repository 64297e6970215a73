// formant.hip -- the grain-resampling synthesis of the pitch stage on the MI355X, for the
// `formant_shift` keyword of the pipeline: TD-PSOLA grains laid down at the marks pitch.hip finds, each
// read `beta` times faster under the same Hann window, so the period stays and the spectral envelope
// moves by beta. No reference counterpart: the reference's age and gender are property tokens, which a
// cloned voice does not get.
//
// The arithmetic contract is in include/rwkvtts.h: the numerator term of grain
// (s, a, p) at output o is w[p][r] * xi, xi a 16-tap sum in ascending tap order over row
// ((P & 65535) >> 10) of a 64-phase windowed-sinc table around sample P >> 16, P = (a << 16) +
// (r - p) * B in int64. Everything else -- periods, marks, pairing, Hann rows, denominator, the divide --
// is the pitch stage's. Pinned bitwise to a numpy restatement (tests/test_gpu_formant.py).
//
// Work: a workgroup owns one 320-sample piece of one job. Thread 0 finds the grains that can reach the
// piece with two binary searches; every thread then folds the read span of some of those grains into
// an LDS minimum and maximum; the span of x and the job's table go to LDS; a lane owns an output
// sample and walks the grains in ascending order: 16 LDS reads of x and 16 of its table row per
// grain, issued together ahead of the sequential f32 chain. The table lies tap-major in LDS
// (ht[t * 64 + phase]): at a given tap the lanes of a wave read 64 consecutive words indexed by their
// phase -- distinct phases fall in distinct banks, equal phases are one broadcast address -- where a
// phase-major row of 16 words would put every lane on banks t and t + 16 alone. The x reads of
// neighbouring lanes are B / 65536 (0.71 .. 1.41) words apart: consecutive banks, with an address
// shared (broadcast) or skipped now and then.
#include <limits.h>

#include "formant_plan.h"
#include "pitch_dev.h"

namespace rwkvtts {

static_assert(kFormantPiece == kPitchThreads, "a lane per output of the piece");

// grid (320-sample pieces of the longest job, jobs). LDS: ht[16 * 64], then xs[span_cap].
__global__ __launch_bounds__(kPitchThreads) void k_formant_synth(
    const float* __restrict__ x, const float* __restrict__ tab, const float* __restrict__ ftab,
    const PitchJob* __restrict__ jobs, const FormantJob* __restrict__ fjobs, const PitchGrain* __restrict__ gr,
    const PitchState* __restrict__ state, float* __restrict__ y, PitchCfg c, int span_cap) {
  extern __shared__ float s_mem[];
  __shared__ int s_q[2], s_span[2];
  const PitchJob j = jobs[blockIdx.y];
  const int first = blockIdx.x * kPitchThreads;
  if (first >= j.out_count) return;  // (uniform over the workgroup)
  const FormantJob fj = fjobs[blockIdx.y];
  const int tid = threadIdx.x;
  const int o0 = j.out_first + first;                                   // the piece is outputs [o0, o1)
  const int o1 = j.out_first + min(first + kPitchThreads, j.out_count);
  const PitchGrain* G = gr + j.sm_off;
  float* ht = s_mem;
  float* xs = s_mem + kFormantTaps * kFormantPhases;
  if (tid == 0) {
    const int ns = state[blockIdx.y].ns;
    int lo = 0, hi = ns;  // the first synthesis mark whose grain can reach o0: s + Lmax > o0
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (G[mid].s > o0 - c.Lmax) hi = mid; else lo = mid + 1;
    }
    s_q[0] = lo;
    hi = ns;  // the first whose grain starts past the piece's last output: s - Lmax > o1 - 1
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (G[mid].s - c.Lmax > o1 - 1) hi = mid; else lo = mid + 1;
    }
    s_q[1] = lo;
    s_span[0] = INT_MAX;
    s_span[1] = INT_MIN;
  }
  const float* ft = ftab + (size_t)fj.tab * (kFormantTaps * kFormantPhases);
  for (int i = tid; i < kFormantTaps * kFormantPhases; i += kPitchThreads)  // (consecutive LDS words per wave)
    ht[i] = ft[(i & (kFormantPhases - 1)) * kFormantTaps + i / kFormantPhases];
  __syncthreads();
  const int q0 = s_q[0], q1 = s_q[1];
  const int64_t B = fj.B;
  // P >> 16 rises with r, so a grain's reads lie between those of its first and last r in the piece
  for (int q = q0 + tid; q < q1; q += kPitchThreads) {
    const PitchGrain g = G[q];
    const int r0 = max(0, o0 - (g.s - g.p)), r1 = min(2 * g.p, o1 - (g.s - g.p));
    if (r1 > r0) {
      const int64_t a16 = (int64_t)g.a << 16;
      atomicMin(&s_span[0], (int)((a16 + (int64_t)(r0 - g.p) * B) >> 16) - kFormantBack);
      atomicMax(&s_span[1], (int)((a16 + (int64_t)(r1 - 1 - g.p) * B) >> 16) - kFormantBack + kFormantTaps);
    }
  }
  __syncthreads();
  const int x_lo = s_span[0];
  const int nx = x_lo == INT_MAX ? 0 : s_span[1] - x_lo;
  const int i = first + tid;
  if (nx > span_cap) {  // formant_span_cap rules it out; if it ever fails, the piece says so and nothing is read
    if (i < j.out_count) y[j.out_off + i] = __int_as_float(0x7fc00000);
    return;
  }
  for (int k = tid; k < nx; k += kPitchThreads) xs[k] = pitch_x(x, j, (int64_t)x_lo + k);
  __syncthreads();
  if (i >= j.out_count) return;
  const int o = j.out_first + i;
  float num = 0.0f, den = 0.0f;
  for (int q = q0; q < q1; ++q) {
    const PitchGrain g = G[q];
    const int r = o - (g.s - g.p);
    if (r >= 0 && r < 2 * g.p) {
      const float w = tab[(g.p - c.Lmin) * (g.p + c.Lmin - 1) + r];  // (pitch_row_offset)
      const int64_t P = ((int64_t)g.a << 16) + (int64_t)(r - g.p) * B;
      const float* xp = xs + ((int)(P >> 16) - kFormantBack - x_lo);
      const float* hp = ht + ((int)(P & 65535) >> 10);
      float xv[kFormantTaps], hv[kFormantTaps];
#pragma unroll
      for (int t = 0; t < kFormantTaps; ++t) {
        xv[t] = xp[t];
        hv[t] = hp[t * kFormantPhases];
      }
      float xi = 0.0f;
#pragma unroll
      for (int t = 0; t < kFormantTaps; ++t) xi = __fadd_rn(xi, __fmul_rn(hv[t], xv[t]));
      num = __fadd_rn(num, __fmul_rn(w, xi));
      den = __fadd_rn(den, w);
    }
  }
  y[j.out_off + i] = den == 0.0f ? 0.0f : pitch_div(num, den);
}

int formant_synth_launch(const PitchCfg& c, unsigned pieces, unsigned n_jobs, hipStream_t stream, hipEvent_t stop,
                         const float* x, const float* tab, const float* ftab, const PitchJob* jobs,
                         const FormantJob* fjobs, const PitchGrain* gr, const PitchState* state, float* y) {
  const size_t lds = formant_lds_bytes(c);  // 16.6 KB at the widest range, 8.9 KB at the default
  RT_CHECK(lds <= 64 * 1024, RWKVTTS_EINVAL, "formant: the staged span of this lag_max does not fit the LDS");
  hipExtLaunchKernelGGL(k_formant_synth, dim3(pieces, n_jobs), dim3(kPitchThreads), lds, stream, nullptr, stop, 0u, x,
                        tab, ftab, jobs, fjobs, gr, state, y, c, (int)formant_span_cap(c));
  RT_HIP(hipGetLastError());
  return RWKVTTS_OK;
}

}  // namespace rwkvtts

using namespace rwkvtts;

static int formant_config(const rwkvtts_pitch_desc* d, int32_t B, PitchCfg* c, const char* who) {
  const char* bad = pitch_config_of(d, c);
  RT_CHECK(!bad, RWKVTTS_EINVAL, std::string(who) + ": " + bad);
  RT_CHECK(formant_b_ok(B), RWKVTTS_EINVAL, std::string(who) + ": B must be 46341 .. 92682");
  return RWKVTTS_OK;
}

extern "C" int rwkvtts_formant_ratio(double semitones, int32_t* B) {
  RT_CHECK(B, RWKVTTS_EINVAL, "formant_ratio: null output");
  RT_CHECK(formant_b_of(semitones, B), RWKVTTS_EINVAL, "formant_ratio: a formant shift must be in [-6, 6] semitones");
  return RWKVTTS_OK;
}

extern "C" int rwkvtts_formant_table(const rwkvtts_pitch_desc* desc, int32_t B, float* out) {
  PitchCfg c;
  int rc = formant_config(desc, B, &c, "formant_table");
  if (rc) return rc;
  RT_CHECK(out, RWKVTTS_EINVAL, "formant_table: null output");
  formant_make_table(B, out);
  return RWKVTTS_OK;
}

extern "C" int rwkvtts_formant_plan(const rwkvtts_pitch_desc* desc, int32_t B, int64_t n_known, int final,
                                    int64_t out_first, int64_t a_prev, int64_t s_prev, int64_t* out_ready_end,
                                    int64_t* in_first_needed) {
  PitchCfg c;
  int rc = formant_config(desc, B, &c, "formant_plan");
  if (rc) return rc;
  RT_CHECK(n_known >= 0 && n_known <= kPitchMaxSamples && out_first >= 0 && out_first <= kPitchMaxSamples,
           RWKVTTS_EINVAL, "formant_plan: n_known / out_first out of range");
  RT_CHECK(pitch_state_ok(c, out_first, a_prev, s_prev), RWKVTTS_EINVAL,
           "formant_plan: (a_prev, s_prev) is no state a walk can have left");
  if (out_ready_end) *out_ready_end = formant_ready_end(c, B, n_known, final);
  if (in_first_needed) *in_first_needed = formant_in_first_needed(c, B, a_prev);
  return RWKVTTS_OK;
}
