// pitch_dev.h -- what the kernels of pitch.hip and formant.hip share: the job, grain and state
// records, the zero-padded read and the correctly rounded divide.
#pragma once
#include <stdint.h>

#include "common.h"
#include "pitch_plan.h"

namespace rwkvtts {

constexpr int kPitchThreads = 320;  // five waves: the 291 lags of the default range in one pass

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

// A job's grain read (formant.hip): B = round(beta * 65536) and which of the call's tables is B's.
struct FormantJob {
  int32_t B, tab;
};

__device__ inline float pitch_x(const float* __restrict__ x, const PitchJob& j, int64_t idx) {
  return (idx >= j.in_first && idx < j.in_end) ? x[j.in_off + (idx - j.in_first)] : 0.0f;
}

// Correctly rounded f32 divide through double (53 >= 2 * 24 + 2 bits; the device's double divide is
// correctly rounded).
__device__ inline float pitch_div(float a, float b) { return (float)((double)a / (double)b); }

// formant.hip: k_formant_synth in the place of k_pitch_synth, same grid, between the same events.
// ftab: the call's tables back to back; fjobs[i] is job i's. -> RWKVTTS_OK or RWKVTTS_EHIP.
int formant_synth_launch(const PitchCfg& c, unsigned pieces, unsigned n_jobs, hipStream_t stream, hipEvent_t stop,
                         const float* x, const float* tab, const float* ftab, const PitchJob* jobs,
                         const FormantJob* fjobs, const PitchGrain* gr, const PitchState* state, float* y);

}  // namespace rwkvtts
