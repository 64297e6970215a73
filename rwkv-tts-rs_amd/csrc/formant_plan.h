// formant_plan.h -- the host-only part of the formant shift (formant.hip), beside pitch_plan.h: the
// ratio and its range, the polyphase table, the plan with the grain read's longer reach, and the LDS
// span a workgroup of k_formant_synth stages. Plain functions of host data (plain C++17, no HIP
// header). The contract is in include/rwkvtts.h.
#pragma once
#include "pitch_plan.h"

namespace rwkvtts {

constexpr int kFormantTaps = 16;    // T: tap t of a read at P reads x[(P >> 16) - kFormantBack + t]
constexpr int kFormantPhases = 64;  // the phase is ((P & 65535) >> 10): the fraction truncated to 6 bits
constexpr int kFormantBack = 7;
constexpr int kFormantOne = 65536;  // B of beta = 1
constexpr int kFormantBMin = 46341, kFormantBMax = 92682;  // round(2^(-+6 / 12) * 65536)
constexpr int kFormantPiece = 320;  // outputs of a workgroup (kPitchThreads)

inline bool formant_b_ok(int64_t B) { return B >= kFormantBMin && B <= kFormantBMax; }

// B = floor(2^(s / 12) * 65536 + 0.5) in double. -> false outside [-6, 6] (NaN included).
inline bool formant_b_of(double semitones, int32_t* B) {
  if (!(semitones >= -6.0 && semitones <= 6.0)) return false;
  *B = (int32_t)floor(exp2(semitones / 12.0) * 65536.0 + 0.5);
  return true;
}

// The table of B: out[ph * T + t], in double step by step as the header states it.
inline void formant_make_table(int32_t B, float* out) {
#pragma clang fp contract(off)
  const double pi = 3.141592653589793;
  const double fc = B <= kFormantOne ? 1.0 : 65536.0 / (double)B;
  for (int ph = 0; ph < kFormantPhases; ++ph) {
    double v[kFormantTaps], sum = 0.0;
    for (int t = 0; t < kFormantTaps; ++t) {
      const double u = (double)(t - kFormantBack) - (double)ph / (double)kFormantPhases;
      const double z = fc * u;
      double s = 1.0;
      if (z != 0.0) {
        const double a = pi * z;
        s = z == floor(z) ? 0.0 : sin(a) / a;
      }
      const double k = (u + 0.5 * kFormantTaps) / (double)kFormantTaps;
      const double w = 0.35875 - 0.48829 * cos(2.0 * pi * k) + 0.14128 * cos(4.0 * pi * k) - 0.01168 * cos(6.0 * pi * k);
      v[t] = s * (w * w);
      sum = sum + v[t];
    }
    for (int t = 0; t < kFormantTaps; ++t) out[ph * kFormantTaps + t] = (float)(v[t] / sum);
  }
}

// How far a grain's read goes from its analysis mark, either way: r - p in [-p, p - 1] puts P >> 16
// in [a - ceil(p B / 65536), a + floor((p - 1) B / 65536)], and the taps reach 7 below and 8 above it.
inline int64_t formant_reach(const PitchCfg& c, int32_t B) {
  return (((int64_t)c.Lmax * B + 65535) >> 16) + (kFormantTaps - kFormantBack - 1);
}
// pitch_ready_end and pitch_in_first_needed with max(Lmax, reach) in the place of the grain's Lmax: the
// plan never asks for less than the pitch plan (a read slower than 1 reaches less than Lmax, but a
// window is still checked by pitch_window_check, and a stream keeps the few samples more). At
// B == 65536 the pitch path runs, so the plan is the pitch plan.
inline int64_t formant_ready_end(const PitchCfg& c, int32_t B, int64_t n_known, int final) {
  if (B == kFormantOne || final) return pitch_ready_end(c, n_known, final);
  const int64_t look = 2 * (int64_t)c.Lmax + std::max<int64_t>((int64_t)c.Wc + c.Lmax, formant_reach(c, B));
  return std::max<int64_t>(0, n_known - look);
}
inline int64_t formant_in_first_needed(const PitchCfg& c, int32_t B, int64_t a_prev) {
  if (B == kFormantOne) return pitch_in_first_needed(c, a_prev);
  const int64_t back = std::max<int64_t>(c.Lmax, formant_reach(c, B));
  return std::max<int64_t>(0, std::min<int64_t>(a_prev - back, (a_prev / c.Ha) * c.Ha));
}

// The most samples of x the grains of one 320-output piece can read. A grain (s, a, p) reads, for
// output o, around a + (o - s) B / 65536 = o + (a - s) + (o - s)(B - 65536) / 65536: |a - s| <= Lmax
// (the pairing takes the nearest analysis mark, marks are at most Lmax apart and the walk runs past
// every synthesis mark that can reach an output: in fact Lmax / 2), |o - s| <= p <= Lmax, so P >> 16
// lies in [o - Lmax - E - 1, o + Lmax + E] with E = ceil(Lmax * max|B - 65536| / 65536); the taps add
// 7 below and 8 above.
inline int64_t formant_span_cap(const PitchCfg& c) {
  const int64_t e = ((int64_t)c.Lmax * (kFormantBMax - kFormantOne) + 65535) >> 16;
  return kFormantPiece + 2 * (int64_t)c.Lmax + 2 * e + kFormantTaps + 2;
}
inline size_t formant_lds_bytes(const PitchCfg& c) {
  return ((size_t)kFormantTaps * kFormantPhases + (size_t)formant_span_cap(c)) * sizeof(float);
}

}  // namespace rwkvtts
