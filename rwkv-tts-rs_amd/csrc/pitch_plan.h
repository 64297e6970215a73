// pitch_plan.h -- the host-only part of the pitch shifter (pitch.hip): the configuration and its
// ranges, the grain table, the streaming plan, the check of a carried state and of a window, and the
// sizes a window's launches need. Plain functions of host data (plain C++17, no HIP header), so
// tests/native/pitch_plan_main.cpp checks them on a CPU. The contract is in include/rwkvtts.h.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/rwkvtts.h"

namespace rwkvtts {

constexpr int64_t kPitchMaxSamples = (int64_t)1 << 30;

struct PitchCfg {
  int Ha, Wc, Lmin, Lmax, P0;
  float theta, floor;
};

// Fills c from d (0 = the default). -> nullptr, or what is out of range.
inline const char* pitch_config_of(const rwkvtts_pitch_desc* d, PitchCfg* c) {
  if (!d || d->struct_size < sizeof(rwkvtts_pitch_desc)) return "null desc or struct_size too small";
  c->Ha = d->hop ? d->hop : 160;
  c->Wc = d->window ? d->window : 640;
  c->Lmin = d->lag_min ? d->lag_min : 32;
  c->Lmax = d->lag_max ? d->lag_max : 320;
  c->P0 = d->unvoiced ? d->unvoiced : 80;
  c->theta = d->theta != 0.0f ? d->theta : 0.2f;
  c->floor = d->floor != 0.0f ? d->floor : 1e-3f;
  if (!(c->Ha >= 1 && c->Ha <= 4096)) return "hop must be 1 .. 4096 (0 = 160)";
  if (!(c->Wc >= 1 && c->Wc <= 4096)) return "window must be 1 .. 4096 (0 = 640)";
  if (!(c->Lmin >= 2 && c->Lmin <= 1024 && c->Lmax >= c->Lmin && c->Lmax <= 1024))
    return "lag_min must be 2 .. 1024 (0 = 32), lag_max lag_min .. 1024 (0 = 320)";
  if (!(c->P0 >= c->Lmin && c->P0 <= c->Lmax)) return "unvoiced must be lag_min .. lag_max (0 = 80)";
  if (!(c->theta > 0.0f && c->theta <= 1.0f)) return "theta must be in (0, 1]";  // (NaN fails)
  if (!(c->floor > 0.0f && c->floor <= 3.4028234e38f)) return "floor must be finite and positive";
  return nullptr;
}

inline bool pitch_factor_ok(double f) { return f >= 0.5 && f <= 2.0; }  // (NaN fails)

inline size_t pitch_row_offset(const PitchCfg& c, int P) { return (size_t)(P - c.Lmin) * (size_t)(P + c.Lmin - 1); }
inline size_t pitch_table_len(const PitchCfg& c) { return pitch_row_offset(c, c.Lmax) + 2 * (size_t)c.Lmax; }

// the rows Lmin .. Lmax, in double, step by step as the header states them
inline void pitch_make_table(const PitchCfg& c, float* out) {
#pragma clang fp contract(off)
  const double two_pi = 2.0 * 3.141592653589793;
  for (int P = c.Lmin; P <= c.Lmax; ++P) {
    float* row = out + pitch_row_offset(c, P);
    for (int i = 0; i < 2 * P; ++i) {
      const double ph = (two_pi * ((double)i + 0.5)) / (double)(2 * P);
      row[i] = (float)(0.5 - 0.5 * cos(ph));
    }
  }
}

inline int64_t pitch_ready_end(const PitchCfg& c, int64_t n_known, int final) {
  return final ? n_known : std::max<int64_t>(0, n_known - ((int64_t)c.Wc + 3 * (int64_t)c.Lmax));
}
inline int64_t pitch_in_first_needed(const PitchCfg& c, int64_t a_prev) {
  return std::max<int64_t>(0, std::min<int64_t>(a_prev - c.Lmax, (a_prev / c.Ha) * c.Ha));
}
// whether (a_prev, s_prev) can be the state after outputs [0, out_first): the largest synthesis mark
// at or below max(0, out_first - Lmax) (a synthesis step is at most 2 Lmax) and the largest analysis
// mark at or below max(0, s_prev - Lmax) (an analysis step is at most Lmax)
inline bool pitch_state_ok(const PitchCfg& c, int64_t out_first, int64_t a_prev, int64_t s_prev) {
  const int64_t sx = std::max<int64_t>(0, out_first - c.Lmax);
  if (s_prev < 0 || s_prev > sx || s_prev <= sx - 2 * (int64_t)c.Lmax) return false;
  const int64_t ay = std::max<int64_t>(0, s_prev - c.Lmax);
  return a_prev >= 0 && a_prev <= ay && a_prev > ay - c.Lmax;
}

// What a window's launches need: frames [j0, j0 + nf) -- from the frame of a_prev to the frame of
// sample out_end + 2 Lmax - 1 -- and room for the marks of both walks from their start to their first
// mark at or past out_end + Lmax: an analysis step is at least Lmin, a synthesis step at least
// floor(Lmin / 2 + 0.5) (factor <= 2, and P0 >= Lmin).
struct PitchGeom {
  int64_t j0, nf, am_cap, sm_cap;
};
inline PitchGeom pitch_geometry(const PitchCfg& c, int64_t out_first, int64_t out_count, int64_t a_prev,
                                int64_t s_prev) {
  const int64_t end = out_first + out_count;
  const int s_min = (c.Lmin + 1) / 2;
  PitchGeom g;
  g.j0 = a_prev / c.Ha;
  g.nf = (end + 2 * (int64_t)c.Lmax - 1) / c.Ha + 1 - g.j0;
  g.am_cap = (end + c.Lmax - a_prev) / c.Lmin + 3;
  g.sm_cap = (end + c.Lmax - s_prev) / s_min + 3;
  return g;
}

// A window against the plan. -> nullptr, or why it is refused.
inline const char* pitch_window_check(const PitchCfg& c, int64_t in_first, int64_t n_in, int final, double factor,
                                      int64_t out_first, int64_t a_prev, int64_t s_prev, int64_t out_count,
                                      bool has_in, bool has_out) {
  if (!pitch_factor_ok(factor)) return "factor must be 0.5 .. 2.0";
  if (!(in_first >= 0 && n_in >= 0 && out_first >= 0 && out_count >= 0 && in_first <= kPitchMaxSamples &&
        n_in <= kPitchMaxSamples && in_first + n_in <= kPitchMaxSamples && out_first <= kPitchMaxSamples &&
        out_count <= kPitchMaxSamples && (has_in || n_in == 0) && (has_out || out_count == 0)))
    return "bad window (negative size, null buffer or too long)";
  if (!pitch_state_ok(c, out_first, a_prev, s_prev)) return "(a_prev, s_prev) is no state a walk can have left";
  if (out_count == 0) return nullptr;
  if (out_first + out_count > pitch_ready_end(c, in_first + n_in, final))
    return "a requested output needs samples past the given ones";
  if (in_first > pitch_in_first_needed(c, a_prev)) return "a requested output reads before the given samples";
  return nullptr;
}

}  // namespace rwkvtts
