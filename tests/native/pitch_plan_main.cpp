// pitch_plan_main.cpp -- the pitch shifter's host-only rules (csrc/pitch_plan.h) as a stand-alone
// program for a plain C++17 compiler (tests/test_pitch_native_cpu.py builds it under ASan + UBSan):
// the ranges of a desc, the table's length and weights, the plan's formulas, and -- against walks
// simulated here over random period arrays -- that the carried state of every cut passes the state
// check, that the mark lists fit the sizes the launches reserve, that every frame and sample a
// window needs lies inside what the plan makes it keep and wait for.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../rwkv-tts-rs_amd/csrc/pitch_plan.h"

using namespace rwkvtts;

#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
      exit(1);                                                   \
    }                                                            \
  } while (0)

static rwkvtts_pitch_desc desc(int hop, int window, int lo, int hi, int p0, float theta = 0.0f, float floor = 0.0f) {
  rwkvtts_pitch_desc d;
  d.struct_size = sizeof(d);
  d.hop = hop, d.window = window, d.lag_min = lo, d.lag_max = hi, d.unvoiced = p0, d.theta = theta, d.floor = floor;
  return d;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {  // xorshift64*, [0, n)
  rng_state ^= rng_state >> 12, rng_state ^= rng_state << 25, rng_state ^= rng_state >> 27;
  return (uint32_t)(((rng_state * 0x2545F4914F6CDD1Dull) >> 33) % n);
}

static void case_config() {
  PitchCfg c;
  rwkvtts_pitch_desc d = desc(0, 0, 0, 0, 0);
  CHECK(!pitch_config_of(&d, &c));
  CHECK(c.Ha == 160 && c.Wc == 640 && c.Lmin == 32 && c.Lmax == 320 && c.P0 == 80 && c.theta == 0.2f && c.floor == 1e-3f);
  CHECK(pitch_table_len(c) == 101728);
  const float nan = nanf(""), inf = INFINITY;
  const rwkvtts_pitch_desc bad[] = {
      desc(-1, 0, 0, 0, 0), desc(4097, 0, 0, 0, 0), desc(0, -1, 0, 0, 0), desc(0, 4097, 0, 0, 0), desc(0, 0, 1, 0, 0),
      desc(0, 0, 1025, 0, 0), desc(0, 0, 400, 0, 0), desc(0, 0, 0, 1025, 0), desc(0, 0, 0, 16, 0), desc(0, 0, 0, -1, 0),
      desc(0, 0, 0, 0, 31), desc(0, 0, 0, 0, 321), desc(0, 0, 0, 0, -1), desc(0, 0, 0, 0, 0, -0.1f), desc(0, 0, 0, 0, 0, 1.5f),
      desc(0, 0, 0, 0, 0, nan), desc(0, 0, 0, 0, 0, 0.0f, -1.0f), desc(0, 0, 0, 0, 0, 0.0f, inf), desc(0, 0, 0, 0, 0, 0.0f, nan)};
  for (const rwkvtts_pitch_desc& b : bad) CHECK(pitch_config_of(&b, &c));
  d.struct_size = 8;
  CHECK(pitch_config_of(&d, &c) && pitch_config_of(nullptr, &c));
  CHECK(pitch_factor_ok(0.5) && pitch_factor_ok(2.0) && pitch_factor_ok(1.0));
  CHECK(!pitch_factor_ok(0.49999999999999994) && !pitch_factor_ok(2.0000000000000004) && !pitch_factor_ok((double)nan));
}

static void case_table() {
  const int ranges[][2] = {{2, 2}, {4, 16}, {32, 320}, {1000, 1024}};
  for (const auto& r : ranges) {
    PitchCfg c;
    rwkvtts_pitch_desc d = desc(0, 0, r[0], r[1], r[0]);
    CHECK(!pitch_config_of(&d, &c));
    size_t want = 0;
    for (int P = r[0]; P <= r[1]; ++P) {
      CHECK(pitch_row_offset(c, P) == want);
      want += 2 * (size_t)P;
    }
    CHECK(pitch_table_len(c) == want);
    std::vector<float> t(want, -1.0f);  // exactly the stated length: a write past it is the sanitizer's
    pitch_make_table(c, t.data());
    for (float w : t) CHECK(w > 0.0f && w <= 1.0f);
    const float* row = t.data() + pitch_row_offset(c, r[1]);
    CHECK(row[r[1] - 1] > row[0] && fabsf(row[r[1] - 1] - row[r[1]]) <= 1e-7f && row[0] < row[1] &&
          fabsf(row[0] - row[2 * r[1] - 1]) <= 1e-7f);  // rises to the middle, symmetric
  }
}

static void case_plan() {
  PitchCfg c;
  rwkvtts_pitch_desc d = desc(8, 32, 4, 16, 8);
  CHECK(!pitch_config_of(&d, &c));
  int64_t last = 0;
  for (int64_t n = 0; n < 400; ++n) {
    const int64_t e = pitch_ready_end(c, n, 0);
    CHECK(e == (n > 80 ? n - 80 : 0) && e >= last && pitch_ready_end(c, n, 1) == n);
    last = e;
  }
  CHECK(pitch_ready_end(c, kPitchMaxSamples, 0) == kPitchMaxSamples - 80);
  CHECK(pitch_in_first_needed(c, 0) == 0 && pitch_in_first_needed(c, 15) == 0 && pitch_in_first_needed(c, 100) == 84);
  d = desc(64, 32, 4, 16, 8);  // a hop above Lmax: the frame of a_prev starts before its grain
  CHECK(!pitch_config_of(&d, &c));
  CHECK(pitch_in_first_needed(c, 100) == 64 && pitch_in_first_needed(c, 130) == 114);
  // refusals of a window, in the order the library states them
  d = desc(8, 32, 4, 16, 8);
  CHECK(!pitch_config_of(&d, &c));
  CHECK(!pitch_window_check(c, 0, 500, 0, 1.5, 0, 0, 0, 420, true, true));
  CHECK(pitch_window_check(c, 0, 500, 0, 1.5, 0, 0, 0, 421, true, true));
  CHECK(!pitch_window_check(c, 0, 500, 1, 1.5, 0, 0, 0, 500, true, true));
  CHECK(pitch_window_check(c, 0, 500, 1, 1.5, 0, 0, 0, 501, true, true));
  CHECK(pitch_window_check(c, 1, 499, 1, 1.5, 0, 0, 0, 10, true, true));
  CHECK(pitch_window_check(c, 0, 500, 1, 2.5, 0, 0, 0, 10, true, true));
  CHECK(pitch_window_check(c, 0, 500, 1, 1.5, 0, 0, 0, -1, true, true));
  CHECK(pitch_window_check(c, 0, 500, 1, 1.5, 0, 0, 0, 10, false, true));
  CHECK(pitch_window_check(c, 0, 500, 1, 1.5, 0, 0, 0, 10, true, false));
  CHECK(!pitch_window_check(c, 0, 0, 1, 1.5, 0, 0, 0, 0, false, false));
  CHECK(pitch_window_check(c, 0, kPitchMaxSamples + 1, 1, 1.5, 0, 0, 0, 10, true, true));
  CHECK(pitch_window_check(c, 0, 500, 1, 1.5, 16, 0, 1, 10, true, true));  // before Lmax outputs: (0, 0) only
  CHECK(pitch_window_check(c, 0, 500, 1, 1.5, 16, 1, 0, 10, true, true));
}

// Both walks over a random period array, then random cuts: every property a window relies on.
static void case_walks() {
  for (int trial = 0; trial < 300; ++trial) {
    const int lo = 2 + (int)rnd(30), hi = lo + (int)rnd(60), p0 = lo + (int)rnd((uint32_t)(hi - lo + 1));
    const int ha = 1 + (int)rnd(3 * (uint32_t)hi), wc = 1 + (int)rnd(100);
    PitchCfg c;
    rwkvtts_pitch_desc d = desc(ha, wc, lo, hi, p0);
    CHECK(!pitch_config_of(&d, &c));
    const double fs[] = {0.5, 1.0, 2.0, 0.5 + 1.5 * (double)rnd(1000) / 999.0};
    const double f = fs[rnd(4)];
    const int64_t n = 1 + (int64_t)rnd(4000);
    const int64_t n_frames = (n + 8 * hi) / ha + 2;
    std::vector<int> per((size_t)n_frames);
    const uint32_t voiced = rnd(4);  // 0: none voiced
    for (int& p : per) p = rnd(4) < voiced ? lo + (int)rnd((uint32_t)(hi - lo + 1)) : 0;
    auto P = [&](int64_t t) { return t / ha < n_frames ? per[(size_t)(t / ha)] : 0; };
    const int64_t far = n + 6 * hi;
    std::vector<int64_t> a{0}, s{0};
    while (a.back() < far) a.push_back(a.back() + (P(a.back()) ? P(a.back()) : p0));
    while (s.back() < far) {
      const int p = P(s.back());
      int64_t step = p0;
      if (p) step = std::max<int64_t>(1, (int64_t)floor((double)p / f + 0.5));
      CHECK(step <= 2 * hi && step >= (lo + 1) / 2);
      s.push_back(s.back() + step);
    }
    auto last_at_or_below = [](const std::vector<int64_t>& v, int64_t x) {
      int64_t r = v[0];
      for (int64_t m : v)
        if (m <= x) r = m;
      return r;
    };
    int64_t e = 0, a_prev = 0, s_prev = 0;
    while (e < n) {
      const int64_t end = std::min<int64_t>(n, e + 1 + (int64_t)rnd(3 * (uint32_t)(wc + 3 * hi)));
      CHECK(pitch_state_ok(c, e, a_prev, s_prev));
      const PitchGeom g = pitch_geometry(c, e, end - e, a_prev, s_prev);
      const int64_t lim = end + hi, first = pitch_in_first_needed(c, a_prev);
      const int64_t reach = end + wc + 3 * (int64_t)hi;  // out_ready_end(reach) == end: nothing at or past it may be read
      CHECK(pitch_ready_end(c, reach, 0) == end && g.j0 * ha >= first && g.j0 == a_prev / ha);
      // the walks from the state to their first mark at or past lim fit the reserved lists
      int64_t na = 0, ns = 0;
      for (int64_t m : a)
        if (m >= a_prev) {
          ++na;
          if (m < lim) CHECK(m / ha >= g.j0 && m / ha < g.j0 + g.nf);
          if (m >= lim) break;
        }
      for (int64_t m : s)
        if (m >= s_prev) {
          ++ns;
          if (m < lim) CHECK(m / ha >= g.j0 && m / ha < g.j0 + g.nf);
          if (m >= lim) break;
        }
      CHECK(na <= g.am_cap && ns <= g.sm_cap);
      // the last frame a window measures ends below what the plan waited for
      CHECK((g.j0 + g.nf - 1) * ha + wc + hi < reach);
      // every grain that covers an output of the window: its synthesis mark is one the window walks, its
      // analysis mark is at or past a_prev and has a frame, its samples are kept and known
      for (int64_t sq : s) {
        if (sq >= lim) break;
        size_t k = 0;
        for (size_t i = 1; i < a.size(); ++i)
          if (llabs(a[i] - sq) < llabs(a[k] - sq)) k = i;
        const int64_t ak = a[k], pk = P(ak) ? P(ak) : p0;
        if (sq + pk <= e || sq - pk >= end) continue;  // covers no output of this window
        CHECK(sq >= s_prev && ak >= a_prev);
        CHECK(ak / ha < g.j0 + g.nf && (first == 0 || ak - pk >= first));
        CHECK(ak + pk <= reach);
      }
      e = end;
      s_prev = last_at_or_below(s, std::max<int64_t>(0, e - hi));
      a_prev = last_at_or_below(a, std::max<int64_t>(0, s_prev - hi));
      // and what lies just outside the ranges is refused
      CHECK(!pitch_state_ok(c, e, a_prev, std::max<int64_t>(0, e - hi) + 1));
      CHECK(!pitch_state_ok(c, e, std::max<int64_t>(0, s_prev - hi) + 1, s_prev));
      CHECK(!pitch_state_ok(c, e, -1, s_prev) && !pitch_state_ok(c, e, a_prev, -1));
    }
  }
}

int main() {
  case_config();
  case_table();
  case_plan();
  case_walks();
  printf("pitch_plan: ok\n");
  return 0;
}
