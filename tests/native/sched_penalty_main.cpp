// sched_penalty_main.cpp -- per-request penalties through the scheduler's rules (csrc/sched.h
// validate / admission_of / the plans), as a stand-alone program for a plain C++17 compiler
// (tests/test_sched_penalty_cpu.py builds it under ASan + UBSan). The expected values follow
// include/rwkvtts.h: repetition in [0.25, 4], frequency and presence in [-8, 8], window in
// [0, 2048], all finite; penalty_set bit 0 alone; allowed with greedy; (1, 0, 0) keeps the request
// on the controller it had.
#include "../../rwkv-tts-rs_amd/csrc/sched.h"

#include <math.h>
#include <stddef.h>
#include <stdio.h>

using namespace rwkvtts;

static int g_fail = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #cond); \
      ++g_fail;                                                  \
    }                                                            \
  } while (0)

static const int32_t kProps[2] = {11, 12};
static const int32_t kText[3] = {21, 22, 23};
static const int32_t kRefG[2] = {5, 6};
static const int32_t kRefS[2] = {1, 2};
static int32_t g_pin[RWKVTTS_N_GLOBAL];

enum Kind { kNormal, kZeroShot, kPinned };

static rwkvtts_request request(Kind kind) {
  rwkvtts_request q;
  memset(&q, 0, sizeof(q));
  q.property_tokens = kProps;
  q.n_property = 2;
  q.text_tokens = kText;
  q.n_text = 3;
  q.has_seed = 1;
  q.seed = 7;
  q.max_tokens = 20;
  if (kind == kZeroShot) {
    q.ref_global = kRefG;
    q.n_ref_global = 2;
    q.ref_semantic = kRefS;
    q.n_ref_semantic = 2;
  } else if (kind == kPinned) {
    for (int i = 0; i < RWKVTTS_N_GLOBAL; ++i) g_pin[i] = 100 + i;
    q.ref_global = g_pin;
    q.n_ref_global = RWKVTTS_N_GLOBAL;
    q.pinned_voice = 1;
  }
  return q;
}

static bool ok(const rwkvtts_request& q) {
  std::string why;
  const bool r = validate(q, 65536, why);
  CHECK(r == why.empty());
  return r;
}

static bool same_pen(const SlotPenalty& p, float r, float f, float s, int w) {
  return p.repetition == r && p.frequency == f && p.presence == s && p.window == w;
}

static void case_validate() {
  for (Kind kind : {kNormal, kZeroShot, kPinned}) {
    const rwkvtts_request q = request(kind);
    CHECK(ok(q));
    auto with = [&](rwkvtts_penalties p) {
      rwkvtts_request v = q;
      v.penalty_set = RWKVTTS_PENALTY_SET;
      v.penalties = p;
      return v;
    };
    CHECK(ok(with({1.3f, 0.7f, 1.5f, 64})));
    CHECK(ok(with({1.0f, 0.0f, 0.0f, 0})));  // neutral values are valid
    // the range ends are inside ...
    CHECK(ok(with({0.25f, -8.0f, -8.0f, 0})));
    CHECK(ok(with({4.0f, 8.0f, 8.0f, 2048})));
    // ... and the next value on either side is not
    CHECK(!ok(with({nextafterf(0.25f, 0.0f), 0.0f, 0.0f, 0})));
    CHECK(!ok(with({nextafterf(4.0f, 5.0f), 0.0f, 0.0f, 0})));
    CHECK(!ok(with({1.0f, nextafterf(-8.0f, -9.0f), 0.0f, 0})));
    CHECK(!ok(with({1.0f, nextafterf(8.0f, 9.0f), 0.0f, 0})));
    CHECK(!ok(with({1.0f, 0.0f, nextafterf(-8.0f, -9.0f), 0})));
    CHECK(!ok(with({1.0f, 0.0f, nextafterf(8.0f, 9.0f), 0})));
    CHECK(!ok(with({1.0f, 0.0f, 0.0f, -1})));
    CHECK(!ok(with({1.0f, 0.0f, 0.0f, 2049})));
    // repetition 0 and negative (a zero-filled struct with the bit set is refused)
    CHECK(!ok(with({0.0f, 0.0f, 0.0f, 0})));
    CHECK(!ok(with({-1.3f, 0.0f, 0.0f, 0})));
    // non-finite values
    for (float bad : {NAN, INFINITY, -INFINITY}) {
      CHECK(!ok(with({bad, 0.0f, 0.0f, 0})));
      CHECK(!ok(with({1.0f, bad, 0.0f, 0})));
      CHECK(!ok(with({1.0f, 0.0f, bad, 0})));
    }
    {  // bad values behind a clear bit are not looked at
      rwkvtts_request v = with({NAN, 99.0f, -99.0f, -5});
      v.penalty_set = 0;
      CHECK(ok(v));
    }
    for (int bits : {2, 3, 4, 1 | 8, -1, 1 << 30}) {  // unknown bits, with or without bit 0
      rwkvtts_request v = with({1.3f, 0.0f, 0.0f, 0});
      v.penalty_set = bits;
      CHECK(!ok(v));
    }
    {  // allowed with greedy (sampling_set is not), and with sampling_set and fixed_semantic
      rwkvtts_request v = with({1.3f, 0.7f, 0.0f, 16});
      v.greedy = 1;
      CHECK(ok(v));
      v.greedy = 0;
      v.sampling_set = RWKVTTS_SAMPLING_SEMANTIC;
      v.semantic_sampling = {0.8f, 0.95f, 80};
      v.fixed_semantic = 20;
      CHECK(ok(v));
      v.greedy = 1;  // greedy with sampling_set stays refused
      CHECK(!ok(v));
    }
  }
}

static void case_admission() {
  for (Kind kind : {kNormal, kZeroShot, kPinned}) {
    rwkvtts_request q = request(kind);
    const Admission a0 = admission_of(q, 999);
    CHECK(same_pen(a0.samp.pen, 1.0f, 0.0f, 0.0f, 0) && a0.kind == kAdvFixed);
    q.penalties = {1.3f, 0.7f, 1.5f, 64};  // present but not set: unused
    const Admission a0b = admission_of(q, 999);
    CHECK(same_pen(a0b.samp.pen, 1.0f, 0.0f, 0.0f, 0) && a0b.kind == kAdvFixed);
    CHECK(memcmp(&a0.ctrl, &a0b.ctrl, sizeof(SlotCtrl)) == 0);

    q.penalty_set = RWKVTTS_PENALTY_SET;
    const Admission a1 = admission_of(q, 999);  // normal, zero-shot and pinned admissions carry the values
    CHECK(same_pen(a1.samp.pen, 1.3f, 0.7f, 1.5f, 64) && a1.kind == kAdvParams);
    // everything else is the request's without penalties: the control block byte for byte
    CHECK(memcmp(&a0.ctrl, &a1.ctrl, sizeof(SlotCtrl)) == 0);
    CHECK(a1.zero_shot == (kind == kZeroShot) && a1.pinned == (kind == kPinned));
    CHECK(a1.ctrl.mode == (kind == kZeroShot ? 1 : 0) && a1.ctrl.phase == (kind == kNormal ? kPhGlobal : kPhSemantic));
    CHECK(a1.ctrl.n_sem == 0);  // the kernel zeroes a slot's counts at n_sem == 0
    CHECK(a1.prompt == a0.prompt && a1.total == a0.total && a1.gseed == a0.gseed && a1.sseed == a0.sseed);

    // neutral values leave the request on the default controller, whatever the window
    q.penalties = {1.0f, 0.0f, 0.0f, 32};
    const Admission a2 = admission_of(q, 999);
    CHECK(same_pen(a2.samp.pen, 1.0f, 0.0f, 0.0f, 32) && a2.kind == kAdvFixed);
    // each value alone moves it
    for (rwkvtts_penalties p : {rwkvtts_penalties{0.8f, 0.0f, 0.0f, 0}, rwkvtts_penalties{1.0f, -0.5f, 0.0f, 0},
                                rwkvtts_penalties{1.0f, 0.0f, 1.5f, 0}}) {
      q.penalties = p;
      CHECK(admission_of(q, 999).kind == kAdvParams);
    }
    // greedy with penalties: top-k 1 at (1.0, 0.95) through the parameter-reading controller
    q.penalties = {1.3f, 0.0f, 0.0f, 0};
    q.greedy = 1;
    const Admission a3 = admission_of(q, 999);
    CHECK(a3.kind == kAdvParams && a3.ctrl.top_k_g == 1 && a3.ctrl.top_k_s == 1);
    CHECK(a3.ctrl.temp_s == 1.0f && a3.ctrl.top_p_s == 0.95f && a3.ctrl.temp_g == 1.0f && a3.ctrl.top_p_g == 0.95f);
    q.penalty_set = 0;
    CHECK(admission_of(q, 999).kind == kAdvFixed);  // greedy alone stays on the default controller
    // together with sampling_set: both sets of values arrive
    q.greedy = 0;
    q.penalty_set = RWKVTTS_PENALTY_SET;
    q.sampling_set = RWKVTTS_SAMPLING_SEMANTIC;
    q.semantic_sampling = {0.8f, 0.9f, 40};
    const Admission a4 = admission_of(q, 999);
    CHECK(a4.kind == kAdvParams && a4.ctrl.temp_s == 0.8f && a4.ctrl.top_k_s == 40 && same_pen(a4.samp.pen, 1.3f, 0.0f, 0.0f, 0));
  }
}

// A zeroed request's control block is byte for byte what it was before penalties existed (they live
// beside it, in SlotPenalty), with the values tests/native/sched_main.cpp states.
static void case_zeroed_block() {
  const rwkvtts_request q = request(kNormal);
  const Admission a = admission_of(q, 999);
  SlotCtrl want;
  memset(&want, 0, sizeof(want));
  want.mode = 0;
  want.phase = kPhGlobal;
  want.sem_limit = 20;
  want.top_k_g = 20;
  want.top_k_s = 80;
  want.temp_g = want.temp_s = 1.0f;
  want.top_p_g = want.top_p_s = 0.95f;
  CHECK(sizeof(SlotCtrl) == offsetof(SlotCtrl, temp_g) + 16 && sizeof(SlotCtrl) % 8 == 0);
  CHECK(memcmp(&a.ctrl, &want, sizeof(SlotCtrl)) == 0);
  CHECK(sizeof(SlotPenalty) == 16 && same_pen(a.samp.pen, 1.0f, 0.0f, 0.0f, 0));
  // the request struct: the new fields are appended after pinned_voice
  CHECK(offsetof(rwkvtts_request, penalty_set) == offsetof(rwkvtts_request, pinned_voice) + 4);
  CHECK(offsetof(rwkvtts_request, penalties) == offsetof(rwkvtts_request, penalty_set) + 4);
  CHECK(sizeof(rwkvtts_penalties) == 16);
}

// The plans carry the flag of the requests they hold: through admission_of, not set by hand.
static void case_plans() {
  rwkvtts_request plain = request(kNormal), neutral = plain, pen = plain;
  neutral.penalty_set = pen.penalty_set = RWKVTTS_PENALTY_SET;
  neutral.penalties = {1.0f, 0.0f, 0.0f, 8};
  pen.penalties = {1.0f, 0.0f, 0.5f, 8};
  auto active = [](const rwkvtts_request& q, int slot, bool prompt_in) {
    Admission ad = admission_of(q, 999);
    Active a;
    a.slot = slot;
    a.kind = ad.kind;  // as Engine::admit copies it
    a.prompt = ad.prompt;
    a.prefilled = prompt_in ? (int)a.prompt.size() : 0;
    a.total = ad.total;
    return a;
  };
  std::vector<Active> act = {active(plain, 0, true), active(neutral, 1, true)};
  CHECK(decode_plan(act).kind == kAdvFixed);
  std::vector<Active> m = act;
  CHECK(mixed_plan(m, 8, 65536).kind == kAdvFixed);
  act.push_back(active(pen, 2, true));
  CHECK(decode_plan(act).kind == kAdvParams);
  m = act;
  CHECK(mixed_plan(m, 8, 65536).kind == kAdvParams);
  // a penalised request still in its prompt already selects the controller of the mixed step
  m = {active(plain, 0, true), active(pen, 1, false)};
  CHECK(mixed_plan(m, 8, 65536).kind == kAdvParams);
}

int main() {
  case_validate();
  case_admission();
  case_zeroed_block();
  case_plans();
  if (g_fail) {
    fprintf(stderr, "sched penalty: %d check(s) failed\n", g_fail);
    return 1;
  }
  printf("sched penalty: ok\n");
  return 0;
}
