// sched_sampling_main.cpp -- per-request sampling parameters through the scheduler's rules
// (csrc/sched.h validate / admission_of), as a stand-alone program for a plain C++17 compiler
// (tests/test_sched_sampling_cpu.py builds it under ASan + UBSan). The expected values follow
// include/rwkvtts.h: a phase whose sampling_set bit is clear keeps the reference's
// (1.0, 0.95, 20 | 80) of normal_mode_inference.rs:114-127.
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

static rwkvtts_request request(bool zero_shot) {
  rwkvtts_request q;
  memset(&q, 0, sizeof(q));
  q.property_tokens = kProps;
  q.n_property = 2;
  q.text_tokens = kText;
  q.n_text = 3;
  q.has_seed = 1;
  q.seed = 7;
  q.max_tokens = 20;
  if (zero_shot) {
    q.ref_global = kRefG;
    q.n_ref_global = 2;
    q.ref_semantic = kRefS;
    q.n_ref_semantic = 2;
  }
  return q;
}

static bool ok(const rwkvtts_request& q) {
  std::string why;
  const bool r = validate(q, 65536, why);
  CHECK(r == why.empty());
  return r;
}

static void case_validate() {
  const rwkvtts_phase_sampling good = {0.8f, 0.9f, 50};
  for (int zs = 0; zs < 2; ++zs) {
    rwkvtts_request q = request(zs != 0);
    CHECK(ok(q));
    for (int bits = 1; bits <= 3; ++bits) {
      for (int which = 0; which < 2; ++which) {  // the phase that carries the bad value
        if (!(bits & (1 << which))) continue;
        auto with = [&](rwkvtts_phase_sampling s) {
          rwkvtts_request v = q;
          v.sampling_set = bits;
          v.global_sampling = v.semantic_sampling = good;
          (which == 0 ? v.global_sampling : v.semantic_sampling) = s;
          return v;
        };
        CHECK(ok(with(good)));
        // the range ends are inside
        CHECK(ok(with({0.1f, 0.0f, 0})));
        CHECK(ok(with({4.0f, 1.0f, 1 << 30})));
        // non-finite values
        CHECK(!ok(with({NAN, 0.9f, 50})));
        CHECK(!ok(with({INFINITY, 0.9f, 50})));
        CHECK(!ok(with({0.8f, NAN, 50})));
        CHECK(!ok(with({0.8f, INFINITY, 50})));
        // temperature outside [0.1, 4.0]
        CHECK(!ok(with({0.0f, 0.9f, 50})));
        CHECK(!ok(with({nextafterf(0.1f, 0.0f), 0.9f, 50})));
        CHECK(!ok(with({nextafterf(4.0f, 5.0f), 0.9f, 50})));
        CHECK(!ok(with({-1.0f, 0.9f, 50})));
        // top_p outside [0, 1]
        CHECK(!ok(with({0.8f, -0.0001f, 50})));
        CHECK(!ok(with({0.8f, nextafterf(1.0f, 2.0f), 50})));
        // top_k < 0
        CHECK(!ok(with({0.8f, 0.9f, -1})));
      }
    }
    {  // a bad value in a phase whose bit is clear is not looked at
      rwkvtts_request v = q;
      v.sampling_set = RWKVTTS_SAMPLING_SEMANTIC;
      v.semantic_sampling = good;
      v.global_sampling = {NAN, 7.0f, -3};
      CHECK(ok(v));
    }
    {  // unknown bits
      rwkvtts_request v = q;
      v.global_sampling = v.semantic_sampling = good;
      v.sampling_set = 4;
      CHECK(!ok(v));
      v.sampling_set = 3 | 8;
      CHECK(!ok(v));
      v.sampling_set = -1;
      CHECK(!ok(v));
    }
    {  // greedy together with sampling_set
      rwkvtts_request v = q;
      v.global_sampling = v.semantic_sampling = good;
      v.greedy = 1;
      CHECK(ok(v));
      v.sampling_set = RWKVTTS_SAMPLING_SEMANTIC;
      CHECK(!ok(v));
    }
  }
}

static void expect(const SlotCtrl& c, float tg, float pg, int kg, float ts, float ps, int ks) {
  CHECK(c.temp_g == tg && c.top_p_g == pg && c.top_k_g == kg);
  CHECK(c.temp_s == ts && c.top_p_s == ps && c.top_k_s == ks);
}

static void case_admission() {
  const rwkvtts_phase_sampling G = {0.7f, 0.5f, 0}, S = {1.3f, 1.0f, 300};
  for (int zs = 0; zs < 2; ++zs) {
    rwkvtts_request q = request(zs != 0);
    const Admission a0 = admission_of(q, 999);
    expect(a0.ctrl, 1.0f, 0.95f, 20, 1.0f, 0.95f, 80);
    CHECK(a0.kind == kAdvFixed);
    q.global_sampling = G;  // present but not set: unused
    q.semantic_sampling = S;
    const Admission a0b = admission_of(q, 999);
    CHECK(memcmp(&a0.ctrl, &a0b.ctrl, sizeof(SlotCtrl)) == 0 && a0b.kind == kAdvFixed);

    q.sampling_set = RWKVTTS_SAMPLING_GLOBAL;
    const Admission a1 = admission_of(q, 999);
    expect(a1.ctrl, 0.7f, 0.5f, 0, 1.0f, 0.95f, 80);
    CHECK(a1.kind == kAdvParams);
    q.sampling_set = RWKVTTS_SAMPLING_SEMANTIC;
    const Admission a2 = admission_of(q, 999);
    expect(a2.ctrl, 1.0f, 0.95f, 20, 1.3f, 1.0f, 300);
    CHECK(a2.kind == kAdvParams);
    q.sampling_set = RWKVTTS_SAMPLING_GLOBAL | RWKVTTS_SAMPLING_SEMANTIC;
    const Admission a3 = admission_of(q, 999);
    expect(a3.ctrl, 0.7f, 0.5f, 0, 1.3f, 1.0f, 300);
    // the mode's own fields are those of the request without sampling
    for (const Admission* a : {&a1, &a2, &a3}) {
      CHECK(a->zero_shot == (zs != 0) && a->ctrl.mode == zs && a->ctrl.phase == (zs ? kPhSemantic : kPhGlobal));
      CHECK(a->prompt == a0.prompt && a->total == a0.total && a->gseed == a0.gseed && a->sseed == a0.sseed);
      CHECK(a->ctrl.sem_limit == a0.ctrl.sem_limit && a->ctrl.hard_min == a0.ctrl.hard_min);
    }
    // only top-k set away from the phase's own: the compiled-in (1.0, 0.95) controller still serves
    q.sampling_set = RWKVTTS_SAMPLING_SEMANTIC;
    q.semantic_sampling = {1.0f, 0.95f, 50};
    const Admission a4 = admission_of(q, 999);
    expect(a4.ctrl, 1.0f, 0.95f, 20, 1.0f, 0.95f, 50);
    CHECK(a4.kind == kAdvFixed);
    // ... while a top-k outside the fast path's [1, 256] needs the controller with the general path
    for (int k : {0, 257, 8193}) {
      q.semantic_sampling.top_k = k;
      CHECK(admission_of(q, 999).kind == kAdvParams);
    }
    q.semantic_sampling.top_k = 256;
    CHECK(admission_of(q, 999).kind == kAdvFixed);
  }
}

// A zeroed request's control block, outside the new fields, is byte for byte what it was before
// the fields existed: every earlier field keeps its offset (the new ones are appended), and the
// values are the ones tests/native/sched_main.cpp states.
static void case_zeroed_block() {
  const rwkvtts_request q = request(false);
  const Admission a = admission_of(q, 999);
  SlotCtrl want;
  memset(&want, 0, sizeof(want));
  want.mode = 0;
  want.phase = kPhGlobal;
  want.sem_limit = 20;
  want.top_k_g = 20;
  want.top_k_s = 80;
  const size_t old_size = offsetof(SlotCtrl, temp_g);
  CHECK(old_size == 14 * 4 + 2 * 32 + 2 * 8 + 32 * 4 + 2 * 8 + 2 * 64);  // the block as it was
  CHECK(offsetof(SlotCtrl, next_token) == 9 * 4 && offsetof(SlotCtrl, gkey) == 14 * 4);
  CHECK(sizeof(SlotCtrl) == old_size + 16 && sizeof(SlotCtrl) % 8 == 0);
  CHECK(memcmp(&a.ctrl, &want, old_size) == 0);
  // the plans carry the flag of the requests they hold
  std::vector<Active> act(2);
  act[0].slot = 0;
  act[0].prompt = {1, 2};
  act[0].prefilled = 2;
  act[0].total = 50;
  act[1] = act[0];
  act[1].slot = 1;
  CHECK(decode_plan(act).kind == kAdvFixed);
  act[1].kind = kAdvParams;
  CHECK(decode_plan(act).kind == kAdvParams);
  std::vector<Active> m = act;
  CHECK(mixed_plan(m, 8, 65536).kind == kAdvParams);
  m = act;
  m[1].kind = kAdvFixed;
  CHECK(mixed_plan(m, 8, 65536).kind == kAdvFixed);
}

int main() {
  case_validate();
  case_admission();
  case_zeroed_block();
  if (g_fail) {
    fprintf(stderr, "sched sampling: %d check(s) failed\n", g_fail);
    return 1;
  }
  printf("sched sampling: ok\n");
  return 0;
}
