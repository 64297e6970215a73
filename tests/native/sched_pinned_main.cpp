// sched_pinned_main.cpp -- the pinned voice through the scheduler's rules (csrc/sched.h validate /
// admission_of / head_rows_of), as a stand-alone program for a plain C++17 compiler
// (tests/test_sched_pinned_cpu.py builds it under ASan + UBSan). The expected values follow
// include/rwkvtts.h: a pinned request is a normal-mode request whose prompt already holds what a
// normal request feeds itself up to TAG_1 (normal_mode_inference.rs:277-278).
#include "../../rwkv-tts-rs_amd/csrc/sched.h"

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

static const int32_t kProps[2] = {77823, 77838};
static const int32_t kText[3] = {21, 22, 23};
static const int32_t kRefS[2] = {1, 2};

static std::vector<int32_t> globals(int n) {
  std::vector<int32_t> g((size_t)n);
  for (int i = 0; i < n; ++i) g[(size_t)i] = (i * 131 + 7) % 4096;
  if (n > 0) g[0] = 0;
  if (n > 1) g[1] = 4095;  // both ends of the range are inside
  return g;
}

static rwkvtts_request request(const std::vector<int32_t>& g, bool pinned) {
  rwkvtts_request q;
  memset(&q, 0, sizeof(q));
  q.property_tokens = kProps;
  q.n_property = 2;
  q.text_tokens = kText;
  q.n_text = 3;
  q.has_seed = 1;
  q.seed = 7;
  q.max_tokens = 20;
  if (pinned) {
    q.ref_global = g.data();
    q.n_ref_global = (int32_t)g.size();
    q.pinned_voice = 1;
  }
  return q;
}

static bool ok(const rwkvtts_request& q) {
  std::string why;
  const bool r = validate(q, 77923, why);
  CHECK(r == why.empty());
  return r;
}

static void case_validate() {
  const std::vector<int32_t> g = globals(32);
  CHECK(ok(request(g, true)));
  CHECK(ok(request(g, false)));
  for (int n : {0, 1, 31, 33, 64}) {  // exactly 32 ids
    const std::vector<int32_t> h = globals(n);
    rwkvtts_request q = request(h, true);
    if (n == 0) q.ref_global = kRefS;  // (non-null, no ids)
    CHECK(!ok(q));
  }
  for (int pos : {0, 17, 31})
    for (int bad : {-1, 4096, 1 << 20}) {  // ids in [0, 4096)
      std::vector<int32_t> h = g;
      h[(size_t)pos] = bad;
      CHECK(!ok(request(h, true)));
    }
  {  // ref_semantic set, even empty
    rwkvtts_request q = request(g, true);
    q.ref_semantic = kRefS;
    q.n_ref_semantic = 2;
    CHECK(!ok(q));
    q.n_ref_semantic = 0;
    CHECK(!ok(q));
  }
  {  // ref_global NULL
    rwkvtts_request q = request(g, true);
    q.ref_global = nullptr;
    CHECK(!ok(q));
    q.n_ref_global = 0;
    CHECK(!ok(q));
  }
  for (int v : {2, -1, 256}) {  // only 0 and 1 have a meaning
    rwkvtts_request q = request(g, true);
    q.pinned_voice = v;
    CHECK(!ok(q));
  }
  {  // the model's vocabulary must hold the global tokens
    std::string why;
    CHECK(!validate(request(g, true), RWKVTTS_GLOBAL_TOKEN_OFFSET + 4095, why));
  }
  {  // without the flag, globals alone stay what they were: accepted, a normal request
    rwkvtts_request q = request(g, true);
    q.pinned_voice = 0;
    CHECK(ok(q) && !is_pinned(q) && !is_zero_shot(q));
  }
}

static void case_admission() {
  const std::vector<int32_t> g = globals(32);
  const rwkvtts_request n = request(g, false), p = request(g, true);
  const Admission an = admission_of(n, 999), ap = admission_of(p, 999);
  CHECK(!an.pinned && !an.zero_shot && ap.pinned && !ap.zero_shot);
  // prompt: property tokens, TAG_2, text, TAG_0, g + 8196 .., TAG_1 -- the normal prompt, then what
  // a normal request feeds itself
  std::vector<uint32_t> want = {77823, 77838, RWKVTTS_TAG_2, 21, 22, 23, RWKVTTS_TAG_0};
  CHECK(an.prompt == want);
  for (int i = 0; i < 32; ++i) want.push_back((uint32_t)(g[(size_t)i] + RWKVTTS_GLOBAL_TOKEN_OFFSET));
  want.push_back(RWKVTTS_TAG_1);
  CHECK(ap.prompt == want);
  // control block: mode 0 in the semantic phase with the globals in place, the rest a normal request's
  SlotCtrl c = an.ctrl;
  c.phase = kPhSemantic;
  c.n_global = 32;
  for (int i = 0; i < 32; ++i) c.global_out[i] = g[(size_t)i];
  CHECK(memcmp(&c, &ap.ctrl, sizeof(SlotCtrl)) == 0);
  CHECK(ap.ctrl.mode == 0 && ap.ctrl.hard_min == 0 && ap.ctrl.win_len == 0 && ap.ctrl.fixed == 0);
  CHECK(ap.ctrl.sem_limit == 20 && ap.ctrl.top_k_s == 80 && ap.ctrl.temp_s == 1.0f && ap.ctrl.top_p_s == 0.95f);
  CHECK(ap.ctrl.sdraw == 0 && ap.ctrl.n_sem == 0);
  // seeds as for a normal request: the semantic stream is seed + 2000 by default
  CHECK(ap.sseed == an.sseed && ap.sseed == 7 + 2000 && ap.gseed == an.gseed);
  CHECK(ap.kind == an.kind && ap.kind == kAdvFixed);
  // total: the semantic limit (a normal request: 32 globals, the g31 feed, then the limit)
  CHECK(an.total == 32 + 1 + 20 && ap.total == 20);
  {  // layered randomness, fixed_semantic and per-request sampling as for a normal request
    rwkvtts_request q = p, m = n;
    for (rwkvtts_request* r : {&q, &m}) {
      r->layered_set = 1;
      r->use_independent_seeds = 0;
      r->fixed_semantic = 40;
      r->sampling_set = RWKVTTS_SAMPLING_SEMANTIC;
      r->semantic_sampling = {0.8f, 0.9f, 50};
    }
    const Admission aq = admission_of(q, 999), am = admission_of(m, 999);
    CHECK(aq.sseed == 7 + 200 && aq.sseed == am.sseed);
    CHECK(aq.ctrl.fixed == 1 && aq.ctrl.sem_limit == 40 && aq.total == 40 && am.total == 73);
    CHECK(aq.ctrl.temp_s == 0.8f && aq.ctrl.top_p_s == 0.9f && aq.ctrl.top_k_s == 50 && aq.kind == kAdvParams && am.kind == kAdvParams);
  }
  {  // no seed: the entropy stands in, as for a normal request
    rwkvtts_request q = p;
    q.has_seed = 0;
    CHECK(admission_of(q, 999).sseed == 999 + 2000);
  }
  {  // max_tokens above the limit
    rwkvtts_request q = p;
    q.max_tokens = 8000;
    CHECK(admission_of(q, 999).total == RWKVTTS_SEMANTIC_LIMIT);
  }
}

static void case_without_tokens() {
  const std::vector<int32_t> g = globals(32);
  rwkvtts_request q = request(g, true);
  CHECK(!pinned_without_tokens(q));
  q.max_tokens = 0;
  CHECK(ok(q) && pinned_without_tokens(q));  // ends at admission: 32 globals, no semantic tokens, no slot
  q.fixed_semantic = 4;                      // benchmark mode emits its tokens whatever max_tokens says
  CHECK(!pinned_without_tokens(q) && admission_of(q, 1).total == 4);
  rwkvtts_request n = request(g, false);
  n.max_tokens = 0;
  CHECK(!pinned_without_tokens(n) && admission_of(n, 1).total == 33);  // a normal request still samples its globals
}

static Active active_of(const Admission& a, int slot) {
  Active x;
  x.slot = slot;
  x.prompt = a.prompt;
  x.total = a.total;
  x.zero_shot = a.zero_shot;
  x.pinned = a.pinned;
  x.kind = a.kind;
  return x;
}

static void case_head_rows() {
  const std::vector<int32_t> g = globals(32);
  const Admission ap = admission_of(request(g, true), 1), an = admission_of(request(g, false), 1);
  const int V = 65536;
  {  // a normal slot alone samples globals from 4096 head rows ...
    std::vector<Active> act = {active_of(an, 0)};
    const StepPlan p = mixed_plan(act, 128, V);
    CHECK(p.head_rows == 4096 && p.lg_rows.size() == 1);
  }
  {  // ... a pinned slot needs the semantic rows from its first logits row
    std::vector<Active> act = {active_of(ap, 0)};
    const StepPlan p = mixed_plan(act, 128, V);
    CHECK(p.head_rows == 8193 && p.lg_rows.size() == 1 && p.lg_rows[0] == (int)ap.prompt.size() - 1);
    CHECK(p.tok.size() == ap.prompt.size() && p.tok.back() == RWKVTTS_TAG_1);
    CHECK(act[0].advances == 1 && !act[0].in_prompt());
    CHECK(head_rows_of(act, V) == 8193);
    CHECK(window_len(act, 8, false) == 8);
    act[0].advances = 19;
    CHECK(window_len(act, 8, false) == 1 && head_rows_of(act, V) == 8193);
  }
  {  // a prompt that spans two mixed steps: no logits row, then the first one
    std::vector<Active> act = {active_of(ap, 0)};
    const StepPlan p1 = mixed_plan(act, 16, V);
    CHECK(p1.lg_rows.empty() && act[0].prefilled == 16 && act[0].advances == 0);
    CHECK(p1.head_rows == 4096);  // (no logits row in the step: nothing is sampled)
    const StepPlan p2 = mixed_plan(act, 64, V);
    CHECK(p2.lg_rows.size() == 1 && p2.head_rows == 8193 && act[0].advances == 1);
  }
  {  // beside a normal slot still in its global phase, the step carries the semantic rows
    std::vector<Active> act = {active_of(an, 0), active_of(ap, 1)};
    const StepPlan p = mixed_plan(act, 128, V);
    CHECK(p.head_rows == 8193 && p.lg_rows.size() == 2);
    CHECK(head_rows_of(act, V) == 8193);
    act.pop_back();
    CHECK(head_rows_of(act, V) == 4096);
  }
  // token progress: the range a unit may have added starts at the first advance
  const ProgressRange r = progress_range(0, ap.ctrl.sem_limit, 1);
  CHECK(r.lo == 0 && r.hi == 1);
}

// A zeroed request's admission is what it was before the field existed, and the field is the
// struct's last.
static void case_zeroed() {
  rwkvtts_request q = request(globals(32), false);
  const Admission a = admission_of(q, 999);
  SlotCtrl want;
  memset(&want, 0, sizeof(want));
  want.phase = kPhGlobal;
  want.sem_limit = 20;
  want.top_k_g = 20;
  want.top_k_s = 80;
  want.temp_g = want.temp_s = 1.0f;
  want.top_p_g = want.top_p_s = 0.95f;
  CHECK(memcmp(&a.ctrl, &want, sizeof(SlotCtrl)) == 0);
  CHECK(a.prompt.size() == 7 && a.total == 53 && a.gseed == 1007 && a.sseed == 2007 && !a.pinned && !a.zero_shot);
  CHECK(offsetof(rwkvtts_request, pinned_voice) + sizeof(int32_t) <= sizeof(rwkvtts_request));
  CHECK(offsetof(rwkvtts_request, pinned_voice) >= offsetof(rwkvtts_request, semantic_sampling) + sizeof(rwkvtts_phase_sampling));
  // zero-shot is untouched by the flag's absence
  q.ref_global = kRefS;
  q.n_ref_global = 2;
  q.ref_semantic = kRefS;
  q.n_ref_semantic = 2;
  const Admission z = admission_of(q, 999);
  CHECK(z.zero_shot && !z.pinned && z.ctrl.mode == 1 && z.prompt.size() == 7 + 2 + 1);
}

int main() {
  case_validate();
  case_admission();
  case_without_tokens();
  case_head_rows();
  case_zeroed();
  if (g_fail) {
    fprintf(stderr, "sched pinned: %d check(s) failed\n", g_fail);
    return 1;
  }
  printf("sched pinned: ok\n");
  return 0;
}
