// sched_main.cpp -- the scheduler's rules (csrc/sched.h) on hand-worked cases, as a stand-alone
// program for a plain C++17 compiler (tests/test_sched_cpu.py builds it under ASan + UBSan).
// The expected values are worked out from the rules as the reference states them
// (dynamic_batch_manager.rs, normal_mode_inference.rs, zero_shot_inference.rs), not taken from a
// run of the code under test.
#include "../../rwkv-tts-rs_amd/csrc/sched.h"

#include <stdio.h>
#include <stdlib.h>

#include <random>

using namespace rwkvtts;

static int g_fail = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #cond); \
      ++g_fail;                                                  \
    }                                                            \
  } while (0)

static bool same(const Int4& a, int x, int y, int z, int w) { return a.x == x && a.y == y && a.z == z && a.w == w; }

static const int32_t kProps[2] = {11, 12};
static const int32_t kText[3] = {21, 22, 23};

static rwkvtts_request normal_request() {
  rwkvtts_request q;
  memset(&q, 0, sizeof(q));
  q.property_tokens = kProps;
  q.n_property = 2;
  q.text_tokens = kText;
  q.n_text = 3;
  q.has_seed = 1;
  q.seed = 7;
  q.max_tokens = 20;
  return q;
}

// a slot past its prompt (2 tokens, both in) after `advances` controller steps
static Active decoding(int slot, int advances, int total, bool zero_shot = false) {
  Active a;
  a.slot = slot;
  a.prompt = {1, 2};
  a.prefilled = 2;
  a.advances = advances;
  a.total = total;
  a.zero_shot = zero_shot;
  return a;
}
// a slot with `n` prompt tokens (100 * slot + i), `prefilled` of them in
static Active prompting(int slot, int n, int prefilled = 0, bool zero_shot = false) {
  Active a;
  a.slot = slot;
  for (int i = 0; i < n; ++i) a.prompt.push_back((uint32_t)(100 * slot + i));
  a.prefilled = prefilled;
  a.total = 1 << 20;
  a.zero_shot = zero_shot;
  return a;
}

static void case1_normal() {
  const rwkvtts_request q = normal_request();
  const Admission a = admission_of(q, 999);
  const std::vector<uint32_t> want = {11, 12, RWKVTTS_TAG_2, 21, 22, 23, RWKVTTS_TAG_0};
  CHECK(a.prompt == want);
  CHECK(!a.zero_shot && a.ctrl.mode == 0 && a.ctrl.phase == kPhGlobal);
  CHECK(a.ctrl.top_k_g == 20 && a.ctrl.top_k_s == 80);
  CHECK(a.ctrl.fixed == 0 && a.ctrl.sem_limit == 20 && a.total == 53);
  CHECK(a.gseed == 1007 && a.sseed == 2007);
  CHECK(a.ctrl.n_global == 0 && a.ctrl.n_sem == 0 && a.ctrl.hard_min == 0);
  for (int i = 0; i < 8; ++i) CHECK(a.ctrl.gkey[i] == 0 && a.ctrl.skey[i] == 0);
  {
    rwkvtts_request v = q;  // no seed: the entropy value
    v.has_seed = 0;
    const Admission b = admission_of(v, 999);
    CHECK(b.gseed == 1999 && b.sseed == 2999);
  }
  {
    rwkvtts_request v = q;
    v.layered_set = 1;
    v.use_independent_seeds = 0;
    const Admission b = admission_of(v, 999);
    CHECK(b.gseed == 107 && b.sseed == 207);
  }
  {
    rwkvtts_request v = q;
    v.layered_set = 1;
    v.use_independent_seeds = 1;
    v.global_seed_offset = 7;
    v.semantic_seed_offset = 9;
    const Admission b = admission_of(v, 999);
    CHECK(b.gseed == 14 && b.sseed == 16);
  }
  {
    rwkvtts_request v = q;
    v.greedy = 1;
    const Admission b = admission_of(v, 999);
    CHECK(b.ctrl.top_k_g == 1 && b.ctrl.top_k_s == 1);
  }
  {
    rwkvtts_request v = q;
    v.max_tokens = 5000;
    const Admission b = admission_of(v, 999);
    CHECK(b.ctrl.sem_limit == 2048 && sem_limit_of(v) == 2048 && b.total == 32 + 1 + 2048);
  }
  {
    rwkvtts_request v = q;
    v.fixed_semantic = 64;
    const Admission b = admission_of(v, 999);
    CHECK(b.ctrl.fixed == 1 && b.ctrl.sem_limit == 64 && b.total == 32 + 1 + 64);
  }
}

static void case2_zero_shot() {
  static const int32_t ref_g[3] = {-5, 17, 9000};
  static const int32_t ref_s[2] = {1, 2};
  rwkvtts_request q = normal_request();
  q.ref_global = ref_g;
  q.n_ref_global = 3;
  q.ref_semantic = ref_s;
  q.n_ref_semantic = 2;
  const Admission a = admission_of(q, 999);
  const std::vector<uint32_t> want = {11, 12, RWKVTTS_TAG_2, 21, 22, 23, RWKVTTS_TAG_0, 8196 + 0, 8196 + 17, 8196 + 4095,
                                      RWKVTTS_TAG_1};
  CHECK(a.prompt == want);
  CHECK(a.ctrl.n_global == 3 && a.ctrl.global_out[0] == 0 && a.ctrl.global_out[1] == 17 && a.ctrl.global_out[2] == 4095);
  CHECK(a.zero_shot && a.ctrl.mode == 1 && a.ctrl.phase == kPhSemantic);
  CHECK(a.ctrl.sem_limit == 2048 && a.total == 2048);
  CHECK(a.gseed == 1007 && a.sseed == 2007);
  // hard_min = min(floorf(2048 * 0.9f), max(clamp(n / 4, 8, 64), ceilf(n * 1.8f)))
  static const int n_text[8] = {0, 4, 5, 10, 36, 256, 1024, 2000};
  static const int hard_min[8] = {8, 8, 9, 18, 65, 461, 1843, 1843};
  std::vector<int32_t> text(2000, 5);
  for (int i = 0; i < 8; ++i) {
    rwkvtts_request v = q;
    v.text_tokens = text.data();
    v.n_text = n_text[i];
    CHECK(admission_of(v, 999).ctrl.hard_min == hard_min[i]);
  }
  {
    rwkvtts_request v = q;
    v.layered_set = 1;
    v.use_independent_seeds = 0;
    const Admission b = admission_of(v, 999);
    CHECK(b.gseed == 107 && b.sseed == 0);
  }
  {
    std::vector<int32_t> g40(40);
    for (int i = 0; i < 40; ++i) g40[i] = i;
    rwkvtts_request v = q;
    v.ref_global = g40.data();
    v.n_ref_global = 40;
    const Admission b = admission_of(v, 999);
    CHECK(b.prompt.size() == 7 + 40 + 1 && b.ctrl.n_global == 32);
    CHECK(b.prompt[7 + 39] == 8196 + 39 && b.prompt.back() == RWKVTTS_TAG_1 && b.ctrl.global_out[31] == 31);
  }
}

static void case3_validate() {
  std::string why;
  const rwkvtts_request q = normal_request();
  CHECK(validate(q, 65536, why));
  {
    static const int32_t bad[3] = {21, 70000, 23};
    rwkvtts_request v = q;
    v.text_tokens = bad;
    CHECK(!validate(v, 65536, why));
    CHECK(why == "text_tokens: id 70000 out of range");
    v = q;
    v.property_tokens = bad;
    v.n_property = 3;
    CHECK(!validate(v, 65536, why));
    CHECK(why == "property_tokens: id 70000 out of range");
  }
  {
    rwkvtts_request v = q;
    v.max_tokens = -1;
    CHECK(!validate(v, 65536, why));
    CHECK(why == "max_tokens / fixed_semantic must be >= 0");
  }
  CHECK(!validate(q, 8195, why));
  CHECK(why == "model vocabulary too small for the TTS tags / global tokens");
}

static void case4_mixed_all_global() {
  std::vector<Active> act = {decoding(0, 5, 53), prompting(1, 5), prompting(2, 6)};
  const StepPlan p = mixed_plan(act, 8, 65536);
  static const int rows[8][4] = {{0, 7, -1, 0}, {1, 1, -1, 0}, {1, 0, 1, 0}, {1, 0, 2, 0},
                                 {1, 0, 3, 0},  {1, 2, 4, 0},  {2, 1, -1, 0}, {2, 2, 6, 0}};
  CHECK(p.rows.size() == 8);
  for (size_t i = 0; i < 8 && i < p.rows.size(); ++i) CHECK(same(p.rows[i], rows[i][0], rows[i][1], rows[i][2], rows[i][3]));
  CHECK((p.tok == std::vector<uint32_t>{0, 100, 101, 102, 103, 104, 200, 201}));
  CHECK(p.segs.size() == 3);
  if (p.segs.size() == 3) CHECK(same(p.segs[0], 0, 0, 1, 0) && same(p.segs[1], 1, 1, 5, 0) && same(p.segs[2], 2, 6, 2, 0));
  CHECK((p.lg_rows == std::vector<int>{0, 5}) && (p.lg_slot == std::vector<int>{0, 1}));
  CHECK(p.head_rows == 4096 && p.advance && !p.tok_from_ctrl);
  CHECK(act[0].advances == 6 && act[0].prefilled == 2);
  CHECK(act[1].prefilled == 5 && act[1].advances == 1);
  CHECK(act[2].prefilled == 2 && act[2].advances == 0);
}

static void case5_budget_floor() {
  std::vector<Active> act = {decoding(0, 40, 2048), decoding(1, 3, 2048), prompting(2, 9, 5)};
  const StepPlan p = mixed_plan(act, 2, 65536);
  CHECK(p.rows.size() == 3 && p.segs.size() == 3);
  if (p.rows.size() == 3) CHECK(same(p.rows[2], 2, kRowFirst | kRowLast, -1, 0) && p.rows[2].y == 3);
  CHECK((p.tok == std::vector<uint32_t>{0, 0, 205}));
  CHECK((p.lg_slot == std::vector<int>{0, 1}) && (p.lg_rows == std::vector<int>{0, 1}));
  CHECK(act[2].prefilled == 6 && act[2].advances == 0);
}

static void case6_head_rows() {
  CHECK(head_rows_of({decoding(0, 32, 53)}, 65536) == 4096);
  CHECK(head_rows_of({decoding(0, 33, 53)}, 65536) == 8193);
  CHECK(head_rows_of({decoding(0, 0, 2048, true)}, 65536) == 8193);
  CHECK(head_rows_of({decoding(0, 3, 53), decoding(1, 0, 2048, true)}, 65536) == 8193);
  CHECK(head_rows_of({decoding(0, 33, 53)}, 5000) == 5000);
  CHECK(head_rows_of({decoding(0, 3, 53)}, 5000) == 4096);
}

static void case7_window() {
  CHECK(window_len({decoding(0, 50, 53), decoding(1, 100, 2048)}, 8, false) == 3);
  CHECK(window_len({decoding(0, 53, 53), decoding(1, 2048, 2048)}, 8, false) == 1);
  CHECK(window_len({decoding(0, 3, 53)}, 8, true) == 1);
  std::vector<Active> act = {decoding(0, 30, 1 << 20)};
  const int K = window_len(act, 8, false);
  CHECK(K == 8);
  static const int want[8] = {4096, 4096, 4096, 8193, 8193, 8193, 8193, 8193};
  for (int k = 0; k < K && k < 8; ++k) {  // as the window loop does: the rule, then the step's advance
    CHECK(head_rows_of(act, 65536) == want[k]);
    act[0].advances++;
  }
}

static void case8_decode_plan() {
  const std::vector<Active> act = {decoding(1, 3, 53), decoding(4, 40, 53), decoding(6, 0, 2048, true)};
  const StepPlan p = decode_plan(act);
  static const int slots[3] = {1, 4, 6};
  CHECK(p.rows.size() == 3 && p.segs.size() == 3);
  for (int i = 0; i < 3 && i < (int)p.rows.size(); ++i)
    CHECK(same(p.rows[i], slots[i], 7, -1, 0) && same(p.segs[i], slots[i], i, 1, 0));
  CHECK((p.lg_rows == std::vector<int>{0, 1, 2}) && (p.lg_slot == std::vector<int>{1, 4, 6}));
  CHECK(p.tok_from_ctrl && p.advance && p.tok.empty());
}

static void case9_progress() {
  ProgressRange r = progress_range(3, 20, 9);
  CHECK(r.lo == 3 && r.hi == 9);
  r = progress_range(3, 20, 40);
  CHECK(r.lo == 3 && r.hi == 20);
  r = progress_range(9, 20, 9);
  CHECK(r.hi <= r.lo);
}

static void case10_run_ahead() {
  const std::vector<Active> act = {decoding(0, 10, 53), decoding(1, 100, 2048)};
  // (act, any_prefill, uploaded, graphs, profiling, timeline, can_admit)
  CHECK(may_run_ahead(act, false, false, true, false, false, false));
  CHECK(!may_run_ahead(act, true, false, true, false, false, false));
  CHECK(!may_run_ahead(act, false, true, true, false, false, false));
  CHECK(!may_run_ahead(act, false, false, false, false, false, false));
  CHECK(!may_run_ahead(act, false, false, true, true, false, false));
  CHECK(!may_run_ahead(act, false, false, true, false, true, false));
  CHECK(!may_run_ahead(act, false, false, true, false, false, true));
  CHECK(!may_run_ahead({decoding(0, 10, 53), decoding(1, 2048, 2048)}, false, false, true, false, false, false));
}

// every plan, whatever the mix: one segment per slot at most, its rows consecutive and chained
// inside it, every table consistent, and no more rows than max(chunk, S)
static void check_plan(const StepPlan& p, const std::vector<Active>& before, const std::vector<Active>& after, int chunk,
                       int S) {
  const int R = (int)p.rows.size();
  CHECK(R <= std::max(chunk, S) && (int)p.tok.size() == R);
  std::vector<int> seen(S, 0);
  int next_row = 0;
  for (const Int4& s : p.segs) {
    CHECK(s.x >= 0 && s.x < S && s.z >= 1 && s.w == 0);
    if (s.x < 0 || s.x >= S) return;
    CHECK(++seen[s.x] == 1);
    CHECK(s.y == next_row && s.y + s.z <= R);  // the segments tile the rows in order
    if (s.y != next_row || s.y + s.z > R) return;
    for (int t = 0; t < s.z; ++t) {
      const Int4& r = p.rows[s.y + t];
      CHECK(r.x == s.x && r.w == 0);
      CHECK(r.z == (t == 0 ? -1 : s.y + t - 1));
      CHECK(((r.y & kRowFirst) != 0) == (t == 0) && ((r.y & kRowLast) != 0) == (t == s.z - 1));
      if (r.y & kRowCtrl) CHECK(s.z == 1);
    }
    next_row += s.z;
  }
  CHECK(next_row == R);
  CHECK(p.lg_rows.size() == p.lg_slot.size());
  for (size_t i = 0; i < p.lg_rows.size() && i < p.lg_slot.size(); ++i) {
    CHECK(p.lg_rows[i] >= 0 && p.lg_rows[i] < R);
    if (p.lg_rows[i] >= 0 && p.lg_rows[i] < R) CHECK(p.rows[p.lg_rows[i]].x == p.lg_slot[i] && (p.rows[p.lg_rows[i]].y & kRowLast));
  }
  size_t n_lg = 0;
  for (size_t i = 0; i < before.size(); ++i) {
    const Active &b = before[i], &a = after[i];
    const bool got_logits = !a.in_prompt();
    CHECK(a.advances == b.advances + (got_logits ? 1 : 0));
    CHECK(a.prefilled >= b.prefilled && a.prefilled <= (int)a.prompt.size());
    if (!b.in_prompt()) CHECK(seen[b.slot] == 1);  // a decoding slot never stalls
    n_lg += got_logits;
  }
  CHECK(n_lg == p.lg_rows.size());
}

static void case11_invariants() {
  std::mt19937 rng(12345);
  static const int chunks[4] = {1, 2, 8, 64};
  for (int iter = 0; iter < 400; ++iter) {
    const int S = 1 + (int)(rng() % 8);
    const int chunk = chunks[rng() % 4];
    std::vector<Active> act;
    for (int s = 0; s < S; ++s) {
      if (rng() % 4 == 0) continue;  // a free slot
      const bool zs = rng() % 3 == 0;
      if (rng() % 2)
        act.push_back(decoding(s, (int)(rng() % 60), 1 << 20, zs));
      else {
        const int n = 2 + (int)(rng() % 90);
        act.push_back(prompting(s, n, (int)(rng() % n), zs));
      }
    }
    bool any_prompt = false;
    for (const Active& a : act) any_prompt |= a.in_prompt();
    if (act.empty()) continue;
    if (any_prompt) {
      for (int step = 0; step < 200 && any_prompt; ++step) {  // until every prompt is in
        const std::vector<Active> before = act;
        const StepPlan p = mixed_plan(act, chunk, 65536);
        check_plan(p, before, act, chunk, S);
        CHECK(!p.rows.empty());
        any_prompt = false;
        for (const Active& a : act) any_prompt |= a.in_prompt();
      }
      CHECK(!any_prompt);
    }
    const StepPlan d = decode_plan(act);
    std::vector<Active> after = act;
    for (Active& a : after) a.advances++;
    StepPlan with_tok = d;
    with_tok.tok.assign(d.rows.size(), 0);  // check_plan wants one token per row
    check_plan(with_tok, act, after, chunk, S);
    CHECK(d.rows.size() == act.size());
  }
}

int main() {
  static_assert(sizeof(Int4) == 16 && alignof(Int4) == 16, "Int4 is HIP's int4");
  case1_normal();
  case2_zero_shot();
  case3_validate();
  case4_mixed_all_global();
  case5_budget_floor();
  case6_head_rows();
  case7_window();
  case8_decode_plan();
  case9_progress();
  case10_run_ahead();
  case11_invariants();
  if (g_fail) {
    fprintf(stderr, "sched: %d check(s) failed\n", g_fail);
    return 1;
  }
  printf("sched: ok\n");
  return 0;
}
