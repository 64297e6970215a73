// sched_miro_main.cpp -- the request extension block and Mirostat through the scheduler's rules
// (csrc/sched.h ext_copy / validate / admission_of / the plans), as a stand-alone program for a
// plain C++17 compiler (tests/test_sched_miro_cpu.py builds it under ASan + UBSan). The expected
// values follow include/rwkvtts.h: tau in [0.5, 10], rate in [0.001, 1], both finite;
// mirostat_set bit 0 alone; refused with greedy and with RWKVTTS_SAMPLING_SEMANTIC; a struct_size
// that does not cover the fields read is refused, and nothing past it is read; no block, a block
// with mirostat_set == 0 and the parent's call are one and the same admission.
#include "../../rwkv-tts-rs_amd/csrc/sched.h"

#include <math.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>

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

static rwkvtts_request_ext miro(float tau, float rate, int bits = RWKVTTS_MIROSTAT_SET) {
  rwkvtts_request_ext x;
  memset(&x, 0, sizeof(x));
  x.struct_size = (uint32_t)sizeof(x);
  x.mirostat_set = bits;
  x.mirostat.tau = tau;
  x.mirostat.rate = rate;
  return x;
}

// as Engine::admit sees a job: the block by value, turned back into a pointer (or none)
static bool ok(const rwkvtts_request& q, const rwkvtts_request_ext* caller) {
  const HeldExt held = ext_copy(caller);
  std::string why;
  const bool r = validate(q, 65536, why, held.ptr());
  CHECK(r == why.empty());
  return r;
}
static bool ok(const rwkvtts_request& q, const rwkvtts_request_ext& x) { return ok(q, &x); }

static bool same_admission(const Admission& a, const Admission& b) {
  return memcmp(&a.ctrl, &b.ctrl, sizeof(SlotCtrl)) == 0 && memcmp(&a.samp, &b.samp, sizeof(SlotSampling)) == 0 &&
         a.prompt == b.prompt && a.gseed == b.gseed && a.sseed == b.sseed && a.zero_shot == b.zero_shot &&
         a.pinned == b.pinned && a.total == b.total && a.kind == b.kind;
}

static void case_layout() {
  CHECK(sizeof(rwkvtts_request_ext) == 16);
  CHECK(offsetof(rwkvtts_request_ext, struct_size) == 0 && offsetof(rwkvtts_request_ext, mirostat_set) == 4);
  CHECK(offsetof(rwkvtts_request_ext, mirostat) == 8 && sizeof(SlotMiro) == 16);
  // the slot's one block beside its control block: penalties, then the Mirostat state
  CHECK(sizeof(SlotSampling) == 32 && offsetof(SlotSampling, pen) == 0 && offsetof(SlotSampling, miro) == 16);
  // the request struct ends where it ended: at its penalties (rounded up to its 8-byte alignment)
  CHECK(sizeof(rwkvtts_request) == (offsetof(rwkvtts_request, penalties) + sizeof(rwkvtts_penalties) + 7) / 8 * 8);
}

static void case_validate() {
  for (Kind kind : {kNormal, kZeroShot, kPinned}) {
    const rwkvtts_request q = request(kind);
    CHECK(ok(q, nullptr));
    CHECK(ok(q, miro(3.0f, 0.1f)));
    // the range ends are inside ...
    CHECK(ok(q, miro(0.5f, 0.001f)));
    CHECK(ok(q, miro(10.0f, 1.0f)));
    // ... and the next value on either side is not
    CHECK(!ok(q, miro(nextafterf(0.5f, 0.0f), 0.1f)));
    CHECK(!ok(q, miro(nextafterf(10.0f, 11.0f), 0.1f)));
    CHECK(!ok(q, miro(3.0f, nextafterf(0.001f, 0.0f))));
    CHECK(!ok(q, miro(3.0f, nextafterf(1.0f, 2.0f))));
    CHECK(!ok(q, miro(0.0f, 0.0f)));  // a zero-filled block with the bit set
    CHECK(!ok(q, miro(-3.0f, 0.1f)));
    CHECK(!ok(q, miro(3.0f, -0.1f)));
    for (float bad : {NAN, INFINITY, -INFINITY}) {
      CHECK(!ok(q, miro(bad, 0.1f)));
      CHECK(!ok(q, miro(3.0f, bad)));
    }
    CHECK(ok(q, miro(NAN, -99.0f, 0)));  // bad values behind a clear bit are not looked at
    for (int bits : {2, 3, 4, 1 | 8, -1, 1 << 30}) CHECK(!ok(q, miro(3.0f, 0.1f, bits)));  // unknown bits
    {  // the excluded combinations, and only those
      rwkvtts_request v = q;
      v.greedy = 1;
      CHECK(!ok(v, miro(3.0f, 0.1f)));
      CHECK(ok(v, miro(3.0f, 0.1f, 0)) && ok(v, nullptr));  // greedy alone stays valid
      v.greedy = 0;
      v.sampling_set = RWKVTTS_SAMPLING_SEMANTIC;
      v.semantic_sampling = {0.8f, 0.95f, 80};
      CHECK(!ok(v, miro(3.0f, 0.1f)));
      CHECK(ok(v, nullptr));
      v.sampling_set = RWKVTTS_SAMPLING_GLOBAL | RWKVTTS_SAMPLING_SEMANTIC;
      v.global_sampling = {0.8f, 0.95f, 20};
      CHECK(!ok(v, miro(3.0f, 0.1f)));
      v.sampling_set = RWKVTTS_SAMPLING_GLOBAL;  // the global phase keeps its own values
      CHECK(ok(v, miro(3.0f, 0.1f)));
      v.penalty_set = RWKVTTS_PENALTY_SET;  // with penalties and fixed_semantic
      v.penalties = {1.3f, 0.7f, 1.5f, 64};
      v.fixed_semantic = 20;
      CHECK(ok(v, miro(3.0f, 0.1f)));
    }
  }
}

// A caller built with a shorter block: nothing past its struct_size is read (the blocks below are
// heap allocations of exactly that size, so AddressSanitizer sees any read past them), fields it
// does not cover cannot be asked for, and a block that asks for nothing is valid at any size >= 8.
static void case_struct_size() {
  const rwkvtts_request q = request(kNormal);
  auto short_block = [](uint32_t size, int bits) {
    char* p = (char*)malloc(size);
    memset(p, 0, size);
    memcpy(p, &size, 4);
    if (size >= 8) memcpy(p + 4, &bits, 4);
    return (rwkvtts_request_ext*)p;
  };
  for (uint32_t size : {4u, 7u}) {  // does not cover mirostat_set
    rwkvtts_request_ext* x = short_block(size, 0);
    CHECK(!ok(q, x));
    free(x);
  }
  for (uint32_t size : {8u, 12u, 15u}) {  // covers mirostat_set, not mirostat
    rwkvtts_request_ext* x = short_block(size, 0);
    CHECK(ok(q, x));
    CHECK(same_admission(admission_of(q, 999), admission_of(q, 999, ext_copy(x).ptr())));
    free(x);
    x = short_block(size, RWKVTTS_MIROSTAT_SET);
    CHECK(!ok(q, x));
    free(x);
  }
  {  // a longer block from a newer caller: the known prefix is read
    char* p = (char*)calloc(1, 32);
    rwkvtts_request_ext x = miro(4.0f, 0.5f);
    x.struct_size = 32;
    memcpy(p, &x, sizeof(x));
    CHECK(ok(q, (const rwkvtts_request_ext*)p));
    const HeldExt held = ext_copy((const rwkvtts_request_ext*)p);
    CHECK(held.present && held.ext.struct_size == 32 && held.ext.mirostat.tau == 4.0f && held.ext.mirostat.rate == 0.5f);
    free(p);
  }
  {  // struct_size 0 (a zeroed block) is refused, not mistaken for "no block"
    rwkvtts_request_ext z;
    memset(&z, 0, sizeof(z));
    CHECK(!ok(q, &z));
  }
  CHECK(ext_copy(nullptr).ptr() == nullptr && !ext_copy(nullptr).present);
}

static void case_admission() {
  for (Kind kind : {kNormal, kZeroShot, kPinned}) {
    rwkvtts_request q = request(kind);
    const Admission a0 = admission_of(q, 999);  // the parent's call
    CHECK(a0.kind == kAdvFixed && a0.samp.miro.on == 0 && a0.samp.miro.tau == 0.0f && a0.samp.miro.rate == 0.0f &&
          a0.samp.miro.mu == 0.0f);
    // a null block and a block that sets nothing give that admission, byte for byte
    CHECK(same_admission(a0, admission_of(q, 999, nullptr)));
    const rwkvtts_request_ext unset = miro(7.0f, 0.9f, 0);  // values present but not set: unused
    CHECK(same_admission(a0, admission_of(q, 999, &unset)));

    const rwkvtts_request_ext x = miro(3.0f, 0.1f);
    const Admission a1 = admission_of(q, 999, &x);  // normal, zero-shot and pinned admissions carry the block
    CHECK(a1.kind == kAdvMiro && a1.samp.miro.on == 1 && a1.samp.miro.tau == 3.0f && a1.samp.miro.rate == 0.1f &&
          a1.samp.miro.mu == 6.0f);
    // everything else is the request's without Mirostat: the control block byte for byte
    CHECK(memcmp(&a0.ctrl, &a1.ctrl, sizeof(SlotCtrl)) == 0 && memcmp(&a0.samp.pen, &a1.samp.pen, sizeof(SlotPenalty)) == 0);
    CHECK(a1.prompt == a0.prompt && a1.total == a0.total && a1.gseed == a0.gseed && a1.sseed == a0.sseed);
    CHECK(a1.zero_shot == (kind == kZeroShot) && a1.pinned == (kind == kPinned));
    CHECK(a1.ctrl.phase == (kind == kNormal ? kPhGlobal : kPhSemantic));
    for (float tau : {0.5f, 2.5f, 10.0f}) {  // mu = 2 tau
      const rwkvtts_request_ext y = miro(tau, 1.0f);
      CHECK(admission_of(q, 999, &y).samp.miro.mu == 2.0f * tau);
    }
    // with penalties and the global phase's own values: all three sets arrive
    q.penalty_set = RWKVTTS_PENALTY_SET;
    q.penalties = {1.3f, 0.0f, 0.5f, 16};
    q.sampling_set = RWKVTTS_SAMPLING_GLOBAL;
    q.global_sampling = {0.8f, 0.9f, 10};
    const Admission a2 = admission_of(q, 999, &x);
    CHECK(a2.kind == kAdvMiro && a2.samp.miro.mu == 6.0f && a2.samp.pen.repetition == 1.3f && a2.samp.pen.window == 16 &&
          a2.ctrl.temp_g == 0.8f && a2.ctrl.top_k_g == 10 && a2.ctrl.temp_s == 1.0f && a2.ctrl.top_k_s == 80);
  }
}

// The plans carry the flag of the requests they hold: through admission_of, not set by hand.
static void case_plans() {
  const rwkvtts_request plain = request(kNormal);
  const rwkvtts_request_ext x = miro(3.0f, 0.1f), unset = miro(3.0f, 0.1f, 0);
  auto active = [&](const rwkvtts_request_ext* ext, int slot, bool prompt_in) {
    Admission ad = admission_of(plain, 999, ext);
    Active a;
    a.slot = slot;
    a.kind = ad.kind;  // as Engine::admit copies it
    a.prompt = ad.prompt;
    a.prefilled = prompt_in ? (int)a.prompt.size() : 0;
    a.total = ad.total;
    return a;
  };
  std::vector<Active> act = {active(nullptr, 0, true), active(&unset, 1, true)};
  CHECK(decode_plan(act).kind == kAdvFixed);  // the default controller
  std::vector<Active> m = act;
  const StepPlan mp = mixed_plan(m, 8, 65536);
  CHECK(mp.kind == kAdvFixed);
  act.push_back(active(&x, 2, true));
  CHECK(decode_plan(act).kind == kAdvMiro);
  m = act;
  CHECK(mixed_plan(m, 8, 65536).kind == kAdvMiro);
  // a Mirostat request still in its prompt already selects the controller of the mixed step
  m = {active(nullptr, 0, true), active(&x, 1, false)};
  CHECK(mixed_plan(m, 8, 65536).kind == kAdvMiro);
  // own sampling values without Mirostat keep the flag clear
  rwkvtts_request sp = plain;
  sp.sampling_set = RWKVTTS_SAMPLING_SEMANTIC;
  sp.semantic_sampling = {0.8f, 0.95f, 80};
  Active a;
  a.kind = admission_of(sp, 999).kind;
  a.prefilled = 0;
  std::vector<Active> only = {a};
  CHECK(decode_plan(only).kind == kAdvParams);
}

// The kind of a step is the highest kind among its actives, in whatever order they stand, and it
// falls back when the highest leaves.
static void case_step_kind() {
  const rwkvtts_request plain = request(kNormal);
  rwkvtts_request sp = plain;
  sp.sampling_set = RWKVTTS_SAMPLING_SEMANTIC;
  sp.semantic_sampling = {0.8f, 0.95f, 80};
  const rwkvtts_request_ext x = miro(3.0f, 0.1f);
  const AdvanceKind kinds[3] = {admission_of(plain, 999).kind, admission_of(sp, 999).kind, admission_of(plain, 999, &x).kind};
  CHECK(kinds[0] == kAdvFixed && kinds[1] == kAdvParams && kinds[2] == kAdvMiro);
  CHECK(kAdvFixed < kAdvParams && kAdvParams < kAdvMiro);
  auto plans_are = [](const std::vector<Active>& act, AdvanceKind want) {
    std::vector<Active> m = act;
    CHECK(step_kind(act) == want && decode_plan(act).kind == want && mixed_plan(m, 8, 65536).kind == want);
  };
  int order[3] = {0, 1, 2};
  do {
    std::vector<Active> act;
    for (int i = 0; i < 3; ++i) {
      Active a;
      a.slot = i;
      a.kind = kinds[order[i]];
      a.prompt = {1u};
      a.prefilled = 1;
      a.total = 8;
      act.push_back(a);
    }
    plans_are(act, kAdvMiro);
    for (int drop = 0; drop < 2; ++drop) {  // the highest active leaves: Miro, then Params
      const AdvanceKind top = drop == 0 ? kAdvMiro : kAdvParams;
      for (size_t i = 0; i < act.size(); ++i)
        if (act[i].kind == top) {
          act.erase(act.begin() + i);
          break;
        }
      plans_are(act, drop == 0 ? kAdvParams : kAdvFixed);
    }
  } while (std::next_permutation(order, order + 3));
  plans_are({}, kAdvFixed);
}

int main() {
  case_layout();
  case_validate();
  case_struct_size();
  case_admission();
  case_plans();
  case_step_kind();
  if (g_fail) {
    fprintf(stderr, "sched miro: %d check(s) failed\n", g_fail);
    return 1;
  }
  printf("sched miro: ok\n");
  return 0;
}
