// sched.h -- the continuous-batching scheduler's rules (DynamicBatchManager semantics,
// src/dynamic_batch_manager.rs) as plain functions of host data: what a request's prompt, control
// block and step limit are, which rows a forward step carries, how long a decode window is.
// Engine::serve (engine.hip) applies them; nothing here touches the GPU (plain C++17, no HIP
// header), so tests/native/sched_main.cpp checks them on a CPU.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/rwkvtts.h"
#include "slot_ctrl.h"

namespace rwkvtts {

struct Job;  // engine.h: one request in flight through Engine::serve

// four ints as the kernels read them (HIP's int4; engine.hip asserts size and alignment)
struct alignas(16) Int4 {
  int32_t x, y, z, w;
};

// One forward step description (host side).
struct StepPlan {
  std::vector<uint32_t> tok;   // per row
  std::vector<Int4> rows;      // slot, flags, prev_row, 0
  std::vector<Int4> segs;      // slot, row_begin, n_rows, 0
  std::vector<int> lg_rows;    // rows whose logits are produced
  std::vector<int> lg_slot;    // slot of each logits row (advance)
  int head_rows = 0;
  bool tok_from_ctrl = false;  // decode: token = ctrl[slot].next_token
  bool advance = false;        // run the phase controller on the logits rows
  AdvanceKind kind = kAdvFixed;  // the step's controller: step_kind of the active requests
};

// A request decoding in a state slot.
struct Active {
  Job* job = nullptr;
  int slot = 0;
  std::vector<uint32_t> prompt;
  int prefilled = 0;
  int advances = 0;  // phase-controller invocations so far
  int total = 0;     // advances after which the request is certainly done (its step limit)
  bool zero_shot = false;
  bool pinned = false;        // Admission::pinned: normal mode, the 32 global tokens given
  AdvanceKind kind = kAdvFixed;  // Admission::kind
  // token progress (Job::user): semantic tokens handed to the sink so far, and per unit buffer the
  // end of the range of this slot's d_sem_ that the unit copied to h_prog_
  const rwkvtts_token_sink* sink = nullptr;
  int delivered = 0;
  int copied_hi[2] = {0, 0};
  bool in_prompt() const { return prefilled < (int)prompt.size(); }
};

inline bool is_zero_shot(const rwkvtts_request& q) { return q.ref_global != nullptr && q.ref_semantic != nullptr; }
// pinned voice: a normal-mode request whose global phase is replaced by the 32 ids of ref_global
inline bool is_pinned(const rwkvtts_request& q) { return q.pinned_voice != 0; }

// The extension block as a job carries it, by value: the first min(struct_size, sizeof) bytes of
// the caller's block, the rest zero, struct_size still the caller's (validate judges it), and
// whether there was a block at all.
struct HeldExt {
  rwkvtts_request_ext ext{};
  bool present = false;
  void hold(const rwkvtts_request_ext* e) {
    memset(&ext, 0, sizeof(ext));
    present = e != nullptr;
    if (e) {
      uint32_t sz = 0;
      memcpy(&sz, e, sizeof(sz));
      memcpy(&ext, e, std::min<size_t>(std::max<size_t>(sz, sizeof(sz)), sizeof(ext)));
    }
  }
  const rwkvtts_request_ext* ptr() const { return present ? &ext : nullptr; }
};
inline HeldExt ext_copy(const rwkvtts_request_ext* e) {
  HeldExt h;
  h.hold(e);
  return h;
}
inline bool has_mirostat(const rwkvtts_request_ext* ext) { return ext && (ext->mirostat_set & RWKVTTS_MIROSTAT_SET); }

// The ranges of the three sampling options, for validate and the k_advance test hook
// (Engine::debug_advance): each fills `why` and returns false for a bad value. Comparisons are
// false for NaN, so a non-finite value fails its range.
inline bool phase_sampling_ok(const rwkvtts_phase_sampling& s, const char* what, std::string& why) {
  if (!(s.temperature >= 0.1f && s.temperature <= 4.0f)) why = std::string(what) + ": temperature must be in [0.1, 4.0]";
  else if (!(s.top_p >= 0.0f && s.top_p <= 1.0f)) why = std::string(what) + ": top_p must be in [0, 1]";
  else if (s.top_k < 0) why = std::string(what) + ": top_k must be >= 0";
  else return true;
  return false;
}
inline bool penalties_ok(const rwkvtts_penalties& p, std::string& why) {
  if (!(p.repetition >= 0.25f && p.repetition <= 4.0f)) why = "penalties: repetition must be in [0.25, 4.0]";
  else if (!(p.frequency >= -8.0f && p.frequency <= 8.0f)) why = "penalties: frequency must be in [-8.0, 8.0]";
  else if (!(p.presence >= -8.0f && p.presence <= 8.0f)) why = "penalties: presence must be in [-8.0, 8.0]";
  else if (p.window < 0 || p.window > RWKVTTS_SEMANTIC_LIMIT) why = "penalties: window must be in [0, 2048]";
  else return true;
  return false;
}
inline bool mirostat_ok(float tau, float rate, std::string& why) {
  if (!(tau >= 0.5f && tau <= 10.0f)) why = "mirostat: tau must be in [0.5, 10]";
  else if (!(rate >= 0.001f && rate <= 1.0f)) why = "mirostat: rate must be in [0.001, 1]";
  else return true;
  return false;
}

// Checks a request (and its extension block, if any) before admission; fills `why` and returns
// false for a bad one.
inline bool validate(const rwkvtts_request& q, int n_vocab, std::string& why, const rwkvtts_request_ext* ext = nullptr) {
  auto ids_ok = [&](const int32_t* p, int n, int lo, int hi, const char* what) {
    if (n < 0 || (n > 0 && !p)) {
      why = std::string(what) + ": bad array";
      return false;
    }
    for (int i = 0; i < n; ++i)
      if (p[i] < lo || p[i] >= hi) {
        why = std::string(what) + ": id " + std::to_string(p[i]) + " out of range";
        return false;
      }
    return true;
  };
  const int V = n_vocab;
  if (!ids_ok(q.text_tokens, q.n_text, 0, V, "text_tokens")) return false;
  if (!ids_ok(q.property_tokens, q.n_property, 0, V, "property_tokens")) return false;
  if ((q.ref_global && q.n_ref_global < 0) || (q.ref_semantic && q.n_ref_semantic < 0)) {
    why = "reference token counts must be >= 0";
    return false;
  }
  if (q.max_tokens < 0 || q.fixed_semantic < 0) {
    why = "max_tokens / fixed_semantic must be >= 0";
    return false;
  }
  if (q.pinned_voice != 0) {
    if (q.pinned_voice != 1) why = "pinned_voice must be 0 or 1";
    else if (q.ref_semantic) why = "pinned_voice: ref_semantic must be NULL";
    else if (!q.ref_global || q.n_ref_global != RWKVTTS_N_GLOBAL)
      why = "pinned_voice: ref_global must hold exactly " + std::to_string(RWKVTTS_N_GLOBAL) + " ids";
    else if (!ids_ok(q.ref_global, q.n_ref_global, 0, 4096, "pinned_voice: ref_global")) return false;
    if (!why.empty()) return false;
  }
  const bool zero_shot = is_zero_shot(q);
  if (V <= RWKVTTS_TAG_2 || (!zero_shot && V <= RWKVTTS_GLOBAL_TOKEN_OFFSET + 4095) ||
      (zero_shot && q.n_ref_global > 0 && V <= RWKVTTS_GLOBAL_TOKEN_OFFSET + 4095)) {
    why = "model vocabulary too small for the TTS tags / global tokens";
    return false;
  }
  if (q.sampling_set & ~(RWKVTTS_SAMPLING_GLOBAL | RWKVTTS_SAMPLING_SEMANTIC)) {
    why = "sampling_set: unknown bits";
    return false;
  }
  if (q.sampling_set && q.greedy) {
    why = "greedy and sampling_set exclude each other";
    return false;
  }
  if ((q.sampling_set & RWKVTTS_SAMPLING_GLOBAL) && !phase_sampling_ok(q.global_sampling, "global_sampling", why)) return false;
  if ((q.sampling_set & RWKVTTS_SAMPLING_SEMANTIC) && !phase_sampling_ok(q.semantic_sampling, "semantic_sampling", why))
    return false;
  if (q.penalty_set & ~RWKVTTS_PENALTY_SET) {
    why = "penalty_set: unknown bits";
    return false;
  }
  if (q.penalty_set && !penalties_ok(q.penalties, why)) return false;  // (allowed together with greedy)
  if (ext) {  // a field is read only where the caller's struct_size covers it
    const size_t have = ext->struct_size;
    if (have < offsetof(rwkvtts_request_ext, mirostat_set) + sizeof(ext->mirostat_set)) {
      why = "ext: struct_size does not cover mirostat_set";
      return false;
    }
    if (ext->mirostat_set & ~RWKVTTS_MIROSTAT_SET) {
      why = "mirostat_set: unknown bits";
      return false;
    }
    if (ext->mirostat_set) {
      if (have < offsetof(rwkvtts_request_ext, mirostat) + sizeof(ext->mirostat)) why = "ext: struct_size does not cover mirostat";
      else if (!mirostat_ok(ext->mirostat.tau, ext->mirostat.rate, why)) return false;
      else if (q.greedy) why = "mirostat and greedy exclude each other";
      else if (q.sampling_set & RWKVTTS_SAMPLING_SEMANTIC)
        why = "mirostat replaces the semantic phase's top-k, top-p and temperature: semantic_sampling excludes it";
      if (!why.empty()) return false;
    }
  }
  return true;
}

// Semantic-step limit of a request, as the reference derives it.
inline int sem_limit_of(const rwkvtts_request& q) {
  if (q.fixed_semantic > 0) return std::min(q.fixed_semantic, RWKVTTS_SEMANTIC_LIMIT);
  if (is_zero_shot(q)) return RWKVTTS_SEMANTIC_LIMIT;                  // zero_shot_inference.rs:128-142
  return std::min(std::max(q.max_tokens, 0), RWKVTTS_SEMANTIC_LIMIT);  // normal_mode_inference.rs:316
}

// A valid pinned request that emits nothing (max_tokens == 0 without fixed_semantic): it ends at
// admission with status 0, its 32 global tokens and no semantic tokens, and takes no state slot.
inline bool pinned_without_tokens(const rwkvtts_request& q) { return is_pinned(q) && sem_limit_of(q) == 0; }

// What admission derives from the request alone.
struct Admission {
  std::vector<uint32_t> prompt;
  SlotCtrl ctrl;         // the slot's initial control block, gkey / skey still zero
  // the slot's sampling block: penalties (1, 0, 0, 0) without penalty_set; Mirostat {tau, rate,
  // mu = 2 tau, on = 1} with rwkvtts_request_ext::mirostat, all zero without
  SlotSampling samp;
  uint64_t gseed, sseed;  // the engine derives gkey / skey from them (StdRng::seed_from_u64)
  bool zero_shot;
  bool pinned;           // is_pinned: decodes as normal mode from its first logits row on
  int total;             // Active::total
  // the controller the slot's steps need: kAdvMiro with a Mirostat block; else kAdvParams where a
  // phase's temperature or top-p differs from the reference's (1.0, 0.95), its top-k is outside
  // the fast path's [1, kFastTopK] or the penalties are not neutral; else kAdvFixed
  AdvanceKind kind;
};

// (1, 0, 0): the semantic rows are sampled as they arrive
inline bool penalties_neutral(const SlotPenalty& p) {
  return p.repetition == 1.0f && p.frequency == 0.0f && p.presence == 0.0f;
}

// the controller of a step: the highest kind among the active requests
inline AdvanceKind step_kind(const std::vector<Active>& act) {
  AdvanceKind k = kAdvFixed;
  for (const Active& a : act) k = std::max(k, a.kind);
  return k;
}

// entropy: the seed of a request without one (dynamic_batch_manager.rs:491-499, from_entropy)
inline Admission admission_of(const rwkvtts_request& q, uint64_t entropy, const rwkvtts_request_ext* ext = nullptr) {
  Admission a;
  a.zero_shot = is_zero_shot(q);
  a.pinned = is_pinned(q);
  for (int i = 0; i < q.n_property; ++i) a.prompt.push_back((uint32_t)q.property_tokens[i]);
  a.prompt.push_back(RWKVTTS_TAG_2);
  for (int i = 0; i < q.n_text; ++i) a.prompt.push_back((uint32_t)q.text_tokens[i]);
  a.prompt.push_back(RWKVTTS_TAG_0);
  SlotCtrl& c = a.ctrl;
  memset(&c, 0, sizeof(c));
  // RNG streams: normal_mode_inference.rs:138-174, zero_shot_inference.rs:204-216,
  // dynamic_batch_manager.rs:491-499 (no seed -> from_entropy)
  const uint64_t seed = q.has_seed ? q.seed : entropy;
  const bool indep = q.layered_set ? q.use_independent_seeds != 0 : true;
  const uint64_t goff = q.layered_set ? q.global_seed_offset : 1000, soff = q.layered_set ? q.semantic_seed_offset : 2000;
  a.gseed = indep ? seed + goff : seed + 100;
  a.sseed = indep ? seed + soff : seed + 200;
  if (a.zero_shot && !indep) a.sseed = 0;  // StdRng::seed_from_u64(0) handed to the zero-shot path
  c.top_k_g = q.greedy ? 1 : 20;
  c.top_k_s = q.greedy ? 1 : 80;
  c.temp_g = c.temp_s = 1.0f;  // normal_mode_inference.rs:114-127, unless the request sets a phase
  c.top_p_g = c.top_p_s = 0.95f;
  if (q.sampling_set & RWKVTTS_SAMPLING_GLOBAL) {
    c.temp_g = q.global_sampling.temperature;
    c.top_p_g = q.global_sampling.top_p;
    c.top_k_g = q.global_sampling.top_k;
  }
  if (q.sampling_set & RWKVTTS_SAMPLING_SEMANTIC) {
    c.temp_s = q.semantic_sampling.temperature;
    c.top_p_s = q.semantic_sampling.top_p;
    c.top_k_s = q.semantic_sampling.top_k;
  }
  a.samp = SlotSampling{{1.0f, 0.0f, 0.0f, 0}, {0.0f, 0.0f, 0.0f, 0}};
  if (q.penalty_set & RWKVTTS_PENALTY_SET)
    a.samp.pen = SlotPenalty{q.penalties.repetition, q.penalties.frequency, q.penalties.presence, q.penalties.window};
  if (has_mirostat(ext)) a.samp.miro = SlotMiro{ext->mirostat.tau, ext->mirostat.rate, 2.0f * ext->mirostat.tau, 1};
  const bool own = c.temp_g != 1.0f || c.temp_s != 1.0f || c.top_p_g != 0.95f || c.top_p_s != 0.95f || c.top_k_g < 1 ||
                   c.top_k_g > kFastTopK || c.top_k_s < 1 || c.top_k_s > kFastTopK || !penalties_neutral(a.samp.pen);
  a.kind = a.samp.miro.on ? kAdvMiro : (own ? kAdvParams : kAdvFixed);
  c.fixed = q.fixed_semantic > 0;
  c.sem_limit = sem_limit_of(q);
  if (a.zero_shot) {
    c.mode = 1;
    c.phase = kPhSemantic;
    for (int i = 0; i < q.n_ref_global; ++i) {
      const int g = std::min(std::max(q.ref_global[i], 0), 4095);
      a.prompt.push_back((uint32_t)(g + RWKVTTS_GLOBAL_TOKEN_OFFSET));
      if (i < RWKVTTS_N_GLOBAL) c.global_out[c.n_global++] = g;
    }
    a.prompt.push_back(RWKVTTS_TAG_1);
    const int tlen = q.n_text;
    const int min_sem = std::min(std::max(tlen / 4, 8), 64);
    const int est = (int)ceilf((float)tlen * 1.8f);
    const int upper = (int)floorf((float)RWKVTTS_SEMANTIC_LIMIT * 0.9f);
    c.hard_min = std::min(upper, std::max(min_sem, est));
    a.total = std::max(c.sem_limit, 1);
  } else if (a.pinned) {
    // what a normal request has fed itself when its semantic phase starts (kPhGFeed, then TAG_1,
    // normal_mode_inference.rs:277-278): mode 0 stops at EOS, the semantic draw counter starts at
    // 0 as it does there, the global stream is never drawn from. sem_limit == 0 is not admitted
    // (pinned_without_tokens): the first logits row would emit a token.
    c.mode = 0;
    c.phase = kPhSemantic;
    for (int i = 0; i < RWKVTTS_N_GLOBAL; ++i) {
      a.prompt.push_back((uint32_t)(q.ref_global[i] + RWKVTTS_GLOBAL_TOKEN_OFFSET));
      c.global_out[c.n_global++] = q.ref_global[i];
    }
    a.prompt.push_back(RWKVTTS_TAG_1);
    a.total = c.sem_limit;
  } else {
    c.mode = 0;
    c.phase = kPhGlobal;
    a.total = RWKVTTS_N_GLOBAL + 1 + c.sem_limit;
  }
  return a;
}

// ---- the row tables of a step: one segment per slot, its rows consecutive
// a decoding slot's row: the token comes from its control block, the logits go to the controller
inline void append_decode_row(StepPlan& p, int slot) {
  const int r = (int)p.rows.size();
  p.rows.push_back({slot, kRowFirst | kRowLast | kRowCtrl, -1, 0});
  if (!p.tok_from_ctrl) p.tok.push_back(0);
  p.segs.push_back({slot, r, 1, 0});
  p.lg_rows.push_back(r);
  p.lg_slot.push_back(slot);
}

enum LogitRows { kLogitsNone, kLogitsLast, kLogitsAll };

// `take` > 0 tokens of a slot, each row after the first chained to the one before it
inline void append_token_rows(StepPlan& p, int slot, const uint32_t* tok, int take, LogitRows lg) {
  const int r0 = (int)p.rows.size();
  for (int t = 0; t < take; ++t) {
    const int flags = (t == 0 ? kRowFirst : 0) | (t == take - 1 ? kRowLast : 0);
    p.rows.push_back({slot, flags, t == 0 ? -1 : r0 + t - 1, 0});
    p.tok.push_back(tok[t]);
    if (lg == kLogitsAll || (lg == kLogitsLast && t == take - 1)) {
      p.lg_rows.push_back(r0 + t);
      p.lg_slot.push_back(slot);
    }
  }
  p.segs.push_back({slot, r0, take, 0});
}

// Head rows of a step: 4096 while every slot that gets a logits row (its prompt is in) samples
// global tokens (normal_mode_inference.rs:236-240: from [0, 4096)) or feeds g31, else 8193 (:332:
// semantic ids from [0, 8192]; a zero-shot or pinned slot from its first logits row on).
// Evaluated before the step's advances are counted.
inline int head_rows_of(const std::vector<Active>& act, int n_vocab) {
  bool all_global = true;
  for (const Active& a : act)
    if (!a.in_prompt()) all_global &= !a.zero_shot && !a.pinned && a.advances <= RWKVTTS_N_GLOBAL;
  return std::min(all_global ? 4096 : 8193, n_vocab);
}

// Mixed step: every decoding slot's row (token from its control block) plus prompt rows of the
// admitted slots, up to `chunk` rows; the decoding slots never stall. `act` is sorted by slot.
inline StepPlan mixed_plan(std::vector<Active>& act, int chunk, int n_vocab) {
  StepPlan p;
  p.advance = true;
  int budget = chunk;
  for (const Active& a : act) {
    if (a.in_prompt()) continue;
    append_decode_row(p, a.slot);
    --budget;
  }
  budget = std::max(budget, 1);
  for (Active& a : act) {
    const int left = (int)a.prompt.size() - a.prefilled;
    if (left <= 0 || budget <= 0) continue;
    const int take = std::min(left, budget);
    append_token_rows(p, a.slot, a.prompt.data() + a.prefilled, take, take == left ? kLogitsLast : kLogitsNone);
    a.prefilled += take;
    budget -= take;
  }
  p.head_rows = head_rows_of(act, n_vocab);
  p.kind = step_kind(act);
  for (Active& a : act) a.advances += !a.in_prompt();  // one advance per logits row
  return p;
}

// Decode plan: one row per active slot, tokens from the control blocks.
inline StepPlan decode_plan(const std::vector<Active>& act) {
  StepPlan p;
  p.tok_from_ctrl = true;
  p.advance = true;
  p.kind = step_kind(act);
  for (const Active& a : act) append_decode_row(p, a.slot);
  return p;
}

// Decode window: up to `lookahead` steps queued back to back before the host reads the control
// blocks; no slot can pass its step limit inside the window (EOS may end a request earlier: its
// slot then idles through the rest of the window, k_advance skips it). single: profiling or the
// debug timeline, one step per window.
inline int window_len(const std::vector<Active>& act, int lookahead, bool single) {
  int K = single ? 1 : lookahead;
  for (const Active& a : act) K = std::min(K, std::max(1, a.total - a.advances));
  return K;
}

// Whether the next window may go out before this unit's snapshot is read: steady decode only --
// no prompt rows in the unit, its plan uploaded earlier, graph replay without profiling or the
// timeline, no admission possible (can_admit: the source is open and a slot is free) and no slot
// able to pass its step limit.
inline bool may_run_ahead(const std::vector<Active>& act, bool any_prefill, bool uploaded, bool graphs, bool profiling,
                          bool timeline, bool can_admit) {
  bool ahead = !any_prefill && !uploaded && graphs && !profiling && !timeline && !can_admit;
  for (const Active& a : act) ahead &= a.total - a.advances >= 1;
  return ahead;
}

// Token progress: the semantic ids a unit may have added to a slot. A slot holds at most one id
// per advance, and the host knows the ids it has handed out: [delivered, min(sem_limit, advances))
// covers whatever the unit's snapshot will show. Empty when hi <= lo.
struct ProgressRange {
  int lo, hi;
};
inline ProgressRange progress_range(int delivered, int sem_limit, int advances) {
  return {delivered, std::min(sem_limit, advances)};
}

}  // namespace rwkvtts
