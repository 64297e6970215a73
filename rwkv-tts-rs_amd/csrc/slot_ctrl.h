// slot_ctrl.h -- the types the host scheduler (sched.h) shares with the kernels: a slot's control
// block and the row flags of a forward step. Plain C++, no HIP header.
#pragma once
#include <stdint.h>

namespace rwkvtts {

constexpr int kRowFirst = 1;  // row flags
constexpr int kRowLast = 2;
constexpr int kRowCtrl = 4;   // the row's token is its slot's SlotCtrl::next_token (decode)

constexpr int kFastTopK = 256;  // largest top-k of the sampler's fast path (sampler.hip kFastK)

// Which phase controller a slot needs (sched.h admission_of) and a step launches (sampler.hip
// launch_advance). kAdvFixed: k_advance, the reference's (temperature 1.0, top_p 0.95) compiled
// in, for a top-k in [1, kFastTopK]. kAdvParams: k_advance_params reads the three per row from the
// control block, carries every top-k path and applies the slot's penalties. kAdvMiro:
// k_advance_miro is k_advance_params plus the Mirostat path for the semantic rows of slots whose
// block is on. The kernels form a chain -- each kind's kernel gives a row of a lower kind the same
// token -- so the values are ordered and the kind of a step is the maximum over its slots.
enum AdvanceKind : int32_t { kAdvFixed = 0, kAdvParams = 1, kAdvMiro = 2 };

enum SlotPhase : int32_t { kPhGlobal = 0, kPhGFeed = 1, kPhSemantic = 2, kPhDone = 3 };

// Per-slot control block living in device memory.
struct SlotCtrl {
  int32_t mode;        // 0 normal, 1 zero-shot
  int32_t phase;       // SlotPhase
  int32_t n_global;
  int32_t n_sem;
  int32_t sem_limit;
  int32_t hard_min;    // zero-shot: EOS forbidden while n_sem < hard_min
  int32_t fixed;       // benchmark: EOS always masked
  int32_t top_k_g, top_k_s;
  int32_t next_token;  // token fed at the next step
  int32_t win_bits;    // zero-shot EOS window (bit i = non-EOS, newest at bit 0)
  int32_t win_len;
  int32_t status;
  int32_t pad0;
  uint32_t gkey[8];
  uint32_t skey[8];
  uint64_t gdraw;
  uint64_t sdraw;
  int32_t global_out[32];
  // ChaCha12 keystream block cache of each stream (k_advance): 16 consecutive draws share one
  // block, so 15 of 16 draws are a word read instead of a ChaCha12 block on the critical path.
  // *_blk_id = block index + 1 (0: empty -- the host zero-fills a new request's block)
  uint64_t gblk_id;
  uint64_t sblk_id;
  uint32_t gblk[16];
  uint32_t sblk[16];
  // Sampling parameters of the two phases (top_k_g / top_k_s above are their top-k; 0: no top-k).
  // The reference fixes (1.0, 0.95) (normal_mode_inference.rs:114-127); a request may set others.
  float temp_g, temp_s;
  float top_p_g, top_p_s;
};
static_assert(sizeof(SlotCtrl) % 8 == 0, "control blocks are copied as an array; next_token is read at a 4-byte stride");

// The sampling options of a slot's semantic phase that do not fit the control block, which keeps
// the size and layout its snapshots and tests/native/sched_sampling_main.cpp know: one array of
// SlotSampling beside the control blocks (AdvanceArgs::samp). The host writes a slot's whole block
// at every admission, in stream order before the slot's first step -- neutral penalties and
// on = 0 for a request without them, so nothing survives from the slot's previous owner; after
// that the kernel alone moves miro.mu. The address is fixed, so the step stays capturable in the
// decode graph.

// Penalties (rwkvtts.h rwkvtts_penalties): k_advance_params applies them to the logits of every
// token that occurs in the last `window` semantic tokens (0: in all of them). Neutral (1, 0, 0):
// the row is sampled as it arrived and the slot's count row (AdvanceArgs::pen_counts) is neither
// read nor written.
struct SlotPenalty {
  float repetition, frequency, presence;
  int32_t window;
};
static_assert(sizeof(SlotPenalty) == 16, "penalty blocks are copied as an array");

// Mirostat state (rwkvtts.h rwkvtts_request_ext::mirostat): mu = 2 tau at admission, then moved
// by k_advance_miro once per emitted semantic token.
struct SlotMiro {
  float tau, rate, mu;
  int32_t on;
};
static_assert(sizeof(SlotMiro) == 16, "Mirostat blocks are copied as an array");

struct SlotSampling {
  SlotPenalty pen;
  SlotMiro miro;
};
static_assert(sizeof(SlotSampling) == 32, "sampling blocks are copied as an array");

}  // namespace rwkvtts
