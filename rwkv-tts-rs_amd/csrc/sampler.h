// sampler.h -- device sampler (src/rwkv_sampler.rs:55-211) and the on-device phase controller
// (src/normal_mode_inference.rs:222-391, src/zero_shot_inference.rs:128-309).
#pragma once
#include "common.h"
#include "slot_ctrl.h"

namespace rwkvtts {

constexpr int kSampleMaxN = 16384;       // row length held in LDS (longer rows: global scratch)
constexpr int kSampleMaxSorted = 4096;   // survivors sortable for top-p in LDS
constexpr int kSampleMaxRowLen = 1 << 24;  // generic sampler API row limit

struct SampleRowArgs {
  const float* logits;  // [rows][ld]
  int ld;
  int n;
  float temperature;
  float top_p;
  int top_k;
  int forbid;
  const uint32_t* keys;     // [rows][8] or null (-> StdRng(42), draw 0)
  const uint64_t* draws;    // [rows]
  int32_t* out;             // [rows]
  float* dbg;               // optional [rows][2]: softmax sum, r
  uint64_t* stamps;         // optional [rows][16]: s_memtime at phase boundaries (diagnostics)
  char* scratch;            // n > kSampleMaxN: [rows][scratch_stride] bytes (wide_scratch_bytes(n))
  size_t scratch_stride;
};

struct AdvanceArgs {
  const float* logits;   // [n_part][rows][ld] split-K partial logits (summed in order)
  int ld;
  int n_part;
  int64_t part_stride;
  const int* row_slot;   // step row -> slot (rows of this decode/prefill step with logits)
  SlotCtrl* ctrl;
  int32_t* sem_out;      // [S][2048]
  int n_rows;
  unsigned long long* tl;  // debug timeline slot (null in production)
  int cert;              // set by launch_advance: 1 certified fast path allowed (sample_cert)
  uint64_t* stamps;      // debug: [rows][16] s_memtime phase stamps (RWKVTTS_DEBUG_STAMPS adv=; null in production)
  AdvanceKind kind;      // the kernel launch_advance picks (slot_ctrl.h): the highest kind among the rows' slots
  // [S] sampling block of each slot: k_advance_params and k_advance_miro read pen, k_advance_miro
  // alone reads miro and moves miro.mu. May be null when kind == kAdvFixed.
  SlotSampling* samp;
  // [S][kPenCounts] occurrences of each semantic id in a penalised slot's history window
  // (samp[slot].pen). Derived state that k_advance_params keeps by itself: a slot's row is zeroed
  // at its first semantic step instead of being read, the emitted id is counted after every step
  // and the id that leaves the window is uncounted. Rows of slots without penalties are never
  // touched. May be null when no row's slot is penalised.
  uint16_t* pen_counts;
};
constexpr int kPenCounts = RWKVTTS_EOS_TOKEN;  // ids [0, 8192): EOS never enters the history

size_t wide_scratch_bytes(int n);
void launch_sample_rows(const SampleRowArgs& a, int rows, hipStream_t st);
// cert: 1 = the certified fast path allowed (the default), 0 = the exact walk always
int launch_advance(const AdvanceArgs& a, hipStream_t st, int cert = 1);

}  // namespace rwkvtts
