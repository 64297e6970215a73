/*
 * rwkvtts.h -- C-ABI drop-in boundary for the RWKV-TTS inference hot path on MI355X (gfx950).
 *
 * Every entry point here replaces one reference interface of liuzl/rwkv-tts-rs @ 2025-12-05
 * (paths relative to the reference root); the Rust-side binding a maintainer would add is in
 * INTEGRATION.md. Conventions: plain pointers + sizes, opaque handles, int status (0 = OK,
 * negative = error, message via rwkvtts_last_error()), no exceptions across the ABI, all
 * buffers caller-owned. One engine per GPU. Engine entry points serialise on a per-engine
 * lock (concurrent callers queue; they do not share GPU steps); the request manager
 * (rwkvtts_manager_*: DynamicBatchManager) is the thread-safe, batching front door: any number
 * of threads submit, one owner thread per GPU engine runs continuous batching.
 */
#ifndef RWKVTTS_H
#define RWKVTTS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- constants: src/rwkv_sampler.rs:294-299, src/properties_util.rs:5 ------------------ */
#define RWKVTTS_EOS_TOKEN 8192          /* TTS_EOS_TOKEN */
#define RWKVTTS_TAG_0 8193              /* TTS_TAG_0 */
#define RWKVTTS_TAG_1 8194              /* TTS_TAG_1 */
#define RWKVTTS_TAG_2 8195              /* TTS_TAG_2 */
#define RWKVTTS_GLOBAL_TOKEN_OFFSET 8196 /* GLOBAL_TOKEN_OFFSET */
#define RWKVTTS_SPECIAL_TOKEN_OFFSET 77823 /* TTS_SPECIAL_TOKEN_OFFSET */
#define RWKVTTS_N_GLOBAL 32             /* normal_mode_inference.rs:220 global_tokens_size */
#define RWKVTTS_SEMANTIC_LIMIT 2048     /* normal_mode_inference.rs:316 */
#define RWKVTTS_HOP 320                 /* 参考/C/tts/sparktts.h:55 latent_hop_length */
#define RWKVTTS_SAMPLE_RATE 16000       /* 参考/C/tts/sparktts.h:53 */

/* status codes */
#define RWKVTTS_OK 0
#define RWKVTTS_EINVAL -1
#define RWKVTTS_EHIP -2
#define RWKVTTS_ENOMEM -3
#define RWKVTTS_EUNSUPPORTED -4
#define RWKVTTS_EBUSY -5     /* manager: result not ready yet (poll / wait timeout) */
#define RWKVTTS_ECLOSED -6   /* manager: shut down before the request ran */

/* weight storage dtypes (matrices; vectors are always f32) */
#define RWKVTTS_DTYPE_BF16 0
#define RWKVTTS_DTYPE_F16 1

/* ---- model description ------------------------------------------------------------------ */
/* RWKV-7 "x070" dims (tensor names A.3). web-rwkv ModelInfo analogue. */
typedef struct {
  int32_t n_layer;   /* L */
  int32_t n_embd;    /* C */
  int32_t head_size; /* N (64); H = C / N */
  int32_t n_ffn;     /* F */
  int32_t n_vocab;   /* V */
  int32_t d_decay;   /* w LoRA rank */
  int32_t d_aaa;     /* a LoRA rank */
  int32_t d_mv;      /* v LoRA rank */
  int32_t d_gate;    /* g LoRA rank */
} rwkvtts_dims;

/* Packed weight blob: tensor index -> byte offset. Matrices in [out][in] row-major
 * (the LoRA matrices are stored transposed relative to the checkpoint so that every
 * projection reads contiguous rows of its input dimension). */
enum {
  RWKVTTS_T_EMB = 0, RWKVTTS_T_LN0_W, RWKVTTS_T_LN0_B, RWKVTTS_T_LNOUT_W, RWKVTTS_T_LNOUT_B,
  RWKVTTS_T_HEAD, RWKVTTS_T_GLOBAL_COUNT
};
enum {
  RWKVTTS_L_LN1_W = 0, RWKVTTS_L_LN1_B, RWKVTTS_L_LN2_W, RWKVTTS_L_LN2_B,
  RWKVTTS_L_XR, RWKVTTS_L_XW, RWKVTTS_L_XK, RWKVTTS_L_XV, RWKVTTS_L_XA, RWKVTTS_L_XG,
  RWKVTTS_L_W0, RWKVTTS_L_A0, RWKVTTS_L_V0, RWKVTTS_L_KK, RWKVTTS_L_KA, RWKVTTS_L_RK,
  RWKVTTS_L_LNX_W, RWKVTTS_L_LNX_B, RWKVTTS_L_FFN_XK,
  /* ---- matrices from here on ---- */
  RWKVTTS_L_WR, RWKVTTS_L_WK, RWKVTTS_L_WV, RWKVTTS_L_WO,
  RWKVTTS_L_W1T, RWKVTTS_L_A1T, RWKVTTS_L_V1T, RWKVTTS_L_G1T, /* [D][C] */
  RWKVTTS_L_W2T, RWKVTTS_L_A2T, RWKVTTS_L_V2T, RWKVTTS_L_G2T, /* [C][D] */
  RWKVTTS_L_FFN_K, /* [F][C] */
  RWKVTTS_L_FFN_V, /* [C][F] */
  RWKVTTS_L_COUNT
};
#define RWKVTTS_L_FIRST_MAT RWKVTTS_L_WR

/* Fill rows/cols of one tensor. Returns 1 for a matrix (2-byte dtype), 0 for an f32 vector. */
static inline int rwkvtts_tensor_shape(const rwkvtts_dims* d, int layer, int t, int64_t* rows,
                                       int64_t* cols) {
  const int64_t C = d->n_embd, V = d->n_vocab, F = d->n_ffn;
  if (layer < 0) {
    switch (t) {
      case RWKVTTS_T_EMB: *rows = V; *cols = C; return 1;
      case RWKVTTS_T_HEAD: *rows = V; *cols = C; return 1;
      default: *rows = 1; *cols = C; return 0;
    }
  }
  switch (t) {
    case RWKVTTS_L_WR: case RWKVTTS_L_WK: case RWKVTTS_L_WV: case RWKVTTS_L_WO:
      *rows = C; *cols = C; return 1;
    case RWKVTTS_L_W1T: *rows = d->d_decay; *cols = C; return 1;
    case RWKVTTS_L_A1T: *rows = d->d_aaa; *cols = C; return 1;
    case RWKVTTS_L_V1T: *rows = d->d_mv; *cols = C; return 1;
    case RWKVTTS_L_G1T: *rows = d->d_gate; *cols = C; return 1;
    case RWKVTTS_L_W2T: *rows = C; *cols = d->d_decay; return 1;
    case RWKVTTS_L_A2T: *rows = C; *cols = d->d_aaa; return 1;
    case RWKVTTS_L_V2T: *rows = C; *cols = d->d_mv; return 1;
    case RWKVTTS_L_G2T: *rows = C; *cols = d->d_gate; return 1;
    case RWKVTTS_L_FFN_K: *rows = F; *cols = C; return 1;
    case RWKVTTS_L_FFN_V: *rows = C; *cols = F; return 1;
    default: *rows = 1; *cols = C; return 0;
  }
}

/* Byte offset of tensor t of `layer` (-1 = global tensors) in the packed blob; every tensor
 * starts on a 256-byte boundary. With layer == -2 returns the total blob size. */
static inline int64_t rwkvtts_tensor_offset(const rwkvtts_dims* d, int layer, int t) {
  int64_t off = 256; /* header */
  int64_t r, c;
  for (int l = -1; l < d->n_layer; ++l) {
    const int n = (l < 0) ? RWKVTTS_T_GLOBAL_COUNT : RWKVTTS_L_COUNT;
    for (int i = 0; i < n; ++i) {
      if (l == layer && i == t) return off;
      int m = rwkvtts_tensor_shape(d, l, i, &r, &c);
      int64_t bytes = r * c * (m ? 2 : 4);
      off += (bytes + 255) & ~(int64_t)255;
    }
  }
  return off;
}
static inline int64_t rwkvtts_blob_bytes(const rwkvtts_dims* d) {
  return rwkvtts_tensor_offset(d, -2, 0);
}

/* Blob header (first 256 bytes). */
typedef struct {
  uint32_t magic;   /* 'RWT7' = 0x37545752 */
  uint32_t version; /* 1 */
  int32_t dtype;    /* RWKVTTS_DTYPE_* of the matrices */
  int32_t pad0;
  rwkvtts_dims dims;
} rwkvtts_blob_header;
#define RWKVTTS_BLOB_MAGIC 0x37545752u

/* Deterministic synthetic weights (N(0, 0.02) matrices, decay w0 chosen so that
 * w in (0.3, 0.99), lerp coefficients in [0,1]); counter-based so every tool regenerates the
 * same blob. `out` must hold rwkvtts_blob_bytes(dims) bytes. */
int rwkvtts_synth_weights(const rwkvtts_dims* dims, int dtype, uint64_t seed, void* out);

/* ---- engine: SharedRwkvRuntime::new / v7::Bundle::new (src/shared_runtime.rs:70-208) ---- */
typedef struct rwkvtts_engine rwkvtts_engine;

typedef struct {
  int32_t device;           /* HIP device ordinal */
  int32_t max_slots;        /* state slots = Bundle max_batch (shared_runtime.rs:177) */
  int32_t token_chunk_size; /* prompt rows per forward step, shared by the admitted requests (the
                               reference's per-request RnnInput token_chunk_size, 512 at
                               lightweight_tts_pipeline.rs:799; outputs are chunk-invariant) */
  int32_t use_graphs;       /* capture decode steps in hipGraphs */
  int32_t wkv_variant;      /* ignored: every value selects the one WKV kernel the shape has; kept
                               for layout compatibility */
  /* web-rwkv ModelBuilder::quant(HashMap<layer, Quant>) as the server builds it from
   * --quant-layers / --quant-type (bin/server.rs:1029-1071, src/shared_runtime.rs:156-160):
   * layers [0, quant_layers) store their r / k / v / o and FFN key / value matrices quantised
   * (the LoRA matrices, embedding and head stay 16-bit). RWKVTTS_QUANT_NONE when 0 layers. */
  int32_t quant_layers;
  int32_t quant_type;       /* RWKVTTS_QUANT_* */
  /* Decode-step forms. 0 (the default) = the shipping forms. Each RWKVTTS_FORM_* bit switches one
   * fused form back to the launches it replaces; tokens and the recurrent state are bitwise equal
   * either way (tests/test_gpu_ffn_persist.py, test_gpu_emb_fusion.py). For verification and A/B
   * timing: no bit makes the engine faster. No reference counterpart (web-rwkv has one form). */
  uint32_t forms;
} rwkvtts_engine_desc;

#define RWKVTTS_FORM_SEPARATE_ATT 1u   /* attention half: LN1 / rkv / WKV / Wo launches, not k_att_persist */
#define RWKVTTS_FORM_SEPARATE_FFN 2u   /* FFN half: LN2 / key / value launches, not k_ffn_persist */
#define RWKVTTS_FORM_LN_ROWS 4u        /* one-row steps: LayerNorm workgroups, not the row-fused LayerNorm */
#define RWKVTTS_FORM_SLAB_HANDOFF 8u   /* one-row steps: partial slabs + counters, not data-tagged granules */
#define RWKVTTS_FORM_SEPARATE_LNOUT 16u /* one-row steps: ln_out launch, not folded into the head GEMM */
#define RWKVTTS_FORM_SEPARATE_EMBED 32u /* decode steps: k_embed launch, not folded into layer 0's LayerNorm */
#define RWKVTTS_FORM_EXACT_SAMPLER 64u /* k_advance: always the exact sequential-sum walk (no certificate) */
#define RWKVTTS_FORM_VALUE_TILE_32X64 128u /* k_ffn_persist, 17..32 rows: 32 x 64 value tiles, not 16 x 128 */

#define RWKVTTS_QUANT_NONE 0
#define RWKVTTS_QUANT_INT8 1 /* 128-element blocks along K: f16 (min, max), u8 q; w = min + q (max - min)/255 */
#define RWKVTTS_QUANT_NF4 2  /* 64-element blocks along K: f16 absmax, 4-bit NormalFloat index; w = nf4[q] absmax */
#define RWKVTTS_QUANT_SF4 3  /* rejected (RWKVTTS_EUNSUPPORTED): its code table is not available offline */

/* weights: packed blob (header included). blob_on_device != 0: `weights` is a device pointer
 * on desc->device (e.g. a buffer filled by an RCCL broadcast); it is copied. */
int rwkvtts_engine_create(const rwkvtts_engine_desc* desc, const void* weights, size_t bytes,
                          int blob_on_device, rwkvtts_engine** out);
int rwkvtts_engine_destroy(rwkvtts_engine* e);
const char* rwkvtts_last_error(void);
int rwkvtts_engine_dims(const rwkvtts_engine* e, rwkvtts_dims* out);

/* ---- state: State::init/load/back (normal_mode_inference.rs:66-70) --------------------- */
/* Per-slot state = per layer [att_shift C | wkv H*N*N (value-major S[i][j]) | ffn_shift C] f32. */
int64_t rwkvtts_state_floats(const rwkvtts_engine* e);
int rwkvtts_slot_reset(rwkvtts_engine* e, int slot);                 /* State::load(init, slot) */
int rwkvtts_slot_read(rwkvtts_engine* e, int slot, float* host_out); /* State::back(slot) */
int rwkvtts_slot_write(rwkvtts_engine* e, int slot, const float* host_in);

/* ---- LM runtime: Runtime<Rnn>::infer (normal_mode_inference.rs:62-80) ------------------ */
#define RWKVTTS_OPT_LAST 0 /* RnnOption::Last */
#define RWKVTTS_OPT_FULL 1 /* RnnOption::Full (logits for every token) */
typedef struct {
  int32_t slot;           /* batch index == state slot */
  const uint32_t* tokens; /* pending input tokens of this batch */
  int32_t n_tokens;
  int32_t option;         /* RWKVTTS_OPT_* */
} rwkvtts_input;

/* Consumes up to token_chunk_size tokens in total across `inputs` (each batch advances by
 * consumed[i]). For every batch whose input is exhausted by this call and option == LAST,
 * writes logits of its last token to logits[i * head_rows ... + head_rows) and sets
 * has_logits[i] = 1 (RnnOutput[i].0.size() > 0); otherwise has_logits[i] = 0.
 * head_rows <= n_vocab selects the leading vocabulary rows (all samplers read a prefix).
 * OPT_FULL writes logits for every consumed token at logits[(row) * head_rows], rows in
 * input order. logits is a HOST buffer. */
int rwkvtts_infer(rwkvtts_engine* e, const rwkvtts_input* inputs, int n_inputs, int head_rows,
                  float* logits, int32_t* consumed, int32_t* has_logits);

/* ---- sampler: sample_logits_with_top_p_k (src/rwkv_sampler.rs:55-211) ------------------ */
/* rand 0.8.5 StdRng (ChaCha12, seed_from_u64 via PCG32) is represented statelessly by its
 * 32-byte key and the index of the next u32 draw. */
typedef struct {
  uint32_t key[8];
  uint64_t draw_index;
} rwkvtts_rng;
void rwkvtts_rng_seed_from_u64(uint64_t seed, rwkvtts_rng* out); /* StdRng::seed_from_u64 */

typedef struct {
  float temperature;
  float top_p;
  int32_t top_k;
  int32_t forbid_token; /* -1 = None */
} rwkvtts_sample_args;

/* Samples n_rows rows of `logits` (host, n_rows x row_len f32) on the GPU; rng[i] == NULL
 * mirrors `rng: &mut None` (fixed StdRng(42) draw). rngs advance by one draw per row.
 * Any row_len up to 2^24 and every (temperature, top_p, top_k) of the reference is accepted:
 * rows up to 16384 run in LDS, longer rows (the 77,923-token vocabulary) in a device scratch.
 * out_tokens receives the index per row. */
int rwkvtts_sample(rwkvtts_engine* e, const float* logits, int n_rows, int row_len,
                   const rwkvtts_sample_args* args, rwkvtts_rng* const* rngs, int32_t* out_tokens);

/* ---- phase controllers + scheduler ------------------------------------------------------ */
/* TtsBatchRequest (src/rwkv_sampler.rs:222-231) after tokenisation
 * (dynamic_batch_manager.rs:512-515) and property-token construction (properties_util.rs:76-98). */
#define RWKVTTS_MODE_AUTO 0      /* zero-shot iff both ref token sets present (dbm.rs:526-540) */
typedef struct {
  float temperature, top_p;
  int32_t top_k;
} rwkvtts_phase_sampling;
typedef struct {
  float repetition, frequency, presence; /* neutral: 1, 0, 0 */
  int32_t window;                        /* last `window` semantic tokens; 0: all of them */
} rwkvtts_penalties;
typedef struct {
  const int32_t* text_tokens;
  int32_t n_text;
  const int32_t* property_tokens;
  int32_t n_property;
  const int32_t* ref_global;   /* NULL = None */
  int32_t n_ref_global;
  const int32_t* ref_semantic; /* NULL = None */
  int32_t n_ref_semantic;
  int32_t has_seed;
  uint64_t seed;
  int32_t max_tokens;          /* SamplerArgs.max_tokens; normal mode emits at most
                                  min(max_tokens, 2048) semantic tokens (normal_mode_inference.rs:316),
                                  so 0 -> none; must be >= 0 (usize) */
  int32_t fixed_semantic;      /* >0: benchmark mode -- EOS masked, exactly this many semantic tokens */
  int32_t greedy;              /* 1: top_k = 1 for both phases (config 1 plumbing check) */
  /* SamplerArgs.layered_randomness (LayeredRandomnessConfig, rwkv_sampler.rs:251-275) as used
   * by normal_mode_inference.rs:138-174 and zero_shot_inference.rs:204-216.
   * layered_set == 0 selects LayeredRandomnessConfig::default() (independent, 1000 / 2000). */
  int32_t layered_set;
  int32_t use_independent_seeds; /* 1: StdRng(seed + offset); 0: StdRng(seed + 100 / + 200),
                                    zero-shot StdRng(0) (dynamic_batch_manager.rs:491-494) */
  uint64_t global_seed_offset;
  uint64_t semantic_seed_offset;
  /* Per-request sampling of the two phases. The reference fixes (temperature, top_p, top_k) per
   * phase -- (1.0, 0.95, 20) global, (1.0, 0.95, 80) semantic, normal_mode_inference.rs:114-127 --
   * whatever the request says; a zero-filled request keeps exactly that. sampling_set bit 0:
   * global_sampling holds, bit 1: semantic_sampling holds (zero-shot has no global phase:
   * global_sampling is accepted there and unused). A set phase needs temperature in [0.1, 4.0],
   * top_p in [0, 1] and top_k >= 0 (0 or >= the row length: no top-k; top_p >= 1: no top-p);
   * anything else, unknown bits, or `greedy` together with sampling_set fails the request alone.
   * Cost per decode step: temperature 1 with 1 <= top_k <= 256 is the
   * certified fast path; temperature != 1 adds the exact sequential softmax sum (no certificate
   * covers powf); top_k 0 or > 256 takes the general path (a sort over the row). */
  int32_t sampling_set;
  rwkvtts_phase_sampling global_sampling, semantic_sampling;
  /* Pinned voice (no reference counterpart: a normal-mode request of the reference always samples
   * its own 32 global tokens). 1: ref_global holds exactly RWKVTTS_N_GLOBAL ids in [0, 4096) and
   * ref_semantic is NULL; anything else fails the request alone (RWKVTTS_EINVAL). The request is
   * normal mode with the global phase replaced by the given tokens: its prompt is property
   * tokens, TAG_2, text, TAG_0, g_0 + 8196 .. g_31 + 8196, TAG_1 -- what a normal request feeds
   * itself while decoding (normal_mode_inference.rs:277-278) -- the property tokens are kept, EOS
   * ends it (no hard minimum, no window, no re-draw), the semantic stream is seeded as for a normal
   * request and the global stream is unused. So a pinned request with the globals G a normal
   * request sampled returns that request's (G, S), bit for bit. max_tokens == 0 (without
   * fixed_semantic) gives status 0, the 32 globals and no semantic tokens. 0: as before. */
  int32_t pinned_voice;
  /* Repetition, frequency and presence penalties (src/sampler_manager.rs:229-292; the reference's
   * TTS path never calls them). penalty_set bit 0: `penalties` holds; any other bit fails the
   * request alone; 0: the request is sampled as before, by the kernel that served it before.
   * They apply to the SEMANTIC phase only: the global phase draws its 32 tokens once, from logits
   * over another id range, and has nothing to loop over. For one semantic step of a request that
   * has emitted h[0, n_sem): H = h[max(0, n_sem - window), n_sem) (window 0: all of h), cnt[t] =
   * occurrences of t in H, x = the f32 logit of t as the sampler receives it, before EOS masking.
   * Every t with cnt[t] > 0 is adjusted, in this order, each operation one f32 operation rounded
   * to nearest:
   *   1. repetition != 1: cnt[t] times x = x > 0 ? x / repetition : x * repetition. PER
   *      OCCURRENCE, as apply_repetition_penalty loops over the token list: it compounds. It is
   *      not the once-per-distinct-token rule of other libraries.
   *   2. frequency != 0: x = x - (frequency * (float)cnt[t]), a multiply, then a subtract (no FMA).
   *   3. presence != 0:  x = x - presence.
   * -inf stays -inf. The sampler then runs as before on the adjusted row (EOS mask, top-k, top-p,
   * temperature, draw); the zero-shot re-draw with EOS masked uses the same adjusted row. EOS is
   * never part of the history -- a step that draws it ends the request or re-draws with it masked
   * -- so EOS is never penalised.
   * repetition in [0.25, 4], frequency and presence in [-8, 8], window in [0, 2048], all finite;
   * anything else fails the request alone (RWKVTTS_EINVAL). Unlike sampling_set, penalties may be
   * combined with `greedy` (top-k 1 at (1.0, 0.95)): deterministic decoding is where loops are
   * worst. They combine with sampling_set, pinned_voice, fixed_semantic and zero-shot mode. The
   * neutral values (1, 0, 0) are valid and change nothing, the kernel included; any other value
   * puts the request's steps on the parameter-reading controller. */
  int32_t penalty_set;
  rwkvtts_penalties penalties;
} rwkvtts_request;
#define RWKVTTS_SAMPLING_GLOBAL 1
#define RWKVTTS_SAMPLING_SEMANTIC 2
#define RWKVTTS_PENALTY_SET 1

/* ---- request extension block ----------------------------------------------------------------
 * rwkvtts_request keeps its size and layout; what a request may ask for beyond it travels in a
 * block beside it (rwkvtts_generate_batch_ex, rwkvtts_manager_submit_ex). struct_size is
 * sizeof(rwkvtts_request_ext) as the caller was built with it: a library reads no field that lies
 * past it, and a request whose struct_size is smaller than the fields it asks the library to read
 * fails alone with RWKVTTS_EINVAL. No block, or mirostat_set == 0: the request is the plain one.
 *
 * Mirostat (mirostat_set bit 0: `mirostat` holds; any other bit fails the request alone), the
 * reference's one sampler with state from step to step (参考/ai00_server/crates/ai00-core/src/
 * sampler/mirostat.rs; its TTS path never calls it). SEMANTIC phase only -- the global phase has 32
 * draws and nothing to adapt over -- where it REPLACES the phase's top-k, top-p and temperature:
 * each step's distribution is cut at a surprise threshold mu, and mu moves so that the running
 * surprise of the emitted tokens stays near tau. For one semantic attempt of a slot with threshold
 * mu, on the row as the sampler receives it, after any penalty adjustment, every operation one f32
 * operation rounded to nearest:
 *   1. p[i] exactly as the sampler's softmax: the forbid / EOS mask to -inf, the max, glibc
 *      expf(x - max), the sequential f32 sum in index order, the divide.
 *   2. c = #{i : p[i] > 0 and -lg(p[i]) <= mu}, n_pos = #{i : p[i] > 0}, K = min(c + 1, n_pos).
 *   3. The kept set is the first K ranks in the order (p descending, index ascending). (ai00's
 *      "first rank whose surprise exceeds the threshold, inclusive", written as a count: it can
 *      be taken in parallel and stays well defined where lg is not monotone in its last bit.)
 *   4. cum[r] = the sequential f32 sum over ranks 0..r; S = cum[K-1].
 *   5. u = r32 * S, one rounded multiply; r32 is the semantic stream's next draw (the same
 *      draw + attempt indexing as without Mirostat).
 *   6. The token is the first rank with u <= cum[r] (rank K-1 always satisfies it).
 *   7. After the attempt whose token is emitted, and only then: s = lg(S) - lg(p_tok);
 *      e = s - tau; mu = mu - rate * e, a multiply and then a subtract, never an FMA;
 *      mu = fminf(mu, 4 * tau).
 * A zero-shot attempt that draws EOS and is re-drawn leaves mu unchanged, and the re-draw uses the
 * same mu; an EOS that ends the request needs no update. Initial mu = 2 * tau, set at admission.
 * lg(x) = (float) of the double log2_inline of glibc 2.35's powf (the 16-entry table and the
 * degree-5 polynomial with its written fmas; csrc/exact_math.h lg2f, one source for host and
 * kernel; rwkvtts_debug_lg2 exports it).
 * tau in [0.5, 10], rate in [0.001, 1], both finite; anything else fails the request alone, and so
 * does Mirostat together with `greedy` or with RWKVTTS_SAMPLING_SEMANTIC (ai00's sampler kinds
 * exclude each other). It combines with RWKVTTS_SAMPLING_GLOBAL, penalty_set, pinned_voice,
 * fixed_semantic and zero-shot mode. The threshold is not returned. */
typedef struct {
  uint32_t struct_size;  /* sizeof(rwkvtts_request_ext) the caller was built with */
  int32_t mirostat_set;  /* bit 0: `mirostat` holds; other bits fail the request alone */
  struct { float tau, rate; } mirostat; /* ai00's defaults: 3.0, 0.1 */
} rwkvtts_request_ext;
#define RWKVTTS_MIROSTAT_SET 1

typedef struct {
  int32_t status;         /* 0 ok; <0 this request failed -> (vec![], vec![]) as dbm.rs:466-469
                             (the others of its batch still complete) */
  int32_t n_global;
  int32_t n_semantic;
  int32_t global_tokens[RWKVTTS_N_GLOBAL];
  int32_t* semantic_tokens; /* caller buffer, capacity >= RWKVTTS_SEMANTIC_LIMIT */
} rwkvtts_result;

/* DynamicBatchManager::generate_tts_batch (dynamic_batch_manager.rs:124-164) with real GPU
 * continuous batching: up to max_slots requests decode together, one slot each; a request is
 * admitted as soon as a slot frees, and its prompt rows ride in the same forward steps as the
 * other slots' decode rows. Per-request outputs are identical to running the requests one at a
 * time. Returns RWKVTTS_OK when the batch ran (per-request failures are in results[i].status),
 * or a negative code when the engine itself failed (then every status is that code). */
int rwkvtts_generate_batch(rwkvtts_engine* e, const rwkvtts_request* reqs, int n,
                           rwkvtts_result* results);

/* ---- token progress (streaming; no reference counterpart: generate_tts returns at the end) -- */
/* fn(user, global_tokens, n_global, semantic, first, count, done, status): semantic tokens
 * [first, first + count) of one request (`semantic` points at the first of them; the pointers are
 * valid during the call only), with the global tokens known so far (all 32 before the first
 * semantic token of a normal-mode request). Tokens arrive in order, each exactly once; the last
 * call has done = 1 and the request's status (then count may be 0). A request that fails ends with
 * done = 1 and a negative status; tokens of a unit of work that faulted are never delivered. */
typedef void (*rwkvtts_token_fn)(void* user, const int32_t* global_tokens, int32_t n_global,
                                 const int32_t* semantic, int32_t first, int32_t count, int32_t done,
                                 int32_t status);
typedef struct {
  rwkvtts_token_fn fn; /* NULL: no progress for this request */
  void* user;
} rwkvtts_token_sink;
/* rwkvtts_generate_batch with one sink per request (sinks == NULL: none). The sinks run on the
 * calling thread, between the engine's units of work (a mixed prompt step, or up to 8 decode steps);
 * they must not call into this engine. Results are those of rwkvtts_generate_batch, and a batch
 * without sinks enqueues exactly the GPU work rwkvtts_generate_batch enqueues. */
int rwkvtts_generate_batch_stream(rwkvtts_engine* e, const rwkvtts_request* reqs, int n,
                                  rwkvtts_result* results, const rwkvtts_token_sink* sinks);
/* rwkvtts_generate_batch_stream with one extension block per request: exts == NULL, a NULL element
 * or mirostat_set == 0 is that call exactly (it and rwkvtts_generate_batch are wrappers over this
 * one). The blocks are copied when the call starts. */
int rwkvtts_generate_batch_ex(rwkvtts_engine* e, const rwkvtts_request* reqs, const rwkvtts_request_ext* const* exts,
                              int n, rwkvtts_result* results, const rwkvtts_token_sink* sinks);

/* ---- request manager: DynamicBatchManager (dynamic_batch_manager.rs:22-164,185-405) ------ */
/* The reference collects requests (enqueue_worker: first request, then try_recv up to
 * max_batch_size; a lone request waits >= 10 ms for company, :185-264) and hands each batch to
 * whichever infer worker is free (:350-405), which then runs the batch sequentially on state
 * slot 0. Here one owner thread per engine (one engine per GPU: request-level data parallelism
 * over the node's GPUs) runs continuous batching; each collected batch is routed to
 * the least-loaded engine (fewest requests active + queued), and an engine admits queued
 * requests between forward steps whenever it has free slots. Any thread may submit / wait. */
typedef struct rwkvtts_manager rwkvtts_manager;
#define RWKVTTS_MAX_ENGINES 16
typedef struct {
  int32_t n_engines;                      /* engines (owner threads) */
  int32_t devices[RWKVTTS_MAX_ENGINES];   /* HIP device of each engine (repeats allowed) */
  rwkvtts_engine_desc engine;             /* per-engine settings (its .device is ignored) */
  int32_t max_batch_size;                 /* DynamicBatchConfig.max_batch_size (batch_types.rs:71) */
  int32_t collect_timeout_ms;             /* DynamicBatchConfig.collect_timeout_ms (batch_types.rs:73) */
} rwkvtts_manager_desc;
/* weights: one host blob. It crosses PCIe once, into the first engine's device; the manager then
 * broadcasts it over RCCL (ncclBroadcast over xGMI, one rank per distinct device, ncclCommInitAll)
 * to the other devices, and engines that share a device copy it device-to-device. With a single
 * distinct device RCCL is never loaded; if RCCL is missing or cannot initialise, the blob goes to
 * the other devices by hipMemcpyPeer (stats.bcast_rccl = 0). RWKVTTS_MANAGER_NO_RCCL=1 disables
 * RCCL; RWKVTTS_MANAGER_FORCE_RCCL=1 runs it even for one device (and fails create if it fails).
 * The caller's current HIP device is unchanged on return. This replaces
 * the reference's single model load handed to every infer worker (src/shared_runtime.rs:143-184,
 * src/dynamic_batch_manager.rs:33-87). */
int rwkvtts_manager_create(const rwkvtts_manager_desc* desc, const void* weights, size_t bytes,
                           rwkvtts_manager** out);
/* Stops the collector and the engine threads after the requests already submitted finish.
 * Threads blocked in rwkvtts_manager_wait when destroy starts return (their result, or
 * RWKVTTS_ECLOSED) before destroy frees the handle. No call on the handle may START while
 * destroy runs or after it: the caller serialises destroy against new submit / wait /
 * get_stats calls (as dropping the reference's manager requires no outstanding borrow). */
int rwkvtts_manager_destroy(rwkvtts_manager* m);
/* generate_tts (dynamic_batch_manager.rs:90-121) split in two: submit copies the request
 * (token arrays included) and returns a ticket; wait blocks up to timeout_ms (< 0: forever) and
 * returns RWKVTTS_OK with the result (the ticket is then released), RWKVTTS_EBUSY if the
 * request has not finished yet. out->semantic_tokens must hold RWKVTTS_SEMANTIC_LIMIT ids. */
int rwkvtts_manager_submit(rwkvtts_manager* m, const rwkvtts_request* req, uint64_t* ticket);
int rwkvtts_manager_wait(rwkvtts_manager* m, uint64_t ticket, int timeout_ms, rwkvtts_result* out);
/* Streaming by polling (no foreign thread ever calls back into the caller): submit_stream is submit
 * for a request whose token progress the engine publishes after every unit of work. wait_tokens
 * blocks up to timeout_ms (< 0: forever) until more than have_semantic semantic tokens are known or
 * the request is done, then copies everything known so far: global32 (32 ids), *n_global,
 * semantic_out (capacity RWKVTTS_SEMANTIC_LIMIT), *n_semantic, *done and *status (the request's,
 * once done). RWKVTTS_EBUSY on a timeout (the outputs are filled all the same). It does not release
 * the ticket: rwkvtts_manager_wait still returns the final result and releases it. Completion
 * publishes whatever was not published before, so a stream always terminates; a ticket from plain
 * submit can be polled too (its tokens then appear at completion). One thread at a time may be in
 * wait / wait_tokens on a ticket. */
int rwkvtts_manager_submit_stream(rwkvtts_manager* m, const rwkvtts_request* req, uint64_t* ticket);
/* submit (stream == 0) or submit_stream (stream != 0) with an extension block, which is copied;
 * ext == NULL is the plain call (both are wrappers over this one). */
int rwkvtts_manager_submit_ex(rwkvtts_manager* m, const rwkvtts_request* req, const rwkvtts_request_ext* ext,
                              int stream, uint64_t* ticket);
int rwkvtts_manager_wait_tokens(rwkvtts_manager* m, uint64_t ticket, int32_t have_semantic, int timeout_ms,
                                int32_t* global32, int32_t* n_global, int32_t* semantic_out,
                                int32_t* n_semantic, int32_t* done, int32_t* status);
/* generate_tts_batch (dynamic_batch_manager.rs:124-164): submit all, wait all. */
int rwkvtts_manager_generate_batch(rwkvtts_manager* m, const rwkvtts_request* reqs, int n,
                                   rwkvtts_result* results);
typedef struct {
  int64_t submitted;
  int64_t completed;
  int64_t batches;                          /* batches the collector formed */
  int64_t served[RWKVTTS_MAX_ENGINES];      /* requests completed per engine */
  int64_t max_active[RWKVTTS_MAX_ENGINES];  /* most slots an engine had decoding at once */
  int64_t steps[RWKVTTS_MAX_ENGINES];       /* forward steps per engine */
  int32_t bcast_ranks;                      /* distinct devices in the weight broadcast (RCCL ranks) */
  int32_t bcast_rccl;                       /* 1: the weights went out by ncclBroadcast */
  double bcast_ms;                          /* upload + broadcast wall time at create */
  int32_t waiters;                          /* threads blocked in rwkvtts_manager_wait now */
  int32_t reserved;
  int32_t persistent[RWKVTTS_MAX_ENGINES];  /* 1: the engine runs the persistent decode launches (at most
                                               one engine per GPU, across processes: rwkvtts_stats) */
} rwkvtts_manager_stats;
int rwkvtts_manager_get_stats(rwkvtts_manager* m, rwkvtts_manager_stats* out);

/* Step-level statistics of the last generate call (bench / roofline). */
typedef struct {
  int64_t steps;            /* decode steps */
  int64_t prefill_steps;
  double decode_ms;         /* HIP-event time of all decode steps */
  double prefill_ms;
  double sample_ms;         /* sampler kernels inside decode steps */
  int64_t decode_rows;      /* sum over decode steps of active rows */
  int32_t profile_kernel_count;
  int32_t persistent;       /* 1: this engine holds its GPU's persistent-launch slot (the first engine
                               created on the device in any process, RWKVTTS_LOCK_DIR lock file);
                               others run the separate launches (same outputs, bit for bit) */
} rwkvtts_stats;
int rwkvtts_get_stats(rwkvtts_engine* e, rwkvtts_stats* out);

/* Per-kernel timing: rwkvtts_set_profiling(e, 1) = HIP events on eager launches (graphs off);
 * (e, 2) = in-graph timing: the decode graphs are recaptured with launch-timeline slots and the
 * last step of every graph-replayed decode window is sampled (first workgroup start to last
 * workgroup end per launch, the interval rocprofv3 --kernel-trace reports); 0 = off. Calling
 * it again with the same mode clears the accumulated entries. Entries: name, launches, total ms. */
int rwkvtts_set_profiling(rwkvtts_engine* e, int on);
int rwkvtts_profile_entry(rwkvtts_engine* e, int idx, char* name, int name_cap, int64_t* launches,
                          double* total_ms);

/* Test hook, not part of the drop-in surface (no reference counterpart): runs the production
 * decode-step sampler/controller k_advance (sample_logits_with_top_p_k + the phase controllers of
 * normal_mode_inference.rs:222-391 / zero_shot_inference.rs, as the decode graphs run it) on
 * caller-given logit rows [n_rows][8193] and controller states, n_steps launches; exact = 1 forces
 * the exact sequential-sum walk. `rows` points to n_rows records of 72 bytes: int32 mode (0 normal,
 * 1 zero-shot), phase (0 global, 2 semantic), top_k, fixed, n_sem, hard_min, win_bits, win_len;
 * uint32 key[8] (ChaCha12 key of the phase's stream); uint64 draw (next u32 draw index).
 * Outputs out_tok / out_used / out_phase are [n_steps][n_rows]. */
int rwkvtts_debug_advance(rwkvtts_engine* e, const float* logits, int n_rows, const void* rows, int exact,
                          int n_steps, int32_t* out_tok, int32_t* out_used, int32_t* out_phase);
/* The same with per-row sampling parameters: `rows` points to n_rows records of 88 bytes, the 72
 * above followed by uint32 struct_size (= 88), float temperature, float top_p and 4 bytes of
 * padding. top_k may be 0 here (no top-k); temperature in [0.1, 4.0], top_p in [0, 1]. A row with
 * (1.0, 0.95) gives what rwkvtts_debug_advance gives for its first 72 bytes. */
int rwkvtts_debug_advance_ex(rwkvtts_engine* e, const float* logits, int n_rows, const void* rows, int exact,
                             int n_steps, int32_t* out_tok, int32_t* out_used, int32_t* out_phase);
/* The same with per-row penalties: `rows` points to n_rows records of 104 bytes, the 88 above
 * (struct_size = 104) followed by float repetition, frequency, presence and int32 window, in the
 * ranges of rwkvtts_request::penalties. n_steps may be up to 256 here: the fixed logits are sampled
 * step after step while the row's semantic history grows. A row with penalties other than (1, 0, 0)
 * must start at n_sem 0. A row with (1, 0, 0) gives what rwkvtts_debug_advance_ex gives for its
 * first 88 bytes. */
int rwkvtts_debug_advance_pen(rwkvtts_engine* e, const float* logits, int n_rows, const void* rows, int exact,
                              int n_steps, int32_t* out_tok, int32_t* out_used, int32_t* out_phase);
/* The same with per-row Mirostat: `rows` points to n_rows records of 120 bytes, the 104 above
 * (struct_size = 120) followed by float tau, rate, the initial mu and int32 on (0: the row is
 * sampled as rwkvtts_debug_advance_pen samples its first 104 bytes; 1: tau and rate in the ranges
 * of rwkvtts_request_ext::mirostat, mu finite). Up to 256 launches on the same logits; out_mu
 * [n_steps][n_rows] receives every row's mu after each launch (the initial mu where on == 0). */
int rwkvtts_debug_advance_miro(rwkvtts_engine* e, const float* logits, int n_rows, const void* rows, int exact,
                               int n_steps, int32_t* out_tok, int32_t* out_used, int32_t* out_phase, float* out_mu);
/* Host self-test entry point: out[i] = lg(x[i]) of the Mirostat contract above, for positive
 * finite x (subnormals included). Needs no engine and no GPU. */
void rwkvtts_debug_lg2(const float* x, int n, float* out);

/* Test hook, not part of the drop-in surface: rows [0, n_rows) x head_rows of the logits that the
 * engine's last forward step left on the device (n_rows <= the engine's row capacity; a decode step
 * of R slots wrote rows [0, R)). `out` is a HOST buffer of n_rows x head_rows floats. */
int rwkvtts_debug_last_logits(rwkvtts_engine* e, int n_rows, int head_rows, float* out);

/* ---- codec: BiCodecDetokenize via ORT (lightweight_tts_pipeline.rs:606-622,706-730) ----- */
typedef struct rwkvtts_codec rwkvtts_codec;
typedef struct {
  int32_t codebook_size;  /* 8192 semantic codes */
  int32_t codebook_dim;   /* 8 */
  int32_t latent_dim;     /* 1024 */
  int32_t n_global;       /* 32 speaker tokens */
  int32_t fsq_levels;     /* 4 (per dim) */
  int32_t fsq_dims;       /* 6 -> 4^6 = 4096 codes */
  int32_t spk_dim;        /* d-vector 1024 */
  int32_t prenet_dim;     /* ConvNeXt dim 384 */
  int32_t prenet_inter;   /* 2048 */
  int32_t prenet_layers;  /* 12 */
  int32_t dec_channels;   /* 1536 */
  int32_t n_up;           /* 4 */
  int32_t up_rates[4];    /* 8,5,4,2 */
  int32_t up_kernels[4];  /* 16,11,8,4 */
} rwkvtts_codec_dims;
int64_t rwkvtts_codec_blob_bytes(const rwkvtts_codec_dims* d);
/* rwkvtts_codec_create refuses, with RWKVTTS_EINVAL and before it touches a device, dims the decoder
 * cannot run: a product of up_rates other than RWKVTTS_HOP (the PCM buffers hold 320 samples per
 * frame), a ConvTranspose with k < s, odd k - s or more than 7 taps per phase (ceil(k / s)), channel
 * counts that are no multiples of 64 (last stage: of 32, at most 112), prenet_dim above 512. */
int rwkvtts_codec_synth_weights(const rwkvtts_codec_dims* d, uint64_t seed, float* out);
int rwkvtts_codec_create(int device, const rwkvtts_codec_dims* d, const float* weights,
                         rwkvtts_codec** out);
/* As rwkvtts_codec_create with the conv weight path chosen by the caller:
 * RWKVTTS_CODEC_WEIGHTS_AUTO (what rwkvtts_codec_create does): the weight hi + lo planes (three
 * MFMAs per product) iff some conv weight is not bf16-exact, so f32 checkpoints keep ~2^-16
 * relative weights; _BF16: bf16 weights (two MFMAs; faster, the weights rounded to bf16);
 * _HILO: hi + lo planes always (on bf16-exact weights bitwise the _BF16 PCM, tested). */
#define RWKVTTS_CODEC_WEIGHTS_AUTO 0
#define RWKVTTS_CODEC_WEIGHTS_BF16 1
#define RWKVTTS_CODEC_WEIGHTS_HILO 2
int rwkvtts_codec_create_ex(int device, const rwkvtts_codec_dims* d, const float* weights, int weight_path,
                            rwkvtts_codec** out);
int rwkvtts_codec_destroy(rwkvtts_codec* c);
/* semantic [T] i64, global [n_global] i64 -> pcm [T * 320] f32 (output "wav_rec"). */
int rwkvtts_codec_decode(rwkvtts_codec* c, const int64_t* semantic, int T, const int64_t* global,
                         float* pcm);
/* decode_audio_batch (lightweight_tts_pipeline.rs:625-703): n utterances in one pass. */
int rwkvtts_codec_decode_batch(rwkvtts_codec* c, const int64_t* const* semantic, const int* T,
                               const int64_t* const* global, int n, float* const* pcm);
/* ---- codec, streaming: exact windowed decode (no reference counterpart: the reference decodes a
 * finished utterance only) --------------------------------------------------------------------
 * The decoder is a finite stack of convolutions (its LayerNorms work per frame, the speaker vector
 * comes from the global tokens alone), so the samples of frames [t0, t1) depend only on the tokens
 * [t0 - H, t1 + H), with zero padding at the true ends of the utterance only. H = prenet_halo +
 * wave_halo frames per side: wave_halo for conv_in .. conv_out (10 at the SparkTTS rates), and
 * prenet_halo = 3 * (prenet_layers + 1) for the prenet's 7-tap convolutions. Host only. */
int rwkvtts_codec_halo(const rwkvtts_codec_dims* d, int32_t* prenet_halo, int32_t* wave_halo);
/* New structs start with struct_size = sizeof(the struct) as the caller compiled it, so they can
 * grow without a new entry point. */
typedef struct {
  uint32_t struct_size;
  int32_t ctx0, ctx1;   /* tokens [ctx0, ctx1) the prenet runs on: at most (t1 - t0) + 2 H */
  int32_t wave0, wave1; /* frames [wave0, wave1) conv_in .. conv_out run on: at most (t1 - t0) + 2 wave_halo */
} rwkvtts_codec_plan;
/* The work rwkvtts_codec_decode_windows does for one window (it calls this same function). Host
 * only. Ranges are clipped at 0 and at n_known. RWKVTTS_EINVAL unless 0 <= t0 < t1 <= n_known and
 * (final or t1 + H <= n_known). */
int rwkvtts_codec_window_plan(const rwkvtts_codec_dims* d, int32_t t0, int32_t t1, int32_t n_known,
                              int32_t final, rwkvtts_codec_plan* out);
typedef struct {
  uint32_t struct_size;
  int32_t n_known;         /* semantic tokens known so far */
  int32_t final;           /* 1: n_known is the utterance's length */
  int32_t t0, t1;          /* frames to decode */
  const int64_t* semantic; /* [n_known], from frame 0 */
  const int64_t* global;   /* [n_global] */
  float* pcm;              /* capacity (t1 - t0) * 320 */
} rwkvtts_codec_window;
/* n windows (ragged, of any utterances) in one batched pass. pcm = samples [t0 * 320, t1 * 320) of
 * rwkvtts_codec_decode over the whole utterance, bitwise (tests/test_gpu_codec_windows.py), whatever
 * tokens follow t1 + H. A window that breaks window_plan's precondition, or a code out of range
 * inside its context, fails the call with RWKVTTS_EINVAL before anything is launched. */
int rwkvtts_codec_decode_windows(rwkvtts_codec* c, const rwkvtts_codec_window* w, int n);
/* Verification forms of later decode calls (0 = shipping); the PCM is bitwise equal either way
 * (tests/test_gpu_codec.py). No reference counterpart (ORT runs one graph). */
#define RWKVTTS_CODEC_FORM_SEPARATE_RESUNIT 1u /* 96-channel residual units as conv7 + conv1 launches */
#define RWKVTTS_CODEC_FORM_CHANNEL_LAST 2u     /* WaveGenerator planes [t][c] instead of [c / 32][t][32] */
int rwkvtts_codec_set_forms(rwkvtts_codec* c, uint32_t forms);
/* ---- codec test hooks, not part of the drop-in surface -------------------------------------
 * One record per k_conv launch of a decode, in launch order: what the launch computes and which
 * k_conv instantiation, grid and LDS size the host chooses for it. The decode path takes its choice
 * from the same function that fills these records. Tensor references are
 * group * 1000000 + index * 100 + tensor of include/rwkvtts_codec_layout.h, -1 for none. */
typedef struct {
  uint32_t struct_size;
  int32_t kind;             /* 0 conv, 1 ConvTranspose, 2 fused residual unit (conv7 -> Snake -> conv1) */
  int32_t ci, co, k, dil, pad, s;
  int32_t tin_mul;          /* input rows per frame; output rows per frame: tin_mul (* s for kind 1) */
  int32_t tn, kt, wlo, nwv; /* k_conv<TN, KT, WLO, NWV, kind == 2> */
  int32_t shm_bytes;
  int32_t xmap, gx, gy;     /* XCD-mapped 1-D grid; time tiles; phases * column tiles */
  int32_t grid[3];
  int32_t act;              /* 1: exact GELU */
  int32_t has_y, has_planes, has_res, has_rbias;
  int32_t w, bias, gamma, y_alpha, mid_alpha, w1, bias1;
} rwkvtts_codec_launch;
/* The launches of a decode of n utterances of at most Tmax frames, for a decoder on the weight hi
 * + lo path (weight_lo != 0) or not, with the given RWKVTTS_CODEC_FORM_* bits. Fills up to `cap`
 * records of `out` (nullable) and returns the number of launches, or a negative RWKVTTS_E* code
 * (dims that rwkvtts_codec_create refuses, or a launch for which no tile fits). Host only. */
int rwkvtts_codec_debug_launch_plan(const rwkvtts_codec_dims* d, int weight_lo, uint32_t forms, int n, int Tmax,
                                    rwkvtts_codec_launch* out, int cap);
/* Arms launch `launch` (an index into the plan above; -1 disarms) of the NEXT decode call: around
 * that launch the decode synchronises and copies out the launch's inputs (before) and outputs
 * (after). The call after that runs unarmed again. A decode whose launch `launch` does not match
 * the plan's record fails with RWKVTTS_EINVAL. */
int rwkvtts_codec_debug_capture(rwkvtts_codec* c, int launch);
/* The captured launch: its record, utterance count and rows per utterance (Tmax * tin_mul in,
 * * s out for a ConvTranspose). */
int rwkvtts_codec_debug_captured_launch(rwkvtts_codec* c, rwkvtts_codec_launch* rec, int32_t* n, int32_t* rows_in,
                                        int32_t* rows_out);
/* One captured array as logical [n][rows][C], channel blocking undone. what: 0 / 1 input hi / lo
 * planes (bf16 bits, [n][rows_in][ci]); 2 residual (f32, [n][rows_out][co], before the launch);
 * 3 y (f32); 4 / 5 output hi / lo planes (bf16 bits); 6 per-utterance bias (f32 [n][co]). Rows past
 * an utterance's length hold whatever the buffers held. Returns the array's size in bytes (0: the
 * launch has no such array) and copies it to `out` if cap_bytes suffices (out nullable). */
int64_t rwkvtts_codec_debug_captured(rwkvtts_codec* c, int what, void* out, int64_t cap_bytes);
/* Per-stage HIP-event timing of later decode calls (profiling on): name, launches, total ms. */
int rwkvtts_codec_set_profiling(rwkvtts_codec* c, int on);
int rwkvtts_codec_profile_count(rwkvtts_codec* c);
int rwkvtts_codec_profile_entry(rwkvtts_codec* c, int idx, char* name, int name_cap, int64_t* launches,
                                double* total_ms);

/* ---- text tokenizer: web-rwkv Tokenizer::new / encode (src/shared_runtime.rs:187-192,
 * src/dynamic_batch_manager.rs:512-515) over assets/model/tokenizer.json -------------------- */
typedef struct rwkvtts_tokenizer rwkvtts_tokenizer;
/* vocab_json: the vocabulary file's bytes ({"id": "token" | [bytes], ...}). */
int rwkvtts_tokenizer_create(const char* vocab_json, size_t len, rwkvtts_tokenizer** out);
int rwkvtts_tokenizer_destroy(rwkvtts_tokenizer* t);
/* Greedy longest match over UTF-8 bytes. ids == NULL (or cap too small) only counts: *n_ids is
 * always the full count. A byte position no token matches -> RWKVTTS_EINVAL
 * (TokenizerError::NoMatchingTokenFound). */
int rwkvtts_tokenizer_encode(const rwkvtts_tokenizer* t, const uint8_t* text, size_t n, uint32_t* ids,
                             size_t cap, size_t* n_ids);
int rwkvtts_tokenizer_decode(const rwkvtts_tokenizer* t, const uint32_t* ids, size_t n, uint8_t* text,
                             size_t cap, size_t* n_bytes);
int64_t rwkvtts_tokenizer_vocab_size(const rwkvtts_tokenizer* t); /* max id + 1 */

/* ---- zero-shot reference mel (src/tts_pipeline_fixes.rs:12-159) ------------------------- */
/* wav [n] f32 @16 kHz -> mel [128][n_frames] (n_frames = (n + 1024 - 1024) / 320 + 1). */
int rwkvtts_mel(int device, const float* wav, int n, float* mel, int* n_frames);

/* ---- resampler: rubato SincFixedIn as src/ref_audio_utilities.rs:532-576 configures it, on the
 * GPU, for the reference-audio front end and for output rates other than 16 kHz (the reference
 * resamples on the host and only when it loads a reference WAV) --------------------------------
 * The arithmetic contract (what makes every output bitwise-testable):
 *   table   sincs[O][L] f32 (O = oversampling, L = sinc_len): rubato's make_sincs with the
 *           Blackman-Harris^2 window and cutoff = f_cutoff if ratio >= 1 else f_cutoff * ratio
 *   ratio   = (double)sr_out / (double)sr_in, t_ratio = 1.0 / ratio
 *   n_out   = (int64)ceil(n * ratio), in double
 *   position of output o, every step one IEEE double operation (never fused):
 *           idx = (double)o * t_ratio - delay, start = floor(idx), pos = (idx - start) * O,
 *           p0 = floor(pos), w1 = (float)(pos - p0)
 *   taps    tap k (0 .. L-1) reads input sample j = start + k - L/2 + 1, zero outside [0, n)
 *   sums    a = sum_k x[j_k] * sincs[p0 % O][k], b = sum_k x[j_k] * sincs[(p0 + 1) % O][k]: each a
 *           sequential f32 sum in ascending k starting from +0, one rounded multiply then one
 *           rounded add per tap (no fused multiply-add)
 *   result  out[o] = a + (b - a) * w1: three rounded f32 operations, no fma
 *   align   RUBATO: delay = L/2 (rubato's start delay kept, the tail cut by L/2 input samples: the
 *           behaviour of the Python restatement, for the reference-audio front end);
 *           ZERO: delay = 0 (output o sits at input time o * t_ratio: for synthesised output). */
#define RWKVTTS_RESAMPLE_ALIGN_RUBATO 0
#define RWKVTTS_RESAMPLE_ALIGN_ZERO 1
typedef struct {
  uint32_t struct_size;
  int32_t sr_in, sr_out; /* 1 .. 192000 each */
  int32_t sinc_len;      /* L: a multiple of 8, 8 .. 1024; 0 = 256 */
  int32_t oversampling;  /* O: 1 .. 1024; 0 = 256 */
  double f_cutoff;       /* in (0, 1]; 0 = 0.95 */
  int32_t align;         /* RWKVTTS_RESAMPLE_ALIGN_* */
} rwkvtts_resample_desc;
/* The library's own table builder (host only): out[O * L]. The normalising sum is taken in double.
 * Anything outside the ranges above is RWKVTTS_EINVAL, here and in every call that takes a desc. */
int rwkvtts_resample_sincs(const rwkvtts_resample_desc* desc, float* out);
/* ceil(n_in * ratio) (host only); -1 for a bad desc or n_in < 0. */
int64_t rwkvtts_resample_out_len(const rwkvtts_resample_desc* desc, int64_t n_in);
/* Streaming plan (host only, a pure function). With samples [0, n_known) of a signal known:
 * *out_ready_end = the first output some tap of which reaches sample n_known or later; never more
 * than out_len(n_known), the signal's output count if it ended here (outputs from there on wait for
 * more samples or for final). With final (n_known is the signal's length) it is out_len(n_known).
 * *in_first_needed = max(0, lowest tap index of output out_first): samples before it are never read
 * again once outputs [0, out_first) are done -- the tail a stream must keep. Either pointer may be
 * NULL. It is monotone in n_known and in out_first. */
int rwkvtts_resample_plan(const rwkvtts_resample_desc* desc, int64_t n_known, int final, int64_t out_first,
                          int64_t* out_ready_end, int64_t* in_first_needed);
typedef struct rwkvtts_resampler rwkvtts_resampler;
/* table == NULL: the table of rwkvtts_resample_sincs; otherwise the caller's [O][L] table (copied). */
int rwkvtts_resampler_create(int device, const rwkvtts_resample_desc* desc, const float* table,
                             rwkvtts_resampler** out);
int rwkvtts_resampler_destroy(rwkvtts_resampler* r);
/* n signals (ragged) in one launch; host buffers; out[i] has capacity out_len(n_in[i]).
 * n_in[i] == 0 is allowed and writes nothing. Calls on one resampler serialise on its lock. */
int rwkvtts_resample_batch(rwkvtts_resampler* r, const float* const* in, const int64_t* n_in, int n,
                           float* const* out);
typedef struct {
  uint32_t struct_size;
  const float* in;    /* points at sample in_first of the signal */
  int64_t in_first;
  int64_t n_in;
  int32_t final;      /* 1: in_first + n_in is the signal's length */
  int64_t out_first;  /* outputs [out_first, out_first + out_count) */
  int64_t out_count;
  float* out;         /* capacity out_count */
} rwkvtts_resample_window;
/* n windows (of any signals) in one launch: outputs [out_first, out_first + out_count) of the
 * whole-signal resample, bitwise, whatever follows the known samples. RWKVTTS_EINVAL before anything
 * is launched (and nothing written) if a tap of a requested output falls outside the given samples --
 * out_first + out_count > out_ready_end(in_first + n_in, final) or in_first >
 * in_first_needed(out_first) by rwkvtts_resample_plan: taps below sample 0 and, with final, taps
 * past the end are the only zeros. */
int rwkvtts_resample_windows(rwkvtts_resampler* r, const rwkvtts_resample_window* w, int n);
/* HIP-event time of the last launch's kernel alone (no copies), in ms; 0 before the first launch. */
int rwkvtts_resampler_kernel_ms(rwkvtts_resampler* r, double* ms);

/* ---- time stretch: pitch-preserving time-scale modification (WSOLA, waveform-similarity
 * overlap-add) on the GPU, the `tempo` of the pipeline (no reference counterpart: the reference's
 * only rate control is the `speed` property token) ----------------------------------------------
 * Rate-agnostic; the pipeline applies it to the vocoder's 16 kHz PCM, before any resampling.
 * The arithmetic contract (every output bit is defined by IEEE f32 add, subtract and multiply: no
 * division, no square root):
 *   W, Hs, D  window (even), synthesis hop Hs = W/2, search radius
 *   tempo     double, per signal, 0.25 .. 4.0; above 1 is faster speech
 *   window    w[i] = (float)(0.5 - 0.5 * cos(2 * pi * i / W)), in double, i in [0, W)
 *   n_out     = (int64)ceil((double)n / tempo), 0 for n = 0
 *   frames    M = ceil(n_out / Hs) blocks; frames m = -1, 0, .. M-1 start at input sample s_m:
 *             s_-1 = -Hs, s_0 = 0; for m >= 1 the anchor is a_m = (int64)floor((double)(m * Hs) * tempo)
 *             (one double multiply) and s_m = a_m + shift_m
 *   search    (m >= 1) template t[i] = x[s_{m-1} + Hs + i], i in [0, Hs): where frame m-1 would go on.
 *             Candidate shifts in [-D, D), ranked k = 0, 1, 2, .. for 0, -1, +1, -2, +2, ..,
 *             -(D-1), +(D-1), -D. d(shift) = sum_i (t[i] - x[a_m + shift + i])^2: a sequential f32
 *             sum in ascending i starting from +0, each term one rounded subtract, one rounded
 *             multiply and one rounded add (never fused). shift_m has the smallest d and, among
 *             equal d, the lowest rank; a NaN d counts as +inf. As d >= 0 otherwise, the key
 *             (f32 bits of d) << 32 | k is totally ordered as an unsigned 64-bit integer: the winner
 *             is its minimum, whatever the reduction tree.
 *   output    block j covers o in [j * Hs, (j+1) * Hs) below n_out; with i = o - j * Hs:
 *             y[o] = w[Hs + i] * x[s_{j-1} + Hs + i] + w[i] * x[s_j + i]: two rounded multiplies and
 *             one rounded add, the earlier frame's product on the left
 *   zeros     every read of x outside [0, n) is +0
 * So on silence every shift is 0, and at tempo 1.0 every shift is 0 (d(0) = 0 exactly) and the output
 * differs from the input by the rounding of w[Hs + i] + w[i] alone. */
typedef struct {
  uint32_t struct_size;
  int32_t window; /* W: even, 32 .. 2048; 0 = 512 */
  int32_t search; /* D: 1 .. 1024; 0 = 128 (0 is the default, not a radius: negative is out of range) */
} rwkvtts_tsm_desc;
/* The window table (host only): out[W]. Anything outside the ranges above, and a tempo outside
 * 0.25 .. 4.0 (NaN included), is RWKVTTS_EINVAL, here and in every call that takes a desc or a tempo. */
int rwkvtts_tsm_window(const rwkvtts_tsm_desc* desc, float* out);
/* ceil(n_in / tempo) (host only); -1 for a bad desc, a bad tempo or n_in < 0. */
int64_t rwkvtts_tsm_out_len(const rwkvtts_tsm_desc* desc, double tempo, int64_t n_in);
/* Streaming plan (host only, a pure function). With samples [0, n_known) of a signal known, blocks
 * [0, block_first) done and s_prev = s_{block_first - 1} (-Hs for block_first 0; anything that is no
 * possible start of that frame is RWKVTTS_EINVAL):
 * *out_ready_end = the end (an output index, a multiple of Hs) of the ready blocks from block_first
 * on, block_first * Hs if there is none. A block is ready when every sample that its two frames'
 * searches and its own products can read lies below n_known -- for block block_first that is
 * max(s_prev + 2 Hs, a_m + D + Hs - 1), for a later block the same with the highest start its earlier
 * frame can take, a_{m-1} + D - 1 -- and the block lies wholly below out_len(n_known). So block j is
 * ready at the latest when ceil((j+1) * Hs * tempo) + D + 2 Hs <= n_known. With final (n_known is the
 * signal's length) it is out_len(n_known).
 * *in_first_needed = max(0, min(s_prev + Hs, a_block_first - D)): samples before it are never read
 * again -- the tail a stream must keep, fewer than 2 D + 2 Hs * max(tempo, 1) + 2 samples once the
 * ready blocks are out. Either pointer may be NULL. Monotone in n_known. */
int rwkvtts_tsm_plan(const rwkvtts_tsm_desc* desc, double tempo, int64_t n_known, int final, int64_t block_first,
                     int64_t s_prev, int64_t* out_ready_end, int64_t* in_first_needed);
typedef struct rwkvtts_tsm rwkvtts_tsm;
/* table == NULL: the window of rwkvtts_tsm_window; otherwise the caller's [W] table (copied). */
int rwkvtts_tsm_create(int device, const rwkvtts_tsm_desc* desc, const float* table, rwkvtts_tsm** out);
int rwkvtts_tsm_destroy(rwkvtts_tsm* t);
/* n signals (ragged), each with its own tempo, in one launch pair (search, overlap-add): one
 * workgroup walks a signal's frames in order. Host buffers; out[i] has capacity
 * out_len(tempo[i], n_in[i]). n_in[i] == 0 writes nothing. Calls on one handle serialise on its lock. */
int rwkvtts_tsm_batch(rwkvtts_tsm* t, const float* const* in, const int64_t* n_in, const double* tempo, int n,
                      float* const* out);
typedef struct {
  uint32_t struct_size;
  const float* in;     /* points at sample in_first of the signal */
  int64_t in_first;
  int64_t n_in;
  int32_t final;       /* 1: in_first + n_in is the signal's length */
  double tempo;
  int64_t block_first; /* outputs [block_first * Hs, block_first * Hs + out_count) */
  int64_t s_prev;      /* s_{block_first - 1}: -Hs for block_first 0, else the last call's s_last */
  int64_t out_count;
  float* out;          /* capacity out_count */
  int64_t s_last;      /* out: the start of the last frame used (s_prev if out_count is 0) */
} rwkvtts_tsm_window_t;
/* n windows (of any signals, any tempos) in one launch pair: outputs [block_first * Hs, + out_count)
 * of the whole-signal result, bitwise, whatever follows the known samples. RWKVTTS_EINVAL before
 * anything is launched (and nothing written, s_last included) if a window asks for more than
 * rwkvtts_tsm_plan allows: block_first * Hs + out_count > out_ready_end(in_first + n_in, final,
 * block_first, s_prev), in_first > in_first_needed, or an impossible s_prev. */
int rwkvtts_tsm_windows(rwkvtts_tsm* t, rwkvtts_tsm_window_t* w, int n);
/* HIP-event time of the last launch pair (both kernels, no copies), in ms; 0 before the first. */
int rwkvtts_tsm_kernel_ms(rwkvtts_tsm* t, double* ms);

/* ---- join: the PCM of a long text's segments into one signal, each segment's silent edges cut to
 * a kept margin and faded, a controlled pause after it, on the GPU (no reference counterpart: the
 * reference synthesises one request per text and stops at 2048 semantic tokens) ------------------
 * Rate-agnostic; the pipeline applies it to the vocoder's 16 kHz PCM, before the stretch and the
 * resampler. The arithmetic contract (integer bounds, one rounded f32 multiply per faded sample,
 * every other sample a copy):
 *   desc      threshold (f32, finite, >= 0; 0 = 0.01, the reference's silence_threshold), keep
 *             (samples, >= 0), fade (samples, 0 .. 4096), trim (0 or 1)
 *   job       n_seg segments x_s[0, n_s), each followed by gap_s >= 0 zero samples; n_s == 0 allowed
 *   bounds    trim == 0: a_s = 0, b_s = n_s, no fades. trim == 1: a sample is loud iff
 *             fabsf(x) > threshold (false for NaN); no loud sample: a_s = b_s = 0 (an empty piece);
 *             otherwise, lo and hi the first and last loud index, a_s = max(0, lo - keep) and
 *             b_s = min(n_s, hi + 1 + keep): integers, whatever the reduction tree
 *   ramp      r[k] = (float)((k + 0.5) / fade), in double, k in [0, fade)
 *   piece     (trim == 1) len_s = b_s - a_s, f_s = min(fade, len_s / 2); p[i] = x[a_s + i] * r[i]
 *             for i < f_s, p[i] = x[a_s + i] * r[len_s - 1 - i] for i >= len_s - f_s (one rounded
 *             f32 multiply each), every other sample x[a_s + i] bit for bit. Both edges fade whether
 *             or not a cut was made there. trim == 0: the piece is the segment.
 *   layout    off_0 = 0, off_{s+1} = off_s + len_s + gap_s (64-bit); the piece at off_s, then gap_s
 *             samples of +0.0f; n_out = off_{n_seg}
 * A piece depends on its own segment only, so the join of a job equals the joins of its segments
 * one by one, back to back, bitwise: a stream may emit segment by segment. */
typedef struct {
  uint32_t struct_size;
  float threshold;
  int32_t keep;
  int32_t fade;
  int32_t trim;
} rwkvtts_join_desc;
/* The ramp table (host only): out[fade] (nothing is written for fade 0). Anything outside the
 * ranges above (a NaN or infinite threshold included) is RWKVTTS_EINVAL, here and in every call
 * that takes a desc. */
int rwkvtts_join_ramp(const rwkvtts_join_desc* desc, float* out);
/* sum n_s + sum gap_s: the capacity of a job's output, reached when nothing is cut (host only);
 * -1 for a negative length or gap, n_seg outside 0 .. 4096 or a segment above 2^30 samples. */
int64_t rwkvtts_join_capacity(const int64_t* n, const int64_t* gap, int32_t n_seg);
typedef struct rwkvtts_join rwkvtts_join;
/* table == NULL: the ramp of rwkvtts_join_ramp; otherwise the caller's [fade] table (copied). */
int rwkvtts_join_create(int device, const rwkvtts_join_desc* desc, const float* table, rwkvtts_join** out);
int rwkvtts_join_destroy(rwkvtts_join* j);
typedef struct {
  uint32_t struct_size;
  int32_t n_seg;            /* 0 .. 4096 */
  const float* const* seg;  /* [n_seg] host pointers (NULL allowed where n is 0) */
  const int64_t* n;         /* [n_seg] samples per segment, each 0 .. 2^30 */
  const int64_t* gap;       /* [n_seg] zero samples after each segment */
  float* out;               /* capacity rwkvtts_join_capacity(n, gap, n_seg); [n_out, capacity) is +0 */
  int64_t* a;               /* out: [n_seg] a_s (NULL: not wanted) */
  int64_t* b;               /* out: [n_seg] b_s (NULL: not wanted) */
  int64_t n_out;            /* out */
} rwkvtts_join_job;
/* n jobs (1 .. 1024, ragged) in one pass of three launches -- bounds (per-segment integer min / max
 * over workgroups; not launched for trim 0), layout (the prefix over a job's segments), write (a
 * lane per output sample: copy, fade or zero). Host buffers. n_out and every (a_s, b_s) are read
 * back before the call's one synchronisation. Nothing is launched and nothing written unless every
 * job passes the checks above. Calls on one handle serialise on its lock. */
int rwkvtts_join_jobs(rwkvtts_join* j, rwkvtts_join_job* jobs, int n);
/* HIP-event time of the last call's kernels (no copies), in ms; 0 before the first. */
int rwkvtts_join_kernel_ms(rwkvtts_join* j, double* ms);

/* ---- level: a look-ahead loudness leveller with a peak ceiling on the GPU, the `loudness` of the
 * pipeline (no reference counterpart: the reference peak-normalises a finished WAV to 0.8, which sets
 * no loudness and cannot be streamed) -----------------------------------------------------------
 * Runs on the 16 kHz PCM, after the stretch and before the resampler. One causal definition with a
 * bounded look-ahead, so a stream's pieces are bitwise the one-shot result. The arithmetic contract
 * (every output bit is defined by IEEE f32 operations: rounded add, subtract and multiply, never
 * fused, and correctly rounded divide and square root; no log, no pow):
 *   B, L, A   block length, FIR length, look-ahead in blocks; H the memory in blocks (0: unbounded)
 *   T2        the target, an f32 mean square per signal: (float)10^((loudness_dB + 0.691) / 10), in
 *             double (rwkvtts_level_target)
 *   table     h[0, L) then r[0, B), f32. h: the first L samples of the impulse response of the two
 *             BS.1770 K-weighting biquads re-derived for 16 kHz, in double, rounded to f32. Bilinear
 *             design, K = tan(pi * f0 / fs). Shelf (f0 = 1681.974450955533, G = 3.999843853973347 dB,
 *             Q = 0.7071752369554196): Vh = 10^(G/20), Vb = Vh^0.4996667741545416,
 *             a0 = 1 + K/Q + K*K, b = [(Vh + Vb*K/Q + K*K), 2(K*K - Vh), (Vh - Vb*K/Q + K*K)] / a0,
 *             a = [1, 2(K*K - 1)/a0, (1 - K/Q + K*K)/a0]. High-pass (f0 = 38.13547087602444,
 *             Q = 0.5003270373238773): b = [1, -2, 1], a of the same form. Each biquad is run in
 *             direct form I on the unit impulse, shelf first, every step one double operation:
 *             y[n] = (((b0*x[n] + b1*x[n-1]) + b2*x[n-2]) - a1*y[n-1]) - a2*y[n-2].
 *             r[i] = (float)((double)(i + 1) / (double)B).
 *   measure   z[n] = sum_k h[k] * x[n-k]: a sequential f32 sum in ascending k from +0, one rounded
 *             multiply then one rounded add per tap; x below sample 0 is +0. Block j covers samples
 *             [jB, (j+1)B); z and x at or past the signal's end are +0 (the last block may be
 *             partial). E_j from 64 partials: p[l] = sum of z[i]*z[i] over the block's i = l (mod 64),
 *             ascending from +0 (one rounded multiply, one rounded add), then p[l] += p[l+s] for
 *             l < s, s = 32, 16, 8, 4, 2, 1; E_j = p[0]. pk_j = max |x| over the block.
 *             P_j = ((((+0 + E_{j-3}) + E_{j-2}) + E_{j-1}) + E_j) / (float)(4B); E below block 0 is +0.
 *   gain      a serial scan: before g_j, every block k <= min(j + A, last) not yet entered enters in
 *             ascending k: if P_k >= gate then, while N < H or H == 0, S = S + P_k and N = N + 1,
 *             otherwise S = (S - S / (float)H) + P_k. From S = +0, N = 0.
 *             g_j = 1 if N == 0, else sqrt(T2 / (S / (float)N)); then g_j = g_min if g_j < g_min;
 *             then g_j = g_max if g_j > g_max; then, with p = max(pk_j, pk_{j+1}) (0 for a block
 *             that does not exist): if g_j * p > C then g_j = C / p. The peak cap wins over g_min.
 *   apply     sample i of block j: y = x * (g_{j-1} + (g_j - g_{j-1}) * r[i]), g_{-1} = g_0.
 * So n_out = n; silence comes back bit for bit (g = 1, and x * 1 = x); and |y| <= C * (1 + 2^-20):
 * both ends of block j's ramp were capped against pk_j, and at most five roundings follow. A
 * non-finite sample leaves the outputs from its block on unspecified; nothing is read or written
 * out of bounds. Every default below is untuned: the repository has no real checkpoint. */
typedef struct {
  uint32_t struct_size;
  int32_t block;     /* B: a multiple of 64, 64 .. 4800; 0 = 1600 (100 ms) */
  int32_t taps;      /* L: a multiple of 64, 64 .. 2048; 0 = 1024 */
  int32_t lookahead; /* A: 1 .. 16; 0 = 4 */
  float gate;        /* finite, > 0; 0 = 1e-5 (-50 dB) */
  float ceiling;     /* C: finite, > 0; 0 = 0.891 */
  float g_min;       /* finite, > 0; 0 = 0.1 */
  float g_max;       /* finite, >= g_min; 0 = 10, the cap of the reference's WAV normalisation */
  int32_t horizon;   /* H: 0 .. 2^24; 0 = unbounded */
} rwkvtts_level_desc;
/* The library's own table builder (host only): out[L + B]. Anything outside the ranges above (NaN
 * included) is RWKVTTS_EINVAL, here and in every call that takes a desc. */
int rwkvtts_level_table(const rwkvtts_level_desc* desc, float* out);
/* T2 of a loudness in dB (host only): (float)pow(10, (loudness_db + 0.691) / 10). */
float rwkvtts_level_target(double loudness_db);
/* Streaming plan (host only, a pure function). With samples [0, n_known) of a signal known and
 * blocks [0, block_first) done:
 * *out_ready_end = B * max(0, floor(n_known / B) - A): block j is exact once blocks up to j + A are
 * complete. With final (n_known is the signal's length) it is n_known.
 * *in_first_needed = max(0, min(block_first * B, (block_first + A - 3) * B - (L - 1))): the cursor
 * block's own samples, and the FIR history of the first block whose energy has yet to enter --
 * samples before it are never read again. Either pointer may be NULL. Monotone in both. */
int rwkvtts_level_plan(const rwkvtts_level_desc* desc, int64_t n_known, int final, int64_t block_first,
                       int64_t* out_ready_end, int64_t* in_first_needed);
typedef struct rwkvtts_level rwkvtts_level;
/* table == NULL: the table of rwkvtts_level_table; otherwise the caller's [L + B] table (copied). */
int rwkvtts_level_create(int device, const rwkvtts_level_desc* desc, const float* table, rwkvtts_level** out);
int rwkvtts_level_destroy(rwkvtts_level* v);
/* n signals (ragged), each with its own target t2[i] (finite, > 0), in one launch triple (measure,
 * gain, apply). Host buffers; out[i] has capacity n_in[i]. n_in[i] == 0 writes nothing. Calls on one
 * handle serialise on its lock. */
int rwkvtts_level_batch(rwkvtts_level* v, const float* const* in, const int64_t* n_in, const float* t2, int n,
                        float* const* out);
typedef struct {
  uint32_t struct_size;
  const float* in;     /* points at sample in_first of the signal */
  int64_t in_first;
  int64_t n_in;
  int32_t final;       /* 1: in_first + n_in is the signal's length */
  float t2;
  int64_t block_first; /* outputs [block_first * B, block_first * B + out_count) */
  float s_prev;        /* the state after block block_first - 1: S, N and g of that block, as the */
  int64_t n_prev;      /* last call returned them; S = 0, N = 0 (g ignored) for block_first 0 */
  float g_prev;
  int64_t out_count;   /* whole blocks, or up to the signal's end with final */
  float* out;          /* capacity out_count */
  float s_last;        /* out: the state after the last block written (the state given if */
  int64_t n_last;      /* out_count is 0) */
  float g_last;
} rwkvtts_level_window;
/* n windows (of any signals, any targets) in one launch triple: outputs [block_first * B,
 * + out_count) of the whole-signal result, bitwise, whatever follows the known samples.
 * RWKVTTS_EINVAL before anything is launched (and nothing written, the state included) if a window
 * asks for more than rwkvtts_level_plan allows: block_first * B + out_count >
 * out_ready_end(in_first + n_in, final), in_first > in_first_needed(block_first), an out_count that
 * ends inside a block before the signal's end, or a state that no scan can have left. */
int rwkvtts_level_windows(rwkvtts_level* v, rwkvtts_level_window* w, int n);
/* HIP-event time of the last launch triple (all three kernels, no copies), in ms; 0 before the first. */
int rwkvtts_level_kernel_ms(rwkvtts_level* v, double* ms);

/* ---- pitch: a formant-preserving pitch shift (period estimation and pitch-synchronous overlap-add,
 * TD-PSOLA) on the GPU, the `pitch_shift` of the pipeline (no reference counterpart: the reference's
 * only pitch control is the `pitch` property token, which a cloned voice does not get) -------------
 * Runs on the 16 kHz PCM, first of the stages: before the stretch, the leveller and the resampler.
 * n_out = n. One causal definition with a bounded look-ahead, so a stream's pieces are bitwise the
 * one-shot result. The arithmetic contract (every output bit is defined by IEEE f32 rounded add,
 * subtract and multiply, never fused, and one correctly rounded f32 divide; every decision is an
 * integer):
 *   Ha, Wc    frame hop and comparison length; Lmin, Lmax the period range; P0 the hop where unvoiced
 *   f         double, per signal, 0.5 .. 2.0 (2^(semitones / 12)); above 1 is a higher voice
 *   table     rows P = Lmin .. Lmax back to back, row P of 2P floats at offset
 *             (P - Lmin) * (P + Lmin - 1): w_P[i] = (float)(0.5 - 0.5 * cos(2 * pi * (i + 0.5) / (2P))),
 *             in double, i in [0, 2P). Every w is > 0.
 *   zeros     every read of x outside [0, n) is +0
 *   period    frame j (j >= 0) starts at c = j * Ha. For every lag t in [Lmin - 1, Lmax + 1]:
 *             d(t) = sum_i (x[c+i] - x[c+i+t])^2 and m(t) = sum_i (x[c+i]^2 + x[c+i+t]^2), i in
 *             [0, Wc): each a sequential f32 sum in ascending i from +0 -- a d term is one rounded
 *             subtract and one rounded multiply, an m term two rounded multiplies and one rounded add,
 *             then one rounded add onto the sum. Lag t in [Lmin, Lmax] qualifies iff
 *             d(t) <= d(t-1) and d(t) <= d(t+1) and d(t) <= theta * m(t) (one rounded multiply) and
 *             m(t) > floor; every comparison with a NaN is false. P_j = the lowest qualifying lag
 *             (the minimum of an integer key, whatever the reduction tree), 0 (unvoiced) if none.
 *             P(t) = P_{floor(t / Ha)} for a sample position t >= 0. Frames wholly past the signal's
 *             end read zeros only, so they are unvoiced.
 *   marks     two serial integer walks from sample 0. Analysis: a_0 = 0, a_{k+1} = a_k + p_k with
 *             p_k = P(a_k), or P0 where that is 0. Synthesis: s_0 = 0, s_{q+1} = s_q +
 *             max(1, (int)floor((double)P(s_q) / f + 0.5)) (one double divide, one double add), or
 *             + P0 where P(s_q) is 0. Synthesis mark q takes the analysis mark k(q) nearest to it,
 *             |a_k - s_q| least, the lower k on a tie.
 *   output    grain q is x[a_k - p_k + i] * w_{p_k}[i], i in [0, 2 p_k), k = k(q), placed at
 *             s_q - p_k + i. Over the grains that cover output o, in ascending q, from num = den = +0:
 *             num = num + w * x (one rounded multiply, one rounded add), den = den + w.
 *             y[o] = num / den (correctly rounded), +0 where no grain covers o.
 * So silence comes back bit for bit (no frame is voiced, num = +0, den > 0). Where every frame is
 * unvoiced (a_k = s_k = k * P0), and at f = 1.0 (s_q = a_q), every grain that covers o reads x[o]
 * itself: y = (sum w x) / (sum w) over G same-signed products, so |y - x| <= 2 G u |x| (1 + 2^-20) +
 * G 2^-149 with u = 2^-24; G = 2 where all is unvoiced, under 4 ulp. A non-finite sample leaves the
 * outputs from its first frame on unspecified; nothing is read or written out of bounds. Every
 * default below is untuned and nobody has listened to the output: the repository has no real
 * checkpoint. */
typedef struct {
  uint32_t struct_size;
  int32_t hop;      /* Ha: 1 .. 4096; 0 = 160 (10 ms) */
  int32_t window;   /* Wc: 1 .. 4096; 0 = 640 */
  int32_t lag_min;  /* Lmin: 2 .. 1024; 0 = 32 (500 Hz) */
  int32_t lag_max;  /* Lmax: Lmin .. 1024; 0 = 320 (50 Hz) */
  int32_t unvoiced; /* P0: Lmin .. Lmax; 0 = 80 */
  float theta;      /* in (0, 1]; 0 = 0.2 */
  float floor;      /* finite, > 0; 0 = 1e-3 */
} rwkvtts_pitch_desc;
/* The library's own table builder (host only): out[(Lmax - Lmin + 1) * (Lmax + Lmin)]. Anything
 * outside the ranges above (NaN included), and a factor outside 0.5 .. 2.0 (NaN included), is
 * RWKVTTS_EINVAL, here and in every call that takes a desc or a factor. */
int rwkvtts_pitch_table(const rwkvtts_pitch_desc* desc, float* out);
/* Streaming plan (host only, a pure function). The state after outputs [0, e) is two marks:
 * s = the largest synthesis mark <= max(0, e - Lmax), a = the largest analysis mark <=
 * max(0, s - Lmax). Both walks go on from a mark by the periods alone, no grain of an earlier
 * synthesis mark reaches output e (a grain is at most 2 Lmax long), and no earlier analysis mark is
 * the nearest to a later synthesis mark (the next one, at most Lmax on, is nearer): two integers are
 * the whole state, the periods being recomputed from the kept samples. With samples [0, n_known)
 * known, outputs [0, out_first) done and (a_prev, s_prev) their state (a pair outside the ranges a
 * walk can leave -- s_prev in (max(0, out_first - Lmax) - 2 Lmax, max(0, out_first - Lmax)], a_prev in
 * (max(0, s_prev - Lmax) - Lmax, max(0, s_prev - Lmax)], neither negative -- is RWKVTTS_EINVAL):
 * *out_ready_end = max(0, n_known - (Wc + 3 Lmax)): output o is covered by grains of synthesis marks
 * below o + Lmax, whose analysis marks lie below o + 2 Lmax, whose frames start at or below that and
 * read Wc + Lmax samples on; the grains read below o + 3 Lmax. With final (n_known is the signal's
 * length) it is n_known.
 * *in_first_needed = max(0, min(a_prev - Lmax, floor(a_prev / Ha) * Ha)): the earliest grain and the
 * frame of a_prev -- samples before it are never read again; a stream keeps fewer than
 * Wc + 9 Lmax + Ha samples once the ready outputs are out. Either pointer may be NULL. Monotone in
 * n_known. */
int rwkvtts_pitch_plan(const rwkvtts_pitch_desc* desc, int64_t n_known, int final, int64_t out_first, int64_t a_prev,
                       int64_t s_prev, int64_t* out_ready_end, int64_t* in_first_needed);
typedef struct rwkvtts_pitch rwkvtts_pitch;
/* table == NULL: the table of rwkvtts_pitch_table; otherwise the caller's table (copied). */
int rwkvtts_pitch_create(int device, const rwkvtts_pitch_desc* desc, const float* table, rwkvtts_pitch** out);
int rwkvtts_pitch_destroy(rwkvtts_pitch* p);
/* n signals (ragged, each at most 2^30 samples), each with its own factor, in one launch triple
 * (period: a workgroup per frame; marks: a wave per signal; synthesis: a lane per output sample).
 * Host buffers; out[i] has capacity n_in[i]. n_in[i] == 0 writes nothing. Calls on one handle
 * serialise on its lock. */
int rwkvtts_pitch_batch(rwkvtts_pitch* p, const float* const* in, const int64_t* n_in, const double* factor, int n,
                        float* const* out);
typedef struct {
  uint32_t struct_size;
  const float* in;    /* points at sample in_first of the signal */
  int64_t in_first;
  int64_t n_in;
  int32_t final;      /* 1: in_first + n_in is the signal's length */
  double factor;
  int64_t out_first;  /* outputs [out_first, out_first + out_count) */
  int64_t a_prev;     /* the state after outputs [0, out_first): 0, 0 for out_first 0, else the */
  int64_t s_prev;     /* last call's a_last, s_last */
  int64_t out_count;
  float* out;         /* capacity out_count */
  int64_t a_last;     /* out: the state after the last output written (the state given if */
  int64_t s_last;     /* out_count is 0) */
} rwkvtts_pitch_window;
/* n windows (of any signals, any factors) in one launch triple: outputs [out_first, + out_count) of
 * the whole-signal result, bitwise, whatever follows the known samples. RWKVTTS_EINVAL before
 * anything is launched (and nothing written, the state included) if a window asks for more than
 * rwkvtts_pitch_plan allows: out_first + out_count > out_ready_end(in_first + n_in, final),
 * in_first > in_first_needed, or a state that no walk can have left. */
int rwkvtts_pitch_windows(rwkvtts_pitch* p, rwkvtts_pitch_window* w, int n);
/* HIP-event time of the last launch triple (all three kernels, no copies), in ms; 0 before the first. */
int rwkvtts_pitch_kernel_ms(rwkvtts_pitch* p, double* ms);
/* HIP-event time of the last call's marks kernel alone, the serial part, in ms; 0 before the first. */
int rwkvtts_pitch_walk_ms(rwkvtts_pitch* p, double* ms);

/* ---- wm: a provenance watermark on the GPU, the `watermark` of the pipeline -- a time-domain
 * spread-spectrum mark that carries a payload under a key, and its detector (no reference counterpart:
 * the reference marks nothing) -----------------------------------------------------------------
 * Embedding runs on the 16 kHz PCM, last of the stages at that rate: after the leveller and before
 * the resampler. n_out = n. One causal definition, so a stream's pieces are bitwise the one-shot
 * result. The embedder's arithmetic contract (every output bit is defined by IEEE f32 operations:
 * rounded add, subtract and multiply, never fused, and correctly rounded divide and square root;
 * DESIGN.md §30):
 *   B, L      block length and filter length; NB payload bits, TB samples per bit; the mark's period
 *             is NP = NB * TB samples
 *   s         the strength, an f32 per signal: (float)10^(strength_dB / 20), in double
 *             (rwkvtts_wm_strength)
 *   table     h[0, L) then r[0, B), f32, built in double and rounded once. With t = k - (L - 1) / 2,
 *             w[k] = 0.42 - 0.5 cos(2 pi k / (L - 1)) + 0.08 cos(4 pi k / (L - 1)) (Blackman),
 *             fh = 2 band_hi / 16000, fl = 2 band_lo / 16000 and sinc(x) = sin(pi x) / (pi x):
 *             g[k] = w[k] * (fh sinc(fh t) - fl sinc(fl t)), h[k] = g[k] / sqrt(sum g^2) (unit energy).
 *             r[i] = (float)((double)(i + 1) / (double)B).
 *   chips     splitmix64(x): z = x + 0x9E3779B97F4A7C15; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;
 *             z = (z ^ (z >> 27)) * 0x94D049BB133111EB; z ^ (z >> 31), all mod 2^64.
 *             c(key, m) = +1 if the top bit of splitmix64(splitmix64(key) + m) is set, else -1, for m
 *             in [0, NP) (the inner hash keeps neighbouring keys from giving shifted copies of one
 *             sequence). The chip at sample n is c(key, n mod NP) * (+1 if payload bit
 *             (n mod NP) / TB is set, else -1); n mod NP is taken in [0, NP) for n < 0 too.
 *   carrier   u[n] = sum_k h[k] * chip[n - k]: a sequential f32 sum in ascending k from +0, one rounded
 *             multiply (exact: the chip is +-1) then one rounded add per tap. Chips below sample 0 are
 *             the periodic sequence's, not zeros: a crop is indistinguishable from a start.
 *   gain      block j covers samples [jB, (j+1)B); x at or past the signal's end is +0 (the last block
 *             may be partial). E_j from 64 partials as the leveller's: p[l] = sum of x[i]*x[i] over the
 *             block's i = l (mod 64), ascending from +0, then p[l] += p[l+s] for l < s, s = 32 .. 1;
 *             E_j = p[0]. a_j = s * sqrt(E_j / (float)B). a_{-1} = a_0.
 *   apply     sample i of block j, n = jB + i: y = x + (a_{j-1} + (a_j - a_{j-1}) * r[i]) * u[n].
 * So +0 silence comes back bit for bit (a = +0, and +0 + (+-0) = +0); |y - x| <= max(a_{j-1}, a_j) *
 * sum|h| (the ramp lies between its ends and |u| <= sum|h|; exact in real arithmetic, where a random
 * +-1 sum leaves |u| far below sum|h| -- the f32 roundings of u, of the ramp and of the last add could
 * pass it only by 2^-20 of it plus half an ulp of y, at a sample whose chips all align with h); there is no
 * clamp (a mark on a full-scale signal can pass 1.0: the leveller's ceiling leaves 1 dB); a stream lags
 * one block, 20 ms at the default; and the only carried state is a_{j-1}. A non-finite sample leaves its
 * block and the next unspecified; nothing is read or written out of bounds.
 *
 * The detector takes 16 kHz PCM of any origin and a key. It is not bitwise: its contract is the
 * float64 restatement (tests/wm_ref.py) and the forward-error bound of its f32 sums.
 *   whiten    w[n] = x[n] / (sqrt(E_j / B) + 2^-17), blocks counted from the clip's first sample
 *   filter    v[n] = sum_k h[k] * w[n + k], n in [0, N); w past the end is 0
 *   fold      F[m] = sum v[n] over n = m (mod NP), ascending n, m in [0, NP)
 *   search    for every offset tau in [0, NP) and bit slot b (phases m in [b TB, (b+1) TB)):
 *             r_b = sum_m F[(m - tau) mod NP] * c(key, m), d_b = sum_m F[(m - tau) mod NP]^2, ascending
 *             m; z_b = r_b / sqrt(d_b), 0 where d_b is 0 (a slot the clip never covers);
 *             S(tau) = sum_b z_b^2
 *   result    offset = argmax S (the lowest tau on a tie) -- the phase of the mark at the clip's first
 *             sample; score = S(offset); payload = the slots with z_b > 0; seen = the slots with
 *             d_b > 0; min_z = min |z_b| over them; detected = score >= T.
 * Each r_b and d_b lies within TB * 2^-24 * sum|addend| of the float64 value. For an unmarked clip or a
 * wrong key the chips are independent +-1, independent of the audio, so Var(r_b) = sum F^2 = d_b
 * exactly, however coloured v is and whatever the clip's folds share (a host periodic in NP, another
 * key's mark): z_b is a unit-variance sum of TB bounded terms, S is chi-square with NB degrees of
 * freedom at every tau to the accuracy of the central limit, and T (rwkvtts_wm_threshold) is the
 * smallest T with NP * Q(T; NB) <= 1e-6, Q the chi-square upper tail: e^{-T/2} sum_{i < NB/2}
 * (T/2)^i / i! for even NB. (Dividing by the fold of v^2 instead is the same where the folds are
 * independent and lets whatever folds coherently pass T: DESIGN.md §30.2.) Every default below is
 * untuned and nobody has listened to the output: the repository has no real checkpoint. */
typedef struct {
  uint32_t struct_size;
  int32_t block;     /* B: a multiple of 64, 64 .. 4800; 0 = 320 (one vocoder frame, 20 ms) */
  int32_t taps;      /* L: odd, 3 .. 1023; 0 = 129 */
  int32_t bits;      /* NB: 1 .. 32; 0 = 16 */
  int32_t bit_len;   /* TB: a multiple of B, at most 6400; 0 = 1600 (100 ms) */
  float band_lo;     /* Hz, > 0; 0 = 1000 */
  float band_hi;     /* Hz, band_lo < band_hi < 8000; 0 = 3400 (below 0.95 * 4 kHz: survives 8 kHz output) */
  float strength_db; /* -60 .. -6; 0 = -26: the strength of an embed call that gives none */
} rwkvtts_wm_desc;
/* The library's own table builder (host only): out[L + B]. Anything outside the ranges above (NaN
 * included) is RWKVTTS_EINVAL, here and in every call that takes a desc. */
int rwkvtts_wm_table(const rwkvtts_wm_desc* desc, float* out);
/* s of a strength in dB (host only): (float)pow(10, strength_db / 20). A value outside -60 .. -6 (NaN
 * included) returns NaN, which every embed call refuses. */
float rwkvtts_wm_strength(double strength_db);
/* The detection threshold T of the desc's NB and NP (host only; both parities of NB). */
int rwkvtts_wm_threshold(const rwkvtts_wm_desc* desc, double* out);
/* Streaming plan (host only, a pure function). With samples [0, n_known) of a signal known and blocks
 * [0, block_first) done: *out_ready_end = B * floor(n_known / B) -- block j is exact once it is
 * complete -- or n_known with final. *in_first_needed = block_first * B. Either pointer may be NULL. */
int rwkvtts_wm_plan(const rwkvtts_wm_desc* desc, int64_t n_known, int final, int64_t block_first,
                    int64_t* out_ready_end, int64_t* in_first_needed);
typedef struct rwkvtts_wm rwkvtts_wm;
/* table == NULL: the table of rwkvtts_wm_table; otherwise the caller's [L + B] table (copied). */
int rwkvtts_wm_create(int device, const rwkvtts_wm_desc* desc, const float* table, rwkvtts_wm** out);
int rwkvtts_wm_destroy(rwkvtts_wm* w);
/* n signals (ragged), each with its own key, payload (bits at and above NB must be 0) and strength s
 * (finite, 0 < s <= 1; strength == NULL: the desc's for every signal), in one launch. Host buffers; out[i] has capacity n_in[i]. n_in[i] == 0 writes
 * nothing. Calls on one handle serialise on its lock. */
int rwkvtts_wm_embed_batch(rwkvtts_wm* w, const float* const* in, const int64_t* n_in, const uint64_t* key,
                           const uint32_t* payload, const float* strength, int n, float* const* out);
typedef struct {
  uint32_t struct_size;
  const float* in;     /* points at sample in_first of the signal */
  int64_t in_first;
  int64_t n_in;
  int32_t final;       /* 1: in_first + n_in is the signal's length */
  float strength;
  uint64_t key;
  uint32_t payload;
  float a_prev;        /* a of block block_first - 1, as the last call returned it (ignored for block_first 0) */
  int64_t block_first; /* outputs [block_first * B, block_first * B + out_count) */
  int64_t out_count;   /* whole blocks, or up to the signal's end with final */
  float* out;          /* capacity out_count */
  float a_last;        /* out: a of the last block written (a_prev if out_count is 0) */
} rwkvtts_wm_window;
/* n windows (of any signals, keys, payloads, strengths) in one launch: outputs [block_first * B,
 * + out_count) of the whole-signal result, bitwise, whatever follows the known samples.
 * RWKVTTS_EINVAL before anything is launched (and nothing written, a_last included) if a window asks
 * for more than rwkvtts_wm_plan allows: block_first * B + out_count > out_ready_end(in_first + n_in,
 * final), in_first > block_first * B, an out_count that ends inside a block before the signal's end,
 * or an a_prev that is negative or not finite. */
int rwkvtts_wm_embed_windows(rwkvtts_wm* w, rwkvtts_wm_window* win, int n);
typedef struct {
  uint32_t struct_size;
  int32_t detected;  /* score >= T */
  float score;       /* S(offset) */
  int32_t offset;    /* tau*: the mark's phase at the clip's first sample */
  uint32_t payload;  /* bit b set: z_b(offset) > 0 */
  uint32_t seen;     /* bit b set: d_b(offset) > 0 */
  float min_z;       /* min |z_b(offset)| over the seen slots; 0 if none */
  float* dbg_r;      /* in: NULL, or capacity NB * NP: r_b(tau) at [b * NP + tau] (tests) */
  float* dbg_d;      /* in: NULL, or capacity NB * NP: d_b(tau) likewise */
} rwkvtts_wm_result;
/* n clips (ragged, 16 kHz, each at most 2^30 samples), a key each, in one launch sequence (whiten,
 * filter and fold, search, reduce). results: n structs whose stride is results[0].struct_size; dbg_r /
 * dbg_d are read from each. An empty clip gives detected 0, score 0, seen 0. */
int rwkvtts_wm_detect_batch(rwkvtts_wm* w, const float* const* in, const int64_t* n_in, const uint64_t* key, int n,
                            rwkvtts_wm_result* results);
/* HIP-event time of the last call's kernels (embed: one launch; detect: all four; no copies), in ms;
 * 0 before the first. */
int rwkvtts_wm_kernel_ms(rwkvtts_wm* w, double* ms);

/* ---- flac: lossless compressed output on the GPU, the `format: "flac"` of the TTS routes -- f32 PCM
 * in, the frames of a FLAC stream out (no reference counterpart: the reference sends WAV only) ------
 * Standard FLAC (RFC 9639) in the streamable subset: mono, 16 bits, a fixed block size B of 256, 512,
 * 1024, 2048 or 4096 (the header codes for 256 * 2^n); a signal's last block may hold 1 .. B - 1
 * samples, its size then an explicit 8-bit (up to 256 samples) or 16-bit value; the seven output
 * rates have direct header codes. A frame depends on its own samples, its frame number, the rate and
 * B, nothing else, so a stream's pieces are byte for byte the one-shot frames. Every output bit is
 * defined (the numpy restatement is tests/flac_ref.py):
 *   quantise  q = trunc(clamp(x * scale, -1, 1) * 32767): f32, each operation rounded on its own --
 *             samples_to_pcm16 of the server after convert_samples_to_wav's scale. A non-finite
 *             sample gives an unspecified q in range.
 *   subframe  candidates in this order: CONSTANT when all samples are equal (then nothing else is
 *             tried); FIXED orders 0 .. 4; LPC orders 1 .. 12 (unless the window turns LPC off);
 *             VERBATIM. An order that is not below the block's length n is not tried. The candidate
 *             of the fewest bits wins, the earlier on a tie; VERBATIM wins unless another is smaller
 *             than its 8 + 16 n bits. Wasted bits are always 0.
 *   window    Q15 Welch, integer: w[i] = 32768 - floor(32768 d^2 / D^2), d = 2 i - n + 1, D = n + 1
 *             (the table holds it for n = B; a short block uses the formula at its own n).
 *   autocorr  v[i] = (q[i] * w[i]) >> 10 (arithmetic); R[l] = sum_{i >= l} v[i] v[i - l], l = 0 ..
 *             min(12, n - 1), in int64: |R| <= 2^52, so the sum is exact in any order and so is its f64.
 *   levinson  f64, every operation rounded on its own: E = R[0]; for i = 0 .. : stop unless E > 0;
 *             acc = R[i + 1]; acc = acc - a[j] * R[i - j] for j = 0 .. i - 1 in turn; k = acc / E;
 *             a'[j] = a[j] - k * a[i - 1 - j] for j < i, a'[i] = k; E = E * (1 - k * k). a' is the
 *             predictor of order i + 1: a[j] multiplies q[t - 1 - j].
 *   quantise  12-bit coefficients: with 2^(e-1) <= max|a| < 2^e, shift = min(11 - e, 15); the order is
 *             dropped if shift < 0 or max|a| is 0 or not finite; c[j] = clamp(rint(a[j] * 2^shift),
 *             -2048, 2047), rint to even.
 *   predict   r[t] = q[t] - ((sum_j c[j] * q[t - 1 - j]) >> shift), int64 sum, arithmetic shift (the
 *             sum stays below 2^31 and r fits int32 for 16-bit samples, so no candidate is ever
 *             dropped for its residual); FIXED: the order-th difference.
 *   rice      partitioned Rice, 4-bit parameters k in 0 .. 14, no escape code. Partition order o in 0 ..
 *             the largest o <= 8 with 2^o | n and (n >> o) > order. For every o the exact bit count with
 *             the best k of each partition (the lowest k on a tie: sum (zz >> k) + (k + 1) * count,
 *             zz = (r << 1) ^ (r >> 31)), 4 bits per partition; the lowest o on a tie.
 *   frame     sync 0xFFF8, block-size and rate codes, 0x08 (mono, 16 bits), the frame number in the
 *             UTF-8-like coding (up to 6 bytes), the explicit block size if any, CRC-8 (0x07) of the
 *             header; the subframe; zero bits to a byte; CRC-16 (0x8005, initial 0) of all before it.
 * The largest frame is 2 n + 16 bytes. */
#define RWKVTTS_FLAC_LAST 1u   /* the window ends its signal: a short last block is allowed */
#define RWKVTTS_FLAC_NO_LPC 2u /* CONSTANT, FIXED and VERBATIM only */
/* The window of block size B (host only): out[B], int32. */
int rwkvtts_flac_table(int32_t block_size, int32_t* out);
/* The largest byte count n samples can give at block size B: 2 n + 16 ceil(n / B); -1 for a bad B or n
 * outside 0 .. 2^40 (host only). */
int64_t rwkvtts_flac_bound(int64_t n, int32_t block_size);
/* "fLaC" and one STREAMINFO block (the last metadata block), 42 bytes, into out (host only): both block
 * sizes B, the frame sizes, the rate, mono, 16 bits, the sample count and the MD5 of the int16
 * little-endian samples (md5 NULL: zeros). Zeros in min_frame / max_frame / total_samples / md5 mean
 * "unknown", which the format allows: the header of a stream whose length is not known yet. */
int rwkvtts_flac_streaminfo(int32_t sample_rate, int32_t block_size, int32_t min_frame, int32_t max_frame,
                            int64_t total_samples, const uint8_t* md5, uint8_t* out);
typedef struct rwkvtts_flac rwkvtts_flac;
/* table == NULL: the windows of rwkvtts_flac_table for 256, 512, 1024, 2048 and 4096 back to back (7936
 * int32); otherwise the caller's (copied). */
int rwkvtts_flac_create(int device, const int32_t* table, rwkvtts_flac** out);
int rwkvtts_flac_destroy(rwkvtts_flac* f);
typedef struct {
  uint32_t struct_size;
  const float* in;     /* n_in samples, host */
  int64_t n_in;        /* a multiple of block_size unless flags has RWKVTTS_FLAC_LAST */
  float scale;         /* finite, >= 0 */
  int32_t sample_rate; /* 8000, 16000, 22050, 24000, 32000, 44100 or 48000 */
  int32_t block_size;  /* 256, 512, 1024, 2048 or 4096 */
  uint32_t flags;      /* RWKVTTS_FLAC_* */
  int64_t first_frame; /* the frame number of the window's first block */
  uint8_t* out;        /* the frames back to back, host */
  int64_t out_cap;     /* >= rwkvtts_flac_bound(n_in, block_size) */
  int64_t out_len;     /* out: bytes written */
  int32_t min_frame;   /* out: the smallest and the largest frame of the window, bytes (0 without frames) */
  int32_t max_frame;
} rwkvtts_flac_window;
/* n windows (of any signals, rates, block sizes and scales) in one launch pair: the frames
 * [first_frame, first_frame + ceil(n_in / block_size)) of each signal. RWKVTTS_EINVAL before anything is
 * launched (and nothing written) if a window has an unknown rate or block size, n_in that is not a
 * multiple of block_size without RWKVTTS_FLAC_LAST, out_cap below the bound, or first_frame + blocks
 * above 2^31. Calls on one handle serialise on its lock. */
int rwkvtts_flac_encode(rwkvtts_flac* f, rwkvtts_flac_window* win, int n);
/* HIP-event time of the last call's two kernels (no copies), in ms; 0 before the first. */
int rwkvtts_flac_kernel_ms(rwkvtts_flac* f, double* ms);

/* ---- pause: silences capped on the GPU, the `max_pause` of the pipeline (no reference counterpart:
 * the reference sends whatever silence the semantic model decided on) -- no silence inside the result
 * longer than M samples, none at either end longer than half of it ---------------------------------
 * Rate-agnostic; the pipeline applies it to the vocoder's 16 kHz PCM, first of the stages. The first
 * stage whose output length depends on the data: n_out <= n. The arithmetic contract (comparisons and
 * integers; one rounded f32 multiply per faded sample, every other sample a copy):
 *   desc      block B (samples, a multiple of 4, 4 .. 4096; 0 = 160), hang H (blocks, 1 .. 32; 0 = 5),
 *             fade F (samples, 1 .. 4096; 0 = 80), threshold (f32, finite, >= 0; 0 = 0.01, the join's)
 *   signal    x[0, n), n <= 2^30, and M, the cap in samples, 2F <= M <= 2^30; hd = M - M / 2 (integer
 *             division), tl = M / 2
 *   blocks    block k covers [kB, min((k + 1)B, n)), k in [0, nb), nb = ceil(n / B). loud_k iff
 *             fabsf(x) > threshold (an f32 compare, false for NaN) for a sample of the block. active_k
 *             iff loud_j for an existing j with |j - k| <= H. No sums: nothing depends on an order.
 *   runs      a quiet run is a maximal run of non-active blocks, samples [s, e), R = e - s (its last
 *             block may be partial). Activity before it: its head is its first hd samples; activity
 *             after it: its tail is its last tl samples.
 *   rule      interior run (activity on both sides): cut iff R > M, head and tail kept (M samples);
 *             leading run (nothing before it): cut iff R > tl, the tail kept; trailing run (nothing
 *             after it): cut iff R > hd, the head kept; a run that is not cut is copied whole. No
 *             active block at all: n_out = 0 (one cut if n > 0).
 *   ramp      r[k] = (float)((k + 0.5) / F), in double, k in [0, F): the join's
 *   fades     on a cut only: head sample i in [hd - F, hd) becomes x * r[hd - 1 - i], tail sample j in
 *             [0, F) becomes x * r[j]: one rounded f32 multiply each, never fused. Everything else --
 *             active blocks, uncut runs, unfaded kept samples -- is copied bit for bit.
 * So the output is a subsequence of the input but for at most 2F faded samples per cut, and every faded
 * sample lies in a block that is not loud.
 * Streams: the rule is decidable with bounded memory. The state after blocks [0, c) is three integers:
 * c, seen (an active block lies before c) and q (the samples of the quiet run that ends at cB; 0 if
 * block c - 1 is active). active_k is decided once blocks up to k + H are complete (or the signal has
 * ended). Of an open run after activity, the first hd - F samples go out at once, the next F once the
 * run has ended or passed M (then it is cut whatever follows), its tail when it ends; a leading run is
 * withheld until activity is decided. Samples still needed: from
 *   p = cB if q == 0; cB - tl if the cut is certain (seen and q > M, or not seen and q > tl);
 *       else cB - q + (seen ? min(q, hd - F) : 0)
 * and the H blocks before c (their loudness reaches blocks from c on): in_first_needed =
 * max(0, min(p, (c - H)B)), so a stream keeps fewer than M + (2H + 2)B samples however long a silence. */
typedef struct {
  uint32_t struct_size;
  int32_t block;
  int32_t hang;
  int32_t fade;
  float threshold;
} rwkvtts_pause_desc;
/* The ramp table (host only): out[F]. Anything outside the ranges above (a NaN or infinite threshold
 * included) is RWKVTTS_EINVAL, here and in every call that takes a desc. */
int rwkvtts_pause_ramp(const rwkvtts_pause_desc* desc, float* out);
typedef struct rwkvtts_pause rwkvtts_pause;
/* table == NULL: the ramp of rwkvtts_pause_ramp; otherwise the caller's [F] table (copied). */
int rwkvtts_pause_create(int device, const rwkvtts_pause_desc* desc, const float* table, rwkvtts_pause** out);
int rwkvtts_pause_destroy(rwkvtts_pause* p);
/* n signals (ragged, an M per signal) in one launch triple -- flags (a wave per 64 blocks: vector loads,
 * a compare per sample, a ballot; one bit per block), plan (a workgroup per signal: dilation by H, the
 * runs, the rule, the prefix of what is removed; a table of cuts), gather (a workgroup per output tile:
 * copy, or multiply by the ramp). Host buffers; out[i] has capacity n_in[i]; n_out[i] and n_cuts[i]
 * (NULL: not wanted) are read back first, with a synchronisation of their own, then n_out[i] samples
 * of each output. RWKVTTS_EINVAL before anything is launched, nothing written, for an M below 2F or
 * above 2^30, a negative or too long signal or a null buffer. Calls on one handle serialise on its lock. */
int rwkvtts_pause_batch(rwkvtts_pause* p, const float* const* in, const int64_t* n_in,
                        const int64_t* max_pause_samples, int n, float* const* out, int64_t* n_out,
                        int64_t* n_cuts);
typedef struct {
  uint32_t struct_size;
  int32_t final;               /* the known samples end the signal */
  const float* in;             /* signal samples [in_first, in_first + n_in), host */
  int64_t in_first;            /* <= in_first_needed of the state below */
  int64_t n_in;
  int64_t max_pause_samples;   /* M, the same for every window of a signal */
  int64_t block_next;          /* c: blocks [0, c) are decided (0 at the start) */
  int64_t quiet;               /* q (0 at the start) */
  int32_t seen;                /* 0 or 1 (0 at the start) */
  int32_t seen_last;           /* out: the state after this window */
  int64_t block_last;          /* out */
  int64_t quiet_last;          /* out (0 after a final window: no run is open) */
  float* out;                  /* host, capacity out_cap */
  int64_t out_cap;             /* >= (the end of what this window decides) - p: n_in is always enough */
  int64_t out_count;           /* out: samples written */
  int64_t n_cuts;              /* out: cuts decided in this window (a cut counts where its run ends) */
  int64_t in_first_needed;     /* out: the first sample the next window must still carry */
} rwkvtts_pause_window;
/* n windows (of any signals) in one launch triple: each gives the outputs that its known samples decide
 * beyond its state, bitwise the whole-signal result whatever follows them. The caller cannot plan the
 * count, so the capacity is part of the struct. RWKVTTS_EINVAL before anything is launched, nothing
 * written, for an M outside its range, too little capacity, samples that start after in_first_needed
 * or end before block c, or a state no scan can have left (c < 0, seen not 0 or 1, q negative, no
 * multiple of B or above cB, seen with q above (c - 1)B, not seen with q below cB). */
int rwkvtts_pause_windows(rwkvtts_pause* p, rwkvtts_pause_window* w, int n);
/* HIP-event time of the last call's three kernels (no copies), in ms; 0 before the first. */
int rwkvtts_pause_kernel_ms(rwkvtts_pause* p, double* ms);

#ifdef __cplusplus
}
#endif
#endif /* RWKVTTS_H */
