"""ctypes binding of include/rwkvtts.h (the C-ABI drop-in boundary).

This is the Python twin of the Rust `extern "C"` block in INTEGRATION.md: same structs, same
entry points. The product library is loaded from this directory (built in-tree by
`make -C rwkv-tts-rs_amd/csrc`); there is no fallback -- a missing library is an error.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# RWKVTTS_LIB: an alternative build of the same library (A/B timing tools only)
LIB_PATH = os.environ.get("RWKVTTS_LIB") or os.path.join(_HERE, "librwkvtts.so")


def build_id() -> str:
    """Identity of the in-tree library's build: sha256 over the sources it is built from
    (csrc/*.hip, *.cpp, *.h, the Makefile and include/*.h, in name order), first 16 hex digits.
    Profile summaries under profiles/ carry it (tools/), so bench.py cites only summaries that were
    measured on the library it runs."""
    import glob
    import hashlib
    csrc = os.path.join(_HERE, "..", "csrc")
    inc = os.path.join(_HERE, "..", "..", "include")
    files = sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.cpp")) +
                   glob.glob(os.path.join(csrc, "*.h")) + [os.path.join(csrc, "Makefile")] +
                   glob.glob(os.path.join(inc, "*.h")), key=os.path.basename)
    h = hashlib.sha256()
    for f in files:
        h.update(os.path.basename(f).encode())
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]

EOS_TOKEN = 8192
TAG_0, TAG_1, TAG_2 = 8193, 8194, 8195
GLOBAL_TOKEN_OFFSET = 8196
SPECIAL_TOKEN_OFFSET = 77823
N_GLOBAL = 32
SEMANTIC_LIMIT = 2048
HOP = 320
SAMPLE_RATE = 16000

OK, EINVAL, EHIP, ENOMEM, EUNSUPPORTED, EBUSY, ECLOSED = 0, -1, -2, -3, -4, -5, -6
MAX_ENGINES = 16
DTYPE_BF16, DTYPE_F16 = 0, 1
OPT_LAST, OPT_FULL = 0, 1


class Dims(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in (
        "n_layer", "n_embd", "head_size", "n_ffn", "n_vocab", "d_decay", "d_aaa", "d_mv", "d_gate")]


class EngineDesc(ctypes.Structure):
    # wkv_variant: ignored by the engine, kept for layout compatibility (include/rwkvtts.h)
    _fields_ = [("device", ctypes.c_int32), ("max_slots", ctypes.c_int32),
                ("token_chunk_size", ctypes.c_int32), ("use_graphs", ctypes.c_int32),
                ("wkv_variant", ctypes.c_int32), ("quant_layers", ctypes.c_int32),
                ("quant_type", ctypes.c_int32), ("forms", ctypes.c_uint32)]


# rwkvtts_engine_desc.forms (include/rwkvtts.h RWKVTTS_FORM_*): each bit switches one fused decode form
# back to the launches it replaces (bitwise-equal outputs; verification and A/B timing only)
FORM_SEPARATE_ATT, FORM_SEPARATE_FFN, FORM_LN_ROWS, FORM_SLAB_HANDOFF = 1, 2, 4, 8
FORM_SEPARATE_LNOUT, FORM_SEPARATE_EMBED, FORM_EXACT_SAMPLER = 16, 32, 64
FORM_VALUE_TILE_32X64 = 128  # k_ffn_persist at 17..32 rows: the 32 x 64 value tile, not 16 x 128
# codec weight paths and forms (RWKVTTS_CODEC_WEIGHTS_* / RWKVTTS_CODEC_FORM_*)
CODEC_WEIGHTS_AUTO, CODEC_WEIGHTS_BF16, CODEC_WEIGHTS_HILO = 0, 1, 2
CODEC_FORM_SEPARATE_RESUNIT, CODEC_FORM_CHANNEL_LAST = 1, 2


QUANT_NONE, QUANT_INT8, QUANT_NF4, QUANT_SF4 = 0, 1, 2, 3


class Input(ctypes.Structure):
    _fields_ = [("slot", ctypes.c_int32), ("tokens", ctypes.POINTER(ctypes.c_uint32)),
                ("n_tokens", ctypes.c_int32), ("option", ctypes.c_int32)]


class Rng(ctypes.Structure):
    _fields_ = [("key", ctypes.c_uint32 * 8), ("draw_index", ctypes.c_uint64)]


class SampleArgs(ctypes.Structure):
    _fields_ = [("temperature", ctypes.c_float), ("top_p", ctypes.c_float),
                ("top_k", ctypes.c_int32), ("forbid_token", ctypes.c_int32)]


class PhaseSampling(ctypes.Structure):
    _fields_ = [("temperature", ctypes.c_float), ("top_p", ctypes.c_float), ("top_k", ctypes.c_int32)]


class Penalties(ctypes.Structure):
    _fields_ = [("repetition", ctypes.c_float), ("frequency", ctypes.c_float), ("presence", ctypes.c_float),
                ("window", ctypes.c_int32)]


SAMPLING_GLOBAL, SAMPLING_SEMANTIC = 1, 2
PENALTY_SET = 1
MIROSTAT_SET = 1


class MirostatParams(ctypes.Structure):
    _fields_ = [("tau", ctypes.c_float), ("rate", ctypes.c_float)]


class RequestExt(ctypes.Structure):
    """rwkvtts_request_ext: what a request asks for beyond rwkvtts_request, whose layout stays."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("mirostat_set", ctypes.c_int32), ("mirostat", MirostatParams)]


class Request(ctypes.Structure):
    _fields_ = [("text_tokens", ctypes.POINTER(ctypes.c_int32)), ("n_text", ctypes.c_int32),
                ("property_tokens", ctypes.POINTER(ctypes.c_int32)), ("n_property", ctypes.c_int32),
                ("ref_global", ctypes.POINTER(ctypes.c_int32)), ("n_ref_global", ctypes.c_int32),
                ("ref_semantic", ctypes.POINTER(ctypes.c_int32)), ("n_ref_semantic", ctypes.c_int32),
                ("has_seed", ctypes.c_int32), ("seed", ctypes.c_uint64),
                ("max_tokens", ctypes.c_int32), ("fixed_semantic", ctypes.c_int32),
                ("greedy", ctypes.c_int32), ("layered_set", ctypes.c_int32),
                ("use_independent_seeds", ctypes.c_int32), ("global_seed_offset", ctypes.c_uint64),
                ("semantic_seed_offset", ctypes.c_uint64),
                ("sampling_set", ctypes.c_int32), ("global_sampling", PhaseSampling),
                ("semantic_sampling", PhaseSampling), ("pinned_voice", ctypes.c_int32),
                ("penalty_set", ctypes.c_int32), ("penalties", Penalties)]


class Result(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int32), ("n_global", ctypes.c_int32),
                ("n_semantic", ctypes.c_int32), ("global_tokens", ctypes.c_int32 * N_GLOBAL),
                ("semantic_tokens", ctypes.POINTER(ctypes.c_int32))]


class Stats(ctypes.Structure):
    _fields_ = [("steps", ctypes.c_int64), ("prefill_steps", ctypes.c_int64),
                ("decode_ms", ctypes.c_double), ("prefill_ms", ctypes.c_double),
                ("sample_ms", ctypes.c_double), ("decode_rows", ctypes.c_int64),
                ("profile_kernel_count", ctypes.c_int32), ("persistent", ctypes.c_int32)]


class ManagerDesc(ctypes.Structure):
    _fields_ = [("n_engines", ctypes.c_int32), ("devices", ctypes.c_int32 * MAX_ENGINES),
                ("engine", EngineDesc), ("max_batch_size", ctypes.c_int32),
                ("collect_timeout_ms", ctypes.c_int32)]


class ManagerStats(ctypes.Structure):
    _fields_ = [("submitted", ctypes.c_int64), ("completed", ctypes.c_int64), ("batches", ctypes.c_int64),
                ("served", ctypes.c_int64 * MAX_ENGINES), ("max_active", ctypes.c_int64 * MAX_ENGINES),
                ("steps", ctypes.c_int64 * MAX_ENGINES), ("bcast_ranks", ctypes.c_int32),
                ("bcast_rccl", ctypes.c_int32), ("bcast_ms", ctypes.c_double),
                ("waiters", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("persistent", ctypes.c_int32 * MAX_ENGINES)]


class CodecDims(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in (
        "codebook_size", "codebook_dim", "latent_dim", "n_global", "fsq_levels", "fsq_dims",
        "spk_dim", "prenet_dim", "prenet_inter", "prenet_layers", "dec_channels", "n_up")] + [
        ("up_rates", ctypes.c_int32 * 4), ("up_kernels", ctypes.c_int32 * 4)]


# rwkvtts_token_fn(user, global_tokens, n_global, semantic, first, count, done, status)
TokenFn = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32), ctypes.c_int32,
                           ctypes.POINTER(ctypes.c_int32), ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                           ctypes.c_int32)


class TokenSink(ctypes.Structure):
    _fields_ = [("fn", TokenFn), ("user", ctypes.c_void_p)]


class CodecPlan(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("ctx0", ctypes.c_int32), ("ctx1", ctypes.c_int32),
                ("wave0", ctypes.c_int32), ("wave1", ctypes.c_int32)]


class CodecWindow(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("n_known", ctypes.c_int32), ("final", ctypes.c_int32),
                ("t0", ctypes.c_int32), ("t1", ctypes.c_int32), ("semantic", ctypes.c_void_p),
                ("global_", ctypes.c_void_p), ("pcm", ctypes.c_void_p)]


class CodecLaunch(ctypes.Structure):
    """rwkvtts_codec_launch: one k_conv launch of a decode (rwkvtts_codec_debug_launch_plan)."""
    _fields_ = [("struct_size", ctypes.c_uint32)] + [(n, ctypes.c_int32) for n in (
        "kind", "ci", "co", "k", "dil", "pad", "s", "tin_mul", "tn", "kt", "wlo", "nwv", "shm_bytes",
        "xmap", "gx", "gy")] + [("grid", ctypes.c_int32 * 3)] + [(n, ctypes.c_int32) for n in (
            "act", "has_y", "has_planes", "has_res", "has_rbias",
            "w", "bias", "gamma", "y_alpha", "mid_alpha", "w1", "bias1")]


RESAMPLE_ALIGN_RUBATO, RESAMPLE_ALIGN_ZERO = 0, 1


class ResampleDesc(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("sr_in", ctypes.c_int32), ("sr_out", ctypes.c_int32),
                ("sinc_len", ctypes.c_int32), ("oversampling", ctypes.c_int32), ("f_cutoff", ctypes.c_double),
                ("align", ctypes.c_int32)]


class ResampleWindow(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("in_", ctypes.c_void_p), ("in_first", ctypes.c_int64),
                ("n_in", ctypes.c_int64), ("final", ctypes.c_int32), ("out_first", ctypes.c_int64),
                ("out_count", ctypes.c_int64), ("out", ctypes.c_void_p)]


class TsmDesc(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("window", ctypes.c_int32), ("search", ctypes.c_int32)]


class TsmWindow(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("in_", ctypes.c_void_p), ("in_first", ctypes.c_int64),
                ("n_in", ctypes.c_int64), ("final", ctypes.c_int32), ("tempo", ctypes.c_double),
                ("block_first", ctypes.c_int64), ("s_prev", ctypes.c_int64), ("out_count", ctypes.c_int64),
                ("out", ctypes.c_void_p), ("s_last", ctypes.c_int64)]


class JoinDesc(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("threshold", ctypes.c_float), ("keep", ctypes.c_int32),
                ("fade", ctypes.c_int32), ("trim", ctypes.c_int32)]


class JoinJob(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("n_seg", ctypes.c_int32), ("seg", ctypes.c_void_p),
                ("n", ctypes.c_void_p), ("gap", ctypes.c_void_p), ("out", ctypes.c_void_p), ("a", ctypes.c_void_p),
                ("b", ctypes.c_void_p), ("n_out", ctypes.c_int64)]


class LevelDesc(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("block", ctypes.c_int32), ("taps", ctypes.c_int32),
                ("lookahead", ctypes.c_int32), ("gate", ctypes.c_float), ("ceiling", ctypes.c_float),
                ("g_min", ctypes.c_float), ("g_max", ctypes.c_float), ("horizon", ctypes.c_int32)]


class LevelWindow(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("in_", ctypes.c_void_p), ("in_first", ctypes.c_int64),
                ("n_in", ctypes.c_int64), ("final", ctypes.c_int32), ("t2", ctypes.c_float),
                ("block_first", ctypes.c_int64), ("s_prev", ctypes.c_float), ("n_prev", ctypes.c_int64),
                ("g_prev", ctypes.c_float), ("out_count", ctypes.c_int64), ("out", ctypes.c_void_p),
                ("s_last", ctypes.c_float), ("n_last", ctypes.c_int64), ("g_last", ctypes.c_float)]


class PitchDesc(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("hop", ctypes.c_int32), ("window", ctypes.c_int32),
                ("lag_min", ctypes.c_int32), ("lag_max", ctypes.c_int32), ("unvoiced", ctypes.c_int32),
                ("theta", ctypes.c_float), ("floor", ctypes.c_float)]


class PitchWindow(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("in_", ctypes.c_void_p), ("in_first", ctypes.c_int64),
                ("n_in", ctypes.c_int64), ("final", ctypes.c_int32), ("factor", ctypes.c_double),
                ("out_first", ctypes.c_int64), ("a_prev", ctypes.c_int64), ("s_prev", ctypes.c_int64),
                ("out_count", ctypes.c_int64), ("out", ctypes.c_void_p), ("a_last", ctypes.c_int64),
                ("s_last", ctypes.c_int64)]


class WmDesc(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("block", ctypes.c_int32), ("taps", ctypes.c_int32),
                ("bits", ctypes.c_int32), ("bit_len", ctypes.c_int32), ("band_lo", ctypes.c_float),
                ("band_hi", ctypes.c_float), ("strength_db", ctypes.c_float)]


class WmWindow(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("in_", ctypes.c_void_p), ("in_first", ctypes.c_int64),
                ("n_in", ctypes.c_int64), ("final", ctypes.c_int32), ("strength", ctypes.c_float),
                ("key", ctypes.c_uint64), ("payload", ctypes.c_uint32), ("a_prev", ctypes.c_float),
                ("block_first", ctypes.c_int64), ("out_count", ctypes.c_int64), ("out", ctypes.c_void_p),
                ("a_last", ctypes.c_float)]


class WmResult(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("detected", ctypes.c_int32), ("score", ctypes.c_float),
                ("offset", ctypes.c_int32), ("payload", ctypes.c_uint32), ("seen", ctypes.c_uint32),
                ("min_z", ctypes.c_float), ("dbg_r", ctypes.c_void_p), ("dbg_d", ctypes.c_void_p)]


FLAC_LAST, FLAC_NO_LPC = 1, 2


class PauseDesc(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("block", ctypes.c_int32), ("hang", ctypes.c_int32),
                ("fade", ctypes.c_int32), ("threshold", ctypes.c_float)]


class PauseWindow(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("final", ctypes.c_int32), ("in_", ctypes.c_void_p),
                ("in_first", ctypes.c_int64), ("n_in", ctypes.c_int64), ("max_pause_samples", ctypes.c_int64),
                ("block_next", ctypes.c_int64), ("quiet", ctypes.c_int64), ("seen", ctypes.c_int32),
                ("seen_last", ctypes.c_int32), ("block_last", ctypes.c_int64), ("quiet_last", ctypes.c_int64),
                ("out", ctypes.c_void_p), ("out_cap", ctypes.c_int64), ("out_count", ctypes.c_int64),
                ("n_cuts", ctypes.c_int64), ("in_first_needed", ctypes.c_int64)]


class FlacWindow(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("in_", ctypes.c_void_p), ("n_in", ctypes.c_int64),
                ("scale", ctypes.c_float), ("sample_rate", ctypes.c_int32), ("block_size", ctypes.c_int32),
                ("flags", ctypes.c_uint32), ("first_frame", ctypes.c_int64), ("out", ctypes.c_void_p),
                ("out_cap", ctypes.c_int64), ("out_len", ctypes.c_int64), ("min_frame", ctypes.c_int32),
                ("max_frame", ctypes.c_int32)]


# Every symbol include/rwkvtts.h declares (checked by tests/test_abi.py against the header).
EXPORTS = {
    "rwkvtts_synth_weights": (ctypes.c_int, [ctypes.POINTER(Dims), ctypes.c_int, ctypes.c_uint64, ctypes.c_void_p]),
    "rwkvtts_engine_create": (ctypes.c_int, [ctypes.POINTER(EngineDesc), ctypes.c_void_p, ctypes.c_size_t,
                                             ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]),
    "rwkvtts_engine_destroy": (ctypes.c_int, [ctypes.c_void_p]),
    "rwkvtts_last_error": (ctypes.c_char_p, []),
    "rwkvtts_engine_dims": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(Dims)]),
    "rwkvtts_state_floats": (ctypes.c_int64, [ctypes.c_void_p]),
    "rwkvtts_slot_reset": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "rwkvtts_slot_read": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]),
    "rwkvtts_slot_write": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]),
    "rwkvtts_infer": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(Input), ctypes.c_int, ctypes.c_int,
                                     ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "rwkvtts_rng_seed_from_u64": (None, [ctypes.c_uint64, ctypes.POINTER(Rng)]),
    "rwkvtts_sample": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                      ctypes.POINTER(SampleArgs), ctypes.c_void_p, ctypes.c_void_p]),
    "rwkvtts_generate_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(Request), ctypes.c_int,
                                              ctypes.POINTER(Result)]),
    # streaming: token progress
    "rwkvtts_generate_batch_stream": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(Request), ctypes.c_int,
                                                     ctypes.POINTER(Result), ctypes.POINTER(TokenSink)]),
    "rwkvtts_generate_batch_ex": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(Request),
                                                 ctypes.POINTER(ctypes.POINTER(RequestExt)), ctypes.c_int,
                                                 ctypes.POINTER(Result), ctypes.POINTER(TokenSink)]),
    "rwkvtts_manager_submit_ex": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(Request), ctypes.POINTER(RequestExt),
                                                 ctypes.c_int, ctypes.POINTER(ctypes.c_uint64)]),
    "rwkvtts_manager_submit_stream": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(Request),
                                                     ctypes.POINTER(ctypes.c_uint64)]),
    "rwkvtts_manager_wait_tokens": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int32, ctypes.c_int,
                                                   ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32), ctypes.c_void_p,
                                                   ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32),
                                                   ctypes.POINTER(ctypes.c_int32)]),
    "rwkvtts_manager_create": (ctypes.c_int, [ctypes.POINTER(ManagerDesc), ctypes.c_void_p, ctypes.c_size_t,
                                              ctypes.POINTER(ctypes.c_void_p)]),
    "rwkvtts_manager_destroy": (ctypes.c_int, [ctypes.c_void_p]),
    "rwkvtts_manager_submit": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(Request),
                                              ctypes.POINTER(ctypes.c_uint64)]),
    "rwkvtts_manager_wait": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.POINTER(Result)]),
    "rwkvtts_manager_generate_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(Request), ctypes.c_int,
                                                      ctypes.POINTER(Result)]),
    "rwkvtts_manager_get_stats": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ManagerStats)]),
    "rwkvtts_get_stats": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(Stats)]),
    "rwkvtts_set_profiling": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    # test hook (tests/test_gpu_advance.py): the decode-step sampler on caller-given rows
    "rwkvtts_debug_advance": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                             ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_void_p]),
    "rwkvtts_debug_advance_ex": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                                ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                                ctypes.c_void_p]),
    "rwkvtts_debug_advance_pen": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                                 ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                                 ctypes.c_void_p]),
    "rwkvtts_debug_advance_miro": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                                  ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                                  ctypes.c_void_p, ctypes.c_void_p]),
    # host self-test hook of the Mirostat contract (tests/miro_ref.py): lg for arrays
    "rwkvtts_debug_lg2": (None, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]),
    # test hook (tests/test_gpu_value_tile.py): the logits the last forward step left on the device
    "rwkvtts_debug_last_logits": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]),
    "rwkvtts_profile_entry": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int,
                                             ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double)]),
    "rwkvtts_codec_blob_bytes": (ctypes.c_int64, [ctypes.POINTER(CodecDims)]),
    "rwkvtts_codec_synth_weights": (ctypes.c_int, [ctypes.POINTER(CodecDims), ctypes.c_uint64, ctypes.c_void_p]),
    "rwkvtts_codec_create": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(CodecDims), ctypes.c_void_p,
                                            ctypes.POINTER(ctypes.c_void_p)]),
    "rwkvtts_codec_create_ex": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(CodecDims), ctypes.c_void_p,
                                               ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]),
    "rwkvtts_codec_set_forms": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32]),
    "rwkvtts_codec_destroy": (ctypes.c_int, [ctypes.c_void_p]),
    "rwkvtts_codec_decode": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                            ctypes.c_void_p]),
    "rwkvtts_codec_decode_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                  ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]),
    # streaming: exact windowed decode
    "rwkvtts_codec_halo": (ctypes.c_int, [ctypes.POINTER(CodecDims), ctypes.POINTER(ctypes.c_int32),
                                          ctypes.POINTER(ctypes.c_int32)]),
    "rwkvtts_codec_window_plan": (ctypes.c_int, [ctypes.POINTER(CodecDims), ctypes.c_int32, ctypes.c_int32,
                                                 ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(CodecPlan)]),
    "rwkvtts_codec_decode_windows": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(CodecWindow), ctypes.c_int]),
    # test hooks (tests/test_codec_plan_cpu.py, tests/test_gpu_codec_dims.py): the launch plan (host
    # only) and one launch's captured inputs and outputs
    "rwkvtts_codec_debug_launch_plan": (ctypes.c_int, [ctypes.POINTER(CodecDims), ctypes.c_int, ctypes.c_uint32,
                                                       ctypes.c_int, ctypes.c_int, ctypes.POINTER(CodecLaunch),
                                                       ctypes.c_int]),
    "rwkvtts_codec_debug_capture": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "rwkvtts_codec_debug_captured_launch": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(CodecLaunch),
                                                           ctypes.POINTER(ctypes.c_int32),
                                                           ctypes.POINTER(ctypes.c_int32),
                                                           ctypes.POINTER(ctypes.c_int32)]),
    "rwkvtts_codec_debug_captured": (ctypes.c_int64, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                                      ctypes.c_int64]),
    "rwkvtts_codec_set_profiling": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "rwkvtts_codec_profile_count": (ctypes.c_int, [ctypes.c_void_p]),
    "rwkvtts_codec_profile_entry": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int,
                                                   ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double)]),
    "rwkvtts_tokenizer_create": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p)]),
    "rwkvtts_tokenizer_destroy": (ctypes.c_int, [ctypes.c_void_p]),
    "rwkvtts_tokenizer_encode": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p,
                                                ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]),
    "rwkvtts_tokenizer_decode": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                                ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]),
    "rwkvtts_tokenizer_vocab_size": (ctypes.c_int64, [ctypes.c_void_p]),
    "rwkvtts_mel": (ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                   ctypes.POINTER(ctypes.c_int)]),
    # resampler: table, plan (host only), one-shot / batched / exact stream windows
    "rwkvtts_resample_sincs": (ctypes.c_int, [ctypes.POINTER(ResampleDesc), ctypes.c_void_p]),
    "rwkvtts_resample_out_len": (ctypes.c_int64, [ctypes.POINTER(ResampleDesc), ctypes.c_int64]),
    "rwkvtts_resample_plan": (ctypes.c_int, [ctypes.POINTER(ResampleDesc), ctypes.c_int64, ctypes.c_int,
                                             ctypes.c_int64, ctypes.POINTER(ctypes.c_int64),
                                             ctypes.POINTER(ctypes.c_int64)]),
    "rwkvtts_resampler_create": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(ResampleDesc), ctypes.c_void_p,
                                                ctypes.POINTER(ctypes.c_void_p)]),
    "rwkvtts_resampler_destroy": (ctypes.c_int, [ctypes.c_void_p]),
    "rwkvtts_resample_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                              ctypes.c_void_p]),
    "rwkvtts_resample_windows": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ResampleWindow), ctypes.c_int]),
    "rwkvtts_resampler_kernel_ms": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)]),
    # time stretch (WSOLA): window, plan (host only), batched / exact stream windows
    "rwkvtts_tsm_window": (ctypes.c_int, [ctypes.POINTER(TsmDesc), ctypes.c_void_p]),
    "rwkvtts_tsm_out_len": (ctypes.c_int64, [ctypes.POINTER(TsmDesc), ctypes.c_double, ctypes.c_int64]),
    "rwkvtts_tsm_plan": (ctypes.c_int, [ctypes.POINTER(TsmDesc), ctypes.c_double, ctypes.c_int64, ctypes.c_int,
                                        ctypes.c_int64, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64),
                                        ctypes.POINTER(ctypes.c_int64)]),
    "rwkvtts_tsm_create": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(TsmDesc), ctypes.c_void_p,
                                          ctypes.POINTER(ctypes.c_void_p)]),
    "rwkvtts_tsm_destroy": (ctypes.c_int, [ctypes.c_void_p]),
    "rwkvtts_tsm_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_int, ctypes.c_void_p]),
    "rwkvtts_tsm_windows": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(TsmWindow), ctypes.c_int]),
    "rwkvtts_tsm_kernel_ms": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)]),
    # join: ramp and capacity (host only), ragged jobs of segments in one pass
    "rwkvtts_join_ramp": (ctypes.c_int, [ctypes.POINTER(JoinDesc), ctypes.c_void_p]),
    "rwkvtts_join_capacity": (ctypes.c_int64, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32]),
    "rwkvtts_join_create": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(JoinDesc), ctypes.c_void_p,
                                           ctypes.POINTER(ctypes.c_void_p)]),
    "rwkvtts_join_destroy": (ctypes.c_int, [ctypes.c_void_p]),
    "rwkvtts_join_jobs": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(JoinJob), ctypes.c_int]),
    "rwkvtts_join_kernel_ms": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)]),
    # level: table, target and plan (host only), batched / exact stream windows
    "rwkvtts_level_table": (ctypes.c_int, [ctypes.POINTER(LevelDesc), ctypes.c_void_p]),
    "rwkvtts_level_target": (ctypes.c_float, [ctypes.c_double]),
    "rwkvtts_level_plan": (ctypes.c_int, [ctypes.POINTER(LevelDesc), ctypes.c_int64, ctypes.c_int, ctypes.c_int64,
                                          ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]),
    "rwkvtts_level_create": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(LevelDesc), ctypes.c_void_p,
                                            ctypes.POINTER(ctypes.c_void_p)]),
    "rwkvtts_level_destroy": (ctypes.c_int, [ctypes.c_void_p]),
    "rwkvtts_level_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_int, ctypes.c_void_p]),
    "rwkvtts_level_windows": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(LevelWindow), ctypes.c_int]),
    "rwkvtts_level_kernel_ms": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)]),
    # pitch: table and plan (host only), batched / exact stream windows
    "rwkvtts_pitch_table": (ctypes.c_int, [ctypes.POINTER(PitchDesc), ctypes.c_void_p]),
    "rwkvtts_pitch_plan": (ctypes.c_int, [ctypes.POINTER(PitchDesc), ctypes.c_int64, ctypes.c_int, ctypes.c_int64,
                                          ctypes.c_int64, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64),
                                          ctypes.POINTER(ctypes.c_int64)]),
    "rwkvtts_pitch_create": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(PitchDesc), ctypes.c_void_p,
                                            ctypes.POINTER(ctypes.c_void_p)]),
    "rwkvtts_pitch_destroy": (ctypes.c_int, [ctypes.c_void_p]),
    "rwkvtts_pitch_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_int, ctypes.c_void_p]),
    "rwkvtts_pitch_windows": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(PitchWindow), ctypes.c_int]),
    "rwkvtts_pitch_kernel_ms": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)]),
    "rwkvtts_pitch_walk_ms": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)]),
    # watermark: table, strength, threshold and plan (host only), batched / exact stream embedding, the detector
    "rwkvtts_wm_table": (ctypes.c_int, [ctypes.POINTER(WmDesc), ctypes.c_void_p]),
    "rwkvtts_wm_strength": (ctypes.c_float, [ctypes.c_double]),
    "rwkvtts_wm_threshold": (ctypes.c_int, [ctypes.POINTER(WmDesc), ctypes.POINTER(ctypes.c_double)]),
    "rwkvtts_wm_plan": (ctypes.c_int, [ctypes.POINTER(WmDesc), ctypes.c_int64, ctypes.c_int, ctypes.c_int64,
                                       ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]),
    "rwkvtts_wm_create": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(WmDesc), ctypes.c_void_p,
                                         ctypes.POINTER(ctypes.c_void_p)]),
    "rwkvtts_wm_destroy": (ctypes.c_int, [ctypes.c_void_p]),
    "rwkvtts_wm_embed_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                              ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]),
    "rwkvtts_wm_embed_windows": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(WmWindow), ctypes.c_int]),
    "rwkvtts_wm_detect_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                               ctypes.c_int, ctypes.POINTER(WmResult)]),
    "rwkvtts_wm_kernel_ms": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)]),
    # flac: window table, bound and stream header (host only), ragged windows in one launch pair
    "rwkvtts_flac_table": (ctypes.c_int, [ctypes.c_int32, ctypes.c_void_p]),
    "rwkvtts_flac_bound": (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int32]),
    "rwkvtts_flac_streaminfo": (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                               ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]),
    "rwkvtts_flac_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)]),
    "rwkvtts_flac_destroy": (ctypes.c_int, [ctypes.c_void_p]),
    "rwkvtts_flac_encode": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(FlacWindow), ctypes.c_int]),
    "rwkvtts_flac_kernel_ms": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)]),
    # pause: ramp (host only), batched / exact stream windows; the output length depends on the data
    "rwkvtts_pause_ramp": (ctypes.c_int, [ctypes.POINTER(PauseDesc), ctypes.c_void_p]),
    "rwkvtts_pause_create": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(PauseDesc), ctypes.c_void_p,
                                            ctypes.POINTER(ctypes.c_void_p)]),
    "rwkvtts_pause_destroy": (ctypes.c_int, [ctypes.c_void_p]),
    "rwkvtts_pause_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "rwkvtts_pause_windows": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(PauseWindow), ctypes.c_int]),
    "rwkvtts_pause_kernel_ms": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)]),
}

_lib = None


def lib():
    """Load librwkvtts.so (raises if it was not built: the product has no CPU fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: build it with `make -C rwkv-tts-rs_amd/csrc` "
                               "(the HIP extension is required; there is no CPU fallback)")
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in EXPORTS.items():
            if os.environ.get("RWKVTTS_LIB") and not hasattr(L, name):
                continue  # (an A/B build of an earlier revision: entry points it predates stay unbound)
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


class RwkvTtsError(RuntimeError):
    def __init__(self, rc, where):
        self.code = rc
        msg = lib().rwkvtts_last_error()
        super().__init__(f"{where} failed ({rc}): {msg.decode() if msg else ''}")
        self.rc = rc


def check(rc, where):
    if rc != OK:
        raise RwkvTtsError(rc, where)
    return rc
