"""BiCodec detokenizer on the MI355X (host mirror of the reference's vocoder calls).

Mirrors `LightweightTtsPipeline::decode_audio` / `decode_audio_batch` /
`detokenize_audio_with_session` (src/lightweight_tts_pipeline.rs:606-730): global tokens (32 FSQ
speaker codes, offset already removed) + semantic tokens -> 16 kHz f32 PCM, `T * 320` samples.
The batch call returns an empty array for an utterance that fails, as the reference's
spawn_blocking tasks do (:650-690); the single call raises.
"""
import ctypes
import threading
from typing import List, Optional, Sequence

import numpy as np

from . import _ffi
from ._ffi import check, lib

# Assumed SparkTTS BiCodec decoder dims and a tiny variant for fast tests.
CODEC_DIMS_FULL = dict(codebook_size=8192, codebook_dim=8, latent_dim=1024, n_global=32, fsq_levels=4,
                       fsq_dims=6, spk_dim=1024, prenet_dim=384, prenet_inter=2048, prenet_layers=12,
                       dec_channels=1536, n_up=4, up_rates=(8, 5, 4, 2), up_kernels=(16, 11, 8, 4))
CODEC_DIMS_TINY = dict(codebook_size=8192, codebook_dim=8, latent_dim=128, n_global=32, fsq_levels=4,
                       fsq_dims=6, spk_dim=128, prenet_dim=64, prenet_inter=128, prenet_layers=2,
                       dec_channels=512, n_up=4, up_rates=(8, 5, 4, 2), up_kernels=(16, 11, 8, 4))


def make_codec_dims(d: dict) -> _ffi.CodecDims:
    c = _ffi.CodecDims()
    for k, v in d.items():
        if k in ("up_rates", "up_kernels"):
            arr = getattr(c, k)
            for i, x in enumerate(v):
                arr[i] = x
        else:
            setattr(c, k, v)
    return c


def codec_blob_floats(d: dict) -> int:
    return int(lib().rwkvtts_codec_blob_bytes(ctypes.byref(make_codec_dims(d)))) // 4


def synth_codec_blob(d: dict, seed: int = 20251205) -> np.ndarray:
    """Deterministic synthetic decoder weights (f32 blob; MFMA operands bf16-exact)."""
    out = np.empty(codec_blob_floats(d), dtype=np.float32)
    check(lib().rwkvtts_codec_synth_weights(ctypes.byref(make_codec_dims(d)), ctypes.c_uint64(seed),
                                            out.ctypes.data_as(ctypes.c_void_p)), "codec_synth_weights")
    return out


def synth_codec_blob_f32(d: dict, seed: int = 20251205, rel: float = 2.0 ** -12) -> np.ndarray:
    """synth_codec_blob with every weight perturbed by a relative 2^-12 (seeded): f32 values that
    bf16 cannot hold, as a real fp32 checkpoint's (the reference runs BiCodec in fp32 on ORT).
    The 64-float header (the dims) is left alone."""
    w = synth_codec_blob(d, seed)
    u = np.random.default_rng(seed ^ 0x5EED).uniform(-1.0, 1.0, w.size - 64)
    w[64:] = (w[64:].astype(np.float64) * (1.0 + rel * u)).astype(np.float32)
    return w


def codec_halo(d: dict) -> tuple:
    """(prenet_halo, wave_halo) frames per side of an exact decode window (rwkvtts_codec_halo; host only)."""
    hp, hw = ctypes.c_int32(), ctypes.c_int32()
    check(lib().rwkvtts_codec_halo(ctypes.byref(make_codec_dims(d)), ctypes.byref(hp), ctypes.byref(hw)),
          "codec_halo")
    return hp.value, hw.value


def window_plan(d: dict, t0: int, t1: int, n_known: int, final: bool) -> dict:
    """The work decode_windows does for frames [t0, t1): tokens ctx = (c0, c1) through the prenet,
    frames wave = (w0, w1) through the WaveGenerator (rwkvtts_codec_window_plan; host only).
    Raises RwkvTtsError(EINVAL) unless 0 <= t0 < t1 <= n_known and (final or t1 + halo <= n_known)."""
    p = _ffi.CodecPlan(struct_size=ctypes.sizeof(_ffi.CodecPlan))
    check(lib().rwkvtts_codec_window_plan(ctypes.byref(make_codec_dims(d)), t0, t1, n_known, 1 if final else 0,
                                          ctypes.byref(p)), "codec_window_plan")
    return {"ctx": (p.ctx0, p.ctx1), "wave": (p.wave0, p.wave1)}


def launch_plan(d: dict, wlo: bool, forms: int, n: int, Tmax: int) -> List[dict]:
    """Every k_conv launch of a decode of n utterances of at most Tmax frames, in launch order, one
    dict per launch with the fields of rwkvtts_codec_launch (rwkvtts_codec_debug_launch_plan; host
    only -- the decode takes its tile, grid and LDS choice from the same function)."""
    cd = make_codec_dims(d)
    cnt = lib().rwkvtts_codec_debug_launch_plan(ctypes.byref(cd), 1 if wlo else 0, int(forms), n, Tmax, None, 0)
    if cnt < 0:
        raise _ffi.RwkvTtsError(cnt, "codec_debug_launch_plan")
    recs = (_ffi.CodecLaunch * cnt)()
    check(min(0, lib().rwkvtts_codec_debug_launch_plan(ctypes.byref(cd), 1 if wlo else 0, int(forms), n, Tmax,
                                                       recs, cnt)), "codec_debug_launch_plan")
    return [_launch_dict(r) for r in recs]


def _launch_dict(r) -> dict:
    out = {n: getattr(r, n) for n, _ in _ffi.CodecLaunch._fields_ if n not in ("struct_size", "grid")}
    out["grid"] = tuple(r.grid)
    return out


class BiCodecDetokenizer:
    """One decoder per GPU (replaces the 4-session ORT pool of src/onnx_session_pool.rs:204-279)."""

    def __init__(self, weights: np.ndarray, dims: Optional[dict] = None, device: int = 0,
                 weight_path: int = 0):
        """weight_path: _ffi.CODEC_WEIGHTS_AUTO (hi + lo weight planes iff some conv weight is not
        bf16-exact), CODEC_WEIGHTS_BF16 or CODEC_WEIGHTS_HILO (rwkvtts_codec_create_ex)."""
        self.dims = dict(dims or CODEC_DIMS_FULL)
        self.device = int(device)
        self._cd = make_codec_dims(self.dims)
        w = np.ascontiguousarray(weights, dtype=np.float32)
        h = ctypes.c_void_p()
        check(lib().rwkvtts_codec_create_ex(device, ctypes.byref(self._cd), w.ctypes.data_as(ctypes.c_void_p),
                                            int(weight_path), ctypes.byref(h)), "codec_create")
        self._h = h
        # one decode at a time: the decoder owns one stream and one set of activation buffers, and
        # streaming callers (the server's worker threads) decode many small windows concurrently
        self._lock = threading.Lock()

    def set_forms(self, forms: int):
        """Verification forms of later decode calls (_ffi.CODEC_FORM_*; 0 = shipping, PCM bitwise equal)."""
        check(lib().rwkvtts_codec_set_forms(self._h, int(forms)), "codec_set_forms")

    def close(self):
        if self._h:
            lib().rwkvtts_codec_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def decode_audio(self, global_tokens: Sequence[int], semantic_tokens: Sequence[int]) -> np.ndarray:
        g = np.ascontiguousarray(global_tokens, dtype=np.int64)
        s = np.ascontiguousarray(semantic_tokens, dtype=np.int64)
        if g.size != self.dims["n_global"] or s.size == 0:
            raise ValueError(f"decode_audio: need {self.dims['n_global']} global and >0 semantic tokens")
        pcm = np.empty(s.size * _ffi.HOP, dtype=np.float32)
        with self._lock:
            rc = lib().rwkvtts_codec_decode(self._h, s.ctypes.data_as(ctypes.c_void_p), int(s.size),
                                            g.ctypes.data_as(ctypes.c_void_p), pcm.ctypes.data_as(ctypes.c_void_p))
            check(rc, "codec_decode")
        return pcm

    def decode_audio_batch(self, batch: Sequence[tuple]) -> List[np.ndarray]:
        """[(global_tokens, semantic_tokens)] -> [pcm]; invalid items give empty arrays."""
        ok, gs, ss = [], [], []
        for g, s in batch:
            g = np.ascontiguousarray(g, dtype=np.int64)
            s = np.ascontiguousarray(s, dtype=np.int64)
            valid = g.size == self.dims["n_global"] and s.size > 0
            ok.append(valid)
            if valid:
                gs.append(g)
                ss.append(s)
        outs = [np.empty(s.size * _ffi.HOP, dtype=np.float32) for s in ss]
        if ss:
            n = len(ss)
            P = ctypes.c_void_p * n
            sem = P(*[s.ctypes.data for s in ss])
            glob = P(*[g.ctypes.data for g in gs])
            pcm = P(*[o.ctypes.data for o in outs])
            T = (ctypes.c_int * n)(*[s.size for s in ss])
            with self._lock:
                rc = lib().rwkvtts_codec_decode_batch(self._h, sem, T, glob, n, pcm)
            if rc != 0:
                outs = [np.empty(0, dtype=np.float32) for _ in ss]
        it = iter(outs)
        return [next(it) if v else np.empty(0, dtype=np.float32) for v in ok]

    # ---- streaming: exact windowed decode ----
    def halo(self) -> int:
        """Frames of look-ahead (and look-back) an exact window needs: 49 at the full dims."""
        return sum(codec_halo(self.dims))

    def decode_windows(self, items: Sequence[tuple]) -> List[np.ndarray]:
        """[(global_tokens, semantic_tokens_known_so_far, t0, t1, final)] -> [pcm of frames [t0, t1)],
        all windows in one batched pass (they may be ragged and of different utterances). Each pcm
        is bitwise samples [t0 * 320, t1 * 320) of decode_audio over the finished utterance; a
        window needs `final` (the tokens given are the whole utterance) or t1 + halo() tokens.
        Raises on a window that breaks that (nothing is decoded then)."""
        n = len(items)
        if n == 0:
            return []
        ws = (_ffi.CodecWindow * n)()
        keep, outs = [], []
        for w, (g, s, t0, t1, final) in zip(ws, items):
            g = np.ascontiguousarray(g, dtype=np.int64)
            s = np.ascontiguousarray(s, dtype=np.int64)
            if g.size != self.dims["n_global"] or not 0 <= t0 < t1 <= s.size:
                raise ValueError(f"decode_windows: need {self.dims['n_global']} global tokens and "
                                 f"0 <= t0 < t1 <= len(semantic), got {g.size}, [{t0}, {t1}) of {s.size}")
            out = np.empty((t1 - t0) * _ffi.HOP, dtype=np.float32)
            keep.append((g, s))
            outs.append(out)
            w.struct_size = ctypes.sizeof(_ffi.CodecWindow)
            w.n_known, w.final, w.t0, w.t1 = int(s.size), 1 if final else 0, int(t0), int(t1)
            w.semantic, w.global_, w.pcm = s.ctypes.data, g.ctypes.data, out.ctypes.data
        with self._lock:
            check(lib().rwkvtts_codec_decode_windows(self._h, ws, n), "codec_decode_windows")
        return outs

    # ---- test hook: one launch's inputs and outputs ----
    def capture_launch(self, k: int, batch: Sequence[tuple]):
        """Decode `batch` ([(global_tokens, semantic_tokens)]) with launch k of launch_plan() captured
        (rwkvtts_codec_debug_capture). Returns (pcm list, capture): capture["rec"] the launch's record,
        "x_hi" / "x_lo" uint16 [n][rows_in][ci] (bf16 bits), "res" / "y" float32 [n][rows_out][co],
        "y_hi" / "y_lo" uint16, "rbias" float32 [n][co]; an array the launch does not have is None."""
        check(lib().rwkvtts_codec_debug_capture(self._h, int(k)), "codec_debug_capture")
        pcm = self.decode_audio_batch(batch)  # (the decode call disarms the capture, whatever its outcome)
        rec = _ffi.CodecLaunch()
        n, ri, ro = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        check(lib().rwkvtts_codec_debug_captured_launch(self._h, ctypes.byref(rec), ctypes.byref(n), ctypes.byref(ri),
                                                        ctypes.byref(ro)), "codec_debug_captured_launch")
        cap = {"rec": _launch_dict(rec), "n": n.value, "rows_in": ri.value, "rows_out": ro.value}
        shapes = {"x_hi": (0, np.uint16, (ri.value, rec.ci)), "x_lo": (1, np.uint16, (ri.value, rec.ci)),
                  "res": (2, np.float32, (ro.value, rec.co)), "y": (3, np.float32, (ro.value, rec.co)),
                  "y_hi": (4, np.uint16, (ro.value, rec.co)), "y_lo": (5, np.uint16, (ro.value, rec.co)),
                  "rbias": (6, np.float32, (rec.co,))}
        for name, (what, dt, shp) in shapes.items():
            nbytes = lib().rwkvtts_codec_debug_captured(self._h, what, None, 0)
            if nbytes < 0:
                raise _ffi.RwkvTtsError(int(nbytes), "codec_debug_captured")
            if nbytes == 0:
                cap[name] = None
                continue
            a = np.empty((n.value,) + shp, dtype=dt)
            assert a.nbytes == nbytes, (name, a.nbytes, nbytes)
            lib().rwkvtts_codec_debug_captured(self._h, what, a.ctypes.data_as(ctypes.c_void_p), a.nbytes)
            cap[name] = a
        return pcm, cap

    # ---- profiling (per-stage HIP-event timing) ----
    def set_profiling(self, on: bool):
        check(lib().rwkvtts_codec_set_profiling(self._h, 1 if on else 0), "codec_set_profiling")

    def profile(self):
        out = {}
        for i in range(lib().rwkvtts_codec_profile_count(self._h)):
            name = ctypes.create_string_buffer(64)
            n = ctypes.c_int64()
            ms = ctypes.c_double()
            check(lib().rwkvtts_codec_profile_entry(self._h, i, name, 64, ctypes.byref(n), ctypes.byref(ms)),
                  "codec_profile_entry")
            out[name.value.decode()] = (n.value, ms.value)
        return out
