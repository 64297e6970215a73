"""Zero-shot reference-audio front end (host mirror of src/ref_audio_utilities.rs:115-222,532-631
and the clip / silence helpers it uses), feeding the HIP mel kernel (features.py).

* `load_audio(path, target_sr, volume_normalize)` (:115-222): WAV via the hound rules of
  `load_audio_with_hound` (:225-283: 16 / 24 / 32-bit int as s / 2^(bits-1), 32-bit float as is;
  1..8 channels, first channel kept; >= 0.1 s), resampled to target_sr, optionally
  volume-normalised (coeff 0.2), then leading / trailing silence (|x| <= 0.01) trimmed.
  MP3 (symphonia) is not supported: no decoder is available offline.
* `audio_volume_normalize` (:583-624), `detect_silence` / `trim_silence_only` (:1301-1356),
  `zero_mean_unit_variance_normalize` (:636-683), `get_ref_clip`
  (lightweight_tts_pipeline.rs:1130-1155): f32 restatements in the reference's order.
* `resample_audio_high_quality` (:532-576): rubato 0.15 `SincFixedIn` with the reference's
  parameters (sinc_len 256, f_cutoff 0.95, oversampling 256, linear interpolation between sinc
  tables, Blackman-Harris^2 window, one whole-signal chunk). rubato is not vendored and nothing
  in the reference pins its output: **parity unpinned**; restated from the library's published
  algorithm (the output keeps rubato's sinc_len / 2 input-sample delay and its
  ceil(n * ratio) output length).
* `Resampler` (no reference counterpart: the reference resamples on the host, and only a
  reference WAV): the same restatement as a HIP kernel (csrc/resample.hip), one-shot, batched and
  exact over stream chunks, with rubato's alignment or none. The kernel is pinned bitwise to the
  restatement's arithmetic contract (include/rwkvtts.h), not to rubato: parity stays unpinned.
* `TimeStretcher` (no reference counterpart: the reference's only rate control is the `speed`
  property token): pitch-preserving time-scale modification (WSOLA) as HIP kernels (csrc/tsm.hip),
  one-shot, batched with a tempo per signal, and exact over stream chunks. Its arithmetic contract
  (include/rwkvtts.h) has no division and no square root; the kernels are pinned
  bitwise to its numpy restatement (tests/tsm_ref.py).
* `Joiner` (no reference counterpart: the reference synthesises one request per text): the PCM of a
  long text's segments joined into one signal as HIP kernels (csrc/join.hip) -- silent edges cut to a
  kept margin and faded, a pause of zeros after each segment. Integer bounds, one rounded multiply per
  faded sample, every other sample copied (include/rwkvtts.h); pinned bitwise to its
  numpy restatement (tests/join_ref.py).
* `Leveller` (no reference counterpart: the reference peak-normalises a finished WAV to 0.8): a
  look-ahead loudness leveller with a peak ceiling as HIP kernels (csrc/level.hip) -- K-weighted
  momentary power per block, a gated running mean, a clamped and peak-capped gain ramped per block --
  one-shot, batched with a target per signal, and exact over stream chunks. Its arithmetic contract
  (include/rwkvtts.h) is f32 add, subtract, multiply and correctly rounded divide and
  square root; pinned bitwise to its numpy restatement (tests/level_ref.py).
* `Watermarker` (no reference counterpart: the reference marks nothing): a provenance watermark as HIP
  kernels (csrc/wm.hip) -- a spread-spectrum mark under a key that carries a payload, embedded
  one-shot, batched and exact over stream chunks (bitwise its numpy restatement, tests/wm_ref.py),
  and a detector that searches every alignment of the mark's period (held to the float64
  restatement within the error bound of its f32 sums). Contract: include/rwkvtts.h, DESIGN.md §30.
* `FlacEncoder` (no reference counterpart: the reference sends WAV only): a FLAC encoder as HIP kernels
  (csrc/flac.hip) -- the int16 samples of the WAV routes, losslessly compressed, one-shot, batched and
  exact over stream chunks (`FlacStream`); the subframe of each block chosen by exact bit count. Bitwise
  its numpy restatement (tests/flac_ref.py); read back by the independent decoder rwkvtts/flac.py.
  Contract: include/rwkvtts.h, DESIGN.md §31.
* `PauseShaper` (no reference counterpart: the reference sends whatever silence the semantic model
  chose): silences capped as HIP kernels (csrc/pause.hip) -- loud and active blocks by comparison, runs
  of non-active blocks longer than the cap cut to a faded head and tail -- one-shot, batched with a cap
  per signal and exact over stream chunks (`PauseStream`), the output shorter than the input by what
  was cut. Bitwise its numpy restatement (tests/pause_ref.py). Contract: include/rwkvtts.h, DESIGN.md §35.
"""
import ctypes
import struct
import threading
from typing import Tuple

import numpy as np

from . import _ffi

F32 = np.float32


# ---- WAV (hound) -------------------------------------------------------------------------
def read_wav(path: str) -> Tuple[np.ndarray, int, int]:
    """-> (interleaved f32 samples, sample_rate, channels) under load_audio_with_hound's rules."""
    with open(path, "rb") as f:
        data = f.read()
    if len(data) < 12 or data[:4] != b"RIFF" or data[8:12] != b"WAVE":
        raise ValueError("not a RIFF/WAVE file")
    pos, fmt, pcm = 12, None, None
    while pos + 8 <= len(data):
        cid, size = data[pos:pos + 4], struct.unpack("<I", data[pos + 4:pos + 8])[0]
        body = data[pos + 8:pos + 8 + size]
        if cid == b"fmt ":
            fmt = struct.unpack("<HHIIHH", body[:16])
            if fmt[0] == 0xFFFE and len(body) >= 26:  # WAVE_FORMAT_EXTENSIBLE: sub-format code
                fmt = (struct.unpack("<H", body[24:26])[0],) + fmt[1:]
        elif cid == b"data":
            pcm = body
        pos += 8 + size + (size & 1)
    if fmt is None or pcm is None:
        raise ValueError("WAV lacks fmt or data chunk")
    tag, ch, sr, _, _, bits = fmt
    if bits not in (16, 24, 32):
        raise ValueError(f"unsupported bit depth: {bits} (16/24/32)")
    if ch == 0 or ch > 8:
        raise ValueError(f"unsupported channel count: {ch} (1-8)")
    if sr == 0 or sr > 192000:
        raise ValueError(f"unsupported sample rate: {sr} Hz")
    if bits == 16:
        x = np.frombuffer(pcm[:len(pcm) // 2 * 2], dtype="<i2").astype(F32) / F32(32768.0)
    elif bits == 24:
        b = np.frombuffer(pcm[:len(pcm) // 3 * 3], dtype=np.uint8).reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        v = np.where(v >= 1 << 23, v - (1 << 24), v)
        x = v.astype(F32) / F32(8388608.0)
    elif tag == 3:
        x = np.frombuffer(pcm[:len(pcm) // 4 * 4], dtype="<f4").astype(F32)
    else:
        x = np.frombuffer(pcm[:len(pcm) // 4 * 4], dtype="<i4").astype(F32) / F32(2147483648.0)
    return x, sr, ch


# ---- rubato SincFixedIn ---------------------------------------------------------------------
def _blackman_harris2(n: int) -> np.ndarray:
    """rubato WindowFunction::BlackmanHarris2: the Blackman-Harris window squared."""
    k = np.arange(n, dtype=np.float64)
    w = (0.35875 - 0.48829 * np.cos(2 * np.pi * k / n) + 0.14128 * np.cos(4 * np.pi * k / n)
         - 0.01168 * np.cos(6 * np.pi * k / n))
    return (w * w).astype(F32)


def _make_sincs(npoints: int, factor: int, f_cutoff: float) -> np.ndarray:
    """rubato make_sincs: `factor` tables of `npoints` taps, normalised to unit DC gain."""
    tot = npoints * factor
    win = _blackman_harris2(tot)
    x = (np.arange(tot, dtype=np.float64) - tot // 2) * f_cutoff / factor
    y = (win.astype(np.float64) * np.sinc(x)).astype(F32)
    s = F32(np.sum(y, dtype=F32) / F32(factor))
    sincs = np.empty((factor, npoints), dtype=F32)
    for n in range(factor):
        sincs[factor - n - 1] = y[n::factor] / s
    return sincs


def resample_audio_high_quality(audio, original_sr: int, target_sr: int, sinc_len: int = 256,
                                f_cutoff: float = 0.95, oversampling: int = 256, device=None) -> np.ndarray:
    """device None: the numpy restatement below. An integer: the HIP kernel on that GPU with rubato
    alignment (Resampler): the same positions, taps and table; its two sums per output run in
    ascending tap order where einsum's order is unspecified, so the two agree to the forward-error
    bound of an f32 sum, not bitwise (tests/test_gpu_resample.py)."""
    x = np.asarray(audio, dtype=F32)
    if original_sr == target_sr:
        return x.copy()
    if device is not None:
        r = Resampler(original_sr, target_sr, device=int(device), align="rubato", sinc_len=sinc_len,
                      f_cutoff=f_cutoff, oversampling=oversampling)
        try:
            return r.resample(x)
        finally:
            r.close()
    ratio = target_sr / original_sr
    cutoff = f_cutoff if ratio >= 1.0 else f_cutoff * ratio
    sincs = _make_sincs(sinc_len, oversampling, cutoff)
    n_out = int(np.ceil(x.size * ratio))
    # input buffer as rubato holds it: sinc_len zeros of history, then the chunk
    buf = np.concatenate([np.zeros(sinc_len, F32), x, np.zeros(sinc_len, F32)])
    t_ratio = 1.0 / ratio
    idx = np.arange(n_out, dtype=np.float64) * t_ratio - sinc_len / 2.0  # rubato's start delay
    start = np.floor(idx).astype(np.int64)
    frac = idx - start
    pos = frac * oversampling
    p0 = np.floor(pos).astype(np.int64)
    w1 = (pos - p0).astype(F32)
    base = start + sinc_len  # into buf
    out = np.empty(n_out, dtype=F32)
    taps = np.arange(sinc_len)
    for i0 in range(0, n_out, 4096):  # linear interpolation between adjacent sinc tables
        sl = slice(i0, min(i0 + 4096, n_out))
        seg = buf[(base[sl, None] + taps[None, :] - sinc_len // 2 + 1).clip(0, buf.size - 1)]
        a = np.einsum("ij,ij->i", seg, sincs[p0[sl] % oversampling])
        b = np.einsum("ij,ij->i", seg, sincs[(p0[sl] + 1) % oversampling])
        out[sl] = a + (b - a) * w1[sl]
    return out


# ---- what the two GPU stages share (csrc/stage.h is the native side's counterpart) -------------
def _native(name, *args):
    _ffi.check(getattr(_ffi.lib(), "rwkvtts_" + name)(*args), name)


class _NativeStage:
    """A native object (rwkvtts_<_NAME>_create / _destroy / _kernel_ms) made from self._desc and one
    f32 table on self.device, unless an evaluator stands in for it; its call lock; the marshalling of
    a ragged batch."""
    _NAME = None

    def __init__(self, evaluator):
        self._h = None
        self._evaluator = evaluator
        # one native call at a time: the object owns one stream and one set of device buffers
        self._lock = threading.Lock()

    def _create(self, table):
        if self._evaluator is None:
            h = ctypes.c_void_p()
            _native(self._NAME + "_create", self.device, ctypes.byref(self._desc),
                    table.ctypes.data_as(ctypes.c_void_p), ctypes.byref(h))
            self._h = h

    def close(self):
        if self._h:
            getattr(_ffi.lib(), f"rwkvtts_{self._NAME}_destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _call(self, name, *args):
        with self._lock:
            _native(name, self._h, *args)

    @staticmethod
    def _ragged(xs, out_lens):
        """-> (outputs, void* inputs[], int64 lengths[], void* outputs[]) of a *_batch call."""
        outs = [np.empty(n, dtype=F32) for n in out_lens]
        P = ctypes.c_void_p * len(xs)
        return (outs, P(*[x.ctypes.data for x in xs]), (ctypes.c_int64 * len(xs))(*[x.size for x in xs]),
                P(*[o.ctypes.data for o in outs]))

    def _windows(self, name, Struct, items, **own):
        """One rwkvtts_<name> call over items (samples, in_first, final, .., out_count) -> (the
        Struct array, the outputs); own: the stage's further fields by their position in an item."""
        ws = (Struct * len(items))()
        outs = [np.empty(max(it[-1], 0), dtype=F32) for it in items]
        for w, it, out in zip(ws, items, outs):
            w.struct_size = ctypes.sizeof(Struct)
            w.in_, w.in_first, w.n_in, w.final = it[0].ctypes.data, it[1], it[0].size, 1 if it[2] else 0
            w.out_count, w.out = it[-1], out.ctypes.data
            for field, k in own.items():
                setattr(w, field, it[k])
        if items:
            self._call(name, ws, len(items))
        return ws, outs

    def kernel_ms(self) -> float:
        """HIP-event time of the last call's kernels alone (no copies)."""
        ms = ctypes.c_double()
        _native(self._NAME + "_kernel_ms", self._h, ctypes.byref(ms))
        return ms.value


class _ExactStream:
    """feed(pcm_chunk, final=False) -> what became exact with it, over a kept tail of the input. A
    subclass has _emit(n_known, final) -> the ready outputs, computed from _tail (signal samples
    [_tail_first, n_known)), advancing its own cursor, and _first_needed(n_known) -> the first input
    sample the outputs after the cursor still read."""

    def __init__(self):
        self._tail = np.zeros(0, dtype=F32)
        self._tail_first = 0   # signal index of _tail[0]
        self._closed = False

    @property
    def kept(self) -> int:
        return int(self._tail.size)

    def feed(self, pcm_chunk, final: bool = False) -> np.ndarray:
        if self._closed:
            raise ValueError("the stream has ended (a chunk was fed with final=True)")
        x = np.asarray(pcm_chunk, dtype=F32).reshape(-1)
        if x.size:
            self._tail = np.concatenate([self._tail, x])
        n_known = self._tail_first + self._tail.size
        out = self._emit(n_known, final)
        if final:
            self._closed, self._tail = True, np.zeros(0, dtype=F32)
            return out
        first = min(self._first_needed(n_known), n_known)
        if first > self._tail_first:
            self._tail = self._tail[first - self._tail_first:].copy()
            self._tail_first = first
        return out


# ---- the resampler on the GPU ----------------------------------------------------------------
class Resampler(_NativeStage):
    """The restatement above as a HIP kernel (csrc/resample.hip; the arithmetic contract is in
    include/rwkvtts.h): one-shot, batched and exact over stream chunks.

    align "rubato" keeps rubato's sinc_len / 2 start delay and cuts the tail, as
    resample_audio_high_quality does (the reference-audio front end); "zero" puts output o at input
    time o / ratio (synthesised output: no delay, nothing cut). The kernel reads the table
    `_make_sincs` builds, so the restatement has a single source; it is pinned bitwise to the
    contract's numpy form (tests/test_gpu_resample.py), not to rubato (parity unpinned, as above).

    evaluator: a callable (resampler, items) -> [ndarray] standing in for the native window call,
    items being [(samples from in_first on, in_first, final, out_first, out_count)]; no GPU resampler
    is created then (the host-only plan / out_len entry points are still the library's)."""
    _NAME = "resampler"

    def __init__(self, sr_in: int, sr_out: int, device: int = 0, align: str = "zero", sinc_len: int = 256,
                 f_cutoff: float = 0.95, oversampling: int = 256, evaluator=None):
        if align not in ("zero", "rubato"):
            raise ValueError('align must be "zero" or "rubato"')
        self.sr_in, self.sr_out, self.align, self.device = int(sr_in), int(sr_out), align, int(device)
        self.sinc_len, self.oversampling, self.f_cutoff = int(sinc_len), int(oversampling), float(f_cutoff)
        self._desc = _ffi.ResampleDesc(
            struct_size=ctypes.sizeof(_ffi.ResampleDesc), sr_in=self.sr_in, sr_out=self.sr_out,
            sinc_len=self.sinc_len, oversampling=self.oversampling, f_cutoff=self.f_cutoff,
            align=_ffi.RESAMPLE_ALIGN_ZERO if align == "zero" else _ffi.RESAMPLE_ALIGN_RUBATO)
        super().__init__(evaluator)
        self.out_len(0)  # (refuses a bad description before anything is built)
        self.ratio = self.sr_out / self.sr_in
        self.sincs = _make_sincs(self.sinc_len, self.oversampling,
                                 self.f_cutoff if self.ratio >= 1.0 else self.f_cutoff * self.ratio)
        self._create(self.sincs)

    # ---- host-only plan ----
    def out_len(self, n_in: int) -> int:
        n = int(_ffi.lib().rwkvtts_resample_out_len(ctypes.byref(self._desc), int(n_in)))
        if n < 0:
            raise _ffi.RwkvTtsError(_ffi.EINVAL, "resample_out_len")
        return n

    def plan(self, n_known: int, final: bool, out_first: int = 0):
        """(out_ready_end, in_first_needed) of rwkvtts_resample_plan."""
        end, first = ctypes.c_int64(), ctypes.c_int64()
        _native("resample_plan", ctypes.byref(self._desc), int(n_known), 1 if final else 0, int(out_first),
                ctypes.byref(end), ctypes.byref(first))
        return end.value, first.value

    # ---- the kernel ----
    def resample_windows(self, items) -> list:
        """[(samples from in_first on, in_first, final, out_first, out_count)] -> [outputs
        [out_first, out_first + out_count) of the whole-signal resample], all windows in one launch.
        Raises RwkvTtsError(EINVAL), with nothing computed, if a requested output needs a sample
        that was not given (plan())."""
        items = [(np.ascontiguousarray(x, dtype=F32).reshape(-1), int(a), bool(f), int(o), int(c))
                 for x, a, f, o, c in items]
        if self._evaluator is not None:
            return [np.ascontiguousarray(y, dtype=F32) for y in self._evaluator(self, items)]
        return self._windows("resample_windows", _ffi.ResampleWindow, items, out_first=3)[1]

    def resample_batch(self, signals) -> list:
        """[signal] -> [resampled signal], ragged, in one launch; an empty signal gives an empty one."""
        xs = [np.ascontiguousarray(x, dtype=F32).reshape(-1) for x in signals]
        if self._evaluator is not None:
            return self.resample_windows([(x, 0, True, 0, self.out_len(x.size)) for x in xs])
        if not xs:
            return []
        outs, ins, lens, ous = self._ragged(xs, [self.out_len(x.size) for x in xs])
        self._call("resample_batch", ins, lens, len(xs), ous)
        return outs

    def resample(self, x) -> np.ndarray:
        return self.resample_batch([x])[0]

    def stream(self) -> "ResampleStream":
        return ResampleStream(self)


class ResampleStream(_ExactStream):
    """Resampler.stream(): feed(pcm_chunk, final=False) -> the outputs that became exact with it.
    The concatenation of what feed returns is bitwise Resampler.resample(the concatenated input),
    however the input was cut. Only the tail rwkvtts_resample_plan asks for is kept: fewer than
    sinc_len + ceil(1 / ratio) + 1 samples."""

    def __init__(self, resampler: Resampler):
        super().__init__()
        self.r = resampler
        self._out_next = 0     # outputs [0, _out_next) went out

    def _emit(self, n_known, final):
        end, _ = self.r.plan(n_known, final, self._out_next)
        count = end - self._out_next
        if count > 0:
            out = self.r.resample_windows([(self._tail, self._tail_first, final, self._out_next, count)])[0]
        else:
            out = np.zeros(0, dtype=F32)
        self._out_next = max(end, self._out_next)
        return out

    def _first_needed(self, n_known):
        return self.r.plan(n_known, False, self._out_next)[1]


# ---- time stretch on the GPU -----------------------------------------------------------------
def _tsm_window(window: int) -> np.ndarray:
    """w[i] = (float)(0.5 - 0.5 * cos(2 * pi * i / W)), in double: the table both sides read."""
    i = np.arange(window, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * i / float(window))).astype(F32)


class TimeStretcher(_NativeStage):
    """Pitch-preserving time-scale modification (WSOLA) as HIP kernels (csrc/tsm.hip; the arithmetic
    contract is in include/rwkvtts.h): tempo 0.25 .. 4.0 per signal, above 1 is faster speech; the
    output has ceil(n / tempo) samples. One-shot, batched (a tempo per signal in one launch) and exact
    over stream chunks. Rate-agnostic: the pipeline applies it at 16 kHz, before any resampling.

    window (even, 32 .. 2048) and search (1 .. 1024): the Hann window W and the search radius D in
    samples; 0 means the default (512 / 128) as in the C desc. The kernels read the table
    `_tsm_window` builds, so both sides read one table.

    evaluator: a callable (stretcher, items) -> [(ndarray, s_last)] standing in for the native window
    call, items being [(samples from in_first on, in_first, final, tempo, block_first, s_prev,
    out_count)]; no GPU object is created then (the host-only plan / out_len entry points are still
    the library's)."""
    _NAME = "tsm"

    def __init__(self, device: int = 0, window: int = 512, search: int = 128, evaluator=None):
        self.device = int(device)
        self._desc = _ffi.TsmDesc(struct_size=ctypes.sizeof(_ffi.TsmDesc), window=int(window), search=int(search))
        super().__init__(evaluator)
        self.out_len(0, 1.0)  # (refuses a bad description before anything is built)
        self.window = int(window) or 512
        self.search = int(search) or 128
        self.hop = self.window // 2
        self.table = _tsm_window(self.window)
        self._create(self.table)

    # ---- host-only plan ----
    def out_len(self, n_in: int, tempo: float) -> int:
        n = int(_ffi.lib().rwkvtts_tsm_out_len(ctypes.byref(self._desc), float(tempo), int(n_in)))
        if n < 0:
            raise _ffi.RwkvTtsError(_ffi.EINVAL, "tsm_out_len")
        return n

    def plan(self, tempo: float, n_known: int, final: bool, block_first: int = 0, s_prev=None):
        """(out_ready_end, in_first_needed) of rwkvtts_tsm_plan; s_prev None: -hop (block_first 0)."""
        end, first = ctypes.c_int64(), ctypes.c_int64()
        _native("tsm_plan", ctypes.byref(self._desc), float(tempo), int(n_known), 1 if final else 0, int(block_first),
                -self.hop if s_prev is None else int(s_prev), ctypes.byref(end), ctypes.byref(first))
        return end.value, first.value

    # ---- the kernels ----
    def stretch_windows(self, items) -> list:
        """[(samples from in_first on, in_first, final, tempo, block_first, s_prev, out_count)] ->
        [(outputs [block_first * hop, + out_count) of the whole-signal result, s_last)], all windows
        in one launch pair. Raises RwkvTtsError(EINVAL), with nothing computed, if a window asks for
        more than plan() allows."""
        items = [(np.ascontiguousarray(x, dtype=F32).reshape(-1), int(a), bool(f), float(t), int(b), int(s), int(c))
                 for x, a, f, t, b, s, c in items]
        if self._evaluator is not None:
            return [(np.ascontiguousarray(y, dtype=F32), int(s)) for y, s in self._evaluator(self, items)]
        ws, outs = self._windows("tsm_windows", _ffi.TsmWindow, items, tempo=3, block_first=4, s_prev=5)
        return [(o, int(w.s_last)) for o, w in zip(outs, ws)]

    def stretch_batch(self, signals, tempos) -> list:
        """[signal], [tempo] -> [stretched signal], ragged, a tempo per signal, in one launch pair."""
        xs = [np.ascontiguousarray(x, dtype=F32).reshape(-1) for x in signals]
        ts = [float(t) for t in tempos]
        if len(xs) != len(ts):
            raise ValueError("stretch_batch: one tempo per signal")
        if self._evaluator is not None:
            return [y for y, _ in self.stretch_windows([(x, 0, True, t, 0, -self.hop, self.out_len(x.size, t))
                                                        for x, t in zip(xs, ts)])]
        if not xs:
            return []
        outs, ins, lens, ous = self._ragged(xs, [self.out_len(x.size, t) for x, t in zip(xs, ts)])
        self._call("tsm_batch", ins, lens, (ctypes.c_double * len(ts))(*ts), len(xs), ous)
        return outs

    def stretch(self, x, tempo: float) -> np.ndarray:
        return self.stretch_batch([x], [tempo])[0]

    def stream(self, tempo: float) -> "TimeStretchStream":
        return TimeStretchStream(self, tempo)


class TimeStretchStream(_ExactStream):
    """TimeStretcher.stream(tempo): feed(pcm_chunk, final=False) -> the blocks that became exact with
    it. The concatenation of what feed returns is bitwise TimeStretcher.stretch(the concatenated
    input, tempo), however the input was cut. Only the tail rwkvtts_tsm_plan asks for is kept: fewer
    than 2 * search + window * max(tempo, 1) + 2 samples."""

    def __init__(self, stretcher: TimeStretcher, tempo: float):
        super().__init__()
        self.t = stretcher
        self.tempo = float(tempo)
        stretcher.out_len(0, self.tempo)  # (refuses a bad tempo)
        self._block_next = 0              # blocks [0, _block_next) went out
        self._s_prev = -stretcher.hop     # start of frame _block_next - 1

    def _emit(self, n_known, final):
        hop = self.t.hop
        end, _ = self.t.plan(self.tempo, n_known, final, self._block_next, self._s_prev)
        count = end - self._block_next * hop
        if count <= 0:
            return np.zeros(0, dtype=F32)
        out, self._s_prev = self.t.stretch_windows([(self._tail, self._tail_first, final, self.tempo,
                                                     self._block_next, self._s_prev, count)])[0]
        self._block_next += -(-count // hop)
        return out

    def _first_needed(self, n_known):
        return self.t.plan(self.tempo, n_known, False, self._block_next, self._s_prev)[1]


# ---- join on the GPU -------------------------------------------------------------------------
def _join_ramp(fade: int) -> np.ndarray:
    """r[k] = (float)((k + 0.5) / fade), in double: the table both sides read."""
    return ((np.arange(fade, dtype=np.float64) + 0.5) / float(max(fade, 1))).astype(F32)


class Joiner(_NativeStage):
    """The PCM of a long text's segments joined into one signal as HIP kernels (csrc/join.hip; the
    arithmetic contract is in include/rwkvtts.h): with trim, each segment is cut to
    `keep` samples around its first and last sample above `threshold` and both its edges are faded
    over `fade` samples; a gap of zeros follows each segment. Rate-agnostic: the pipeline applies it
    at 16 kHz, before the stretch and the resampler. A piece depends on its own segment only, so the
    join of a job is bitwise the joins of its segments one by one, back to back.

    threshold (finite, >= 0; 0 means the default 0.01 as in the C desc), keep >= 0, fade 0 .. 4096.
    The kernels read the table `_join_ramp` builds, so both sides read one table.

    evaluator: a callable (joiner, jobs) -> [(ndarray, [(a, b)])] standing in for the native call,
    jobs being [([segment], [gap])]; no GPU object is created then."""
    _NAME = "join"

    def __init__(self, device: int = 0, threshold: float = 0.01, keep: int = 800, fade: int = 80, trim: bool = True,
                 evaluator=None):
        self.device = int(device)
        self._desc = _ffi.JoinDesc(struct_size=ctypes.sizeof(_ffi.JoinDesc), threshold=float(threshold),
                                   keep=int(keep), fade=int(fade), trim=1 if trim else 0)
        super().__init__(evaluator)
        self.keep, self.fade, self.trim = int(keep), int(fade), bool(trim)
        self.threshold = float(F32(threshold)) or float(F32(0.01))
        probe = np.zeros(max(self.fade, 1) if 0 <= self.fade <= 4096 else 1, dtype=F32)
        _native("join_ramp", ctypes.byref(self._desc), probe.ctypes.data_as(ctypes.c_void_p))  # (refuses a bad description)
        self.table = _join_ramp(self.fade)
        self._create(self.table if self.fade else np.zeros(1, dtype=F32))

    @staticmethod
    def capacity(lengths, gaps) -> int:
        """sum n_s + sum gap_s (rwkvtts_join_capacity)."""
        n = np.ascontiguousarray(lengths, dtype=np.int64)
        g = np.ascontiguousarray(gaps, dtype=np.int64)
        if n.size != g.size:
            raise ValueError("join: one gap per segment")
        cap = int(_ffi.lib().rwkvtts_join_capacity(n.ctypes.data_as(ctypes.c_void_p), g.ctypes.data_as(ctypes.c_void_p),
                                                   int(n.size)))
        if cap < 0:
            raise _ffi.RwkvTtsError(_ffi.EINVAL, "join_capacity")
        return cap

    def join_batch(self, jobs) -> list:
        """[([segment], [gap])] -> [(joined PCM, [(a_s, b_s)])], ragged, all jobs in one pass."""
        jobs = [([np.ascontiguousarray(x, dtype=F32).reshape(-1) for x in segs], [int(g) for g in gaps])
                for segs, gaps in jobs]
        for segs, gaps in jobs:
            if len(segs) != len(gaps):
                raise ValueError("join: one gap per segment")
        if self._evaluator is not None:
            return [(np.ascontiguousarray(y, dtype=F32), [(int(a), int(b)) for a, b in ab])
                    for y, ab in self._evaluator(self, jobs)]
        if not jobs:
            return []
        js = (_ffi.JoinJob * len(jobs))()
        keep = []
        for j, (segs, gaps) in zip(js, jobs):
            n = np.array([x.size for x in segs], dtype=np.int64)
            g = np.array(gaps, dtype=np.int64)
            ptr = (ctypes.c_void_p * max(len(segs), 1))(*[x.ctypes.data for x in segs])
            out = np.empty(self.capacity(n, g), dtype=F32)
            a, b = np.zeros(len(segs), dtype=np.int64), np.zeros(len(segs), dtype=np.int64)
            j.struct_size, j.n_seg = ctypes.sizeof(_ffi.JoinJob), len(segs)
            j.seg, j.n, j.gap = ctypes.addressof(ptr), n.ctypes.data, g.ctypes.data
            j.out, j.a, j.b = out.ctypes.data, a.ctypes.data, b.ctypes.data
            keep.append((n, g, ptr, out, a, b))
        self._call("join_jobs", js, len(jobs))
        return [(out[:int(j.n_out)].copy(), list(zip(a.tolist(), b.tolist()))) for j, (_, _, _, out, a, b) in zip(js, keep)]

    def join(self, segments, gaps):
        """One job -> (joined PCM, [(a_s, b_s)])."""
        return self.join_batch([(segments, gaps)])[0]


# ---- loudness levelling on the GPU -----------------------------------------------------------
def _level_biquads(fs: float):
    """The two BS.1770 K-weighting biquads at rate fs -> ((b, a) of the shelf, (b, a) of the high-pass):
    the bilinear design of include/rwkvtts.h, one double operation at a time, in its order."""
    import math
    out = []
    for f0, Q, G in ((1681.974450955533, 0.7071752369554196, 3.999843853973347),
                     (38.13547087602444, 0.5003270373238773, None)):
        K = math.tan(math.pi * f0 / fs)
        KQ, KK = K / Q, K * K
        a0 = (1.0 + KQ) + KK
        if G is not None:
            Vh = math.pow(10.0, G / 20.0)
            Vb = math.pow(Vh, 0.4996667741545416)
            b = (((Vh + Vb * KQ) + KK) / a0, (2.0 * (KK - Vh)) / a0, ((Vh - Vb * KQ) + KK) / a0)
        else:
            b = (1.0, -2.0, 1.0)
        out.append((b, (1.0, (2.0 * (KK - 1.0)) / a0, ((1.0 - KQ) + KK) / a0)))
    return out


def _level_table(taps: int, block: int, fs: float = 16000.0) -> np.ndarray:
    """h[0, taps) -- the impulse response of the two biquads in direct form I, shelf first, in double,
    rounded to f32 -- then r[i] = (float)((i + 1) / block): the table both sides read."""
    v = [1.0] + [0.0] * (taps - 1)
    for b, a in _level_biquads(fs):
        y, x1, x2, y1, y2 = [], 0.0, 0.0, 0.0, 0.0
        for x in v:
            t = b[0] * x
            t = t + b[1] * x1
            t = t + b[2] * x2
            t = t - a[1] * y1
            t = t - a[2] * y2
            x2, x1, y2, y1 = x1, x, y1, t
            y.append(t)
        v = y
    r = np.arange(1, block + 1, dtype=np.float64) / float(block)
    return np.concatenate([np.array(v, dtype=np.float64), r]).astype(F32)


def level_target(loudness: float) -> np.float32:
    """T2, the f32 mean square of a loudness in dB: 10^((loudness + 0.691) / 10), taken in double
    (rwkvtts_level_target, host only)."""
    return F32(_ffi.lib().rwkvtts_level_target(float(loudness)))


class Leveller(_NativeStage):
    """A look-ahead loudness leveller with a built-in peak ceiling as HIP kernels (csrc/level.hip; the
    arithmetic contract is in include/rwkvtts.h): the K-weighted momentary power of
    blocks of `block` samples (a `taps`-long FIR), a gated running mean of it that sees `lookahead`
    blocks ahead, a gain sqrt(target / mean) clamped to [g_min, g_max] and capped so that no sample
    passes `ceiling`, ramped linearly over each block. One causal definition, so a stream's pieces
    are bitwise the one-shot result; n_out = n. The pipeline applies it at 16 kHz, after the stretch
    and before the resampler. A loudness is a target in dB per signal (-23, -16, ..).

    0 means the default as in the C desc: block 1600 (100 ms), taps 1024, lookahead 4, gate 1e-5,
    ceiling 0.891, g_min 0.1, g_max 10, horizon 0 (unbounded memory). Every default is untuned: the
    repository has no real checkpoint. The kernels read the table `_level_table` builds.

    evaluator: a callable (leveller, items) -> [(ndarray, S, N, g)] standing in for the native window
    call, items being [(samples from in_first on, in_first, final, t2, block_first, S, N, g_prev,
    out_count)]; no GPU object is created then (the host-only plan / table entry points are still the
    library's)."""
    _NAME = "level"

    def __init__(self, device: int = 0, block: int = 1600, taps: int = 1024, lookahead: int = 4, gate: float = 1e-5,
                 ceiling: float = 0.891, g_min: float = 0.1, g_max: float = 10.0, horizon: int = 0, evaluator=None):
        self.device = int(device)
        self._desc = _ffi.LevelDesc(struct_size=ctypes.sizeof(_ffi.LevelDesc), block=int(block), taps=int(taps),
                                    lookahead=int(lookahead), gate=float(gate), ceiling=float(ceiling),
                                    g_min=float(g_min), g_max=float(g_max), horizon=int(horizon))
        super().__init__(evaluator)
        self.plan(0, False)  # (refuses a bad description before anything is built)
        self.block, self.taps, self.lookahead = int(block) or 1600, int(taps) or 1024, int(lookahead) or 4
        self.gate, self.ceiling = F32(gate) or F32(1e-5), F32(ceiling) or F32(0.891)
        self.g_min, self.g_max, self.horizon = F32(g_min) or F32(0.1), F32(g_max) or F32(10.0), int(horizon)
        self.table = _level_table(self.taps, self.block)
        self._create(self.table)

    # ---- host-only plan ----
    def plan(self, n_known: int, final: bool, block_first: int = 0):
        """(out_ready_end, in_first_needed) of rwkvtts_level_plan."""
        end, first = ctypes.c_int64(), ctypes.c_int64()
        _native("level_plan", ctypes.byref(self._desc), int(n_known), 1 if final else 0, int(block_first),
                ctypes.byref(end), ctypes.byref(first))
        return end.value, first.value

    # ---- the kernels ----
    def level_windows(self, items) -> list:
        """[(samples from in_first on, in_first, final, t2, block_first, S, N, g_prev, out_count)] ->
        [(outputs [block_first * block, + out_count) of the whole-signal result, S, N, g)], the state
        after each window's last block, all windows in one launch triple. Raises
        RwkvTtsError(EINVAL), with nothing computed, if a window asks for more than plan() allows."""
        items = [(np.ascontiguousarray(x, dtype=F32).reshape(-1), int(a), bool(f), float(F32(t)), int(b), float(F32(s)),
                  int(n), float(F32(g)), int(c)) for x, a, f, t, b, s, n, g, c in items]
        if self._evaluator is not None:
            return [(np.ascontiguousarray(y, dtype=F32), F32(s), int(n), F32(g)) for y, s, n, g in self._evaluator(self, items)]
        ws, outs = self._windows("level_windows", _ffi.LevelWindow, items, t2=3, block_first=4, s_prev=5, n_prev=6,
                                 g_prev=7)
        return [(o, F32(w.s_last), int(w.n_last), F32(w.g_last)) for o, w in zip(outs, ws)]

    def level_batch(self, signals, loudness) -> list:
        """[signal], [loudness in dB] -> [levelled signal], ragged, a target per signal, in one launch
        triple; an empty signal gives an empty one."""
        xs = [np.ascontiguousarray(x, dtype=F32).reshape(-1) for x in signals]
        ts = [level_target(v) for v in loudness]
        if len(xs) != len(ts):
            raise ValueError("level_batch: one loudness per signal")
        if self._evaluator is not None:
            return [y for y, _, _, _ in self.level_windows([(x, 0, True, t, 0, 0.0, 0, 1.0, x.size)
                                                            for x, t in zip(xs, ts)])]
        if not xs:
            return []
        outs, ins, lens, ous = self._ragged(xs, [x.size for x in xs])
        self._call("level_batch", ins, lens, (ctypes.c_float * len(ts))(*[float(t) for t in ts]), len(xs), ous)
        return outs

    def level(self, x, loudness: float) -> np.ndarray:
        return self.level_batch([x], [loudness])[0]

    def stream(self, loudness: float) -> "LevelStream":
        return LevelStream(self, loudness)


class LevelStream(_ExactStream):
    """Leveller.stream(loudness): feed(pcm_chunk, final=False) -> the blocks that became exact with
    it. The concatenation of what feed returns is bitwise Leveller.level(the concatenated input,
    loudness), however the input was cut. A block goes out once the `lookahead` blocks after it are
    complete, so the output lags the input by up to lookahead + 1 blocks (0.5 s at the defaults); the
    kept tail is what rwkvtts_level_plan asks for, fewer than (lookahead + 4) * block + taps samples."""

    def __init__(self, leveller: Leveller, loudness: float):
        super().__init__()
        self.v = leveller
        self.t2 = level_target(loudness)
        if not (np.isfinite(self.t2) and self.t2 > 0):
            raise ValueError("loudness gives no finite positive target")
        self._block_next = 0                       # blocks [0, _block_next) went out
        self._state = (F32(0.0), 0, F32(1.0))      # (S, N, g) after block _block_next - 1

    def _emit(self, n_known, final):
        B = self.v.block
        end, _ = self.v.plan(n_known, final, self._block_next)
        count = end - self._block_next * B
        if count <= 0:
            return np.zeros(0, dtype=F32)
        S, N, g = self._state
        out, S, N, g = self.v.level_windows([(self._tail, self._tail_first, final, self.t2, self._block_next, S, N, g,
                                              count)])[0]
        self._state = (S, N, g)
        self._block_next += -(-count // B)
        return out

    def _first_needed(self, n_known):
        return self.v.plan(n_known, False, self._block_next)[1]


# ---- pitch shift on the GPU ------------------------------------------------------------------
def pitch_factor(semitones: float) -> float:
    """f = 2^(semitones / 12), in double: what the native side takes per signal."""
    return 2.0 ** (float(semitones) / 12.0)


def _pitch_table(lag_min: int, lag_max: int) -> np.ndarray:
    """Rows P = lag_min .. lag_max back to back, row P at (P - lag_min) * (P + lag_min - 1):
    w_P[i] = (float)(0.5 - 0.5 * cos(2 * pi * (i + 0.5) / (2P))), in double: the table both sides read."""
    rows = []
    for P in range(lag_min, lag_max + 1):
        i = np.arange(2 * P, dtype=np.float64)
        rows.append((0.5 - 0.5 * np.cos((2.0 * np.pi * (i + 0.5)) / float(2 * P))).astype(F32))
    return np.concatenate(rows)


class PitchShifter(_NativeStage):
    """A formant-preserving pitch shift (period estimation and pitch-synchronous overlap-add,
    TD-PSOLA) as HIP kernels (csrc/pitch.hip; the arithmetic contract is in include/rwkvtts.h,
    DESIGN.md §25): per frame of `hop` samples the period is the lowest lag in lag_min .. lag_max at
    which the squared difference over `window` samples has a local minimum below theta times the
    energy (no such lag: unvoiced); two-period Hann grains around pitch marks one period apart are
    laid down again period / factor apart and normalised by the summed windows. The fundamental moves
    by the factor, the grains (and so the spectral envelope) stay, unvoiced sound and silence pass,
    n_out = n. One causal definition, so a stream's pieces are bitwise the one-shot result. The
    pipeline applies it at 16 kHz, first of the stages. A shift is in semitones per signal, -12 .. 12.

    0 means the default as in the C desc: hop 160, window 640, lag_min 32, lag_max 320 (50 .. 500 Hz),
    unvoiced 80, theta 0.2, floor 1e-3. Every default is untuned and nobody has listened to the
    output: the repository has no real checkpoint. The kernels read the table `_pitch_table` builds.

    evaluator: a callable (shifter, items) -> [(ndarray, a_last, s_last)] standing in for the native
    window call, items being [(samples from in_first on, in_first, final, factor, out_first, a_prev,
    s_prev, out_count)]; no GPU object is created then (the host-only plan / table entry points are
    still the library's)."""
    _NAME = "pitch"

    def __init__(self, device: int = 0, hop: int = 160, window: int = 640, lag_min: int = 32, lag_max: int = 320,
                 unvoiced: int = 80, theta: float = 0.2, floor: float = 1e-3, evaluator=None):
        self.device = int(device)
        self._desc = _ffi.PitchDesc(struct_size=ctypes.sizeof(_ffi.PitchDesc), hop=int(hop), window=int(window),
                                    lag_min=int(lag_min), lag_max=int(lag_max), unvoiced=int(unvoiced),
                                    theta=float(theta), floor=float(floor))
        super().__init__(evaluator)
        self.plan(0, False)  # (refuses a bad description before anything is built)
        self.hop, self.window = int(hop) or 160, int(window) or 640
        self.lag_min, self.lag_max, self.unvoiced = int(lag_min) or 32, int(lag_max) or 320, int(unvoiced) or 80
        self.theta, self.floor = F32(theta) or F32(0.2), F32(floor) or F32(1e-3)
        self.lookahead = self.window + 3 * self.lag_max  # samples an output waits for
        self.table = _pitch_table(self.lag_min, self.lag_max)
        self._create(self.table)

    @staticmethod
    def factor(semitones: float) -> float:
        f = pitch_factor(semitones)
        if not 0.5 <= f <= 2.0:  # (NaN fails)
            raise ValueError("a pitch shift must be in [-12, 12] semitones")
        return f

    # ---- host-only plan ----
    def plan(self, n_known: int, final: bool, out_first: int = 0, a_prev: int = 0, s_prev: int = 0):
        """(out_ready_end, in_first_needed) of rwkvtts_pitch_plan."""
        end, first = ctypes.c_int64(), ctypes.c_int64()
        _native("pitch_plan", ctypes.byref(self._desc), int(n_known), 1 if final else 0, int(out_first), int(a_prev),
                int(s_prev), ctypes.byref(end), ctypes.byref(first))
        return end.value, first.value

    # ---- the kernels ----
    def shift_windows(self, items) -> list:
        """[(samples from in_first on, in_first, final, factor, out_first, a_prev, s_prev, out_count)]
        -> [(outputs [out_first, + out_count) of the whole-signal result, a_last, s_last)], the state
        after each window's last output, all windows in one launch triple. Raises
        RwkvTtsError(EINVAL), with nothing computed, if a window asks for more than plan() allows."""
        items = [(np.ascontiguousarray(x, dtype=F32).reshape(-1), int(a), bool(fin), float(f), int(o), int(ap), int(sp),
                  int(c)) for x, a, fin, f, o, ap, sp, c in items]
        if self._evaluator is not None:
            for x, a, fin, f, o, ap, sp, c in items:  # the native call's own refusals, from the host-only plan
                if not 0.5 <= f <= 2.0:
                    raise _ffi.RwkvTtsError(_ffi.EINVAL, "pitch_windows")
                end, first = self.plan(a + x.size, fin, o, ap, sp)
                if c < 0 or (c > 0 and (o + c > end or a > first)):
                    raise _ffi.RwkvTtsError(_ffi.EINVAL, "pitch_windows")
            return [(np.ascontiguousarray(y, dtype=F32), int(al), int(sl)) for y, al, sl in self._evaluator(self, items)]
        ws, outs = self._windows("pitch_windows", _ffi.PitchWindow, items, factor=3, out_first=4, a_prev=5, s_prev=6)
        return [(o, int(w.a_last), int(w.s_last)) for o, w in zip(outs, ws)]

    def shift_batch(self, signals, semitones) -> list:
        """[signal], [semitones] -> [shifted signal], ragged, a shift per signal, in one launch triple;
        an empty signal gives an empty one."""
        xs = [np.ascontiguousarray(x, dtype=F32).reshape(-1) for x in signals]
        fs = [self.factor(s) for s in semitones]
        if len(xs) != len(fs):
            raise ValueError("shift_batch: one shift per signal")
        if self._evaluator is not None:
            return [y for y, _, _ in self.shift_windows([(x, 0, True, f, 0, 0, 0, x.size) for x, f in zip(xs, fs)])]
        if not xs:
            return []
        outs, ins, lens, ous = self._ragged(xs, [x.size for x in xs])
        self._call("pitch_batch", ins, lens, (ctypes.c_double * len(fs))(*fs), len(xs), ous)
        return outs

    def shift(self, x, semitones: float) -> np.ndarray:
        return self.shift_batch([x], [semitones])[0]

    def stream(self, semitones: float) -> "PitchStream":
        return PitchStream(self, semitones)

    def walk_ms(self) -> float:
        """HIP-event time of the last call's marks kernel alone (the serial walk)."""
        ms = ctypes.c_double()
        _native("pitch_walk_ms", self._h, ctypes.byref(ms))
        return ms.value


class PitchStream(_ExactStream):
    """PitchShifter.stream(semitones): feed(pcm_chunk, final=False) -> the outputs that became exact
    with it. The concatenation of what feed returns is bitwise PitchShifter.shift(the concatenated
    input, semitones), however the input was cut. An output goes out once window + 3 * lag_max samples
    after it are known (0.1 s at the defaults); the kept tail is what rwkvtts_pitch_plan asks for,
    fewer than window + 9 * lag_max + hop samples."""

    def __init__(self, shifter: PitchShifter, semitones: float):
        super().__init__()
        self.p = shifter
        self.f = shifter.factor(semitones)
        self._out_next = 0       # outputs [0, _out_next) went out
        self._state = (0, 0)     # (a, s) after them

    def _emit(self, n_known, final):
        a, s = self._state
        end, _ = self.p.plan(n_known, final, self._out_next, a, s)
        count = end - self._out_next
        if count <= 0:
            return np.zeros(0, dtype=F32)
        out, a, s = self.p.shift_windows([(self._tail, self._tail_first, final, self.f, self._out_next, a, s, count)])[0]
        self._state = (a, s)
        self._out_next += count
        return out

    def _first_needed(self, n_known):
        return self.p.plan(n_known, False, self._out_next, *self._state)[1]


# ---- provenance watermark on the GPU ---------------------------------------------------------
def _wm_table(taps: int, block: int, band_lo: float, band_hi: float, fs: float = 16000.0) -> np.ndarray:
    """h[0, taps) -- a Blackman-windowed band-pass, the difference of two windowed sincs, at unit
    energy -- then r[i] = (float)((i + 1) / block), in double: the table both sides read."""
    import math
    k = np.arange(taps, dtype=np.float64)
    t = k - float((taps - 1) // 2)
    w = (0.42 - 0.5 * np.cos(2.0 * np.pi * k / float(taps - 1))) + 0.08 * np.cos(4.0 * np.pi * k / float(taps - 1))
    fh, fl = 2.0 * float(band_hi) / fs, 2.0 * float(band_lo) / fs
    g = w * (fh * np.sinc(fh * t) - fl * np.sinc(fl * t))
    h = g / math.sqrt(float(np.sum(g * g)))
    r = np.arange(1, block + 1, dtype=np.float64) / float(block)
    return np.concatenate([h, r]).astype(F32)


def wm_strength(strength_db: float) -> np.float32:
    """s, the f32 amplitude of a strength in dB: 10^(strength_db / 20), taken in double
    (rwkvtts_wm_strength, host only); ValueError outside -60 .. -6."""
    s = F32(_ffi.lib().rwkvtts_wm_strength(float(strength_db)))
    if not np.isfinite(s):
        raise ValueError("a watermark strength must be in [-60, -6] dB")
    return s


class Watermarker(_NativeStage):
    """A provenance watermark as HIP kernels (csrc/wm.hip; the contract is in include/rwkvtts.h,
    DESIGN.md §30): a time-domain spread-spectrum mark on 16 kHz PCM. A +-1 chip sequence hashed from
    a 64-bit key, repeating every bits * bit_len samples and multiplied by the payload's bit of the
    moment, is shaped by a `taps`-long band-pass (band_lo .. band_hi Hz) and added at `strength_db`
    relative to the signal's own level, block by block, with a linear ramp over each block. n_out = n,
    silence stays silence, one causal definition, so a stream's pieces are bitwise the one-shot
    result (a lag of one block). The pipeline applies it last at 16 kHz: after the leveller, before
    the resampler. The detector whitens, matched-filters and folds a clip of any origin onto the
    period and tries every alignment; each bit's correlation is divided by the root of its own exact
    variance under random chips, so the score is chi-square with `bits` degrees of freedom where there
    is no mark under the key -- whatever the host, another key's mark included -- and `threshold` is
    set on that law (one false alarm in 10^6 clips).

    0 means the default as in the C desc: block 320 (one vocoder frame), taps 129, bits 16, bit_len
    1600 (100 ms; period 1.6 s), band 1000 .. 3400 Hz, strength -26 dB. Every default is untuned and
    nobody has listened to the output. The kernels read the table `_wm_table` builds.

    evaluator: a callable (marker, items) -> [(ndarray, a_last)] standing in for the native window
    call, items being [(samples from in_first on, in_first, final, s, key, payload, a_prev, block_first,
    out_count)]; detector: a callable (marker, [clip], [key]) -> [dict] standing in for the native
    detect call. No GPU object is created with an evaluator (the host-only entry points are still the
    library's)."""
    _NAME = "wm"

    def __init__(self, device: int = 0, block: int = 320, taps: int = 129, bits: int = 16, bit_len: int = 1600,
                 band_lo: float = 1000.0, band_hi: float = 3400.0, strength_db: float = -26.0, evaluator=None,
                 detector=None):
        self.device = int(device)
        self._desc = _ffi.WmDesc(struct_size=ctypes.sizeof(_ffi.WmDesc), block=int(block), taps=int(taps), bits=int(bits),
                                 bit_len=int(bit_len), band_lo=float(band_lo), band_hi=float(band_hi),
                                 strength_db=float(strength_db))
        super().__init__(evaluator)
        self._detector = detector
        self.plan(0, False)  # (refuses a bad description before anything is built)
        self.block, self.taps, self.bits = int(block) or 320, int(taps) or 129, int(bits) or 16
        self.bit_len = int(bit_len) or 1600
        self.period = self.bits * self.bit_len
        self.band_lo, self.band_hi = float(F32(band_lo)) or 1000.0, float(F32(band_hi)) or 3400.0
        self.strength_db = float(F32(strength_db)) or -26.0
        t = ctypes.c_double()
        _native("wm_threshold", ctypes.byref(self._desc), ctypes.byref(t))
        self.threshold = t.value
        self.table = _wm_table(self.taps, self.block, self.band_lo, self.band_hi)
        self._create(self.table)

    # ---- host-only plan ----
    def plan(self, n_known: int, final: bool, block_first: int = 0):
        """(out_ready_end, in_first_needed) of rwkvtts_wm_plan."""
        end, first = ctypes.c_int64(), ctypes.c_int64()
        _native("wm_plan", ctypes.byref(self._desc), int(n_known), 1 if final else 0, int(block_first),
                ctypes.byref(end), ctypes.byref(first))
        return end.value, first.value

    def _s(self, strength_db):
        return wm_strength(self.strength_db if strength_db is None else strength_db)

    def _payload(self, payload):
        if isinstance(payload, bool) or not isinstance(payload, (int, np.integer)) or not 0 <= int(payload) < 1 << self.bits:
            raise ValueError(f"a watermark payload must be an integer in [0, 2^{self.bits})")
        return int(payload)

    @staticmethod
    def _key(key):
        if isinstance(key, bool) or not isinstance(key, (int, np.integer)) or not 0 <= int(key) < 1 << 64:
            raise ValueError("a watermark key must be an integer in [0, 2^64)")
        return int(key)

    # ---- the embed kernel ----
    def embed_windows(self, items) -> list:
        """[(samples from in_first on, in_first, final, s, key, payload, a_prev, block_first, out_count)]
        -> [(outputs [block_first * block, + out_count) of the whole-signal result, a_last)], all windows
        in one launch; s is the f32 strength (wm_strength). Raises RwkvTtsError(EINVAL), with nothing
        computed, if a window asks for more than plan() allows."""
        items = [(np.ascontiguousarray(x, dtype=F32).reshape(-1), int(a), bool(f), float(F32(s)), self._key(k),
                  self._payload(p), float(F32(ap)), int(b), int(c)) for x, a, f, s, k, p, ap, b, c in items]
        if self._evaluator is not None:
            return [(np.ascontiguousarray(y, dtype=F32), F32(a)) for y, a in self._evaluator(self, items)]
        ws, outs = self._windows("wm_embed_windows", _ffi.WmWindow, items, strength=3, key=4, payload=5, a_prev=6,
                                 block_first=7)
        return [(o, F32(w.a_last)) for o, w in zip(outs, ws)]

    def embed_batch(self, signals, keys, payloads, strengths_db=None) -> list:
        """[signal], [key], [payload] (, [strength in dB]) -> [marked signal], ragged, in one launch; an
        empty signal gives an empty one."""
        xs = [np.ascontiguousarray(x, dtype=F32).reshape(-1) for x in signals]
        ks, ps = [self._key(k) for k in keys], [self._payload(p) for p in payloads]
        ss = [self._s(None)] * len(xs) if strengths_db is None else [self._s(v) for v in strengths_db]
        if not len(xs) == len(ks) == len(ps) == len(ss):
            raise ValueError("embed_batch: one key, one payload and one strength per signal")
        if self._evaluator is not None:
            return [y for y, _ in self.embed_windows([(x, 0, True, s, k, p, 0.0, 0, x.size)
                                                      for x, s, k, p in zip(xs, ss, ks, ps)])]
        if not xs:
            return []
        outs, ins, lens, ous = self._ragged(xs, [x.size for x in xs])
        self._call("wm_embed_batch", ins, lens, (ctypes.c_uint64 * len(ks))(*ks), (ctypes.c_uint32 * len(ps))(*ps),
                   (ctypes.c_float * len(ss))(*[float(s) for s in ss]), len(xs), ous)
        return outs

    def embed(self, x, key: int, payload: int, strength_db=None) -> np.ndarray:
        return self.embed_batch([x], [key], [payload], None if strength_db is None else [strength_db])[0]

    def stream(self, key: int, payload: int, strength_db=None) -> "WatermarkStream":
        return WatermarkStream(self, key, payload, strength_db)

    # ---- the detector ----
    def detect_batch(self, signals, keys, debug: bool = False) -> list:
        """[clip at 16 kHz], [key] -> [{detected, score, threshold, payload, seen, offset, min_z}], ragged,
        in one launch sequence. debug adds r and d, float32 [bits, period]: r_b(tau) and d_b(tau)."""
        xs = [np.ascontiguousarray(x, dtype=F32).reshape(-1) for x in signals]
        ks = [self._key(k) for k in keys]
        if len(xs) != len(ks):
            raise ValueError("detect_batch: one key per clip")
        if self._detector is not None:
            return [dict(d) for d in self._detector(self, xs, ks)]
        if self._evaluator is not None:
            raise RuntimeError("this Watermarker stands on an evaluator without a detector")
        if not xs:
            return []
        res = (_ffi.WmResult * len(xs))()
        dbg = []
        for r in res:
            r.struct_size = ctypes.sizeof(_ffi.WmResult)
            if debug:
                dbg.append((np.zeros((self.bits, self.period), dtype=F32), np.zeros((self.bits, self.period), dtype=F32)))
                r.dbg_r, r.dbg_d = dbg[-1][0].ctypes.data, dbg[-1][1].ctypes.data
        P = ctypes.c_void_p * len(xs)
        self._call("wm_detect_batch", P(*[x.ctypes.data for x in xs]), (ctypes.c_int64 * len(xs))(*[x.size for x in xs]),
                   (ctypes.c_uint64 * len(ks))(*ks), len(xs), res)
        out = []
        for i, r in enumerate(res):
            d = dict(detected=bool(r.detected), score=float(r.score), threshold=self.threshold, payload=int(r.payload),
                     seen=int(r.seen), offset=int(r.offset), min_z=float(r.min_z))
            if debug:
                d["r"], d["d"] = dbg[i]
            out.append(d)
        return out

    def detect(self, x, key: int, debug: bool = False) -> dict:
        return self.detect_batch([x], [key], debug)[0]


class WatermarkStream(_ExactStream):
    """Watermarker.stream(key, payload): feed(pcm_chunk, final=False) -> the blocks that became exact
    with it. The concatenation of what feed returns is bitwise Watermarker.embed(the concatenated
    input, key, payload), however the input was cut. A block goes out once it is complete, so the
    output lags the input by less than one block (20 ms at the default); the kept tail is shorter than
    a block, and the carried state is one float, the last block's amplitude."""

    def __init__(self, marker: Watermarker, key: int, payload: int, strength_db=None):
        super().__init__()
        self.m = marker
        self.key, self.payload, self.s = marker._key(key), marker._payload(payload), marker._s(strength_db)
        self._block_next = 0      # blocks [0, _block_next) went out
        self._a = F32(0.0)        # a of block _block_next - 1

    def _emit(self, n_known, final):
        B = self.m.block
        end, _ = self.m.plan(n_known, final, self._block_next)
        count = end - self._block_next * B
        if count <= 0:
            return np.zeros(0, dtype=F32)
        out, self._a = self.m.embed_windows([(self._tail, self._tail_first, final, self.s, self.key, self.payload,
                                              self._a, self._block_next, count)])[0]
        self._block_next += -(-count // B)
        return out

    def _first_needed(self, n_known):
        return self.m.plan(n_known, False, self._block_next)[1]


# ---- lossless compressed output on the GPU ---------------------------------------------------
FLAC_RATES = (8000, 16000, 22050, 24000, 32000, 44100, 48000)
FLAC_BLOCKS = (256, 512, 1024, 2048, 4096)


def _flac_table() -> np.ndarray:
    """The Q15 Welch windows of the five block sizes back to back, int32: w[i] = 32768 -
    floor(32768 d^2 / D^2), d = 2 i - B + 1, D = B + 1, in integers: the table both sides read."""
    rows = []
    for B in FLAC_BLOCKS:
        d = 2 * np.arange(B, dtype=np.int64) - B + 1
        rows.append(32768 - (32768 * d * d) // ((B + 1) * (B + 1)))
    return np.concatenate(rows).astype(np.int32)


def flac_default_block(rate: int) -> int:
    """1024 samples up to 24 kHz, 2048 above: at most 64 ms of lag in a stream."""
    return 1024 if int(rate) <= 24000 else 2048


class FlacEncoder(_NativeStage):
    """A FLAC encoder as HIP kernels (csrc/flac.hip; the contract is in include/rwkvtts.h, DESIGN.md
    §31): f32 PCM -> a standard mono 16-bit FLAC stream (RFC 9639, streamable subset, fixed block size)
    whose decoded samples are the int16 samples the WAV routes send, byte for byte. Per block the
    subframe is chosen by exact bit count among CONSTANT, FIXED orders 0 .. 4, LPC orders 1 .. 12 (12-bit
    coefficients from an integer-windowed autocorrelation) and VERBATIM, each with the best Rice
    partitioning. A frame depends on its own samples, its number, the rate and the block size only, so
    a stream's frames are byte for byte the one-shot frames (FlacStream). One call encodes a ragged
    batch -- a rate, a block size and a scale per signal -- in one launch pair; only the compressed
    bytes cross to the host. Pinned bitwise to its numpy restatement (tests/flac_ref.py) and read back
    by an independent decoder (rwkvtts.flac); unverified against libFLAC.

    evaluator: a callable (encoder, items) -> [(bytes, min_frame, max_frame)] standing in for the native
    call, items being [(samples, scale, rate, block, first_frame, final, lpc)]; no GPU object is created
    then (the host-only entry points are still the library's)."""
    _NAME = "flac"

    def __init__(self, device: int = 0, evaluator=None):
        self.device = int(device)
        super().__init__(evaluator)
        self.table = _flac_table()
        if self._evaluator is None:
            h = ctypes.c_void_p()
            _native("flac_create", self.device, self.table.ctypes.data_as(ctypes.c_void_p), ctypes.byref(h))
            self._h = h

    # ---- host only ----
    @staticmethod
    def bound(n: int, block: int) -> int:
        """The largest byte count n samples can give (rwkvtts_flac_bound)."""
        b = int(_ffi.lib().rwkvtts_flac_bound(int(n), int(block)))
        if b < 0:
            raise _ffi.RwkvTtsError(_ffi.EINVAL, "flac_bound")
        return b

    @staticmethod
    def header(rate: int, block: int, min_frame: int = 0, max_frame: int = 0, total: int = 0, md5=None) -> bytes:
        """"fLaC" and the STREAMINFO block, 42 bytes (rwkvtts_flac_streaminfo); the zeros of the
        defaults mean "unknown": the header of a stream."""
        out = (ctypes.c_uint8 * 42)()
        m = None if md5 is None else (ctypes.c_uint8 * 16)(*bytes(md5))
        _native("flac_streaminfo", int(rate), int(block), int(min_frame), int(max_frame), int(total), m, out)
        return bytes(out)

    @staticmethod
    def _check(rate, block):
        if rate not in FLAC_RATES:
            raise ValueError(f"FLAC output rate must be one of {FLAC_RATES}")
        if block not in FLAC_BLOCKS:
            raise ValueError(f"FLAC block size must be one of {FLAC_BLOCKS}")

    # ---- the kernels ----
    def encode_windows(self, items) -> list:
        """[(samples, scale, rate, block, first_frame, final, lpc)] -> [(the frames first_frame .. of
        that signal back to back, the smallest frame, the largest frame)], all windows in one launch
        pair. Without final the samples must be whole blocks. Raises RwkvTtsError(EINVAL), with nothing
        computed, on a window that breaks the rules."""
        items = [(np.ascontiguousarray(x, dtype=F32).reshape(-1), float(F32(s)), int(r), int(b), int(f), bool(fin),
                  bool(lpc)) for x, s, r, b, f, fin, lpc in items]
        if self._evaluator is not None:
            for x, s, r, b, f, fin, lpc in items:  # the native call's own refusals
                if (r not in FLAC_RATES or b not in FLAC_BLOCKS or (not fin and x.size % b) or f < 0
                        or f + -(-x.size // b) > 1 << 31 or not 0.0 <= s < float("inf")):
                    raise _ffi.RwkvTtsError(_ffi.EINVAL, "flac_encode")
            return [(bytes(y), int(a), int(b)) for y, a, b in self._evaluator(self, items)]
        if not items:
            return []
        ws = (_ffi.FlacWindow * len(items))()
        outs = []
        for w, (x, s, r, b, f, fin, lpc) in zip(ws, items):
            cap = 2 * x.size + 16 * -(-x.size // max(b, 1))
            out = np.empty(max(cap, 1), dtype=np.uint8)
            outs.append(out)
            w.struct_size = ctypes.sizeof(_ffi.FlacWindow)
            w.in_, w.n_in, w.scale, w.sample_rate, w.block_size = x.ctypes.data, x.size, s, r, b
            w.flags = (_ffi.FLAC_LAST if fin else 0) | (0 if lpc else _ffi.FLAC_NO_LPC)
            w.first_frame, w.out, w.out_cap = f, out.ctypes.data, cap
        self._call("flac_encode", ws, len(items))
        return [(out[:int(w.out_len)].tobytes(), int(w.min_frame), int(w.max_frame)) for w, out in zip(ws, outs)]

    def encode_batch(self, signals, rates, scales=None, blocks=None, lpc: bool = True) -> list:
        """[signal], [rate] (, [scale], [block]) -> [FLAC file], ragged, in one launch pair. Each file's
        STREAMINFO carries the true frame sizes, the sample count and the MD5 of the int16 samples."""
        import hashlib
        xs = [np.ascontiguousarray(x, dtype=F32).reshape(-1) for x in signals]
        rs = [int(r) for r in rates]
        ss = [1.0] * len(xs) if scales is None else [float(s) for s in scales]
        bs = [None] * len(xs) if blocks is None else list(blocks)
        if not len(xs) == len(rs) == len(ss) == len(bs):
            raise ValueError("encode_batch: one rate, one scale and one block size per signal")
        bs = [flac_default_block(r) if b is None else int(b) for r, b in zip(rs, bs)]
        for r, b in zip(rs, bs):
            self._check(r, b)
        res = self.encode_windows([(x, s, r, b, 0, True, lpc) for x, s, r, b in zip(xs, ss, rs, bs)])
        out = []
        for x, s, r, b, (frames, mn, mx) in zip(xs, ss, rs, bs, res):
            y = np.clip(x * F32(s), F32(-1.0), F32(1.0)) * F32(32767.0)
            md5 = hashlib.md5(np.trunc(y).astype("<i2").tobytes()).digest()
            out.append(self.header(r, b, mn, mx, x.size, md5) + frames)
        return out

    def encode(self, pcm, rate: int, scale: float = 1.0, block=None) -> bytes:
        return self.encode_batch([pcm], [rate], [scale], [block])[0]

    def stream(self, rate: int, block=None, scale: float = 1.0) -> "FlacStream":
        return FlacStream(self, rate, block, scale)


class FlacStream:
    """FlacStream(encoder, rate, block): feed(pcm_chunk, final=False) -> bytes. The first call's bytes
    begin with the stream header (STREAMINFO with unknown totals: the length is not known when it goes
    out); then frames as blocks complete, and with final the short last block. Fed in any chunking, the
    bytes are those of FlacEncoder.encode apart from STREAMINFO's totals. The carried state is the
    samples short of a block and the next frame number; the lag is under one block."""

    def __init__(self, encoder: FlacEncoder, rate: int, block=None, scale: float = 1.0):
        self.e, self.rate, self.scale = encoder, int(rate), float(scale)
        self.block = flac_default_block(self.rate) if block is None else int(block)
        encoder._check(self.rate, self.block)
        self._tail = np.zeros(0, dtype=F32)
        self._frame = 0
        self._header_sent = False
        self._closed = False

    def feed(self, pcm_chunk, final: bool = False) -> bytes:
        if self._closed:
            raise ValueError("the stream has ended (a chunk was fed with final=True)")
        x = np.asarray(pcm_chunk, dtype=F32).reshape(-1)
        if x.size:
            self._tail = np.concatenate([self._tail, x])
        out = b""
        if not self._header_sent:
            out, self._header_sent = self.e.header(self.rate, self.block), True
        take = self._tail.size if final else self._tail.size // self.block * self.block
        if take:
            frames, _, _ = self.e.encode_windows([(self._tail[:take], self.scale, self.rate, self.block, self._frame,
                                                   final, True)])[0]
            out += frames
            self._frame += -(-take // self.block)
            self._tail = self._tail[take:].copy()
        if final:
            self._closed = True
        return out


# ---- pause control on the GPU ----------------------------------------------------------------
class PauseShaper(_NativeStage):
    """Silences capped as HIP kernels (csrc/pause.hip; the arithmetic contract is in include/rwkvtts.h,
    DESIGN.md §35): a block of `block` samples is loud if a sample of it passes `threshold`, active if
    a block within `hang` of it is loud; a run of non-active blocks is cut when it is longer than M
    inside the signal (head M - M // 2 and tail M // 2 kept), longer than M // 2 at the start (tail
    kept) or longer than M - M // 2 at the end (head kept), and each kept edge of a cut is faded over
    `fade` samples. Everything else is copied bit for bit, so the output is a subsequence of the input
    but for the faded samples, and n_out <= n: the first stage whose output length depends on the data.
    One-shot, batched with a cap per signal, and exact over stream chunks. The pipeline applies it at
    16 kHz, first of the stages. A cap is in milliseconds at `rate` (shape_batch) or in samples.

    0 means the default as in the C desc: block 160 (10 ms), hang 5, fade 80, threshold 0.01 (the
    join's). Every default, and the half-and-half split of M, is untuned and nobody has listened to the
    output: the repository has no real checkpoint. The kernels read the table `_join_ramp` builds.

    evaluator: a callable (shaper, items) -> [(ndarray, block_next, seen, quiet, in_first_needed,
    n_cuts)] standing in for the native window call, items being [(samples from in_first on, in_first,
    final, M, block_next, seen, quiet)]; no GPU object is created then (the host-only ramp entry point
    is still the library's)."""
    _NAME = "pause"

    def __init__(self, device: int = 0, block: int = 160, hang: int = 5, fade: int = 80, threshold: float = 0.01,
                 evaluator=None, rate: int = 16000):
        self.device, self.rate = int(device), int(rate)
        self._desc = _ffi.PauseDesc(struct_size=ctypes.sizeof(_ffi.PauseDesc), block=int(block), hang=int(hang),
                                    fade=int(fade), threshold=float(threshold))
        super().__init__(evaluator)
        self.block, self.hang, self.fade = int(block) or 160, int(hang) or 5, int(fade) or 80
        self.threshold = float(F32(threshold)) or float(F32(0.01))
        probe = np.zeros(self.fade if 1 <= self.fade <= 4096 else 1, dtype=F32)
        _native("pause_ramp", ctypes.byref(self._desc), probe.ctypes.data_as(ctypes.c_void_p))  # (refuses a bad description)
        self.table = _join_ramp(self.fade)
        self.cuts = []  # the cuts of each signal of the last shape_* call
        self._create(self.table)

    def samples(self, max_pause_ms) -> int:
        """M, the cap in samples at the shaper's rate; ValueError below 2 * fade."""
        if isinstance(max_pause_ms, bool) or not isinstance(max_pause_ms, (int, np.integer)):
            raise ValueError("max_pause must be an integer number of milliseconds")
        m = int(max_pause_ms) * self.rate // 1000
        if not 2 * self.fade <= m <= 1 << 30:
            raise ValueError(f"max_pause gives {m} samples, outside [2 * fade, 2^30]")
        return m

    def kept_bound(self, m: int) -> int:
        """What a stream keeps at most: M + (2 * hang + 2) * block samples."""
        return int(m) + (2 * self.hang + 2) * self.block

    # ---- the kernels ----
    def shape_windows(self, items) -> list:
        """[(samples from in_first on, in_first, final, M, block_next, seen, quiet)] -> [(what the
        window decides beyond its state -- bitwise the whole-signal result, whatever follows --
        block_next, seen, quiet, in_first_needed, n_cuts)], all windows in one launch triple. Raises
        RwkvTtsError(EINVAL), with nothing computed, for an M outside [2 * fade, 2^30], samples that
        start after the state's in_first_needed, or a state no scan can have left."""
        items = [(np.ascontiguousarray(x, dtype=F32).reshape(-1), int(a), bool(f), int(m), int(c), int(s), int(q))
                 for x, a, f, m, c, s, q in items]
        if self._evaluator is not None:
            for x, a, f, m, c, s, q in items:  # the native call's own refusals
                B = self.block
                ok = (2 * self.fade <= m <= 1 << 30 and a >= 0 and c >= 0 and s in (0, 1) and q >= 0 and q % B == 0
                      and ((c >= 1 and q <= (c - 1) * B) if s else q == c * B) and c * B <= a + x.size)
                if not ok:
                    raise _ffi.RwkvTtsError(_ffi.EINVAL, "pause_windows")
            res = [(np.ascontiguousarray(y, dtype=F32), int(c), int(s), int(q), int(need), int(cuts))
                   for y, c, s, q, need, cuts in self._evaluator(self, items)]
        else:
            ws = (_ffi.PauseWindow * len(items))()
            outs = [np.empty(x.size, dtype=F32) for x, *_ in items]
            for w, (x, a, f, m, c, s, q), out in zip(ws, items, outs):
                w.struct_size = ctypes.sizeof(_ffi.PauseWindow)
                w.in_, w.in_first, w.n_in, w.final = x.ctypes.data, a, x.size, 1 if f else 0
                w.max_pause_samples, w.block_next, w.seen, w.quiet = m, c, s, q
                w.out, w.out_cap = out.ctypes.data, out.size
            if items:
                self._call("pause_windows", ws, len(items))
            res = [(out[:int(w.out_count)].copy(), int(w.block_last), int(w.seen_last), int(w.quiet_last),
                    int(w.in_first_needed), int(w.n_cuts)) for w, out in zip(ws, outs)]
        self.cuts = [r[5] for r in res]
        return res

    def shape_samples_batch(self, signals, caps) -> list:
        """[signal], [M in samples] -> [shaped signal], ragged, a cap per signal, in one launch triple;
        an empty signal gives an empty one. self.cuts: the cuts made in each."""
        xs = [np.ascontiguousarray(x, dtype=F32).reshape(-1) for x in signals]
        ms = [int(m) for m in caps]
        if len(xs) != len(ms):
            raise ValueError("shape_batch: one cap per signal")
        if self._evaluator is not None:
            return [r[0] for r in self.shape_windows([(x, 0, True, m, 0, 0, 0) for x, m in zip(xs, ms)])]
        if not xs:
            self.cuts = []
            return []
        outs, ins, lens, ous = self._ragged(xs, [x.size for x in xs])
        n_out, n_cuts = (ctypes.c_int64 * len(xs))(), (ctypes.c_int64 * len(xs))()
        self._call("pause_batch", ins, lens, (ctypes.c_int64 * len(ms))(*ms), len(xs), ous, n_out, n_cuts)
        self.cuts = [int(c) for c in n_cuts]
        return [o[:int(n)].copy() for o, n in zip(outs, n_out)]

    def shape_batch(self, pcm, max_pause_ms) -> list:
        """[signal], a cap in ms for all (or one per signal) -> [shaped signal] (shape_samples_batch)."""
        pcm = list(pcm)
        caps = list(max_pause_ms) if isinstance(max_pause_ms, (list, tuple)) else [max_pause_ms] * len(pcm)
        return self.shape_samples_batch(pcm, [self.samples(m) for m in caps])

    def shape(self, x, max_pause_ms) -> np.ndarray:
        return self.shape_batch([x], max_pause_ms)[0]

    def stream(self, max_pause_ms) -> "PauseStream":
        return PauseStream(self, self.samples(max_pause_ms))


class PauseStream(_ExactStream):
    """PauseShaper.stream(max_pause_ms): feed(pcm_chunk, final=False) -> the samples that became exact
    with it (often none: leading silence is withheld, and the last `fade` samples of a kept head wait
    until the run has ended or passed M). The concatenation of what feed returns is bitwise
    PauseShaper.shape(the concatenated input), however the input was cut. The state is three integers
    and no samples; the kept tail is what the window call asks for, never more than
    M + (2 * hang + 2) * block samples however long a silence (checked on every feed). cuts: the cuts
    made so far."""

    def __init__(self, shaper: PauseShaper, m: int):
        super().__init__()
        self.p, self.m = shaper, int(m)
        if not 2 * shaper.fade <= self.m <= 1 << 30:
            raise ValueError("the cap must be in [2 * fade, 2^30] samples")
        self._state = (0, 0, 0)  # (block_next, seen, quiet)
        self._need = 0
        self.cuts = 0

    def _emit(self, n_known, final):
        out, c, s, q, self._need, cuts = self.p.shape_windows([(self._tail, self._tail_first, final, self.m,
                                                                *self._state)])[0]
        self._state = (c, s, q)
        self.cuts += cuts
        return out

    def _first_needed(self, n_known):
        return self._need

    def feed(self, pcm_chunk, final: bool = False) -> np.ndarray:
        out = super().feed(pcm_chunk, final)
        if self.kept > self.p.kept_bound(self.m):
            raise RuntimeError(f"pause stream keeps {self.kept} samples, above its bound {self.p.kept_bound(self.m)}")
        return out


# ---- normalisation / trimming ------------------------------------------------------------
def audio_volume_normalize(audio, coeff: float = 0.2) -> np.ndarray:
    x = np.asarray(audio, dtype=F32).copy()
    temp = np.sort(np.abs(x))
    if temp.size and temp[-1] < F32(0.1):
        sf = max(temp[-1], F32(1e-3))
        x = x / F32(sf) * F32(0.1)
    temp = temp[temp > F32(0.01)]
    n = temp.size
    if n <= 10:
        return x
    a, b = int(F32(0.9) * F32(n)), int(F32(0.99) * F32(n))
    vol = F32(0.0)
    for v in temp[a:b]:  # sequential f32 sum (Iterator::sum)
        vol = F32(vol + v)
    vol = F32(vol / F32(b - a))
    scale = F32(min(max(F32(coeff) / vol, F32(0.1)), F32(10.0)))
    x = x * scale
    mx = F32(np.max(np.abs(x))) if x.size else F32(0)
    if mx > 1.0:
        x = x / mx
    return x


def detect_silence(audio, threshold: float) -> Tuple[int, int]:
    a = np.abs(np.asarray(audio, dtype=F32))
    n = a.size
    if n == 0:
        return 0, 0
    loud = np.nonzero(a > F32(threshold))[0]
    if loud.size == 0:
        return n // 2, n - n // 2
    start, end = int(loud[0]), int(n - 1 - loud[-1])
    if start + end >= n:
        return n // 2, n - n // 2
    return start, end


def trim_silence_only(audio, silence_threshold: float = 0.01) -> np.ndarray:
    x = np.asarray(audio, dtype=F32)
    s, e = detect_silence(x, silence_threshold)
    a, b = min(s, x.size), max(x.size - e, 0)
    if a >= b:
        return np.zeros(x.size, dtype=F32)
    return x[a:b].copy()


def zero_mean_unit_variance_normalize(values) -> np.ndarray:
    x = np.asarray(values, dtype=F32).copy()
    if x.size == 0:
        return x
    if x.size == 1:
        x[0] = 0.0
        return x
    s = F32(0.0)
    for v in x:
        s = F32(s + v)
    mean = F32(s / F32(x.size))
    if np.all(np.abs(x - mean) < F32(1e-10)):
        return np.zeros_like(x)
    acc = F32(0.0)
    for v in x:
        d = F32(v - mean)
        acc = F32(acc + F32(d * d))
    std = F32(np.sqrt(F32(F32(acc / F32(x.size)) + F32(1e-7))))
    return ((x - mean) / std).astype(F32)


def get_ref_clip(wav, sample_rate: int = 16000, ref_segment_duration: float = 6.0, hop: int = 320) -> np.ndarray:
    x = np.asarray(wav, dtype=F32)
    seg = int(F32(ref_segment_duration) * F32(sample_rate)) // hop * hop
    if seg > x.size:
        reps = seg // x.size + 1
        return np.tile(x, reps)[:seg].copy()
    return x[:seg].copy()


def read_flac(path: str) -> Tuple[np.ndarray, int, int]:
    """A mono 16-bit FLAC file -> (f32 samples as s / 2^15, sample_rate, 1), through rwkvtts.flac.decode
    (no reference counterpart: the reference reads WAV and MP3)."""
    from . import flac
    with open(path, "rb") as f:
        pcm, sr = flac.decode(f.read())
    return pcm.astype(F32) / F32(32768.0), sr, 1


def load_audio(path: str, target_sr: int = 16000, volume_normalize: bool = True, device=None) -> np.ndarray:
    """device: None resamples with the numpy restatement, an integer on that GPU (Resampler). A file
    that begins with "fLaC" is read as FLAC (read_flac), whatever its name."""
    import os
    if not os.path.exists(path):
        raise FileNotFoundError(path)
    size = os.path.getsize(path)
    if size == 0 or size > 100 * 1024 * 1024:
        raise ValueError("audio file empty or larger than 100 MB")
    if path.lower().endswith(".mp3"):
        raise NotImplementedError("MP3 decoding (symphonia) is not available")
    with open(path, "rb") as f:
        is_flac = f.read(4) == b"fLaC"
    x, sr, ch = read_flac(path) if is_flac else read_wav(path)
    if x.size == 0 or x.size < ch:
        raise ValueError("no audio samples")
    if x.size < int(F32(sr) * F32(0.1)):
        raise ValueError("audio shorter than 0.1 s")
    if ch > 1:
        x = x[::ch].copy()
    if sr != target_sr:
        x = resample_audio_high_quality(x, sr, target_sr, device=device)
    if volume_normalize:
        x = audio_volume_normalize(x, 0.2)
    return trim_silence_only(x, 0.01)
