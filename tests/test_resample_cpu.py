"""The resampler's host side without a GPU: the exported plan / out_len / table entry points against
the contract of include/rwkvtts.h, Resampler.stream()'s bookkeeping driven by the numpy restatement
of the contract (tests/test_gpu_resample.py), and `sample_rate` in the server's handlers with
stand-in pipelines. The kernel itself is tested in tests/test_gpu_resample.py."""
import base64
import ctypes
import inspect
import json
import struct

import numpy as np
import pytest

from rwkvtts import _ffi, audio
from rwkvtts import server as SV
from rwkvtts.pipeline import SpeechChunk
from test_gpu_resample import bits, contract_out_len, contract_positions, contract_resample

F32 = np.float32
RATES = [(16000, 48000), (16000, 8000), (16000, 44100), (44100, 16000), (48000, 16000)]
ALIGNS = ["zero", "rubato"]
L, O = 256, 256


def _desc(sr_in, sr_out, align, sinc_len=L, oversampling=O, f_cutoff=0.95):
    return _ffi.ResampleDesc(struct_size=ctypes.sizeof(_ffi.ResampleDesc), sr_in=sr_in, sr_out=sr_out,
                             sinc_len=sinc_len, oversampling=oversampling, f_cutoff=f_cutoff,
                             align=_ffi.RESAMPLE_ALIGN_ZERO if align == "zero" else _ffi.RESAMPLE_ALIGN_RUBATO)


def _plan(desc, n_known, final, out_first):
    end, first = ctypes.c_int64(-1), ctypes.c_int64(-1)
    rc = _ffi.lib().rwkvtts_resample_plan(ctypes.byref(desc), n_known, 1 if final else 0, out_first,
                                          ctypes.byref(end), ctypes.byref(first))
    assert rc == _ffi.OK
    return end.value, first.value


def test_exports_and_out_len():
    lib = _ffi.lib()
    for name in ("rwkvtts_resample_sincs", "rwkvtts_resample_out_len", "rwkvtts_resample_plan",
                 "rwkvtts_resampler_create", "rwkvtts_resampler_destroy", "rwkvtts_resample_batch",
                 "rwkvtts_resample_windows"):
        assert name in _ffi.EXPORTS and hasattr(lib, name)
    for sr_in, sr_out in RATES:
        d = _desc(sr_in, sr_out, "zero")
        for n in (0, 1, 319, 320, 5120):
            assert lib.rwkvtts_resample_out_len(ctypes.byref(d), n) == int(np.ceil(n * (sr_out / sr_in)))
    # defaults (0 = 256 / 256 / 0.95) and refusals, before anything touches a GPU
    assert lib.rwkvtts_resample_out_len(ctypes.byref(_desc(16000, 48000, "zero", 0, 0, 0.0)), 10) == 30
    for bad in (_desc(0, 16000, "zero"), _desc(16000, 192001, "zero"), _desc(16000, 8000, "zero", sinc_len=12),
                _desc(16000, 8000, "zero", sinc_len=1032), _desc(16000, 8000, "zero", oversampling=1025),
                _desc(16000, 8000, "zero", f_cutoff=1.5)):
        assert lib.rwkvtts_resample_out_len(ctypes.byref(bad), 10) == -1
        assert lib.rwkvtts_resample_plan(ctypes.byref(bad), 10, 0, 0, None, None) == _ffi.EINVAL
        h = ctypes.c_void_p()
        assert lib.rwkvtts_resampler_create(0, ctypes.byref(bad), None, ctypes.byref(h)) == _ffi.EINVAL and not h.value
    short = _desc(16000, 8000, "zero")
    short.struct_size = 8
    assert lib.rwkvtts_resample_out_len(ctypes.byref(short), 10) == -1
    d = _desc(16000, 8000, "bad")
    d.align = 2
    assert lib.rwkvtts_resample_plan(ctypes.byref(d), 10, 0, 0, None, None) == _ffi.EINVAL


@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("sr_in,sr_out", RATES)
def test_plan_equals_brute_force(sr_in, sr_out, align):
    """out_ready_end / in_first_needed against an enumeration of every output's tap indices:
    output o reads samples start(o) - L/2 + 1 .. start(o) + L/2."""
    d = _desc(sr_in, sr_out, align)
    n_max = 5120
    o = np.arange(contract_out_len(n_max, sr_in, sr_out) + 4, dtype=np.int64)
    start, _, _ = contract_positions(o, sr_in, sr_out, L, O, align)
    low, high = start - L // 2 + 1, start + L // 2
    assert np.all(np.diff(start) >= 0)
    prev = 0
    for n_known in list(range(0, 700)) + [1000, 2047, 2048, 4095, 5119, 5120]:
        cap = contract_out_len(n_known, sr_in, sr_out)
        past = np.nonzero(high[:cap] >= n_known)[0]      # outputs with a tap at sample n_known or later
        want = int(past[0]) if past.size else cap        # (never more than the signal would have if it ended here)
        end, _ = _plan(d, n_known, False, 0)
        assert end == want, (n_known, end, want)
        assert end >= prev                               # monotone in n_known
        prev = end
        assert _plan(d, n_known, True, 0)[0] == cap      # final: out_len
        # every output before `end` has all its taps inside [.., n_known)
        assert end == 0 or high[end - 1] < n_known
    for out_first in (0, 1, 2, 100, 767, 768, 1700, int(o[-1])):
        assert _plan(d, n_max, False, out_first)[1] == max(0, int(low[out_first])), out_first
    firsts = [_plan(d, n_max, False, k)[1] for k in range(0, 3000, 7)]
    assert firsts == sorted(firsts)


@pytest.mark.parametrize("sr_in,sr_out", RATES)
def test_library_table_against_make_sincs(sr_in, sr_out):
    """rwkvtts_resample_sincs and audio._make_sincs evaluate the same expressions; they differ in the
    normalising sum alone (pairwise f32 in numpy, double in the library). That sum's relative error
    is at most 16 * 2^-24 * sum|y| / |sum y| (the ratio is the same for the normalised table), and
    the quotient's rounding adds one f32 ulp per entry."""
    ratio = sr_out / sr_in
    ref = audio._make_sincs(L, O, 0.95 if ratio >= 1.0 else 0.95 * ratio)
    got = np.empty((O, L), F32)
    d = _desc(sr_in, sr_out, "zero")
    assert _ffi.lib().rwkvtts_resample_sincs(ctypes.byref(d), got.ctypes.data_as(ctypes.c_void_p)) == _ffi.OK
    r64 = ref.astype(np.float64)
    rel = 16.0 * 2.0 ** -24 * np.abs(r64).sum() / abs(r64.sum())
    bound = rel * np.abs(r64) + np.spacing(np.abs(ref)).astype(np.float64)
    diff = np.abs(got.astype(np.float64) - r64)
    print(f"{sr_in}->{sr_out}: rel bound {rel:.3e}, max diff / bound {np.max(diff / bound):.3f}, "
          f"bitwise equal entries {np.mean(bits(got) == bits(ref)):.4f}")
    assert np.all(diff <= bound)
    assert abs(got.astype(np.float64).sum() / O - 1.0) < 1e-5    # unit DC gain per table on average


def _contract_evaluator(log):
    """Stands in for rwkvtts_resample_windows: the numpy contract, plus the check the native call
    makes -- no tap of a requested output outside the given samples, except below 0 or (final) past
    the end."""
    def run(r, items):
        outs = []
        for x, in_first, final, out_first, count in items:
            if count == 0:   # (as the native call: nothing to do)
                outs.append(np.zeros(0, F32))
                continue
            o = np.arange(out_first, out_first + count, dtype=np.int64)
            start, _, _ = contract_positions(o, r.sr_in, r.sr_out, r.sinc_len, r.oversampling, r.align)
            assert max(0, int(start[0]) - r.sinc_len // 2 + 1) >= in_first
            assert final or int(start[-1]) + r.sinc_len // 2 < in_first + x.size
            log.append((in_first, x.size, final, out_first, count))
            outs.append(contract_resample(x, r.sincs, r.sr_in, r.sr_out, r.align, out_first, count, in_first))
        return outs
    return run


@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("sr_in,sr_out", [(16000, 48000), (16000, 8000), (16000, 44100), (44100, 16000)])
def test_stream_bookkeeping(sr_in, sr_out, align):
    log = []
    r = audio.Resampler(sr_in, sr_out, align=align, evaluator=_contract_evaluator(log))
    assert r._h is None
    sizes = [1, 7, 5120, 319, 1, 1, 319, 7, 5120, 7, 319, 1]
    x = (np.random.default_rng(5).standard_normal(sum(sizes)) * 0.3).astype(F32)
    whole = r.resample(x)
    assert whole.size == contract_out_len(x.size, sr_in, sr_out)
    keep_max = L + int(np.ceil(sr_in / sr_out)) + 1
    for last_is_empty in (False, True):
        st, parts, pos = r.stream(), [], 0
        for i, n in enumerate(sizes):
            final = (i == len(sizes) - 1) and not last_is_empty
            parts.append(st.feed(x[pos:pos + n], final=final))
            pos += n
            assert st.kept <= keep_max, (st.kept, keep_max)
        if last_is_empty:
            parts.append(st.feed(np.zeros(0, F32), final=True))
        got = np.concatenate(parts)
        assert got.dtype == F32 and np.array_equal(bits(got), bits(whole)), (sr_in, sr_out, align, last_is_empty)
        assert st.kept == 0
        with pytest.raises(ValueError):
            st.feed(x[:1])
    # the 1- and 7-sample chunks at the start are below the look-ahead: nothing went to the evaluator
    assert all(c > 0 for *_, c in log)
    # a signal shorter than one tap window, and an empty one
    for n in (0, 1, 100):
        st = r.stream()
        got = np.concatenate([st.feed(x[:n // 2]), st.feed(x[n // 2:n], final=True)])
        assert np.array_equal(bits(got), bits(r.resample(x[:n])))


# ---- server: stand-in pipelines in the style of tests/test_server.py -------------------------------
class PlainPipeline:
    """The pipeline surface as it was before `sample_rate` existed: any extra keyword is a TypeError."""
    def __init__(self):
        self.calls = []

    def generate_speech(self, args):
        self.calls.append(("generate_speech", args))
        return np.linspace(-0.5, 0.5, 960, dtype=F32)

    def stream_speech(self, args, chunk_frames=16):
        self.calls.append(("stream_speech", args, chunk_frames))
        for i in range(2):
            yield SpeechChunk.make(np.full(320, 0.25 * (i + 1), F32), i, i + 1, 2, i == 1)


class RatePipeline(PlainPipeline):
    def generate_speech(self, args, sample_rate=None):
        self.calls.append(("generate_speech", args, sample_rate))
        sample_rate = sample_rate or 16000
        return np.linspace(-0.5, 0.5, 960 * sample_rate // 16000, dtype=F32)

    def stream_speech(self, args, chunk_frames=16, sample_rate=None):
        self.calls.append(("stream_speech", args, chunk_frames, sample_rate))
        sample_rate = sample_rate or 16000
        for i in range(2):
            yield SpeechChunk.make(np.full(320 * sample_rate // 16000, 0.25 * (i + 1), F32), i, i + 1, 2, i == 1)


def _stream_header(rate):
    return (b"RIFF" + struct.pack("<I", 0xFFFFFFFF) + b"WAVE" + b"fmt " +
            struct.pack("<IHHIIHH", 16, 1, 1, rate, 2 * rate, 2, 16) + b"data" + struct.pack("<I", 0xFFFFFFFF))


def test_server_without_sample_rate_is_unchanged():
    for body in ({"text": "hi", "seed": 3}, {"text": "hi", "seed": 3, "sample_rate": 16000},
                 {"text": "hi", "seed": 3, "sample_rate": None}):
        p = PlainPipeline()
        code, out = SV.handle_tts_json(json.dumps(body), p)
        assert code == 200 and out["success"]
        assert base64.b64decode(out["audio_base64"]) == SV.convert_samples_to_wav(np.linspace(-0.5, 0.5, 960, dtype=F32), 16000)
        assert len(p.calls) == 1 and len(p.calls[0]) == 2 and p.calls[0][1].seed == 3   # called with args alone
        code, it = SV.handle_tts_stream(body, p, chunk_frames=4)
        parts = list(it)
        assert code == 200 and parts[0] == _stream_header(16000)
        assert b"".join(parts[1:]) == SV.samples_to_pcm16(np.concatenate([np.full(320, 0.25, F32), np.full(320, 0.5, F32)]))
        assert p.calls[1][0] == "stream_speech" and p.calls[1][2] == 4 and len(p.calls[1]) == 3
    assert "sample_rate" not in inspect.signature(PlainPipeline.generate_speech).parameters


def test_server_sample_rate():
    p = RatePipeline()
    code, out = SV.handle_tts_json({"text": "hi", "sample_rate": 24000}, p)
    assert code == 200 and out["success"]
    wav = base64.b64decode(out["audio_base64"])
    assert struct.unpack("<II", wav[24:32]) == (24000, 48000)
    assert len(wav) == 48 + 2 * 1440 and p.calls[-1][2] == 24000
    assert wav == SV.convert_samples_to_wav(np.linspace(-0.5, 0.5, 1440, dtype=F32), 24000)
    code, it = SV.handle_tts_stream({"text": "hi", "sample_rate": 24000}, p, chunk_frames=8)
    parts = list(it)
    assert code == 200 and parts[0] == _stream_header(24000) and struct.unpack("<II", parts[0][24:32]) == (24000, 48000)
    assert len(b"".join(parts[1:])) == 2 * 2 * 480 and p.calls[-1][2:] == (8, 24000)
    for rate in SV.SAMPLE_RATES:
        assert SV.handle_tts_json({"text": "hi", "sample_rate": rate}, RatePipeline())[0] == 200
    assert SV.SAMPLE_RATES == (8000, 16000, 22050, 24000, 32000, 44100, 48000)
    # anything else: a 400 in the handler's JSON error shape, and the pipeline is never called
    for bad in (12345, 0, -8000, 24000.0, "24000", True, [24000]):
        q = RatePipeline()
        code, out = SV.handle_tts_json({"text": "hi", "sample_rate": bad}, q)
        assert code == 400 and out["success"] is False and set(out) == {"success", "error"} and q.calls == []
        code, it = SV.handle_tts_stream({"text": "hi", "sample_rate": bad}, q)
        assert code == 400 and json.loads(b"".join(it).decode("utf-8")) == out and q.calls == []
    assert SV.calculate_rtf(np.zeros(24000), 0.5, 24000) == 0.5 and SV.calculate_rtf(np.zeros(16000), 0.5) == 0.5


def test_pipeline_sample_rate_none_creates_nothing():
    """sample_rate None / 16000: no resampler, the stand-in codec's PCM as it is (tests/test_server.py's
    stand-ins know nothing of resampling)."""
    from rwkvtts.pipeline import LightweightTtsPipeline, LightweightTtsPipelineArgs
    from test_server import FakeCodec, FakeManager
    pipe = LightweightTtsPipeline(FakeManager(), FakeCodec())
    a = LightweightTtsPipelineArgs(text="hi")
    for rate in (None, 16000):
        assert np.array_equal(pipe.generate_speech(a, sample_rate=rate), pipe.generate_speech(a))
        assert len(pipe.generate_speech_batch([a, a], sample_rate=rate)) == 2
        assert pipe.resampler(rate) is None
    assert pipe._resamplers == {}
    sil = pipe.generate_speech(LightweightTtsPipelineArgs(text="\U0001F600"))
    assert sil.shape == (16000,)
