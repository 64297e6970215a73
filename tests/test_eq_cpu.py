"""The equaliser's design (include/rwkvtts.h) on the CPU against an analytic reference and
tests/eq_ref.py, EqStream over the restatement, and `eq` through the pipeline's stage fold and the server's
validation."""
import inspect
import json

import numpy as np
import pytest

import eq_ref as R
from rwkvtts import audio
from rwkvtts import server as SV
from rwkvtts.pipeline import LightweightTtsPipeline, LightweightTtsPipelineArgs, audio_stages
from test_pitch_cpu import FakePipeline

F32, bits = np.float32, R.bits
EIGHT = [("lowshelf", 120, 6, 0.7), ("peak", 400, -4, 2), ("peak", 1000, 3, 1.5), ("peak", 2000, -2, 3),
         ("peak", 3000, 5, 4), ("highshelf", 6000, -6, 0.7), ("highpass", 80, 0, 0.7071), ("lowpass", 7000, 0, 0.7071)]
BAD = ["phone", [], [("peak", 1000, 3, 1)] * 9, [("notch", 1000, 3, 1)], [("peak", 49, 3, 1)], [("peak", 7601, 3, 1)],
       [("peak", 1000, 18.5, 1)], [("peak", 1000, 3, 0.2)], [("peak", 1000, 3, 4.5)], [("peak", float("nan"), 3, 1)],
       [("peak", 1000, True, 1)], [("peak", 1000, 3)], 3.0, [("highpass", 50, 0, 4)]]


@pytest.mark.parametrize("spec", list(audio.EQ_PROFILES) + [EIGHT])
def test_the_taps_have_the_cascades_analytic_response_and_the_restatements_length(spec):
    """H(z) = prod (b0 + b1 z^-1 + b2 z^-2) / (a0 + a1 z^-1 + a2 z^-2), from the cookbook formulas written out
    here; the bound is 2^-22 sum|h64|: the truncation tail (2^-24) plus the taps' f32 rounding (2^-24), doubled
    for libm differences in the coefficients."""
    bands = audio.eq_bands(spec)
    h = audio.Equaliser.design(spec)
    ref, total = R.design(bands)
    assert h.dtype == F32 and h.size == ref.size and h.size % 64 == 0 and np.array_equal(bits(h), bits(ref))
    f = np.geomspace(20.0, 7900.0, 64)
    z1 = np.exp(-2j * np.pi * f / 16000.0)
    H = np.ones(64, dtype=np.complex128)
    for kind, f0, gain, q in bands:
        w, A = 2 * np.pi * f0 / 16000.0, 10.0 ** (gain / 40.0)
        c, al = np.cos(w), np.sin(w) / (2 * q)
        s = 2 * np.sqrt(A) * al
        b, a = {"peak": ((1 + al * A, -2 * c, 1 - al * A), (1 + al / A, -2 * c, 1 - al / A)),
                "lowpass": (((1 - c) / 2, 1 - c, (1 - c) / 2), (1 + al, -2 * c, 1 - al)),
                "highpass": (((1 + c) / 2, -(1 + c), (1 + c) / 2), (1 + al, -2 * c, 1 - al)),
                "lowshelf": ((A * ((A + 1) - (A - 1) * c + s), 2 * A * ((A - 1) - (A + 1) * c), A * ((A + 1) - (A - 1) * c - s)),
                             ((A + 1) + (A - 1) * c + s, -2 * ((A - 1) + (A + 1) * c), (A + 1) + (A - 1) * c - s)),
                "highshelf": ((A * ((A + 1) + (A - 1) * c + s), -2 * A * ((A - 1) + (A + 1) * c), A * ((A + 1) + (A - 1) * c - s)),
                              ((A + 1) - (A - 1) * c + s, 2 * ((A - 1) - (A + 1) * c), (A + 1) - (A - 1) * c - s))}[kind]
        H *= (b[0] + b[1] * z1 + b[2] * z1 * z1) / (a[0] + a[1] * z1 + a[2] * z1 * z1)
    dft = (h.astype(np.float64)[None, :] * z1[:, None] ** np.arange(h.size)[None, :]).sum(axis=1)
    err = float(np.max(np.abs(dft - H)))
    print(f"eq design: N {h.size}, largest response error {err:.3e}, bound {2.0 ** -22 * total:.3e}")
    assert err <= 2.0 ** -22 * total


def test_the_ringing_rule_and_the_profile_table():
    with pytest.raises(ValueError, match="highpass"):
        audio.Equaliser.design([("highpass", 50, 0, 4)])
    peak = [("peak", 1000, 6, 1)]
    assert audio.Equaliser.design(peak).size == R.design(audio.eq_bands(peak))[0].size
    assert audio.eq_bands("telephony") == (("highpass", 300.0, 0.0, 0.7071), ("lowpass", 3400.0, 0.0, 0.7071))
    assert audio.eq_bands("small_speaker") == (("highpass", 250.0, 0.0, 0.7071), ("peak", 2500.0, 3.0, 1.0))
    assert audio.eq_bands("presence") == (("peak", 3000.0, 4.0, 1.0), ("highshelf", 6000.0, 2.0, 0.7071))
    assert audio.eq_bands("warm") == (("lowshelf", 200.0, 3.0, 0.7071), ("highshelf", 5000.0, -3.0, 0.7071))
    assert audio.eq_bands([{"type": "highpass", "freq": 300, "q": 1}]) == (("highpass", 300.0, 0.0, 1.0),)
    band = audio._ffi.EqBand(kind=7, reserved=0, freq_hz=1000.0, gain_db=0.0, q=1.0)  # and at the ABI
    n = audio.ctypes.c_int32()
    assert audio._ffi.lib().rwkvtts_eq_design(audio.ctypes.byref(band), 1, None, audio.ctypes.byref(n), None) == audio._ffi.EINVAL
    band.kind, band.q = 0, float("nan")
    assert audio._ffi.lib().rwkvtts_eq_design(audio.ctypes.byref(band), 1, None, audio.ctypes.byref(n), None) == audio._ffi.EINVAL


@pytest.mark.parametrize("chunk", [1, 319, 2048])
def test_a_stream_cut_anywhere_is_bitwise_the_one_shot_and_never_lags(chunk):
    eq = audio.Equaliser(evaluator=R.evaluator)
    x = (0.9 * np.random.default_rng(3).uniform(-1, 1, 2500)).astype(F32)
    whole = eq.eq(x, "warm")
    assert np.array_equal(bits(whole), bits(R.fir(x, R.design(audio.eq_bands("warm"))[0])))
    st = eq.stream("warm")
    parts = [st.feed(x[a:a + chunk], final=a + chunk >= x.size) for a in range(0, x.size, chunk)]
    assert [p.size for p in parts] == [min(chunk, x.size - a) for a in range(0, x.size, chunk)]
    assert np.array_equal(bits(np.concatenate(parts)), bits(whole)) and st.kept == 0


def test_the_pipeline_keeps_its_signatures_its_order_and_creates_nothing_without_it():
    from test_server import FakeCodec, FakeManager
    names = ("generate_speech", "generate_speech_batch", "stream_speech", "stream_request", "generate_long_speech",
             "stream_long_speech")
    for name in names:
        par = inspect.signature(getattr(LightweightTtsPipeline, name)).parameters
        assert list(par)[-2:] == ["eq", "pitch_shift"] and par["eq"].default is None
    pipe = LightweightTtsPipeline(FakeManager(), FakeCodec())
    a = LightweightTtsPipelineArgs(text="hi")
    plain = pipe.generate_speech(a)
    assert np.array_equal(bits(pipe.generate_speech(a, eq=None)), bits(plain))
    assert pipe.equaliser(None) == (None, None) and pipe._equaliser is None
    for bad in BAD:
        for call in (lambda: pipe.generate_speech(a, eq=bad), lambda: pipe.generate_speech_batch([a], eq=bad),
                     lambda: pipe.stream_speech(a, eq=bad), lambda: next(pipe.stream_request(None, eq=bad)),
                     lambda: pipe.generate_long_speech(a, eq=bad), lambda: next(pipe.stream_long_speech(a, eq=bad))):
            with pytest.raises(ValueError):
                call()
    assert pipe._equaliser is None
    # a real request goes through the equaliser: bitwise the contract of the codec's PCM
    pipe._equaliser = audio.Equaliser(evaluator=R.evaluator)
    want = R.fir(plain, R.design(audio.eq_bands("telephony"))[0])
    assert np.any(want != plain) and np.array_equal(bits(pipe.generate_speech(a, eq="telephony")), bits(want))
    # and the fold puts it between the stretch and the leveller
    order = []

    class Stage:
        def __init__(self, name):
            for m in ("stretch_batch", "eq_batch", "level_batch"):
                setattr(self, m, lambda pcm, *_, n=name: order.append(n) or pcm)

    for batch, _ in audio_stages(Stage("stretch"), 1.5, None, Stage("level"), -20.0, equaliser=Stage("eq"), eq="warm"):
        batch([plain])
    assert order == ["stretch", "eq", "level"]


@pytest.mark.parametrize("bad", BAD + [True, [["peak", 1000, 3, 1]], [{"type": "peak", "freq": "1000", "gain": 3, "q": 1}]])
def test_a_bad_eq_is_a_400_in_both_handlers(bad):
    p = FakePipeline()
    body = json.dumps({"text": "hello", "eq": [dict(zip(("type", "freq", "gain", "q"), b)) if isinstance(b, tuple) else b
                                               for b in bad] if isinstance(bad, list) else bad})
    code, payload = SV.handle_tts_json(body, p)
    assert code == 400 and payload["success"] is False and "telephony" in payload["error"]
    code2, it = SV.handle_tts_stream(body, p)
    assert code2 == 400 and json.loads(b"".join(it).decode("utf-8")) == payload and p.calls == []


def test_the_field_is_passed_only_when_set_and_keeps_the_peak_rule():
    import base64
    p = FakePipeline()
    code, plain = SV.handle_tts_json({"text": "x"}, p)
    code2, shaped = SV.handle_tts_json({"text": "x", "eq": "warm"}, p)
    code3, it = SV.handle_tts_stream({"text": "x", "eq": [{"type": "peak", "freq": 1000, "gain": 3, "q": 1}]}, p)
    assert code == code2 == code3 == 200 and list(it)
    assert [c[1] for c in p.calls] == [{}, {"eq": audio.eq_bands("warm")}, {"eq": (("peak", 1000.0, 3.0, 1.0),)}]
    assert base64.standard_b64decode(shaped["audio_base64"]) == SV.convert_samples_to_wav(p.pcm, 16000)
