"""The limiter's contract itself (include/rwkvtts.h) on the CPU, through tests/limit_ref.py,
LimiterStream over it, and `limit` through the pipeline's stage fold and the server's validation."""
import base64
import json

import numpy as np
import pytest

import limit_ref as R
from rwkvtts import audio
from rwkvtts import server as SV
from test_pitch_cpu import FakePipeline

F32, bits, N = np.float32, R.bits, 2200


def true_peak(y):
    """The largest magnitude of y on an 8x grid, by zero-padding its spectrum (y taken as periodic)."""
    Y = np.fft.rfft(y.astype(np.float64))
    return float(np.max(np.abs(np.fft.irfft(Y, 8 * y.size) * 8.0)))


@pytest.mark.parametrize("limit", [0.0, -1.0, -6.0, -12.0])
def test_no_sample_passes_the_ceiling_and_a_signal_under_it_comes_back(limit):
    c = R.ceiling(limit)
    for n in (1, 70, N):
        x = R.burst(n)
        y = R.limit(x, limit)
        assert y.dtype == F32 and y.size == n and np.max(np.abs(y)) <= c
        assert np.max(np.abs(x)) > c  # (the limiter had work to do)
    quiet = R.burst(N, 0.1 * float(c))  # its largest sample, 0.15 c, leaves the 12-tap estimate far under c
    assert np.array_equal(bits(R.limit(quiet, limit)), bits(quiet))
    assert np.array_equal(bits(R.limit(np.zeros(300, F32), limit)), bits(np.zeros(300, F32)))
    assert R.limit(np.zeros(0, F32), limit).size == 0


def test_an_inter_sample_peak_is_lowered_though_no_sample_passes_the_ceiling():
    """A sine at fs / 4 sampled 45 degrees off its crests, amplitude 1.2, c = 1: the samples are +-0.849.
    The f32 contract's true peak is gated at the float64 reference's plus the chain's f32 rounding: 81
    rounded operations on the way to y (12 taps and a maximum's operand, two divides, 65 adds, a multiply)
    at 2^-24 each, on samples up to 1.2, through an interpolator whose Lebesgue constant is below
    (2 / pi) ln(n) + 1."""
    n = 4096
    x = (1.2 * np.sin(np.pi * np.arange(n) / 2.0 + np.pi / 4.0)).astype(F32)
    assert np.max(np.abs(x)) < 0.85 and abs(true_peak(x) - 1.2) < 1e-6
    y32, y64 = R.limit(x, 0.0), R.limit(x, 0.0, dtype=np.float64)
    tp32, tp64 = true_peak(y32), true_peak(y64)
    eps = 81 * 2.0 ** -24 * 1.2 * ((2.0 / np.pi) * np.log(n) + 1.0)
    print(f"limit: inter-sample sine, true peak in 1.2, out {tp64:.6f} (float64), {tp32:.6f} (f32), eps {eps:.2e}")
    assert np.max(np.abs(y32)) < np.max(np.abs(x))  # lowered, though every |x[n]| < c
    assert tp64 < 1.2 and tp32 <= tp64 + eps


@pytest.mark.parametrize("chunk", [1, 160, 1500])
def test_a_stream_cut_anywhere_is_bitwise_the_one_shot(chunk):
    lim = audio.Limiter(evaluator=R.evaluator)
    x = R.burst(N)
    whole = lim.limit(x, -1.0)
    assert np.array_equal(bits(whole), bits(R.limit(x, -1.0)))
    st = lim.stream(-1.0)
    parts = [st.feed(x[a:a + chunk], final=a + chunk >= N) for a in range(0, N, chunk)]
    assert np.array_equal(bits(np.concatenate(parts)), bits(whole)) and st.kept == 0
    assert max(p.size for p in parts) <= chunk + 70


def test_the_pipeline_creates_nothing_without_it_and_refuses_a_bad_ceiling():
    from rwkvtts.pipeline import LightweightTtsPipeline, LightweightTtsPipelineArgs
    from test_server import FakeCodec, FakeManager
    pipe = LightweightTtsPipeline(FakeManager(), FakeCodec())
    a = LightweightTtsPipelineArgs(text="hi")
    plain = pipe.generate_speech(a)
    assert np.array_equal(bits(pipe.generate_speech(a, limit=None)), bits(plain))
    assert pipe.limiter(None) is None and pipe._limiter is None
    for bad in (-12.5, 0.5, float("nan"), True):
        for call in (lambda: pipe.generate_speech(a, limit=bad), lambda: pipe.generate_speech_batch([a], limit=bad),
                     lambda: pipe.stream_speech(a, limit=bad), lambda: next(pipe.stream_request(None, limit=bad)),
                     lambda: pipe.generate_long_speech(a, limit=bad), lambda: next(pipe.stream_long_speech(a, limit=bad))):
            with pytest.raises(ValueError):
                call()
    assert pipe._limiter is None
    # a real request goes through the limiter last: bitwise the contract of the codec's PCM, also as a stream
    pipe._limiter = audio.Limiter(evaluator=R.evaluator)
    want = R.limit(plain, -12.0)  # (the fake codec's peak is 0.25, the ceiling 0.2512: the estimate passes it)
    assert np.any(want != plain) and np.array_equal(bits(pipe.generate_speech(a, limit=-12)), bits(want))


@pytest.mark.parametrize("bad", [True, "-1", float("nan"), -12.5, 0.5, [0]])
def test_a_bad_limit_is_a_400_naming_the_range(bad):
    p = FakePipeline()
    body = json.dumps({"text": "hello", "limit": bad})
    code, payload = SV.handle_tts_json(body, p)
    assert code == 400 and payload["success"] is False and "-12.0 - 0.0" in payload["error"]
    code2, it = SV.handle_tts_stream(body, p)
    assert code2 == 400 and json.loads(b"".join(it).decode("utf-8")) == payload and p.calls == []


def test_the_field_is_passed_only_when_set_and_the_wav_goes_out_at_scale_one():
    p = FakePipeline()
    code, plain = SV.handle_tts_json({"text": "x"}, p)
    code2, limited = SV.handle_tts_json({"text": "x", "limit": -3}, p)
    assert code == code2 == 200 and [c[1] for c in p.calls] == [{}, {"limit": -3.0}]
    assert base64.standard_b64decode(plain["audio_base64"]) == SV.convert_samples_to_wav(p.pcm, 16000)
    assert base64.standard_b64decode(limited["audio_base64"]) == SV.levelled_samples_to_wav(p.pcm, 16000)
    assert SV.levelled_samples_to_wav(p.pcm, 16000) != SV.convert_samples_to_wav(p.pcm, 16000)
    code3, it = SV.handle_tts_stream({"text": "x", "limit": 0}, p)
    assert code3 == 200 and list(it) and p.calls[-1][:2] == ("stream_speech", {"limit": 0.0})
