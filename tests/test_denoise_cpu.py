"""The noise reducer's contract itself (include/rwkvtts.h) on the CPU, through
tests/denoise_ref.py against a float64 restatement on np.fft, DenoiseStream over it, and `denoise` through the
pipeline's stage fold and the server's validation."""
import inspect
import json

import numpy as np
import pytest

import denoise_ref as R
from rwkvtts import audio
from rwkvtts import server as SV
from rwkvtts.pipeline import LightweightTtsPipeline, LightweightTtsPipelineArgs, audio_stages
from test_pitch_cpu import FakePipeline

F32, bits, FS, DB = np.float32, R.bits, 16000, 12.0
HARMONICS = 120 * np.arange(1, 21)  # of the vowel, in Hz: bins of a one-second transform


@pytest.fixture(scope="module")
def vowel():
    """A second of a 120 Hz vowel (20 harmonics at 1 / h) in white noise of 0.01 rms, then a second of the noise
    alone: every bin's smoothed power is near 0.03 or above, nine orders over the f32 transform's own noise.
    -> (x, the contract's y, the float64 reference's y)."""
    t = np.arange(2 * FS) / FS
    v = 0.3 * sum(np.sin(2 * np.pi * f * t) * (120.0 / f) for f in HARMONICS) * (t < 1.0)
    x = (v + 0.01 * np.random.default_rng(0).standard_normal(t.size)).astype(F32)
    return x, R.denoise(x, DB), R.denoise(x, DB, f64=True)


def test_the_f32_contract_stays_within_its_measured_distance_of_float64(vowel):
    """Measured: 1.2e-7 (the signal's peak is 0.56). The gate is 8 times that, the factor by which the f32
    transform's error moves with the data."""
    x, y32, y64 = vowel
    dev = float(np.max(np.abs(y32.astype(np.float64) - y64)))
    print(f"denoise: largest |f32 contract - float64| {dev:.3e}, peak {np.max(np.abs(x)):.3f}")
    assert y32.dtype == F32 and y32.size == x.size and dev <= 8 * 1.2e-7


def test_the_noise_goes_down_and_the_harmonics_stay_as_in_float64(vowel):
    """Measured on the float64 reference at denoise = 12, alpha = 2: the noise-only second leaves 3.2 dB
    lower (a minimum-statistics floor sits well under the mean noise power, so alpha = 2 takes little) and
    the harmonic peaks fall by 6.3 .. 7.4 dB (a vowel held unchanged for a whole second is its own minimum
    over the floor's window, so the rule takes it for noise; speech does not hold still like that, but it
    shows that the defaults are untuned). The contract must show the same two figures within 0.1 dB;
    neither figure is itself gated beyond the first one's sign."""
    x, y32, y64 = vowel
    quiet = slice(FS + 2048, 2 * FS - 2048)
    att = [10 * np.log10(np.mean(np.square(y[quiet], dtype=np.float64)) / np.mean(np.square(x[quiet], dtype=np.float64)))
           for y in (y32, y64)]
    X = np.abs(np.fft.rfft(x[:FS].astype(np.float64)))[HARMONICS]
    peak = [20 * np.log10(np.abs(np.fft.rfft(np.asarray(y[:FS], dtype=np.float64)))[HARMONICS] / X) for y in (y32, y64)]
    print(f"denoise: noise-only second {att[1]:.2f} dB (float64) {att[0]:.2f} dB (f32); harmonic peaks change by "
          f"{np.min(peak[1]):.2f} .. {np.max(peak[1]):.2f} dB (float64)")
    assert att[1] < 0.0 and abs(att[0] - att[1]) <= 0.1 and np.max(np.abs(peak[0] - peak[1])) <= 0.1


@pytest.mark.parametrize("chunk", [333, 1000, 4097])
def test_a_stream_cut_anywhere_is_bitwise_the_one_shot(vowel, chunk):
    dn = audio.Denoiser(evaluator=R.evaluator)
    x = vowel[0][8000:28000]
    whole = dn.denoise(x, DB)
    assert np.array_equal(bits(whole), bits(R.denoise(x, DB)))
    st = dn.stream(DB)
    parts = [st.feed(x[a:a + chunk], final=a + chunk >= x.size) for a in range(0, x.size, chunk)]
    assert np.array_equal(bits(np.concatenate(parts)), bits(whole)) and st.kept == 0
    assert not parts[0].size and sum(p.size for p in parts[:-1]) >= x.size - chunk - 4864  # the stated lag
    assert not bits(dn.denoise(np.zeros(700, F32), DB)).any() and dn.denoise(np.zeros(0, F32), DB).size == 0


def test_the_pipeline_keeps_its_signatures_its_order_and_creates_nothing_without_it():
    from test_server import FakeCodec, FakeManager
    for name in ("generate_speech", "generate_speech_batch", "stream_speech", "stream_request", "generate_long_speech",
                 "stream_long_speech"):
        par = inspect.signature(getattr(LightweightTtsPipeline, name)).parameters
        assert list(par)[-3:] == ["denoise", "eq", "pitch_shift"] and par["denoise"].default is None
    pipe = LightweightTtsPipeline(FakeManager(), FakeCodec())
    a = LightweightTtsPipelineArgs(text="hi")
    plain = pipe.generate_speech(a)
    assert np.array_equal(bits(pipe.generate_speech(a, denoise=None)), bits(plain))
    assert pipe.denoiser(None) is None and pipe._denoiser is None
    for bad in (2.5, 30.5, float("nan"), True, "12"):
        for call in (lambda: pipe.generate_speech(a, denoise=bad), lambda: pipe.generate_speech_batch([a], denoise=bad),
                     lambda: pipe.stream_speech(a, denoise=bad), lambda: next(pipe.stream_request(None, denoise=bad)),
                     lambda: pipe.generate_long_speech(a, denoise=bad), lambda: next(pipe.stream_long_speech(a, denoise=bad))):
            with pytest.raises(ValueError):
                call()
    assert pipe._denoiser is None
    # a real request goes through the stage: bitwise the contract of the codec's PCM; and the fold puts it first
    pipe._denoiser = audio.Denoiser(evaluator=R.evaluator)
    want = R.denoise(plain, DB)
    assert np.any(want != plain) and np.array_equal(bits(pipe.generate_speech(a, denoise=DB)), bits(want))
    order = []

    class Stage:
        def __init__(self, name):
            for m in ("denoise_batch", "shape_batch", "stretch_batch"):
                setattr(self, m, lambda pcm, *_, n=name: order.append(n) or pcm)

    for batch, _ in audio_stages(Stage("stretch"), 1.5, None, shaper=Stage("pause"), max_pause=100, denoiser=Stage("denoise"),
                                 denoise=DB):
        batch([plain])
    assert order == ["denoise", "pause", "stretch"]


@pytest.mark.parametrize("bad", [True, "12", float("nan"), 2.5, 30.5, [12]])
def test_a_bad_denoise_is_a_400_naming_the_range(bad):
    p = FakePipeline()
    body = json.dumps({"text": "hello", "denoise": bad})
    code, payload = SV.handle_tts_json(body, p)
    assert code == 400 and payload["success"] is False and "3.0 - 30.0" in payload["error"]
    code2, it = SV.handle_tts_stream(body, p)
    assert code2 == 400 and json.loads(b"".join(it).decode("utf-8")) == payload and p.calls == []


def test_the_field_is_passed_only_when_set():
    p = FakePipeline()
    code, _ = SV.handle_tts_json({"text": "x"}, p)
    code2, _ = SV.handle_tts_json({"text": "x", "denoise": 12}, p)
    code3, it = SV.handle_tts_stream({"text": "x", "denoise": 3}, p)
    assert code == code2 == code3 == 200 and list(it)
    assert [c[1] for c in p.calls] == [{}, {"denoise": 12.0}, {"denoise": 3.0}]
