"""`loudness` in the bodies of POST /api/tts and /api/tts/stream, with a stand-in pipeline (CPU only):
validation, the keyword reaching the pipeline only when the body sets it, and /api/tts's WAV at
scale 1.0 -- byte for byte the stream route's PCM -- when it does."""
import base64
import json

import numpy as np
import pytest

from rwkvtts import server as SV
from rwkvtts.pipeline import SpeechChunk


class FakePipeline:
    """generate_speech returns `pcm`; stream_speech yields it in pieces. Both record their keywords."""

    def __init__(self, pcm):
        self.pcm, self.calls = np.asarray(pcm, dtype=np.float32), []

    def generate_speech(self, args, **kw):
        self.calls.append(("generate_speech", kw))
        return self.pcm.copy()

    def stream_speech(self, args, chunk_frames=16, **kw):
        self.calls.append(("stream_speech", kw))
        parts = np.array_split(self.pcm, 3)
        for i, c in enumerate(parts):
            yield SpeechChunk.make(c, 0, 0, 0, i == len(parts) - 1)


def _pcm():
    x = np.random.default_rng(3).uniform(-0.2, 0.2, 700).astype(np.float32)
    x[:5] = [0.891, -0.891, 0.5, 3.0e-5, -1.5]  # the ceiling, truncation toward zero, the clamp
    return x


@pytest.mark.parametrize("bad", [True, False, "-23", "loud", float("nan"), -40.5, -9.0, 0, 23, [-23], {"db": -23}])
def test_a_bad_loudness_is_a_400_and_the_pipeline_is_not_called(bad):
    p = FakePipeline(_pcm())
    body = json.dumps({"text": "hello", "loudness": bad})  # (json.dumps writes NaN as NaN; json.loads reads it back)
    code, payload = SV.handle_tts_json(body, p)
    assert code == 400 and payload["success"] is False and isinstance(payload["error"], str)
    code2, it = SV.handle_tts_stream(body, p)
    assert code2 == 400 and json.loads(b"".join(it).decode("utf-8")) == payload
    assert p.calls == []


def test_the_keyword_is_passed_only_when_the_body_sets_it():
    p = FakePipeline(_pcm())
    for body in ({"text": "x"}, {"text": "x", "loudness": None}):
        assert SV.handle_tts_json(body, p)[0] == 200
        assert SV.handle_tts_stream(body, p)[0] == 200
    assert p.calls == [("generate_speech", {}), ("stream_speech", {})] * 2
    p.calls.clear()
    for v in (-23, -16.5, -40, -10.0):
        assert SV.handle_tts_json({"text": "x", "loudness": v}, p)[0] == 200
        code, it = SV.handle_tts_stream({"text": "x", "loudness": v, "tempo": 1.25}, p)
        assert code == 200
        list(it)
        assert p.calls == [("generate_speech", {"loudness": float(v)}),
                           ("stream_speech", {"tempo": 1.25, "loudness": float(v)})]
        assert type(p.calls[0][1]["loudness"]) is float
        p.calls.clear()


def test_with_loudness_the_wav_is_at_scale_one_and_equals_the_stream():
    x = _pcm()
    p = FakePipeline(x)
    body = {"text": "hello", "seed": 4, "loudness": -23}
    code, payload = SV.handle_tts_json(body, p)
    assert code == 200
    wav = base64.standard_b64decode(payload["audio_base64"])
    want = SV.convert_samples_to_wav(x, 16000)
    head = len(want) - 2 * x.size
    assert wav[:head] == want[:head]                  # the header /api/tts always writes
    assert wav[head:] == SV.samples_to_pcm16(x)       # scale 1.0: no peak rule
    assert wav[head:] != want[head:]
    assert np.frombuffer(wav[head:], "<i2")[:5].tolist() == [int(np.float32(0.891) * np.float32(32767)),
                                                           -int(np.float32(0.891) * np.float32(32767)), 16383, 0, -32767]
    code, it = SV.handle_tts_stream(body, p)
    parts = list(it)
    assert code == 200 and parts[0] == SV.streaming_wav_header(16000)
    assert b"".join(parts[1:]) == wav[head:]
    # another rate: the header carries it, the data rule is the same
    code, payload = SV.handle_tts_json({"text": "hello", "loudness": -16, "sample_rate": 24000}, p)
    wav24 = base64.standard_b64decode(payload["audio_base64"])
    assert wav24[:head] == SV.convert_samples_to_wav(x, 24000)[:head] and wav24[head:] == wav[head:]
    assert p.calls[-1] == ("generate_speech", {"sample_rate": 24000, "loudness": -16.0})


def test_without_loudness_the_wav_is_convert_samples_to_wav():
    x = _pcm()
    for body in ({"text": "hello"}, {"text": "hello", "tempo": 1.5}, {"text": "hello", "loudness": None}):
        code, payload = SV.handle_tts_json(body, FakePipeline(x))
        assert code == 200
        assert base64.standard_b64decode(payload["audio_base64"]) == SV.convert_samples_to_wav(x, 16000)
