"""`watermark` in the bodies of POST /api/tts and /api/tts/stream and the POST /api/watermark/detect
handler, with a stand-in pipeline (CPU only): validation, the keyword reaching the pipeline only when
the body sets it, a server without a key, and a WAV written by /api/tts with `watermark` read back by
the detect handler -- through the int16 rounding and the peak rule's gain."""
import base64
import json
import os

import numpy as np
import pytest

import wm_ref
from rwkvtts import audio
from rwkvtts import server as SV
from rwkvtts.pipeline import SpeechChunk

KEY = 0xABCDEF0123456789


class FakePipeline:
    """generate_speech returns `pcm`, marked by the numpy restatement when the call carries a payload;
    stream_speech yields the same in pieces. Both record their keywords."""

    def __init__(self, pcm, key=KEY):
        self.pcm, self.calls, self.watermark_key = np.asarray(pcm, dtype=np.float32), [], key
        self.marker = audio.Watermarker(evaluator=wm_ref.evaluator, detector=wm_ref.detector)

    def _pcm(self, kw):
        return self.pcm.copy() if kw.get("watermark") is None else self.marker.embed(self.pcm, self.watermark_key, kw["watermark"])

    def generate_speech(self, args, **kw):
        self.calls.append(("generate_speech", kw))
        return self._pcm(kw)

    def stream_speech(self, args, chunk_frames=16, **kw):
        self.calls.append(("stream_speech", kw))
        parts = np.array_split(self._pcm(kw), 3)
        for i, c in enumerate(parts):
            yield SpeechChunk.make(c, 0, 0, 0, i == len(parts) - 1)

    def detect_watermark(self, pcm):
        self.calls.append(("detect_watermark", len(pcm)))
        return self.marker.detect(pcm, self.watermark_key)


@pytest.fixture(scope="module")
def speech():
    return wm_ref.vowel(3 * 16000, 5, peak=0.4)


@pytest.mark.parametrize("bad", [True, False, "7", 1.5, 7.0, float("nan"), -1, 65536, [7], {"payload": 7}])
def test_a_bad_watermark_is_a_400_and_the_pipeline_is_not_called(bad):
    p = FakePipeline(np.zeros(100))
    body = json.dumps({"text": "hello", "watermark": bad})
    code, payload = SV.handle_tts_json(body, p)
    assert code == 400 and payload["success"] is False and isinstance(payload["error"], str)
    code2, it = SV.handle_tts_stream(body, p)
    assert code2 == 400 and json.loads(b"".join(it).decode("utf-8")) == payload
    assert p.calls == []


def test_the_keyword_is_passed_only_when_the_body_sets_it_and_needs_a_key():
    p = FakePipeline(np.zeros(700))
    for body in ({"text": "x"}, {"text": "x", "watermark": None}):
        assert SV.handle_tts_json(body, p)[0] == 200
        assert SV.handle_tts_stream(body, p)[0] == 200
    assert p.calls == [("generate_speech", {}), ("stream_speech", {})] * 2
    p.calls.clear()
    for v in (0, 1, 65535):
        assert SV.handle_tts_json({"text": "x", "watermark": v}, p)[0] == 200
        code, it = SV.handle_tts_stream({"text": "x", "watermark": v, "loudness": -20}, p)
        assert code == 200
        list(it)
        assert p.calls == [("generate_speech", {"watermark": v}), ("stream_speech", {"loudness": -20.0, "watermark": v})]
        assert type(p.calls[0][1]["watermark"]) is int
        p.calls.clear()
    bare = FakePipeline(np.zeros(700), key=None)
    code, payload = SV.handle_tts_json({"text": "x", "watermark": 5}, bare)
    assert code == 400 and payload["success"] is False and "watermark_key" in payload["error"]
    code2, it = SV.handle_tts_stream({"text": "x", "watermark": 5}, bare)
    assert code2 == 400 and json.loads(b"".join(it).decode("utf-8")) == payload
    assert SV.handle_tts_json({"text": "x"}, bare)[0] == 200 and bare.calls == [("generate_speech", {})]
    assert SV.handle_watermark_detect("whatever.wav", bare)[0] == 400


def test_the_detect_handler_reads_the_payload_from_the_wav_of_api_tts(speech, tmp_path):
    p = FakePipeline(speech)
    code, payload = SV.handle_tts_json({"text": "hello", "watermark": 0xC0DE}, p)
    assert code == 200
    path = os.path.join(tmp_path, "marked.wav")
    with open(path, "wb") as f:
        f.write(base64.standard_b64decode(payload["audio_base64"]))
    code, out = SV.handle_watermark_detect(path, p)
    assert code == 200 and set(out) == {"success", "detected", "score", "threshold", "payload", "seen_bits", "offset",
                                        "seconds"}
    assert out["success"] and out["detected"] is True and out["payload"] == 0xC0DE and out["seen_bits"] == 0xFFFF
    assert out["score"] >= 10 * out["threshold"] and abs(out["seconds"] - 3.0) < 0.05
    assert out["threshold"] == wm_ref.threshold(16, 25600)
    json.dumps(out)
    # the same request without the mark: nothing is found
    code, payload = SV.handle_tts_json({"text": "hello"}, p)
    with open(path, "wb") as f:
        f.write(base64.standard_b64decode(payload["audio_base64"]))
    code, out = SV.handle_watermark_detect(path, p)
    assert code == 200 and out["detected"] is False and out["score"] < out["threshold"]
    # no file, not a WAV
    assert SV.handle_watermark_detect(None, p)[0] == 400
    with open(path, "wb") as f:
        f.write(b"not a wav at all")
    code, out = SV.handle_watermark_detect(path, p)
    assert code == 400 and out["success"] is False


def test_the_route_is_wired(speech):
    fastapi = pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    p = FakePipeline(speech)
    wav = base64.standard_b64decode(SV.handle_tts_json({"text": "hello", "watermark": 9}, p)[1]["audio_base64"])
    r = TestClient(SV.create_app(p)).post("/api/watermark/detect", content=wav, headers={"content-type": "audio/wav"})
    assert r.status_code == 200 and r.json()["detected"] is True and r.json()["payload"] == 9
