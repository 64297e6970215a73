"""`long_form`, `segment_tokens` and `voice_tokens` in the bodies of /api/tts and /api/tts/stream,
on the CPU with a stand-in pipeline that records the calls it gets: the routing, the keywords, the
pinned voice, every 400 (with the pipeline never called), the fields a long-form response adds, and
that a body without the keys makes exactly the call it made before."""
import base64
import json

import numpy as np
import pytest

from rwkvtts import server as SV
from rwkvtts.pipeline import LongSpeech, SpeechChunk

VOICE = [(37 * k + 5) % 4096 for k in range(32)]
SEGS = [{"text": "One. ", "status": 0, "n_semantic": 3, "truncated": False, "pause_ms": 300, "a": 10, "b": 900},
        {"text": "Two.", "status": 0, "n_semantic": 2, "truncated": False, "pause_ms": 0, "a": 0, "b": 640}]


class Pipe:
    """Records (entry point, args, keywords); answers with fixed PCM."""

    def __init__(self):
        self.calls = []

    def generate_speech(self, args, **kw):
        self.calls.append(("generate_speech", args, kw))
        return np.full(640, 0.25, np.float32)

    def generate_long_speech(self, args, **kw):
        self.calls.append(("generate_long_speech", args, kw))
        return LongSpeech.make(np.full(1600, 0.25, np.float32), VOICE, SEGS)

    def stream_speech(self, args, chunk_frames=16, **kw):
        self.calls.append(("stream_speech", args, dict(kw, chunk_frames=chunk_frames)))
        return iter([SpeechChunk.make(np.full(320, 0.5, np.float32), 0, 1, 1, True)])

    def stream_long_speech(self, args, **kw):
        self.calls.append(("stream_long_speech", args, kw))
        return iter([LongSpeech.make(np.full(320, 0.5, np.float32), VOICE, SEGS[:1]),
                     LongSpeech.make(np.zeros(0, np.float32), VOICE, []),
                     LongSpeech.make(np.full(160, -0.5, np.float32), VOICE, SEGS[1:])])


def post(pipe, body, tmp_path):
    return SV.handle_tts_json(json.dumps(body), pipe, str(tmp_path))


def stream(pipe, body, tmp_path):
    code, it = SV.handle_tts_stream(json.dumps(body), pipe, str(tmp_path))
    return code, b"".join(it)


def test_body_without_the_keys_makes_the_call_it_made_before(tmp_path):
    pipe = Pipe()
    code, out = post(pipe, {"text": "hi", "seed": 3}, tmp_path)
    assert code == 200 and set(out) == {"success", "message", "audio_base64", "duration_ms", "rtf"}
    code, wav = stream(pipe, {"text": "hi", "seed": 3}, tmp_path)
    assert code == 200 and len(wav) == 44 + 640
    (n1, a1, k1), (n2, a2, k2) = pipe.calls
    assert (n1, k1) == ("generate_speech", {}) and (n2, k2) == ("stream_speech", {"chunk_frames": 16})
    assert a1 == a2 and not a1.pin_voice and a1.voice_global_tokens is None and a1.seed == 3
    # long_form false is the default call too
    post(pipe, {"text": "hi", "long_form": False}, tmp_path)
    assert pipe.calls[-1][0] == "generate_speech" and pipe.calls[-1][2] == {}


def test_long_form_routes_and_adds_the_response_fields(tmp_path):
    pipe = Pipe()
    code, out = post(pipe, {"text": "One. Two.", "long_form": True, "seed": 5, "emotion": "HAPPY"}, tmp_path)
    assert code == 200 and out["success"]
    assert out["voice_tokens"] == VOICE and out["segments"] == SEGS
    json.dumps(out)  # the whole response is JSON
    wav = base64.b64decode(out["audio_base64"])
    assert wav == SV.convert_samples_to_wav(np.full(1600, 0.25, np.float32))
    name, args, kw = pipe.calls[-1]
    assert name == "generate_long_speech" and kw == {} and args.text == "One. Two." and args.seed == 5
    assert args.emotion == "HAPPY" and not args.pin_voice
    # with segment_tokens, sample_rate and tempo
    code, out = post(pipe, {"text": "x", "long_form": True, "segment_tokens": 32, "sample_rate": 24000, "tempo": 1.25},
                     tmp_path)
    assert code == 200 and pipe.calls[-1][0] == "generate_long_speech"
    assert pipe.calls[-1][2] == {"segment_tokens": 32, "sample_rate": 24000, "tempo": 1.25}
    assert base64.b64decode(out["audio_base64"])[24:28] == (24000).to_bytes(4, "little")
    for edge in (8, 256):
        assert post(pipe, {"text": "x", "long_form": True, "segment_tokens": edge}, tmp_path)[0] == 200
        assert pipe.calls[-1][2] == {"segment_tokens": edge}
    # the stream: one item per segment, empty items not sent
    code, wav = stream(pipe, {"text": "One. Two.", "long_form": True, "segment_tokens": 16, "sample_rate": 8000}, tmp_path)
    assert code == 200 and wav[:44] == SV.streaming_wav_header(8000)
    assert wav[44:] == SV.samples_to_pcm16(np.concatenate([np.full(320, 0.5, np.float32), np.full(160, -0.5, np.float32)]))
    assert pipe.calls[-1][0] == "stream_long_speech" and pipe.calls[-1][2] == {"segment_tokens": 16, "sample_rate": 8000}


def test_voice_tokens_pin_the_voice_with_or_without_long_form(tmp_path):
    pipe = Pipe()
    for body, name in (({"text": "hi", "voice_tokens": VOICE, "emotion": "SAD"}, "generate_speech"),
                       ({"text": "hi", "voice_tokens": VOICE, "emotion": "SAD", "long_form": True}, "generate_long_speech")):
        assert post(pipe, body, tmp_path)[0] == 200
        got, args, kw = pipe.calls[-1]
        assert got == name and kw == {}
        assert args.pin_voice and args.voice_global_tokens == VOICE and args.voice_semantic_tokens is None
        assert not args.zero_shot and args.emotion == "SAD"  # the property tokens are kept
    assert stream(pipe, {"text": "hi", "voice_tokens": VOICE}, tmp_path)[0] == 200
    assert pipe.calls[-1][0] == "stream_speech" and pipe.calls[-1][1].pin_voice
    assert stream(pipe, {"text": "hi", "voice_tokens": VOICE, "long_form": True}, tmp_path)[0] == 200
    assert pipe.calls[-1][0] == "stream_long_speech" and pipe.calls[-1][1].voice_global_tokens == VOICE


BAD = [{"long_form": 1}, {"long_form": "true"}, {"long_form": [True]},
       {"long_form": True, "segment_tokens": 7}, {"long_form": True, "segment_tokens": 257},
       {"long_form": True, "segment_tokens": 64.0}, {"long_form": True, "segment_tokens": "64"},
       {"long_form": True, "segment_tokens": True}, {"segment_tokens": 64}, {"long_form": False, "segment_tokens": 64},
       {"voice_tokens": VOICE[:31]}, {"voice_tokens": VOICE + [1]}, {"voice_tokens": VOICE[:31] + [4096]},
       {"voice_tokens": VOICE[:31] + [-1]}, {"voice_tokens": VOICE[:31] + [1.0]}, {"voice_tokens": VOICE[:31] + [True]},
       {"voice_tokens": "abc"}, {"voice_tokens": {"0": 1}}, {"voice_tokens": []},
       {"voice_tokens": VOICE, "voice_id": "some_voice"}]


@pytest.mark.parametrize("extra", BAD)
def test_bad_values_are_400_and_the_pipeline_is_never_called(tmp_path, extra):
    pipe = Pipe()
    code, out = post(pipe, dict({"text": "hi"}, **extra), tmp_path)
    assert code == 400 and out["success"] is False and isinstance(out["error"], str) and set(out) == {"success", "error"}
    code, raw = stream(pipe, dict({"text": "hi"}, **extra), tmp_path)
    assert code == 400 and json.loads(raw) == out
    assert pipe.calls == []


def test_failure_in_the_long_call_is_a_500(tmp_path):
    class Broken(Pipe):
        def generate_long_speech(self, args, **kw):
            raise RuntimeError("boom")

        def stream_long_speech(self, args, **kw):
            raise RuntimeError("boom")
    code, out = post(Broken(), {"text": "hi", "long_form": True}, tmp_path)
    assert code == 500 and not out["success"] and "boom" in out["error"]
    code, raw = stream(Broken(), {"text": "hi", "long_form": True}, tmp_path)
    assert code == 500 and "boom" in json.loads(raw)["error"]
