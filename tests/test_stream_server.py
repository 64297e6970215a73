"""POST /api/tts/stream's handler and stream_speech's chunk scheduling with stand-ins (CPU only);
the GPU end-to-end run is in tests/test_gpu_stream.py."""
import json
import struct

import numpy as np
import pytest

from rwkvtts import server as SV
from rwkvtts.pipeline import LightweightTtsPipeline, LightweightTtsPipelineArgs, SpeechChunk

HEADER = (b"RIFF" + struct.pack("<I", 0xFFFFFFFF) + b"WAVE" + b"fmt " +
          struct.pack("<IHHIIHH", 16, 1, 1, 16000, 32000, 2, 16) + b"data" + struct.pack("<I", 0xFFFFFFFF))


class FakePipeline:
    def __init__(self, chunks=(), fail_at=None):
        self.chunks, self.fail_at, self.seen = list(chunks), fail_at, []

    def stream_speech(self, args, chunk_frames=16):
        self.seen.append((args, chunk_frames))
        for i, c in enumerate(self.chunks):
            if self.fail_at == i:
                raise RuntimeError("boom")
            yield SpeechChunk.make(c, 0, 0, 0, i == len(self.chunks) - 1)
        if self.fail_at == len(self.chunks):
            raise RuntimeError("boom")


def test_stream_header_and_payload():
    rs = np.random.default_rng(0)
    chunks = [rs.uniform(-1.2, 1.2, n).astype(np.float32) for n in (320, 5, 640)]
    chunks[1][:] = [1.0, -1.0, 0.99999, -0.5, 3.0e-5]  # the clamp's edges, truncation toward zero
    p = FakePipeline(chunks)
    code, it = SV.handle_tts_stream(json.dumps({"text": "hello", "seed": 5}), p, chunk_frames=4)
    assert code == 200
    parts = list(it)
    assert parts[0] == HEADER and len(parts[0]) == 44
    assert len(parts) == 1 + len(chunks)
    x = np.concatenate(chunks)
    want = np.trunc(np.clip(x, np.float32(-1), np.float32(1)) * np.float32(32767)).astype("<i2")
    assert b"".join(parts[1:]) == want.tobytes()
    assert list(np.frombuffer(parts[2], "<i2")) == [32767, -32767, 32766, -16383, 0]
    # no peak normalisation: a quiet stream stays quiet (convert_samples_to_wav would scale it up)
    q = np.full(8, 0.01, np.float32)
    _, it = SV.handle_tts_stream({"text": "x"}, FakePipeline([q]))
    assert np.frombuffer(list(it)[1], "<i2").tolist() == [327] * 8
    # the body is parsed as /api/tts parses it
    args, cf = p.seen[0]
    assert args.text == "hello" and args.seed == 5 and args.top_k == 100 and args.gender == "male" and cf == 4


def test_stream_error_bodies(tmp_path):
    p = FakePipeline([np.zeros(4, np.float32)])
    for body in (b"{not json", json.dumps({"prompt_text": "x"}), json.dumps({"text": 5})):
        code, it = SV.handle_tts_stream(body, p)
        want = SV.handle_tts_json(body, p)
        got = json.loads(b"".join(it).decode("utf-8"))
        assert code == want[0] == 400 and got == want[1] and got["success"] is False
    code, it = SV.handle_tts_stream({"text": "x", "voice_id": "nope"}, p, voice_dir=str(tmp_path))
    got = json.loads(b"".join(it).decode("utf-8"))
    assert code == 400 and "nope" in got["error"]
    assert p.seen == []
    # a failure before the first chunk is still a 500 with the reference's body
    code, it = SV.handle_tts_stream({"text": "x"}, FakePipeline([], fail_at=0))
    got = json.loads(b"".join(it).decode("utf-8"))
    assert code == 500 and got == {"success": False, "error": "生成TTS音频失败: boom"}
    # after the first chunk the stream can only end: the header and what was decoded went out
    code, it = SV.handle_tts_stream({"text": "x"}, FakePipeline([np.zeros(3, np.float32)] * 2, fail_at=1))
    assert code == 200
    out = []
    with pytest.raises(RuntimeError):
        for part in it:
            out.append(part)
    assert out == [HEADER, b"\0" * 6]
    # an empty stream is a header alone
    code, it = SV.handle_tts_stream({"text": "x"}, FakePipeline([]))
    assert code == 200 and list(it) == [HEADER]


class FakeCodec:
    """decode_windows returns each frame's index as its 320 samples: a chunk shows what it covers."""
    def __init__(self, halo=5):
        self._halo, self.calls = halo, []

    def halo(self):
        return self._halo

    def decode_windows(self, items):
        self.calls.append([(t0, t1, len(s), bool(final)) for _, s, t0, t1, final in items])
        for _, s, t0, t1, final in items:
            assert final or t1 + self._halo <= len(s)
        return [np.repeat(np.arange(t0, t1, dtype=np.float32), 320) for _, s, t0, t1, _ in items]

    def decode_audio(self, g, s):
        if not len(s):
            raise ValueError("need >0 semantic tokens")
        return np.repeat(np.arange(len(s), dtype=np.float32), 320)


class FakeStreamManager:
    def __init__(self, incs, status=0):
        self.incs, self.last_status, self._status = incs, [], status

    def _tokens(self, text):
        if "\U0001F600" in text:
            raise ValueError("no matching token")
        return [1, 2, 3]

    def stream_tts(self, req):
        for i, (g, new) in enumerate(self.incs):
            done = i == len(self.incs) - 1
            if done:
                self.last_status = [self._status]
            yield g, new, done


def test_stream_speech_schedule():
    G = list(range(32))
    incs = [(None, []), (G, [])] + [(G, list(range(8 * k, 8 * k + 8))) for k in range(4)] + [(G, [32, 33, 34])]
    c = FakeCodec(halo=5)
    pipe = LightweightTtsPipeline(FakeStreamManager(incs), c)
    chunks = list(pipe.stream_speech(LightweightTtsPipelineArgs(text="x"), chunk_frames=4))
    meta = [(k.t0, k.t1, k.n_known, k.done) for k in chunks]
    # chunk [t0, t1) goes out as soon as t1 + 5 tokens are known; the tail when the request is done
    assert meta == [(0, 4, 16, False), (4, 8, 16, False), (8, 12, 24, False), (12, 16, 24, False),
                    (16, 20, 32, False), (20, 24, 32, False), (24, 28, 35, True), (28, 32, 35, True),
                    (32, 35, 35, True)]
    assert all(t1 + 5 <= n or d for _, t1, n, d in meta)
    assert [len(x) for x in c.calls] == [2, 2, 2, 3]   # chunks ready together: one batched decode
    got = np.concatenate(chunks)
    assert np.array_equal(got, c.decode_audio(G, list(range(35)))) and got.dtype == np.float32
    assert b"".join(chunks) == got.tobytes()


def test_stream_speech_failures_yield_silence():
    G = list(range(32))
    c = FakeCodec()
    for mgr in (FakeStreamManager([(None, [])], status=-2), FakeStreamManager([(None, [])], status=0)):
        out = list(LightweightTtsPipeline(mgr, c).stream_speech(LightweightTtsPipelineArgs(text="x")))
        assert len(out) == 1 and out[0].shape == (16000,) and not out[0].any() and out[0].done
    out = list(LightweightTtsPipeline(FakeStreamManager([]), c).stream_speech(
        LightweightTtsPipelineArgs(text="\U0001F600")))
    assert len(out) == 1 and out[0].shape == (16000,) and not out[0].any()
    # a failure after audio went out ends the stream: no silence appended
    incs = [(G, list(range(20))), (None, [])]
    out = list(LightweightTtsPipeline(FakeStreamManager(incs, status=-2), FakeCodec(halo=5)).stream_speech(
        LightweightTtsPipelineArgs(text="x"), chunk_frames=4))
    assert [(k.t0, k.t1) for k in out] == [(0, 4), (4, 8), (8, 12)] and not out[-1].done
    with pytest.raises(ValueError):
        list(LightweightTtsPipeline(FakeStreamManager([(G, [])]), c).stream_speech(LightweightTtsPipelineArgs(text="x"), 0))


def test_fastapi_stream_route():
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    chunks = [np.full(320, 0.25, np.float32), np.full(160, -0.5, np.float32)]
    c = TestClient(SV.create_app(FakePipeline(chunks)))
    r = c.post("/api/tts/stream", json={"text": "hello"})
    assert r.status_code == 200 and r.headers["content-type"].startswith("audio/wav")
    assert r.content == HEADER + SV.samples_to_pcm16(np.concatenate(chunks))
    r = c.post("/api/tts/stream", content=b"{not json")
    assert r.status_code == 400 and r.json()["success"] is False
    # /api/tts is unchanged beside it
    from test_server import FakeCodec as PlainCodec, FakeManager
    r = TestClient(SV.create_app(LightweightTtsPipeline(FakeManager(), PlainCodec()))).post("/api/tts", json={"text": "hello"})
    assert r.status_code == 200 and r.json()["success"]
