"""Penalties from the Python surface down to the C request struct, without a GPU:
runtime.Penalties / SamplerArgs -> request_struct -> _ffi.Request, the pipeline arguments of all
five entry points and both HTTP bodies (/api/tts and its streaming twin), with a stand-in manager
that records the request it is handed."""
import ctypes
import json

import numpy as np
import pytest

import rwkvtts
from rwkvtts import _ffi
from rwkvtts import server as SV
from rwkvtts.pipeline import LightweightTtsPipeline, LightweightTtsPipelineArgs
from rwkvtts.runtime import Penalties, request_struct
from test_sampling_marshalling import FakeCodec, RecordingManager


def _pen(q):
    p = q.penalties
    return (round(float(p.repetition), 6), round(float(p.frequency), 6), round(float(p.presence), 6), int(p.window))


def test_request_struct_layout_and_marshalling():
    # the struct ends with penalty_set and the four values, as include/rwkvtts.h declares them
    assert ctypes.sizeof(_ffi.Penalties) == 16
    assert _ffi.Request.penalty_set.offset == _ffi.Request.pinned_voice.offset + 4
    assert _ffi.Request.penalties.offset == _ffi.Request.penalty_set.offset + 4
    assert ctypes.sizeof(_ffi.Request) == (_ffi.Request.penalties.offset + 16 + 7) // 8 * 8
    assert [n for n, _ in _ffi.Penalties._fields_] == ["repetition", "frequency", "presence", "window"]
    assert "rwkvtts_debug_advance_pen" in _ffi.EXPORTS
    r = rwkvtts.TtsBatchRequest([1, 2, 3], args=rwkvtts.SamplerArgs(seed=1))
    q, _ = request_struct(r)
    assert q.penalty_set == 0 and _pen(q) == (0.0, 0.0, 0.0, 0)  # as a zero-filled request
    r.args.penalties = Penalties()
    q, _ = request_struct(r)
    assert q.penalty_set == _ffi.PENALTY_SET == 1 and _pen(q) == (1.0, 0.0, 0.0, 0)
    r.args.penalties = Penalties(repetition=1.3, frequency=-0.5, presence=1.5, window=64)
    q, _ = request_struct(r)
    assert q.penalty_set == 1 and _pen(q) == (1.3, -0.5, 1.5, 64)
    r.greedy = True  # penalties go with greedy
    q, _ = request_struct(r)
    assert q.greedy == 1 and q.penalty_set == 1
    assert rwkvtts.Penalties is Penalties


BAD = [Penalties(repetition=0.2), Penalties(repetition=4.5), Penalties(repetition=float("nan")),
       Penalties(repetition=0), Penalties(frequency=8.5), Penalties(frequency=-8.5), Penalties(frequency=float("inf")),
       Penalties(presence=9), Penalties(presence=-9), Penalties(presence=float("nan")), Penalties(window=-1),
       Penalties(window=2049), Penalties(window=1.5), Penalties(window=True), Penalties(repetition="1.3"),
       {"repetition": 1.3}]


@pytest.mark.parametrize("bad", BAD)
def test_pipeline_refuses_bad_penalties_before_generating(bad):
    m = RecordingManager()
    pipe = LightweightTtsPipeline(m, FakeCodec())
    args = LightweightTtsPipelineArgs(text="abc", penalties=bad)
    with pytest.raises(ValueError):
        pipe.generate_speech(args)
    with pytest.raises(ValueError):
        pipe.generate_speech_batch([LightweightTtsPipelineArgs(text="ok"), args])
    with pytest.raises(ValueError):
        pipe.stream_speech(args)
    with pytest.raises(ValueError):
        pipe.generate_long_speech(args)
    with pytest.raises(ValueError):
        next(pipe.stream_long_speech(args))  # a generator: it checks at its first item
    with pytest.raises(ValueError):
        next(pipe.stream_request(pipe._request(args)))
    assert not m.seen


def test_range_ends_are_accepted():
    for p in (Penalties(0.25, -8.0, -8.0, 0), Penalties(4.0, 8.0, 8.0, 2048), Penalties(1, 0, 0, 0)):
        assert p.check() is p


def test_pipeline_passes_penalties_through():
    m = RecordingManager()
    pipe = LightweightTtsPipeline(m, FakeCodec())
    pen = Penalties(1.2, 0.5, 0.25, 16)
    args = LightweightTtsPipelineArgs(text="abc", seed=4, penalties=pen)
    pipe.generate_speech(args)
    pipe.generate_speech_batch([args])
    list(pipe.stream_speech(args))
    assert len(m.structs) == 3
    for q in m.structs:
        assert q.penalty_set == 1 and _pen(q) == (1.2, 0.5, 0.25, 16)
    assert all(r.args.penalties is pen for r in m.seen)
    pipe.generate_speech(LightweightTtsPipelineArgs(text="abc"))
    assert m.structs[-1].penalty_set == 0 and m.seen[-1].args.penalties is None
    # every request the pipeline builds from these arguments carries them (the long-form entry
    # points derive each segment's request from this one with dataclasses.replace)
    assert pipe._request(args).args.penalties is pen


def test_http_bodies_set_the_request_fields(tmp_path):
    m = RecordingManager()
    pipe = LightweightTtsPipeline(m, FakeCodec())

    def both(body):
        """(status of /api/tts, status of the streaming route), each with the struct it submitted."""
        n = len(m.structs)
        c1, _ = SV.handle_tts_json(json.dumps(body), pipe, str(tmp_path))
        c2, it = SV.handle_tts_stream(body, pipe, str(tmp_path))
        b"".join(it)
        return (c1, c2), m.structs[n:]

    codes, qs = both({"text": "hi", "penalties": {"repetition": 1.3, "window": 32}})
    assert codes == (200, 200) and len(qs) == 2
    for q in qs:
        assert q.penalty_set == 1 and _pen(q) == (1.3, 0.0, 0.0, 32)
    codes, qs = both({"text": "hi", "penalties": {"frequency": 0.5, "presence": -0.25}})
    assert codes == (200, 200) and [_pen(q) for q in qs] == [(1.0, 0.5, -0.25, 0)] * 2
    codes, qs = both({"text": "hi", "penalties": {}})  # an empty object: the neutral values, set
    assert codes == (200, 200) and [(q.penalty_set, _pen(q)) for q in qs] == [(1, (1.0, 0.0, 0.0, 0))] * 2
    codes, qs = both({"text": "hi", "penalties": {"presence": 1.0},
                      "semantic_sampling": {"temperature": 0.8}})  # together with per-phase sampling
    assert codes == (200, 200)
    for q in qs:
        assert q.penalty_set == 1 and q.sampling_set == _ffi.SAMPLING_SEMANTIC and _pen(q) == (1.0, 0.0, 1.0, 0)
    codes, qs = both({"text": "hi"})  # absent: the request is unchanged
    assert codes == (200, 200) and [q.penalty_set for q in qs] == [0, 0]
    codes, qs = both({"text": "hi", "penalties": None})
    assert codes == (200, 200) and [q.penalty_set for q in qs] == [0, 0]
    for bad in ({"repetition": 9}, {"repetition": 0.1}, {"repetition": "high"}, {"frequency": -9}, {"frequency": True},
                {"presence": 8.5}, {"window": -1}, {"window": 4096}, {"window": 1.5}, {"min_p": 0.1},
                {"repetition_penalty": 1.3}, [1.3], "1.3", 1.3):
        codes, qs = both({"text": "hi", "penalties": bad})
        assert codes == (400, 400) and not qs, bad
        code, payload = SV.handle_tts_json({"text": "hi", "penalties": bad}, pipe, str(tmp_path))
        assert code == 400 and payload["success"] is False and isinstance(payload["error"], str)
