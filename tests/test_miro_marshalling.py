"""Mirostat from the Python surface down to the C extension block, without a GPU:
runtime.Mirostat / SamplerArgs -> request_ext -> _ffi.RequestExt (with _ffi.Request untouched), the
pipeline arguments of all five entry points and both HTTP bodies (/api/tts and its streaming twin),
with a stand-in manager that records the request it is handed."""
import ctypes
import json

import pytest

import rwkvtts
from rwkvtts import _ffi
from rwkvtts import server as SV
from rwkvtts.pipeline import LightweightTtsPipeline, LightweightTtsPipelineArgs
from rwkvtts.runtime import Mirostat, Penalties, PhaseSampling, request_ext, request_struct
from test_sampling_marshalling import FakeCodec, RecordingManager


def _miro(x):
    return (x.mirostat_set, round(float(x.mirostat.tau), 6), round(float(x.mirostat.rate), 6))


def test_ext_layout_and_marshalling():
    # rwkvtts_request_ext as include/rwkvtts.h declares it
    assert ctypes.sizeof(_ffi.RequestExt) == 16
    assert (_ffi.RequestExt.struct_size.offset, _ffi.RequestExt.mirostat_set.offset, _ffi.RequestExt.mirostat.offset) == (0, 4, 8)
    assert [n for n, _ in _ffi.MirostatParams._fields_] == ["tau", "rate"]
    # rwkvtts_request ends where it ended, at its penalties: the new parameters did not grow it
    assert ctypes.sizeof(_ffi.Request) == (_ffi.Request.penalties.offset + 16 + 7) // 8 * 8
    assert not any("miro" in n for n, _ in _ffi.Request._fields_)
    for name in ("rwkvtts_generate_batch_ex", "rwkvtts_manager_submit_ex", "rwkvtts_debug_advance_miro", "rwkvtts_debug_lg2"):
        assert name in _ffi.EXPORTS
    r = rwkvtts.TtsBatchRequest([1, 2, 3], args=rwkvtts.SamplerArgs(seed=1))
    assert r.args.mirostat is None and request_ext(r) is None  # no block: the plain entry points
    before = bytes(request_struct(r)[0])
    r.args.mirostat = Mirostat()  # ai00's defaults
    x = request_ext(r)
    assert x.struct_size == 16 and _miro(x) == (_ffi.MIROSTAT_SET, 3.0, 0.1) and _ffi.MIROSTAT_SET == 1
    assert bytes(request_struct(r)[0]) == before  # the request struct does not know about it
    r.args.mirostat = Mirostat(tau=5.5, rate=0.25)
    assert _miro(request_ext(r)) == (1, 5.5, 0.25)
    r.args.penalties = Penalties(presence=1.0)  # together with penalties: one in each struct
    assert request_struct(r)[0].penalty_set == 1 and _miro(request_ext(r)) == (1, 5.5, 0.25)
    assert rwkvtts.Mirostat is Mirostat


BAD = [Mirostat(tau=0.4), Mirostat(tau=10.5), Mirostat(tau=float("nan")), Mirostat(tau=float("inf")), Mirostat(tau=0),
       Mirostat(rate=0.0005), Mirostat(rate=1.5), Mirostat(rate=0), Mirostat(rate=-0.1), Mirostat(rate=float("nan")),
       Mirostat(tau=True), Mirostat(tau="3"), {"tau": 3.0}, 3.0]


def _refused_everywhere(pipe, m, args):
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


@pytest.mark.parametrize("bad", BAD)
def test_pipeline_refuses_bad_mirostat_before_generating(bad):
    m = RecordingManager()
    _refused_everywhere(LightweightTtsPipeline(m, FakeCodec()), m, LightweightTtsPipelineArgs(text="abc", mirostat=bad))


def test_pipeline_refuses_the_excluded_combination_before_generating():
    m = RecordingManager()
    args = LightweightTtsPipelineArgs(text="abc", mirostat=Mirostat(), semantic_sampling=PhaseSampling(temperature=0.8))
    _refused_everywhere(LightweightTtsPipeline(m, FakeCodec()), m, args)


def test_range_ends_are_accepted():
    for p in (Mirostat(0.5, 0.001), Mirostat(10.0, 1.0), Mirostat(10, 1), Mirostat()):
        assert p.check() is p


def test_pipeline_passes_mirostat_through():
    m = RecordingManager()
    pipe = LightweightTtsPipeline(m, FakeCodec())
    miro = Mirostat(4.0, 0.2)
    args = LightweightTtsPipelineArgs(text="abc", seed=4, mirostat=miro, global_sampling=PhaseSampling(temperature=0.9))
    pipe.generate_speech(args)
    pipe.generate_speech_batch([args])
    list(pipe.stream_speech(args))
    assert len(m.seen) == 3  # (the two long-form entry points join on the GPU: tests/test_gpu_generate_miro.py)
    assert all(r.args.mirostat is miro and _miro(request_ext(r)) == (1, 4.0, 0.2) for r in m.seen)
    assert all(q.sampling_set == _ffi.SAMPLING_GLOBAL for q in m.structs)
    pipe.generate_speech(LightweightTtsPipelineArgs(text="abc"))
    assert m.seen[-1].args.mirostat is None and request_ext(m.seen[-1]) is None
    # every request the pipeline builds from these arguments carries them (the long-form entry
    # points derive each segment's request from this one with dataclasses.replace)
    assert pipe._request(args).args.mirostat is miro


def test_http_bodies_set_the_ext(tmp_path):
    m = RecordingManager()
    pipe = LightweightTtsPipeline(m, FakeCodec())

    def both(body):
        """(status of /api/tts, status of the streaming route), each with the request it submitted."""
        n = len(m.seen)
        c1, _ = SV.handle_tts_json(json.dumps(body), pipe, str(tmp_path))
        c2, it = SV.handle_tts_stream(body, pipe, str(tmp_path))
        b"".join(it)
        return (c1, c2), [request_ext(r) for r in m.seen[n:]]

    codes, xs = both({"text": "hi", "mirostat": {"tau": 4.0, "rate": 0.5}})
    assert codes == (200, 200) and [_miro(x) for x in xs] == [(1, 4.0, 0.5)] * 2
    codes, xs = both({"text": "hi", "mirostat": {"tau": 2}})  # a key left out keeps its default
    assert codes == (200, 200) and [_miro(x) for x in xs] == [(1, 2.0, 0.1)] * 2
    codes, xs = both({"text": "hi", "mirostat": {}})  # an empty object: ai00's defaults, set
    assert codes == (200, 200) and [_miro(x) for x in xs] == [(1, 3.0, 0.1)] * 2
    codes, xs = both({"text": "hi", "mirostat": {"rate": 1.0}, "penalties": {"presence": 1.0},
                      "global_sampling": {"temperature": 0.8}})  # the combinations that are allowed
    assert codes == (200, 200) and [_miro(x) for x in xs] == [(1, 3.0, 1.0)] * 2
    assert all(q.penalty_set == 1 and q.sampling_set == _ffi.SAMPLING_GLOBAL for q in m.structs[-2:])
    codes, xs = both({"text": "hi"})  # absent: the request is unchanged
    assert codes == (200, 200) and xs == [None, None]
    codes, xs = both({"text": "hi", "mirostat": None})
    assert codes == (200, 200) and xs == [None, None]
    for bad in ({"tau": 11}, {"tau": 0.1}, {"tau": "high"}, {"rate": 0}, {"rate": 2}, {"rate": True}, {"eta": 0.1},
                {"learning_rate": 0.1}, [3.0], "3.0", 3.0, True):
        codes, xs = both({"text": "hi", "mirostat": bad})
        assert codes == (400, 400) and not xs, bad
        code, payload = SV.handle_tts_json({"text": "hi", "mirostat": bad}, pipe, str(tmp_path))
        assert code == 400 and payload["success"] is False and isinstance(payload["error"], str)
    # Mirostat replaces the semantic phase's sampling: the two together are a 400
    codes, xs = both({"text": "hi", "mirostat": {}, "semantic_sampling": {"temperature": 0.8}})
    assert codes == (400, 400) and not xs
