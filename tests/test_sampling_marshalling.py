"""Per-request sampling parameters from the Python surface down to the C request struct, without
a GPU: runtime.PhaseSampling / SamplerArgs -> request_struct -> _ffi.Request, the pipeline
arguments and both HTTP bodies (/api/tts and its streaming twin), with a stand-in manager that
records the request it is handed. The top-level temperature / top_p / top_k stay ignored, as in
the reference (normal_mode_inference.rs:114-127)."""
import ctypes
import json

import numpy as np
import pytest

import rwkvtts
from rwkvtts import _ffi
from rwkvtts import server as SV
from rwkvtts.pipeline import LightweightTtsPipeline, LightweightTtsPipelineArgs
from rwkvtts.runtime import PhaseSampling, request_struct


class RecordingManager:
    """Stands in for DynamicBatchManager: records each request and its marshalled struct."""
    last_status = [0]

    def __init__(self):
        self.seen, self.structs = [], []

    def _tokens(self, text):
        return [ord(c) % 100 + 12293 for c in text]

    def _record(self, req):
        self.seen.append(req)
        self.structs.append(request_struct(req)[0])

    def generate_tts_batch(self, reqs):
        for r in reqs:
            self._record(r)
        return [([1] * 32, [5, 6, 7]) for _ in reqs]

    def stream_tts(self, req):
        self._record(req)
        yield [1] * 32, [5, 6, 7], True


class FakeCodec:
    def halo(self):
        return 2

    def decode_audio(self, g, s):
        return np.full(len(s) * 320, 0.25, dtype=np.float32)

    def decode_audio_batch(self, items):
        return [self.decode_audio(g, s) for g, s in items]

    def decode_windows(self, wins):
        return [np.full((b - a) * 320, 0.25, dtype=np.float32) for _, _, a, b, _ in wins]


def _phase(p):
    return (round(float(p.temperature), 6), round(float(p.top_p), 6), int(p.top_k))


def test_request_struct_layout_and_marshalling():
    # the struct ends with sampling_set and the two phases, as include/rwkvtts.h declares them
    assert ctypes.sizeof(_ffi.PhaseSampling) == 12
    assert _ffi.Request.sampling_set.offset == _ffi.Request.semantic_seed_offset.offset + 8
    assert _ffi.Request.global_sampling.offset == _ffi.Request.sampling_set.offset + 4
    assert _ffi.Request.semantic_sampling.offset == _ffi.Request.global_sampling.offset + 12
    r = rwkvtts.TtsBatchRequest([1, 2, 3], args=rwkvtts.SamplerArgs(seed=1, temperature=0.3, top_p=0.2, top_k=5))
    q, _ = request_struct(r)
    assert q.sampling_set == 0  # SamplerArgs.temperature / top_p / top_k do nothing
    r.args.semantic_sampling = PhaseSampling(temperature=0.8)
    q, _ = request_struct(r)
    assert q.sampling_set == _ffi.SAMPLING_SEMANTIC and _phase(q.semantic_sampling) == (0.8, 0.95, 80)
    r.args.global_sampling = PhaseSampling(top_p=0.5, top_k=0)
    q, _ = request_struct(r)
    assert q.sampling_set == 3 and _phase(q.global_sampling) == (1.0, 0.5, 0)
    r.args.semantic_sampling = None
    r.args.global_sampling = PhaseSampling()  # top_k None: the phase's own 20
    q, _ = request_struct(r)
    assert q.sampling_set == _ffi.SAMPLING_GLOBAL and _phase(q.global_sampling) == (1.0, 0.95, 20)


@pytest.mark.parametrize("bad", [PhaseSampling(temperature=0.05), PhaseSampling(temperature=4.5),
                                 PhaseSampling(temperature=float("nan")), PhaseSampling(top_p=1.5),
                                 PhaseSampling(top_p=-0.1), PhaseSampling(top_p=float("inf")),
                                 PhaseSampling(top_k=-1), PhaseSampling(top_k=2.5), {"temperature": 0.8}])
def test_pipeline_refuses_bad_sampling_before_generating(bad):
    m = RecordingManager()
    pipe = LightweightTtsPipeline(m, FakeCodec())
    args = LightweightTtsPipelineArgs(text="abc", semantic_sampling=bad)
    with pytest.raises(ValueError):
        pipe.generate_speech(args)
    with pytest.raises(ValueError):
        pipe.generate_speech_batch([LightweightTtsPipelineArgs(text="ok"), args])
    with pytest.raises(ValueError):
        pipe.stream_speech(args)
    with pytest.raises(ValueError):
        next(pipe.stream_request(pipe._request(args)))
    assert not m.seen


def test_pipeline_passes_sampling_through():
    m = RecordingManager()
    pipe = LightweightTtsPipeline(m, FakeCodec())
    sem, glob = PhaseSampling(0.7, 0.9, 50), PhaseSampling(1.3, 1.0, 0)
    args = LightweightTtsPipelineArgs(text="abc", seed=4, semantic_sampling=sem, global_sampling=glob)
    pipe.generate_speech(args)
    pipe.generate_speech_batch([args])
    list(pipe.stream_speech(args))
    assert len(m.structs) == 3
    for q in m.structs:
        assert q.sampling_set == 3 and _phase(q.semantic_sampling) == (0.7, 0.9, 50)
        assert _phase(q.global_sampling) == (1.3, 1.0, 0)
    pipe.generate_speech(LightweightTtsPipelineArgs(text="abc", temperature=0.5, top_p=0.3, top_k=7))
    assert m.structs[-1].sampling_set == 0


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

    codes, qs = both({"text": "hi", "semantic_sampling": {"temperature": 0.8, "top_k": 40}})
    assert codes == (200, 200) and len(qs) == 2
    for q in qs:
        assert q.sampling_set == _ffi.SAMPLING_SEMANTIC and _phase(q.semantic_sampling) == (0.8, 0.95, 40)
    codes, qs = both({"text": "hi", "global_sampling": {"top_p": 1}, "semantic_sampling": {}})
    assert codes == (200, 200)
    for q in qs:
        assert q.sampling_set == 3 and _phase(q.global_sampling) == (1.0, 1.0, 20)
        assert _phase(q.semantic_sampling) == (1.0, 0.95, 80)
    codes, qs = both({"text": "hi"})
    assert codes == (200, 200) and [q.sampling_set for q in qs] == [0, 0]
    codes, qs = both({"text": "hi", "temperature": 0.5, "top_p": 0.4})  # top level: ignored, as before
    assert codes == (200, 200) and [q.sampling_set for q in qs] == [0, 0]
    for bad in ({"temperature": 9}, {"temperature": "hot"}, {"top_p": -1}, {"top_k": -2}, {"top_k": 1.5},
                {"temperature": True}, {"min_p": 0.1}, [0.8], "0.8", 0.8):
        for key in ("global_sampling", "semantic_sampling"):
            codes, qs = both({"text": "hi", key: bad})
            assert codes == (400, 400) and not qs, (key, bad)
            code, payload = SV.handle_tts_json({"text": "hi", key: bad}, pipe, str(tmp_path))
            assert code == 400 and payload["success"] is False and isinstance(payload["error"], str)
