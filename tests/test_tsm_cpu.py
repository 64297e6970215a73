"""Time stretch (WSOLA) without a GPU: the host-only entry points against the arithmetic contract
(include/rwkvtts.h), the plan's properties, TimeStretchStream over the numpy
restatement (tests/tsm_ref.py), the contract's sanity on a periodic signal, and `tempo` in the
server and the pipeline."""
import base64
import ctypes
import inspect
import json
import math

import numpy as np
import pytest

import tsm_ref
from rwkvtts import _ffi, audio
from rwkvtts import server as SV
from rwkvtts.pipeline import SpeechChunk

F32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _desc(window, search):
    return _ffi.TsmDesc(struct_size=ctypes.sizeof(_ffi.TsmDesc), window=window, search=search)


def _plan_rc(desc, tempo, n_known, final, block_first, s_prev):
    end, first = ctypes.c_int64(-7), ctypes.c_int64(-7)
    rc = _ffi.lib().rwkvtts_tsm_plan(ctypes.byref(desc), tempo, n_known, final, block_first, s_prev,
                                     ctypes.byref(end), ctypes.byref(first))
    return rc, end.value, first.value


# ---- out_len, window, EINVAL ----------------------------------------------------------------------
def test_out_len_and_window_follow_the_contract():
    L = _ffi.lib()
    for W, D in ((512, 128), (64, 10), (32, 5), (2048, 1024), (0, 0)):
        d = _desc(W, D)
        Wv = W or 512
        tab = np.full(Wv, -1.0, F32)
        assert L.rwkvtts_tsm_window(ctypes.byref(d), tab.ctypes.data_as(ctypes.c_void_p)) == 0
        assert np.array_equal(bits(tab), bits(tsm_ref.window(Wv)))
        assert np.array_equal(bits(tab), bits(audio._tsm_window(Wv)))
        assert tab[0] == 0.0 and tab[Wv // 2] == 1.0
        for tempo in (0.25, 0.5, 0.8, 1.0, 1.25, 1.37, 2.0, 4.0):
            for n in (0, 1, 2, 3, 255, 256, 257, 20000, 163840, 2 ** 31 + 5):
                want = 0 if n == 0 else int(math.ceil(float(n) / tempo))
                assert L.rwkvtts_tsm_out_len(ctypes.byref(d), tempo, n) == want == tsm_ref.out_len(n, tempo)
    ts = audio.TimeStretcher(window=0, search=0, evaluator=tsm_ref.evaluator)
    assert (ts.window, ts.search, ts.hop) == (512, 128, 256)  # 0 is the default, in both fields


def test_out_of_range_is_einval_everywhere():
    """search = 0 means the default (128), as window = 0 means 512: it is the desc's "unset", not a
    radius. A negative search, and one above 1024, are out of range."""
    L = _ffi.lib()
    tab = np.zeros(4096, F32)
    bad_descs = [_desc(511, 128), _desc(30, 8), _desc(2050, 8), _desc(-512, 8), _desc(512, -1), _desc(512, 1025),
                 _ffi.TsmDesc(struct_size=4, window=512, search=128)]
    for d in bad_descs:
        assert L.rwkvtts_tsm_window(ctypes.byref(d), tab.ctypes.data_as(ctypes.c_void_p)) == _ffi.EINVAL
        assert L.rwkvtts_tsm_out_len(ctypes.byref(d), 1.0, 100) == -1
        assert _plan_rc(d, 1.0, 100, 0, 0, -256)[0] == _ffi.EINVAL
        h = ctypes.c_void_p()
        assert L.rwkvtts_tsm_create(0, ctypes.byref(d), None, ctypes.byref(h)) == _ffi.EINVAL and not h.value
    assert not np.any(tab)
    good = _desc(512, 128)
    for tempo in (0.2, 4.5, float("nan"), 0.0, -1.0, float("inf")):
        assert L.rwkvtts_tsm_out_len(ctypes.byref(good), tempo, 100) == -1
        rc, end, first = _plan_rc(good, tempo, 100, 0, 0, -256)
        assert rc == _ffi.EINVAL and (end, first) == (-7, -7)
        ts = audio.TimeStretcher(evaluator=tsm_ref.evaluator)
        with pytest.raises(_ffi.RwkvTtsError):
            ts.stream(tempo)
    assert L.rwkvtts_tsm_out_len(ctypes.byref(good), 1.0, -1) == -1
    # s_prev must be a possible start of frame block_first - 1
    assert _plan_rc(good, 1.0, 5000, 0, 0, 0)[0] == _ffi.EINVAL        # block 0: -Hs
    assert _plan_rc(good, 1.0, 5000, 0, 1, 3)[0] == _ffi.EINVAL        # frame 0 starts at 0
    assert _plan_rc(good, 1.0, 5000, 0, 2, 256 + 128)[0] == _ffi.EINVAL  # frame 1: [a - D, a + D)
    assert _plan_rc(good, 1.0, 5000, 0, 2, 256 + 127)[0] == 0
    for bad in ((30, 8), (511, 128), (512, -1)):
        with pytest.raises(_ffi.RwkvTtsError):
            audio.TimeStretcher(window=bad[0], search=bad[1], evaluator=tsm_ref.evaluator)


# ---- plan -----------------------------------------------------------------------------------------
def _random_state(rng, W, D, tempo):
    Hs = W // 2
    bf = int(rng.integers(0, 40))
    if bf == 0:
        s_prev = -Hs
    elif bf == 1:
        s_prev = 0
    else:
        s_prev = tsm_ref.anchor(bf - 1, Hs, tempo) + int(rng.integers(-D, D))
    return bf, s_prev


def test_plan_properties():
    rng = np.random.default_rng(11)
    for W, D in ((512, 128), (64, 10), (32, 5)):
        Hs = W // 2
        ts = audio.TimeStretcher(window=W, search=D, evaluator=tsm_ref.evaluator)
        for _ in range(120):
            tempo = float(rng.choice([0.25, 0.5, 0.8, 1.0, 1.25, 1.37, 2.0, 4.0, rng.uniform(0.25, 4.0)]))
            bf, s_prev = _random_state(rng, W, D, tempo)
            prev_end = None
            n0 = int(rng.integers(0, 30 * W))
            for n_known in sorted({n0, n0 + 1, n0 + Hs, n0 + int(rng.integers(0, 8 * W)), n0 + 40 * W}):
                end, first = ts.plan(tempo, n_known, False, bf, s_prev)
                assert end % Hs == 0 and end >= bf * Hs
                if end > bf * Hs:
                    assert end <= ts.out_len(n_known, tempo)
                assert prev_end is None or end >= prev_end            # monotone in n_known
                prev_end = end
                assert first == max(0, min(s_prev + Hs, tsm_ref.anchor(bf, Hs, tempo) - D))
                # at least as eager as: block j ready when ceil((j+1) Hs tempo) + D + 2 Hs <= n_known
                j = bf
                while math.ceil((j + 1) * Hs * tempo) + D + 2 * Hs <= n_known:
                    j += 1
                assert end >= j * Hs, (W, D, tempo, n_known, bf, s_prev, end, j)
                # final: the signal's output length
                assert ts.plan(tempo, n_known, True, bf, s_prev)[0] == ts.out_len(n_known, tempo)


def test_plan_is_sound():
    """Two signals that share x[:n_known] and differ after it have identical outputs below
    out_ready_end (and identical starts of the frames those blocks use)."""
    rng = np.random.default_rng(12)
    for W, D in ((64, 10), (32, 5), (128, 40)):
        Hs = W // 2
        ts = audio.TimeStretcher(window=W, search=D, evaluator=tsm_ref.evaluator)
        for _ in range(40):
            tempo = float(rng.choice([0.25, 0.5, 0.8, 1.0, 1.25, 1.37, 2.0, 4.0, rng.uniform(0.25, 4.0)]))
            n = int(rng.integers(4 * W, 30 * W))
            n_known = int(rng.integers(0, n))
            x1 = rng.standard_normal(n).astype(F32)
            x2 = x1.copy()
            x2[n_known:] = rng.standard_normal(n - n_known).astype(F32) * F32(3.0)
            y1, s1 = tsm_ref.stretch(x1, tempo, W, D, return_starts=True)
            y2, s2 = tsm_ref.stretch(x2, tempo, W, D, return_starts=True)
            # from the start, and from a later block with the carried start
            end0, _ = ts.plan(tempo, n_known, False, 0, -Hs)
            assert np.array_equal(bits(y1[:end0]), bits(y2[:end0])) and s1[:end0 // Hs + 1] == s2[:end0 // Hs + 1]
            if end0 >= 2 * Hs:
                bf = int(rng.integers(1, end0 // Hs))
                end, _ = ts.plan(tempo, n_known, False, bf, s1[bf])
                assert end >= end0                                   # (the known start is never worse than the worst case)
                assert end <= len(y1) and np.array_equal(bits(y1[:end]), bits(y2[:end])), (W, D, tempo, n, n_known, bf)
                assert s1[:end // Hs + 1] == s2[:end // Hs + 1]


# ---- stream ---------------------------------------------------------------------------------------
def test_stream_is_bitwise_the_whole_signal():
    rng = np.random.default_rng(13)
    W, D = 64, 10
    Hs = W // 2
    log = []

    def ev(stretcher, items):
        log.extend(items)
        return tsm_ref.evaluator(stretcher, items)

    ts = audio.TimeStretcher(window=W, search=D, evaluator=ev)
    x = (rng.standard_normal(1500) * 0.3).astype(F32)
    for tempo in (0.25, 0.8, 1.0, 1.37, 4.0):
        whole = ts.stretch(x, tempo)
        assert np.array_equal(bits(whole), bits(tsm_ref.stretch(x, tempo, W, D)))
        keep_max = 2 * D + math.ceil(W * max(tempo, 1.0)) + 2     # the stated bound on the kept tail
        cuts = [[1] * x.size, [7] * (x.size // 7 + 1), [Hs - 1] * (x.size // (Hs - 1) + 1), [Hs] * (x.size // Hs + 1),
                [W + 1] * (x.size // (W + 1) + 1), [int(v) for v in rng.integers(0, 3 * W, 60)] + [x.size]]
        for sizes in cuts:
            for last_is_empty in (False, True):
                st = ts.stream(tempo)
                parts, pos = [], 0
                for n in sizes:
                    last = pos + n >= x.size
                    parts.append(st.feed(x[pos:pos + n], final=last and not last_is_empty))
                    pos += n
                    if last:
                        break
                    assert st.kept <= keep_max, (st.kept, keep_max)
                if last_is_empty:
                    assert st.kept <= keep_max
                    parts.append(st.feed(np.zeros(0, F32), final=True))
                got = np.concatenate(parts)
                assert got.dtype == F32 and np.array_equal(bits(got), bits(whole)), (tempo, sizes[0], last_is_empty)
                assert all(p.size % Hs == 0 for p in parts[:-1])   # whole blocks until the end
                assert st.kept == 0
                with pytest.raises(ValueError):
                    st.feed(x[:1])
    assert all(it[-1] > 0 for it in log)   # nothing goes to the evaluator while no block is ready
    # signals of length 0, 1 and Hs - 1
    for tempo in (0.5, 1.0, 2.0):
        for n in (0, 1, Hs - 1):
            st = ts.stream(tempo)
            got = np.concatenate([st.feed(x[:n // 2]), st.feed(x[n // 2:n], final=True)])
            assert got.size == ts.out_len(n, tempo) and np.array_equal(bits(got), bits(ts.stretch(x[:n], tempo)))


def test_chained_streams_are_bitwise_the_resample_of_the_stretch():
    """The pipeline's stage fold (pipeline.audio_stages / feed_stages, what stream_request runs per
    vocoder chunk) over both stand-ins: stretch first, then resample, `final` reaching both streams,
    stretched items that are empty passing through the resampler's stream."""
    from rwkvtts.pipeline import audio_stages, feed_stages
    from test_resample_cpu import _contract_evaluator
    ts = audio.TimeStretcher(window=64, search=10, evaluator=tsm_ref.evaluator)
    rs = audio.Resampler(16000, 24000, align="zero", evaluator=_contract_evaluator([]))
    x = (np.random.default_rng(21).standard_normal(6000) * 0.3).astype(F32)
    sizes = [1, 7, 640, 319, 1, 2048, 0, 33, 640, 2311]
    assert sum(sizes) == x.size
    for tempo in (0.8, 1.37):
        want = rs.resample(ts.stretch(x, tempo))
        stages = audio_stages(ts, tempo, rs)
        assert len(stages) == 2
        one = x
        for batch, _ in stages:
            one = batch([one])[0]
        assert np.array_equal(bits(one), bits(want))
        streams = [stream() for _, stream in stages]
        parts, pos = [], 0
        for n in sizes:
            parts.append(feed_stages(streams, x[pos:pos + n], False))
            pos += n
        assert any(p.size == 0 for p in parts)
        parts.append(feed_stages(streams, np.zeros(0, F32), True))
        got = np.concatenate(parts)
        assert got.dtype == F32 and got.size == want.size and np.array_equal(bits(got), bits(want)), tempo
        assert [s.kept for s in streams] == [0, 0]
        for s in streams:
            with pytest.raises(ValueError):
                s.feed(x[:1])
    assert audio_stages(None, None, None) == [] and feed_stages([], x, True) is x


# ---- the contract's sanity ------------------------------------------------------------------------
def test_contract_on_a_periodic_signal():
    sr = 16000
    t = np.arange(sr, dtype=np.float64) / sr
    x = (0.5 * np.sin(2 * np.pi * 200 * t) + 0.3 * np.sin(2 * np.pi * 400 * t)).astype(F32)

    def rms(v):
        return float(np.sqrt(np.mean(v.astype(np.float64) ** 2)))

    ref = rms(x[1024:-1024])
    for tempo in (0.5, 0.8, 1.25, 2.0):
        y = tsm_ref.stretch(x, tempo, 512, 128)
        assert y.size == math.ceil(sr / tempo)
        r = rms(y[1024:-1024]) / ref
        assert abs(r - 1.0) < 0.01, (tempo, r)
    y, s = tsm_ref.stretch(x, 1.0, 512, 128, return_starts=True)
    assert s == [256 * m for m in range(-1, len(s) - 1)]        # every shift 0
    assert y.size == x.size and float(np.max(np.abs(y - x))) <= 2e-7
    z, s = tsm_ref.stretch(np.zeros(3000, F32), 1.37, 64, 10, return_starts=True)
    assert not np.any(z) and s[2:] == [tsm_ref.anchor(m, 32, 1.37) for m in range(1, len(s) - 1)]  # silence: shift 0


# ---- server: stand-in pipelines in the style of tests/test_server.py --------------------------------
class PlainPipeline:
    """The pipeline surface as it was before `sample_rate` and `tempo`: any extra keyword is a TypeError."""
    def __init__(self):
        self.calls = []

    def generate_speech(self, args):
        self.calls.append(("generate_speech", {}))
        return np.linspace(-0.5, 0.5, 960, dtype=F32)

    def stream_speech(self, args, chunk_frames=16):
        self.calls.append(("stream_speech", {"chunk_frames": chunk_frames}))
        yield SpeechChunk.make(np.full(320, 0.25, F32), 0, 1, 1, True)


class KeywordPipeline:
    def __init__(self):
        self.calls = []

    def generate_speech(self, args, **kw):
        self.calls.append(("generate_speech", kw))
        return np.linspace(-0.5, 0.5, 960, dtype=F32)

    def stream_speech(self, args, **kw):
        self.calls.append(("stream_speech", kw))
        yield SpeechChunk.make(np.full(320, 0.25, F32), 0, 1, 1, True)


def test_server_tempo_validation():
    assert (SV.TEMPO_MIN, SV.TEMPO_MAX) == (0.5, 2.0)
    for bad in (0.49, 2.01, "1.2", True, False, [1.2], {"x": 1}, 0, -1.0, 1e9):
        q = KeywordPipeline()
        code, out = SV.handle_tts_json({"text": "hi", "tempo": bad}, q)
        assert code == 400 and out["success"] is False and set(out) == {"success", "error"} and q.calls == [], bad
        code, it = SV.handle_tts_stream({"text": "hi", "tempo": bad}, q)
        assert code == 400 and json.loads(b"".join(it).decode("utf-8")) == out and q.calls == []
    q = KeywordPipeline()
    code, out = SV.handle_tts_json('{"text": "hi", "tempo": NaN}', q)   # (json.loads accepts the NaN literal)
    assert code == 400 and q.calls == []
    for ok in (0.5, 2.0, 1.2, 2, 1):
        assert SV.handle_tts_json({"text": "hi", "tempo": ok}, KeywordPipeline())[0] == 200


def test_server_passes_each_keyword_only_when_set():
    # without tempo, or with 1.0 (or the integer 1, or null): exactly the calls of before
    for body in ({"text": "hi"}, {"text": "hi", "tempo": 1.0}, {"text": "hi", "tempo": 1}, {"text": "hi", "tempo": None},
                 {"text": "hi", "tempo": 1.0, "sample_rate": 16000}):
        p = PlainPipeline()
        code, out = SV.handle_tts_json(json.dumps(body), p)
        assert code == 200 and out["success"]
        assert base64.b64decode(out["audio_base64"]) == SV.convert_samples_to_wav(np.linspace(-0.5, 0.5, 960, dtype=F32))
        code, it = SV.handle_tts_stream(body, p, chunk_frames=4)
        assert code == 200 and len(list(it)) == 2
        assert p.calls == [("generate_speech", {}), ("stream_speech", {"chunk_frames": 4})]
    assert "tempo" not in inspect.signature(PlainPipeline.generate_speech).parameters
    cases = [({"tempo": 1.25}, {"tempo": 1.25}), ({"tempo": 2}, {"tempo": 2.0}),
             ({"sample_rate": 24000}, {"sample_rate": 24000}),
             ({"sample_rate": 24000, "tempo": 1.0}, {"sample_rate": 24000}),
             ({"sample_rate": 16000, "tempo": 0.8}, {"tempo": 0.8}),
             ({"sample_rate": 48000, "tempo": 0.5}, {"sample_rate": 48000, "tempo": 0.5})]
    for extra, want in cases:
        p = KeywordPipeline()
        body = dict({"text": "hi", "speed": 1.4}, **extra)
        code, out = SV.handle_tts_json(body, p)
        assert code == 200 and p.calls == [("generate_speech", want)]
        assert isinstance(p.calls[0][1].get("tempo", 0.0), float)
        rate = want.get("sample_rate", 16000)
        assert int.from_bytes(base64.b64decode(out["audio_base64"])[24:28], "little") == rate
        code, it = SV.handle_tts_stream(body, p, chunk_frames=8)
        parts = list(it)
        assert code == 200 and int.from_bytes(parts[0][24:28], "little") == rate
        assert p.calls[1] == ("stream_speech", dict({"chunk_frames": 8}, **want))


def test_stream_handler_skips_empty_items():
    """A stretched stream item may be empty (its blocks wait for the next chunk): no empty body part
    goes out, which a chunked response would read as its end."""
    class P(KeywordPipeline):
        def stream_speech(self, args, **kw):
            yield SpeechChunk.make(np.zeros(0, F32), 0, 1, 3, False)
            yield SpeechChunk.make(np.full(320, 0.25, F32), 1, 2, 3, False)
            yield SpeechChunk.make(np.zeros(0, F32), 2, 3, 3, True)
    code, it = SV.handle_tts_stream({"text": "hi", "tempo": 1.5}, P(), chunk_frames=1)
    parts = list(it)
    assert code == 200 and len(parts) == 2 and all(parts) and parts[1] == SV.samples_to_pcm16(np.full(320, 0.25, F32))


# ---- pipeline -------------------------------------------------------------------------------------
def test_pipeline_tempo_none_creates_nothing():
    """tempo None / 1.0: no stretcher, the stand-in codec's PCM as it is (tests/test_server.py's
    stand-ins know nothing of time stretching); a tempo out of range fails before anything is generated."""
    from rwkvtts.pipeline import LightweightTtsPipeline, LightweightTtsPipelineArgs
    from test_server import FakeCodec, FakeManager
    pipe = LightweightTtsPipeline(FakeManager(), FakeCodec())
    a = LightweightTtsPipelineArgs(text="hi")
    for tempo in (None, 1.0, 1):
        assert np.array_equal(pipe.generate_speech(a, tempo=tempo), pipe.generate_speech(a))
        assert np.array_equal(pipe.generate_speech(a, sample_rate=16000, tempo=tempo), pipe.generate_speech(a))
        assert len(pipe.generate_speech_batch([a, a], tempo=tempo)) == 2
        assert pipe.stretcher(tempo) is None
    assert pipe._stretcher is None and pipe._resamplers == {}
    for name in ("generate_speech", "generate_speech_batch", "stream_speech", "stream_request"):
        par = inspect.signature(getattr(LightweightTtsPipeline, name)).parameters
        assert par["tempo"].default is None
    for bad in (0.2, 4.5, float("nan")):
        with pytest.raises(ValueError):
            pipe.generate_speech(a, tempo=bad)
    assert pipe._stretcher is None
    # the failed request's second of silence is not stretched (and needs no stretcher on a device)
    pipe._stretcher = audio.TimeStretcher(evaluator=tsm_ref.evaluator)
    sil = pipe.generate_speech(LightweightTtsPipelineArgs(text="\U0001F600"), tempo=2.0)
    assert sil.shape == (16000,) and not np.any(sil)
    # and a real request goes through it: ceil(n / tempo) samples, bitwise the restatement
    pcm = pipe.generate_speech(a)
    fast = pipe.generate_speech(a, tempo=2.0)
    assert fast.size == math.ceil(pcm.size / 2.0) and np.array_equal(bits(fast), bits(tsm_ref.stretch(pcm, 2.0)))
    both = pipe.generate_speech_batch([a, a], tempo=0.5)
    assert all(np.array_equal(bits(b), bits(tsm_ref.stretch(pcm, 0.5))) for b in both)
