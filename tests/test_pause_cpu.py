"""The pause stage without a GPU: the contract's properties on its numpy restatement
(tests/pause_ref.py; include/rwkvtts.h), PauseStream over the stand-in evaluator
against the one-shot result at every chunking and within its bound on kept samples, the library's
host-only ramp and refusals, `max_pause` in the bodies of both routes with a stand-in pipeline, and
the keyword reaching stand-in stages only when it is set."""
import ctypes
import json

import numpy as np
import pytest

import pause_ref
from rwkvtts import _ffi, audio
from rwkvtts import pipeline as PL
from rwkvtts import server as SV
from rwkvtts.pipeline import SpeechChunk

F32 = np.float32
CONFIGS = [(16, 2, 8), (64, 1, 32)]


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _ps(B=16, H=2, F=8, **kw):
    return audio.PauseShaper(block=B, hang=H, fade=F, evaluator=pause_ref.evaluator, **kw)


def _quiet(n, seed):
    """Noise well under the default threshold 0.01: distinct samples, no loud block."""
    return (np.random.default_rng(seed).uniform(-0.004, 0.004, n)).astype(F32)


def _signal(B, H, runs, seed=1, lead=0, trail=0):
    """lead quiet samples, then a loud block, then for each R in runs a quiet run of exactly R samples
    between loud samples, then trail quiet samples. Loud samples sit so that the quiet RUN (non-active
    blocks) is R long: the hang makes H blocks on either side of a loud block active."""
    parts = [_quiet(lead, seed)]
    loud = np.full(B, 0.5, F32)
    parts.append(loud)
    for i, R in enumerate(runs):
        parts.append(_quiet(R + 2 * H * B, seed + 10 + i))
        parts.append(loud)
    parts.append(_quiet(trail, seed + 99))
    return np.concatenate(parts)


def _is_subsequence_but_for_fades(x, y, max_faded):
    """y's samples appear in x in order, except at most max_faded that do not."""
    pos, miss = 0, 0
    xb, yb = bits(x), bits(y)
    for v in yb:
        hit = np.nonzero(xb[pos:] == v)[0]
        if hit.size:
            pos += int(hit[0]) + 1
        else:
            miss += 1
    return miss <= max_faded


# ---- the restatement's properties ----------------------------------------------------------------
@pytest.mark.parametrize("B,H,F", CONFIGS)
def test_interior_run_of_m_is_kept_whole_and_m_plus_one_is_cut_to_m(B, H, F):
    M = 5 * B  # a multiple of B: R = M exists as a run of whole blocks
    x = _signal(B, H, [M])
    y, cuts = pause_ref.shape(x, M, B, H, F)
    assert cuts == 0 and np.array_equal(bits(y), bits(x))
    x = _signal(B, H, [M + B])
    y, cuts = pause_ref.shape(x, M, B, H, F)
    assert cuts == 1 and y.size == x.size - B
    # R = M + 1 needs a partial block, which only the last block can be: a trailing run instead, below.
    # The kept run is head hd + tail tl = M samples; the faded ones are the 2F around the cut
    s = B + H * B
    hd, tl = M - M // 2, M // 2
    r = pause_ref.ramp(F)
    assert np.array_equal(bits(y[:s + hd - F]), bits(x[:s + hd - F]))
    assert np.array_equal(bits(y[s + hd - F:s + hd]), bits(x[s + hd - F:s + hd] * r[::-1]))
    e = s + M + B
    assert np.array_equal(bits(y[s + hd:s + hd + F]), bits(x[e - tl:e - tl + F] * r))
    assert np.array_equal(bits(y[s + hd + F:]), bits(x[e - tl + F:]))
    assert _is_subsequence_but_for_fades(x, y, 2 * F)


@pytest.mark.parametrize("B,H,F", CONFIGS)
def test_edges_at_tl_and_hd(B, H, F):
    M = 4 * B + 6  # odd halves do not matter: hd = tl + (M odd)
    hd, tl = M - M // 2, M // 2
    loud = np.full(B, 0.5, F32)
    for R, cut in ((tl // B * B, False), (tl // B * B + B, True)):  # leading runs are whole blocks
        x = np.concatenate([_quiet(R + H * B, 3), loud, loud])
        y, cuts = pause_ref.shape(x, M, B, H, F)
        assert cuts == int(cut)
        assert y.size == (x.size - R + tl if cut else x.size)
    # a trailing run ends in a partial block, so every R exists: hd is kept whole, hd + 1 is cut to hd
    for R, cut in ((hd, False), (hd + 1, True), (tl, False), (tl + 1, tl + 1 > hd)):
        x = np.concatenate([loud, _quiet(H * B + R, 4)])
        y, cuts = pause_ref.shape(x, M, B, H, F)
        assert cuts == int(cut), R
        assert y.size == (x.size - R + hd if cut else x.size)
        if cut:
            s = B + H * B
            assert np.array_equal(bits(y[:s + hd - F]), bits(x[:s + hd - F]))
            assert np.array_equal(bits(y[s + hd - F:]), bits(x[s + hd - F:s + hd] * pause_ref.ramp(F)[::-1]))
    # interior: M + 1 cannot exist between whole blocks, M + B is the first that is cut (above);
    # trailing R = M + 1 is cut to hd
    x = np.concatenate([loud, _quiet(H * B + M + 1, 5)])
    assert pause_ref.shape(x, M, B, H, F)[0].size == B + H * B + hd


@pytest.mark.parametrize("B,H,F", CONFIGS)
def test_all_quiet_is_empty_all_loud_is_identical_nan_is_not_loud(B, H, F):
    M = 2 * F
    for n in (0, 1, B, 7 * B + 3):
        y, cuts = pause_ref.shape(_quiet(n, 6), M, B, H, F)
        assert y.size == 0 and cuts == (1 if n else 0)
    x = np.random.default_rng(7).uniform(0.02, 0.9, 9 * B + 5).astype(F32)
    y, cuts = pause_ref.shape(x, M, B, H, F)
    assert cuts == 0 and np.array_equal(bits(y), bits(x))
    x = _quiet(40 * B, 8)
    x[3 * B + 1] = np.nan  # no loud block: a NaN does not compare above the threshold
    assert pause_ref.shape(x, M, B, H, F)[0].size == 0
    x[20 * B] = 0.5
    y, _ = pause_ref.shape(x, M, B, H, F)
    assert 0 < y.size < x.size


def test_every_faded_sample_lies_in_a_block_that_is_not_loud_and_n_out_le_n():
    rng = np.random.default_rng(9)
    for trial in range(40):
        B, H, F = CONFIGS[trial % 2]
        n = int(rng.integers(0, 60 * B))
        x = _quiet(n, 100 + trial)
        for _ in range(int(rng.integers(0, 4))):
            a = int(rng.integers(0, max(n, 1)))
            x[a:a + int(rng.integers(1, 2 * B))] = 0.3
        M = int(rng.integers(2 * F, 2 * F + 10 * B))
        y, cuts = pause_ref.shape(x, M, B, H, F)
        assert y.size <= n
        # samples above the threshold are never faded and never removed: they come through in order
        big = np.abs(x) > F32(0.01)
        assert np.array_equal(bits(x[big]), bits(y[np.abs(y) > F32(0.01)]))
        assert _is_subsequence_but_for_fades(x, y, 2 * F * cuts)


# ---- the stand-in stream -----------------------------------------------------------------------
@pytest.mark.parametrize("B,H,F", CONFIGS)
def test_stream_cut_anywhere_is_bitwise_the_one_shot(B, H, F):
    ps = _ps(B, H, F)
    M = 3 * B + 5
    x = _signal(B, H, [M - B, 5 * B, 2 * B, 9 * B], lead=4 * B + 3, trail=6 * B + 7)
    want, cuts = pause_ref.shape(x, M, B, H, F)
    assert cuts == 4 and np.array_equal(bits(ps.shape_samples_batch([x], [M])[0]), bits(want)) and ps.cuts == [4]

    def run(at):
        st = audio.PauseStream(ps, M)
        parts = np.split(x, at)
        out = [st.feed(p, final=i == len(parts) - 1) for i, p in enumerate(parts)]
        assert st.kept == 0 and st.cuts == cuts and all(o.dtype == F32 for o in out)
        return np.concatenate(out)

    rng = np.random.default_rng(5)
    for _ in range(25):
        at = np.sort(rng.integers(0, x.size + 1, size=int(rng.integers(1, 12))))
        assert np.array_equal(bits(run(at)), bits(want)), at
    for o in range(0, 2 * B, 3):
        assert np.array_equal(bits(run([o + 1, 7 * B + o, 20 * B + o])), bits(want)), o
    assert np.array_equal(bits(run(np.arange(7, x.size, 7))), bits(want))       # every chunk shorter than B
    assert np.array_equal(bits(run(np.arange(1, x.size, B - 1))), bits(want))
    st = audio.PauseStream(ps, M)
    st.feed(x[:1], final=True)
    with pytest.raises(ValueError):
        st.feed(x[:1])


@pytest.mark.parametrize("B,H,F", CONFIGS)
def test_kept_stays_within_the_bound_across_a_silence_many_times_m_long(B, H, F):
    ps = _ps(B, H, F)
    M = 4 * B
    bound = M + (2 * H + 2) * B
    assert ps.kept_bound(M) == bound
    for lead in (0, 40 * M):  # after activity, and leading silence
        x = np.concatenate([_quiet(lead, 1), np.full(B, 0.5, F32), _quiet(60 * M, 2), np.full(B, 0.5, F32), _quiet(30 * M, 3)])
        want = pause_ref.shape(x, M, B, H, F)[0]
        st, out, most = audio.PauseStream(ps, M), [], 0
        for p in np.split(x, np.arange(37, x.size, 37)):
            out.append(st.feed(p))
            most = max(most, st.kept)
            assert st.kept <= bound
        out.append(st.feed(np.zeros(0, F32), final=True))
        assert np.array_equal(bits(np.concatenate(out)), bits(want))
        assert most > M // 2  # (the tail is really kept: the bound is not met by keeping nothing)


def test_empty_and_tiny_streams_and_the_stand_ins_refusals():
    ps = _ps()
    st = ps.stream(20)  # 20 ms at 16 kHz = 320 samples
    assert st.m == 320 and st.feed(np.zeros(0, F32), final=True).size == 0
    assert ps.shape(np.zeros(0, F32), 20).size == 0 and ps.shape_batch([], 20) == []
    x = np.full(5, 0.5, F32)
    st = ps.stream(20)
    assert st.feed(x[:2]).size == 0
    assert np.array_equal(bits(st.feed(x[2:], final=True)), bits(x))
    for bad in (True, 2.5, "20", None):
        with pytest.raises(ValueError):
            ps.samples(bad)
    with pytest.raises(ValueError):
        _ps(16, 2, 200).samples(20)  # 320 samples < 2 * fade
    with pytest.raises(_ffi.RwkvTtsError):
        ps.shape_samples_batch([x], [15])  # M < 2F
    for state in ((1, 0, 0), (1, 1, 16), (0, 1, 0), (2, 1, 8), (2, 2, 0), (-1, 0, 0)):
        with pytest.raises(_ffi.RwkvTtsError):
            ps.shape_windows([(np.zeros(64, F32), 0, False, 32, *state)])


# ---- the library's host-only side -----------------------------------------------------------------
def _desc(**kw):
    return _ffi.PauseDesc(struct_size=ctypes.sizeof(_ffi.PauseDesc), **kw)


def test_the_library_ramp_is_pythons_and_a_bad_desc_is_einval():
    L = _ffi.lib()
    for F in (1, 8, 32, 80, 4096):
        tab = np.full(F, -1.0, F32)
        assert L.rwkvtts_pause_ramp(ctypes.byref(_desc(fade=F)), tab.ctypes.data_as(ctypes.c_void_p)) == 0
        assert np.array_equal(bits(tab), bits(pause_ref.ramp(F))) and np.array_equal(bits(tab), bits(audio._join_ramp(F)))
    tab = np.full(80, -1.0, F32)
    assert L.rwkvtts_pause_ramp(ctypes.byref(_desc()), tab.ctypes.data_as(ctypes.c_void_p)) == 0  # 0 = 80
    assert np.array_equal(bits(tab), bits(pause_ref.ramp(80)))
    for B in (16, 64, 160):
        assert L.rwkvtts_pause_ramp(ctypes.byref(_desc(block=B)), tab.ctypes.data_as(ctypes.c_void_p)) == 0
    tab[:] = -1.0
    bad = [_desc(block=2), _desc(block=18), _desc(block=4100), _desc(hang=-1), _desc(hang=33), _desc(fade=-1),
           _desc(fade=4097), _desc(threshold=-0.5), _desc(threshold=float("nan")), _desc(threshold=float("inf")),
           _ffi.PauseDesc(struct_size=8)]
    for d in bad:
        assert L.rwkvtts_pause_ramp(ctypes.byref(d), tab.ctypes.data_as(ctypes.c_void_p)) == _ffi.EINVAL
        h = ctypes.c_void_p()
        assert L.rwkvtts_pause_create(0, ctypes.byref(d), None, ctypes.byref(h)) == _ffi.EINVAL and not h.value
    assert np.all(tab == -1.0)
    with pytest.raises(_ffi.RwkvTtsError):
        _ps(18, 2, 8)
    p = _ps(0, 0, 0, threshold=0.0)
    assert (p.block, p.hang, p.fade, p.threshold) == (160, 5, 80, float(F32(0.01)))


# ---- the routes ----------------------------------------------------------------------------------
class FakePipeline:
    """generate_speech returns `pcm`; stream_speech yields it in pieces, the first of them empty (a
    request still in its leading silence). Both record their keywords."""

    def __init__(self, pcm):
        self.pcm, self.calls = np.asarray(pcm, dtype=F32), []

    def generate_speech(self, args, **kw):
        self.calls.append(("generate_speech", kw))
        return self.pcm.copy()

    def generate_long_speech(self, args, **kw):
        self.calls.append(("generate_long_speech", kw))
        return PL.LongSpeech.make(self.pcm.copy(), None, [])

    def stream_speech(self, args, chunk_frames=16, **kw):
        self.calls.append(("stream_speech", kw))
        parts = [self.pcm[:0]] + np.array_split(self.pcm, 3)
        for i, c in enumerate(parts):
            yield SpeechChunk.make(c, 0, 0, 0, i == len(parts) - 1)


@pytest.mark.parametrize("bad", [True, False, "300", 19, 5001, 0, -20, 300.0, 299.5, float("nan"), [300], {"ms": 300}])
def test_a_bad_max_pause_is_a_400_and_the_pipeline_is_not_called(bad):
    p = FakePipeline(np.zeros(100))
    body = json.dumps({"text": "hello", "max_pause": bad})
    code, payload = SV.handle_tts_json(body, p)
    assert code == 400 and payload["success"] is False and isinstance(payload["error"], str)
    code2, it = SV.handle_tts_stream(body, p)
    assert code2 == 400 and json.loads(b"".join(it).decode("utf-8")) == payload
    assert p.calls == []


def test_tts_args_carries_the_key_only_when_set():
    base = {"text": "x", "tempo": 1.25, "loudness": -23, "sample_rate": 24000}
    err, args0, kw0 = SV._tts_args(dict(base), "assets/raf")
    assert err is None and "max_pause" not in kw0
    err, args1, kw1 = SV._tts_args(dict(base, max_pause=None), "assets/raf")
    assert err is None and kw1 == kw0 and args1 == args0
    for v in (20, 300, 5000):
        err, args2, kw2 = SV._tts_args(dict(base, max_pause=v), "assets/raf")
        assert err is None and args2 == args0 and kw2 == dict(kw0, max_pause=v) and type(kw2["max_pause"]) is int
    assert (SV.MAX_PAUSE_MIN, SV.MAX_PAUSE_MAX) == (20, 5000)


def test_both_routes_pass_the_keyword_and_the_stream_skips_the_empty_item():
    x = np.random.default_rng(3).uniform(-0.2, 0.2, 700).astype(F32)
    p = FakePipeline(x)
    for body in ({"text": "x"}, {"text": "x", "max_pause": None}):
        assert SV.handle_tts_json(body, p)[0] == 200
        code, it = SV.handle_tts_stream(body, p)
        assert code == 200 and len(list(it)) == 4  # the header and three parts: the empty item is not sent
    assert p.calls == [("generate_speech", {}), ("stream_speech", {})] * 2
    p.calls.clear()
    assert SV.handle_tts_json({"text": "x", "max_pause": 300}, p)[0] == 200
    code, it = SV.handle_tts_stream({"text": "x", "max_pause": 250, "tempo": 1.25}, p)
    parts = list(it)
    assert code == 200 and parts[0] == SV.streaming_wav_header(16000) and b"".join(parts[1:]) == SV.samples_to_pcm16(x)
    assert SV.handle_tts_json({"text": "x", "max_pause": 300, "long_form": True}, p)[0] == 200
    assert p.calls == [("generate_speech", {"max_pause": 300}), ("stream_speech", {"tempo": 1.25, "max_pause": 250}),
                       ("generate_long_speech", {"max_pause": 300})]


# ---- stand-in pipelines ---------------------------------------------------------------------------
class _Codec:
    device = 0


def _pipe(monkeypatch):
    """A pipeline whose pause shaper is the stand-in (no GPU object is created)."""
    real = audio.PauseShaper
    monkeypatch.setattr(audio, "PauseShaper", lambda **kw: real(evaluator=pause_ref.evaluator, **kw))
    return PL.LightweightTtsPipeline(manager=None, codec=_Codec())


def test_pause_shaper_validates_caches_and_takes_a_threshold(monkeypatch):
    p = _pipe(monkeypatch)
    assert p.pause_shaper(None) is None and p._shapers == {}
    for bad in (19, 5001, True, False, float("nan"), 300.5, "300", float("inf")):
        with pytest.raises(ValueError):
            p.pause_shaper(bad)
        with pytest.raises(ValueError):
            p._stages(None, None, max_pause=bad)
    assert p._shapers == {}
    a = p.pause_shaper(300)
    assert a is p.pause_shaper(20) is p.pause_shaper(5000) and list(p._shapers) == [None]
    assert (a.block, a.hang, a.fade, a.threshold) == (160, 5, 80, float(F32(0.01)))
    b = p.pause_shaper(300, threshold=0.05)
    assert b is not a and b.threshold == float(F32(0.05)) and p.pause_shaper(300) is b  # the pipeline's from now on
    for bad in (0.0, -1.0, float("nan"), True):
        with pytest.raises(ValueError):
            p.pause_shaper(300, threshold=bad)


def test_stages_put_the_pause_first_and_only_when_set(monkeypatch):
    p = _pipe(monkeypatch)
    seen = []
    real = PL.audio_stages
    monkeypatch.setattr(PL, "audio_stages", lambda *a, **kw: seen.append(kw) or real(*a, **kw))
    stages, rate = p._stages(None, None)
    assert stages == [] and rate == 16000 and seen == [{}]  # the call it always was
    stages, rate = p._stages(None, None, max_pause=40)
    assert len(stages) == 1 and list(seen[1]) == ["shaper", "max_pause"] and seen[1]["max_pause"] == 40
    x = np.concatenate([np.full(160, 0.5, F32), _quiet(16000, 1), np.full(160, 0.5, F32)])
    want = pause_ref.shape(x, 640)[0]
    batch, stream = stages[0]
    assert np.array_equal(bits(batch([x])[0]), bits(want)) and want.size < x.size
    st = stream()
    got = np.concatenate([st.feed(c, final=i == 4) for i, c in enumerate(np.array_split(x, 5))])
    assert np.array_equal(bits(got), bits(want))

    class Stage:  # a stand-in for every other stage: records the order
        def __init__(self, name):
            self.name, self.stream = name, None
            for m in ("shift_batch", "stretch_batch", "level_batch", "embed_batch", "resample_batch"):
                setattr(self, m, lambda pcm, *a, _n=name: order.append(_n) or pcm)
    order = []
    table = PL.audio_stages(Stage("tempo"), 1.2, Stage("rate"), Stage("level"), -23.0, Stage("pitch"), 2.0,
                            Stage("mark"), 1, 2, shaper=p.pause_shaper(40), max_pause=40)
    pcm = [x]
    for batch, _ in table:
        pcm = batch(pcm)
    assert order == ["pitch", "tempo", "level", "mark", "rate"] and len(table) == 6
    assert np.array_equal(bits(pcm[0]), bits(want))  # the shaper ran first: the others passed its output on
