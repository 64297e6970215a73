"""The pitch shifter without a GPU: the library's host-only entry points against the arithmetic
contract (include/rwkvtts.h), the plan's soundness, PitchStream over the numpy
restatement (tests/pitch_ref.py), the restatement against properties it was not built from (the
period of the output, the place of its spectral envelope), the derived bound where nothing is
shifted, and `pitch_shift` through the server's validation and the pipeline's stage fold."""
import ctypes
import inspect
import json

import numpy as np
import pytest

import level_ref
import pitch_ref
import tsm_ref
from rwkvtts import _ffi, audio
from rwkvtts import server as SV
from rwkvtts.pipeline import SpeechChunk

F32 = np.float32
SMALL = dict(hop=8, window=32, lag_min=4, lag_max=16, unvoiced=8)
U = 2.0 ** -24


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _desc(**kw):
    return _ffi.PitchDesc(struct_size=ctypes.sizeof(_ffi.PitchDesc), **kw)


def _ps(**kw):
    return audio.PitchShifter(evaluator=pitch_ref.evaluator, **kw)


def _noise(n, seed, scale=0.3):
    return (np.random.default_rng(seed).standard_normal(n) * scale).astype(F32)


def _vowel(f0, n=16000, fs=16000.0):
    """A one-sided impulse train at f0 through two resonators (700 / 1200 Hz, 80 / 100 Hz wide), peak 0.5."""
    x = np.zeros(n)
    t = 0.0
    while t < n:
        x[int(t)] = 1.0
        t += fs / f0
    for fc, bw in ((700.0, 80.0), (1200.0, 100.0)):
        r, th = np.exp(-np.pi * bw / fs), 2.0 * np.pi * fc / fs
        a1, a2 = -2.0 * r * np.cos(th), r * r
        y, y1, y2 = np.zeros(n), 0.0, 0.0
        for i in range(n):
            v = x[i] - a1 * y1 - a2 * y2
            y[i], y2, y1 = v, y1, v
        x = y
    return (x * 0.5 / np.abs(x).max()).astype(F32)


def _small_voiced(n, period=5, seed=0):
    """A periodic pulse shape plus a little noise: voiced at the small configuration."""
    shape = np.random.default_rng(seed).uniform(-0.5, 0.5, period)
    x = np.tile(shape, n // period + 1)[:n]
    return (x + np.random.default_rng(seed + 1).standard_normal(n) * 0.01).astype(F32)


VOWELS = {}


def vowel(f0):
    if f0 not in VOWELS:
        VOWELS[f0] = _vowel(f0)
        VOWELS[f0].setflags(write=False)
    return VOWELS[f0]


# ---- tables, defaults, EINVAL ---------------------------------------------------------------------
@pytest.mark.parametrize("lo,hi", [(4, 16), (32, 320), (2, 2), (1000, 1024)])
def test_the_library_table_is_pythons(lo, hi):
    n = (hi - lo + 1) * (hi + lo)
    tab = np.full(n, -1.0, F32)
    d = _desc(lag_min=lo, lag_max=hi, unvoiced=lo)
    assert _ffi.lib().rwkvtts_pitch_table(ctypes.byref(d), tab.ctypes.data_as(ctypes.c_void_p)) == 0
    assert np.array_equal(bits(tab), bits(audio._pitch_table(lo, hi)))
    assert np.array_equal(bits(tab), bits(pitch_ref.table(lo, hi)))
    assert tab.min() > 0.0 and tab.max() <= 1.0  # no zero weight: a covered output has den > 0
    for P in (lo, hi):
        row = tab[pitch_ref.row_offset(P, lo):pitch_ref.row_offset(P, lo) + 2 * P]
        assert np.array_equal(row, row[::-1]) or np.max(np.abs(row - row[::-1])) <= 2 * U  # symmetric
    assert pitch_ref.row_offset(hi, lo) + 2 * hi == n


def test_defaults():
    p = _ps(hop=0, window=0, lag_min=0, lag_max=0, unvoiced=0, theta=0, floor=0)
    assert (p.hop, p.window, p.lag_min, p.lag_max, p.unvoiced) == (160, 640, 32, 320, 80)
    assert (p.theta, p.floor, p.lookahead) == (F32(0.2), F32(1e-3), 640 + 960)
    assert p.table.size == 101728


def test_out_of_range_is_einval_everywhere():
    L = _ffi.lib()
    tab = np.zeros(1 << 21, F32)
    bad = [_desc(hop=-1), _desc(hop=4097), _desc(window=-1), _desc(window=4097), _desc(lag_min=1), _desc(lag_min=1025),
           _desc(lag_min=400), _desc(lag_max=1025), _desc(lag_max=16), _desc(lag_max=-1), _desc(unvoiced=31),
           _desc(unvoiced=321), _desc(unvoiced=-1), _desc(theta=-0.1), _desc(theta=1.5), _desc(theta=float("nan")),
           _desc(floor=-1.0), _desc(floor=float("inf")), _desc(floor=float("nan")), _ffi.PitchDesc(struct_size=8)]
    for d in bad:
        assert L.rwkvtts_pitch_table(ctypes.byref(d), tab.ctypes.data_as(ctypes.c_void_p)) == _ffi.EINVAL
        assert L.rwkvtts_pitch_plan(ctypes.byref(d), 100, 0, 0, 0, 0, None, None) == _ffi.EINVAL
        h = ctypes.c_void_p()
        assert L.rwkvtts_pitch_create(0, ctypes.byref(d), None, ctypes.byref(h)) == _ffi.EINVAL and not h.value
    assert not np.any(tab)
    good = _desc()
    for args in ((-1, 0, 0, 0, 0), (10, 0, -1, 0, 0), (2 ** 30 + 1, 0, 0, 0, 0)):
        assert L.rwkvtts_pitch_plan(ctypes.byref(good), *args, None, None) == _ffi.EINVAL
    with pytest.raises(_ffi.RwkvTtsError):
        _ps(lag_min=1)
    p = _ps(**SMALL)
    x = _noise(200, 1)
    eps = 2.0 ** -52
    for f in (0.5 - eps, 2.0 + 4 * eps, float("nan"), 0.0, -1.0, float("inf")):
        with pytest.raises(_ffi.RwkvTtsError):
            p.shift_windows([(x, 0, True, f, 0, 0, 0, x.size)])
    for s in (-12.001, 12.001, float("nan")):
        with pytest.raises(ValueError):
            p.shift_batch([x], [s])
        with pytest.raises(ValueError):
            p.stream(s)
    assert audio.pitch_factor(12) == 2.0 and audio.pitch_factor(-12) == 0.5 and audio.pitch_factor(0) == 1.0


# ---- the plan ---------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [SMALL, {}], ids=["small", "default"])
def test_plan_follows_its_formulas_and_refuses_impossible_states(cfg):
    p = _ps(**cfg)
    Ha, Wc, hi = p.hop, p.window, p.lag_max
    last = -1
    for n in (0, 1, Wc + 3 * hi - 1, Wc + 3 * hi, Wc + 3 * hi + 1, 5 * Wc + 3, 2 ** 30):
        end, first = p.plan(n, False)
        assert end == max(0, n - (Wc + 3 * hi)) and first == 0 and end >= last  # monotone in n_known
        last = end
        assert p.plan(n, True) == (n, 0)
    e = 10 * hi + 3
    sx = e - hi
    for s in (sx, sx - 1, sx - 2 * hi + 1):
        ay = max(0, s - hi)
        for a in (ay, ay - hi + 1):
            assert p.plan(e + Wc + 3 * hi, False, e, a, s) == (e, max(0, min(a - hi, a // Ha * Ha)))
        for a in (ay + 1, ay - hi, -1):
            with pytest.raises(_ffi.RwkvTtsError):
                p.plan(10 ** 6, False, e, a, s)
    for s in (sx + 1, sx - 2 * hi, -1):
        with pytest.raises(_ffi.RwkvTtsError):
            p.plan(10 ** 6, False, e, max(0, s - hi), s)
    for a, s in ((1, 0), (0, 1)):  # before Lmax outputs are out, the only state is (0, 0)
        with pytest.raises(_ffi.RwkvTtsError):
            p.plan(10 ** 6, False, hi, a, s)


@pytest.mark.parametrize("f", [0.5, 2.0 ** (-3 / 12), 2.0 ** (4 / 12), 2.0])
def test_plan_soundness_outputs_below_ready_end_do_not_depend_on_what_follows(f):
    p = _ps(**SMALL)
    n = 700
    a = _small_voiced(n, 5, 3)
    a[300:420] = _noise(120, 4)  # an unvoiced stretch
    ya = pitch_ref.shift(a, f, **SMALL)
    look = p.window + 3 * p.lag_max
    for n_known in (0, 1, look, look + 1, 200, 333, 512, n - 1):
        b = a.copy()
        b[n_known:] = _small_voiced(n - n_known, 7, 9)  # another period from here on
        b = np.concatenate([b, _noise(100, 5)])          # and longer
        end = p.plan(n_known, False)[0]
        yb = pitch_ref.shift(b, f, **SMALL)
        assert np.array_equal(bits(ya[:end]), bits(yb[:end])), n_known


# ---- streaming exactness ----------------------------------------------------------------------
@pytest.mark.parametrize("cfg,n", [(SMALL, 1500), ({}, 9000)], ids=["small", "default"])
def test_stream_cut_anywhere_is_bitwise_the_one_shot(cfg, n):
    p = _ps(**cfg)
    rng = np.random.default_rng(5)
    x = _small_voiced(n, 5, 6) if cfg else vowel(120)[:n].copy()
    x[n // 3:n // 3 + n // 8] = _noise(n // 8, 7, 0.1)
    for semis in (-12.0, -3.0, 4.0, 12.0):
        want = p.shift(x, semis)
        assert want.size == n
        assert np.array_equal(bits(want), bits(pitch_ref.shift(x, audio.pitch_factor(semis), **cfg)))
        st, parts, pos, kept = p.stream(semis), [], 0, 0
        while pos < n:
            k = int(rng.integers(0, 3 * p.lookahead // 2))
            parts.append(st.feed(x[pos:pos + k], final=pos + k >= n))
            pos += k
            kept = max(kept, st.kept if pos < n else 0)
        got = np.concatenate(parts)
        assert np.array_equal(bits(got), bits(want)), semis
        assert kept < p.window + 9 * p.lag_max + p.hop + 3 * p.lookahead // 2  # the bound, plus one chunk not yet used
        with pytest.raises(ValueError):
            st.feed(x[:1])
    # a window beyond the plan, or a forged state, is refused by the same host-only plan
    with pytest.raises(_ffi.RwkvTtsError):
        p.shift_windows([(x[:n // 2], 0, False, 1.2, 0, 0, 0, n // 2 - p.lookahead + 1)])
    with pytest.raises(_ffi.RwkvTtsError):
        p.shift_windows([(x, 0, True, 1.2, 10 * p.lag_max, 0, 3, 10)])


def test_chained_streams_are_bitwise_the_chained_batches():
    """The pipeline's stage fold: shift, then stretch, then level, then resample, over the stand-ins."""
    from rwkvtts.pipeline import audio_stages, feed_stages
    from test_resample_cpu import _contract_evaluator
    ps = _ps(**SMALL)
    ts = audio.TimeStretcher(window=64, search=10, evaluator=tsm_ref.evaluator)
    lv = audio.Leveller(block=64, taps=64, lookahead=2, evaluator=level_ref.evaluator)
    rs = audio.Resampler(16000, 24000, align="zero", evaluator=_contract_evaluator([]))
    x = _small_voiced(4000, 6, 11)
    x[1000:1500] = _noise(500, 12)
    sizes = [1, 7, 640, 319, 1, 1500, 0, 33, 640, 859]
    assert sum(sizes) == x.size
    want = rs.resample(lv.level(ts.stretch(ps.shift(x, 4.0), 1.25), -20.0))
    stages = audio_stages(ts, 1.25, rs, lv, -20.0, ps, 4.0)
    assert len(stages) == 4
    one = x
    for batch, _ in stages:
        one = batch([one])[0]
    assert np.array_equal(bits(one), bits(want))
    streams = [stream() for _, stream in stages]
    assert isinstance(streams[0], audio.PitchStream)
    parts, pos = [], 0
    for k in sizes:
        parts.append(feed_stages(streams, x[pos:pos + k], False))
        pos += k
    parts.append(feed_stages(streams, np.zeros(0, F32), True))
    got = np.concatenate(parts)
    assert got.size == want.size and np.array_equal(bits(got), bits(want))
    assert audio_stages(None, None, None, None, None, None, None) == []
    assert len(audio_stages(None, None, None, shifter=ps, pitch_shift=2.0)) == 1


# ---- the restatement against properties it was not built from --------------------------------------
def _dominant_lag(y):
    seg = y[2000:14000].astype(np.float64)
    return 32 + int(np.argmax([np.dot(seg[:-l], seg[l:]) for l in range(32, 321)]))


def _envelope_peak(y):
    """Hz of the peak of the 300 Hz-smoothed power spectrum between 300 and 1100 Hz."""
    seg = y[2000:14000].astype(np.float64)
    S = np.abs(np.fft.rfft(seg * np.hanning(seg.size), 16384)) ** 2
    hz = 16000.0 / 16384
    k = int(round(300.0 / hz)) | 1
    sm = np.convolve(S, np.ones(k) / k, mode="same")
    lo, hi = int(300.0 / hz), int(1100.0 / hz)
    return (lo + int(np.argmax(sm[lo:hi]))) * hz


@pytest.mark.parametrize("f0", [90, 120])
def test_the_period_moves_and_the_envelope_stays(f0):
    x = vowel(f0)
    peak_in = _envelope_peak(x)
    for semis in (-5, -3, 4, 7):
        f = audio.pitch_factor(semis)
        y, _, _, per, _, _ = pitch_ref.window(x, 0, True, f, 0, 0, 0, x.size, want_marks=True)
        assert np.mean(per[:100] > 0) >= 0.95
        want = 16000.0 / (f0 * f)
        lag = _dominant_lag(y)
        print(f0, semis, "lag", lag, "want", want, "envelope", _envelope_peak(y), "in", peak_in, "scaled", peak_in * f)
        assert abs(lag - want) <= 1.0  # the integer-period quantisation
        pk = _envelope_peak(y)
        assert abs(pk - peak_in) < abs(pk - peak_in * f)


def _bound(x, grains):
    """|y - x| where every grain over a sample reads that sample: 2 G u |x| (1 + 2^-20) + G 2^-149."""
    return 2.0 * grains * U * np.abs(x.astype(np.float64)) * (1.0 + 2.0 ** -20) + grains * 2.0 ** -149


def _max_cover(pairs, n):
    cover = np.zeros(n + 1, dtype=np.int64)
    for s, _, p in pairs:
        cover[max(0, min(n, s - p))] += 1
        cover[max(0, min(n, s + p))] -= 1
    return int(np.cumsum(cover).max())


def test_noise_silence_and_factor_one_come_back_within_the_derived_bound():
    nz = _noise(16000, 0)
    for theta in (0.2, 0.5):
        y, _, _, per, _, pairs = pitch_ref.window(nz, 0, True, audio.pitch_factor(4), 0, 0, 0, nz.size, want_marks=True,
                                                  theta=theta)
        assert not per.any() and _max_cover(pairs, nz.size) == 2
        assert np.all(np.abs(y.astype(np.float64) - nz) <= _bound(nz, 2))
    z = np.zeros(3000, F32)
    for f in (0.5, 1.0, 2.0):
        assert np.array_equal(bits(pitch_ref.shift(z, f)), bits(z))
    for x in (vowel(90), vowel(120)):
        y, _, _, per, _, pairs = pitch_ref.window(x, 0, True, 1.0, 0, 0, 0, x.size, want_marks=True)
        assert per.any() and all(s == a for s, a, _ in pairs)
        assert np.all(np.abs(y.astype(np.float64) - x) <= _bound(x, _max_cover(pairs, x.size)))


def test_ties_take_the_lower():
    # two lags with equal d: an exactly periodic signal has d = 0 at every multiple of its period
    x = np.tile(np.array([0.5, -0.25, 0.125, 0.375, -0.5], F32), 40)
    per = pitch_ref.periods(x, pitch_ref.config(**SMALL), 0, 10)
    assert list(per) == [5] * 10
    # a synthesis mark half way between two analysis marks: period 8, factor 2 -> marks 0, 4, 8, ..
    x = np.tile(np.array([0.5, -0.25, 0.125, 0.375, -0.5, 0.25, 0.0625, -0.125], F32), 30)
    _, _, _, per, a, pairs = pitch_ref.window(x, 0, True, 2.0, 0, 0, 0, 160, want_marks=True, **SMALL)
    assert list(per[:10]) == [8] * 10 and a[:3] == [0, 8, 16]
    assert pairs[:4] == [(0, 0, 8), (4, 0, 8), (8, 8, 8), (12, 8, 8)]


# ---- server and pipeline --------------------------------------------------------------------------
class FakePipeline:
    def __init__(self):
        self.pcm, self.calls = np.linspace(-0.2, 0.2, 700).astype(F32), []

    def generate_speech(self, args, **kw):
        self.calls.append(("generate_speech", kw, args.pitch))
        return self.pcm.copy()

    def stream_speech(self, args, chunk_frames=16, **kw):
        self.calls.append(("stream_speech", kw, args.pitch))
        yield SpeechChunk.make(self.pcm, 0, 0, 0, True)


@pytest.mark.parametrize("bad", [True, False, "4", "high", float("nan"), -12.5, 12.001, 24, [4], {"st": 4}])
def test_a_bad_pitch_shift_is_a_400_naming_the_range(bad):
    p = FakePipeline()
    body = json.dumps({"text": "hello", "pitch_shift": bad})
    code, payload = SV.handle_tts_json(body, p)
    assert code == 400 and payload["success"] is False and "-12.0 - 12.0" in payload["error"]
    code2, it = SV.handle_tts_stream(body, p)
    assert code2 == 400 and json.loads(b"".join(it).decode("utf-8")) == payload
    assert p.calls == []


def test_the_keyword_is_passed_only_when_set_and_is_not_the_pitch_class():
    p = FakePipeline()
    for body in ({"text": "x"}, {"text": "x", "pitch_shift": None}, {"text": "x", "pitch_shift": 0},
                 {"text": "x", "pitch_shift": 0.0}):
        assert SV.handle_tts_json(body, p)[0] == 200
        assert SV.handle_tts_stream(body, p)[0] == 200
    assert [c[:2] for c in p.calls] == [("generate_speech", {}), ("stream_speech", {})] * 4
    p.calls.clear()
    for v in (4, -3.5, -12, 12.0):
        assert SV.handle_tts_json({"text": "x", "pitch_shift": v, "pitch": "high"}, p)[0] == 200
        code, it = SV.handle_tts_stream({"text": "x", "pitch_shift": v, "tempo": 1.25, "loudness": -20}, p)
        assert code == 200
        list(it)
        assert p.calls == [("generate_speech", {"pitch_shift": float(v)}, SV.map_pitch("high")),
                           ("stream_speech", {"tempo": 1.25, "loudness": -20.0, "pitch_shift": float(v)}, SV.map_pitch(None))]
        assert type(p.calls[0][1]["pitch_shift"]) is float
        p.calls.clear()


def test_pipeline_pitch_shift_none_and_zero_create_nothing():
    from rwkvtts.pipeline import LightweightTtsPipeline, LightweightTtsPipelineArgs
    from test_server import FakeCodec, FakeManager
    pipe = LightweightTtsPipeline(FakeManager(), FakeCodec())
    a = LightweightTtsPipelineArgs(text="hi")
    plain = pipe.generate_speech(a)
    for s in (None, 0, 0.0, -0.0):
        assert np.array_equal(bits(pipe.generate_speech(a, pitch_shift=s)), bits(plain))
        assert len(pipe.generate_speech_batch([a, a], pitch_shift=s)) == 2
        assert pipe.shifter(s) is None
    assert pipe._shifter is None
    for name in ("generate_speech", "generate_speech_batch", "stream_speech", "stream_request", "generate_long_speech",
                 "stream_long_speech"):
        par = inspect.signature(getattr(LightweightTtsPipeline, name)).parameters
        assert list(par)[-1] == "pitch_shift" and par["pitch_shift"].default is None
    for bad in (-12.5, 13, float("nan"), True):
        with pytest.raises(ValueError):
            pipe.generate_speech(a, pitch_shift=bad)
        with pytest.raises(ValueError):
            pipe.generate_speech_batch([a], pitch_shift=bad)
        with pytest.raises(ValueError):
            pipe.stream_speech(a, pitch_shift=bad)
        with pytest.raises(ValueError):
            pipe.generate_long_speech(a, pitch_shift=bad)
        with pytest.raises(ValueError):
            next(pipe.stream_long_speech(a, pitch_shift=bad))
    assert pipe._shifter is None
    # a real request goes through the shifter first: bitwise the restatement of the codec's PCM
    pipe._shifter = audio.PitchShifter(evaluator=pitch_ref.evaluator)
    got = pipe.generate_speech(a, pitch_shift=3.0)
    assert np.array_equal(bits(got), bits(pitch_ref.shift(plain, audio.pitch_factor(3.0))))
    sil = pipe.generate_speech(LightweightTtsPipelineArgs(text="\U0001F600"), pitch_shift=3.0)
    assert sil.shape == (16000,) and not np.any(sil)
