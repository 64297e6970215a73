"""The formant shift without a GPU (include/rwkvtts.h): the library's table against the
float64 restatement, the plan's reach against the reads of the numpy restatement (tests/formant_ref.py),
the interpolator alone against exact band-limited evaluation, FormantStream over the restatement, and
`formant_shift` through the server's validation."""
import json
import math

import numpy as np
import pytest

import formant_ref as FR
import pitch_ref
from rwkvtts import audio
from rwkvtts import server as SV
from test_pitch_cpu import FakePipeline, _dominant_lag, _small_voiced, bits

F32 = np.float32
U = 2.0 ** -24
# a range whose grain read reaches further than its period frames (window + lag_max = 20 < 16 * 1.41 + 8)
REACHY = dict(hop=8, window=4, lag_min=4, lag_max=16, unvoiced=8)


@pytest.fixture(scope="module")
def ps():
    return audio.PitchShifter(evaluator=FR.evaluator, **REACHY)


@pytest.mark.parametrize("semis", [-6.0, -3.0, 0.0, 4.0, 6.0])
def test_the_library_table_is_the_restatement(ps, semis):
    B = ps.formant_ratio(semis)
    assert B == FR.ratio(semis) and 46341 <= B <= 92682
    tab = ps.formant_table(B)
    assert np.array_equal(bits(tab), bits(FR.table(B)))
    # h = fl(v / sum v): each of the 16 roundings moves a tap by at most u |h|, and the doubles sum to 1
    for row in tab.astype(np.float64):
        assert abs(math.fsum(row) - 1.0) <= U * math.fsum(np.abs(row)) * (1.0 + U) + 2.0 ** -48
    if B <= 65536:  # cutoff 1: an integer position reads the sample itself
        assert np.array_equal(tab[0], np.eye(16, dtype=F32)[7])
    for bad in (46340, 92683, 0, -65536):
        with pytest.raises(Exception):
            ps.formant_table(bad)
    for bad in (6.001, -6.5, float("nan"), True):
        with pytest.raises(ValueError):
            ps.formant_ratio(bad)


@pytest.mark.parametrize("semis", [-6.0, 6.0])
def test_the_plan_covers_what_the_restatement_reads(ps, semis):
    """Every window a stream would cut reads inside [in_first_needed, n_known) and equals the whole."""
    x = _small_voiced(700, period=16, seed=3)  # p = lag_max
    B, f = ps.formant_ratio(semis), audio.pitch_factor(3.0)
    tab = ps.formant_table(B)
    want = FR.shift(x, f, B, tab, **REACHY)
    reach = (16 * B + 65535 >> 16) + 8
    done, first, state, parts = 0, 0, (0, 0), []
    for known in list(range(37, x.size, 37)) + [x.size]:
        final = known == x.size
        end, need = ps.plan(known, final, done, *state, B)
        assert need >= first and (final or end == max(0, known - (32 + max(20, reach))))
        first = min(need, known)
        if end > done:
            y, a, s, lo, hi = FR.window(x[first:known], first, final, f, B, tab, done, *state, end - done,
                                        want_reads=True, **REACHY)
            assert (lo >= first or first == 0) and (hi < known or final), (known, lo, hi, first)
            parts.append(y)
            done, state = end, (a, s)
    assert np.array_equal(bits(np.concatenate(parts)), bits(want))
    if semis > 0:  # the grain read, not the period frames, sets this range's look-ahead
        assert reach > 20 and ps.stream(3.0, semis).lag == 32 + reach > ps.lookahead


@pytest.mark.parametrize("semis", [-6.0, -3.0, -0.5, 3.0, 6.0])
def test_the_plan_never_asks_for_less_than_the_pitch_plan(semis):
    """A window cut by the formant plan also passes the pitch stage's own check (default range: a read
    slower than 1 reaches less than lag_max)."""
    sh = audio.PitchShifter(evaluator=FR.evaluator)
    pitch, formant = sh.plan(5000, False, 2000, 900, 1500), sh.plan(5000, False, 2000, 900, 1500, sh.formant_ratio(semis))
    assert formant[0] <= pitch[0] and formant[1] <= pitch[1] == 580


# measured: against the exact value at the read position, and at the position truncated
# to its phase (the table's own error); the gate is 1.5 times each -- the figures are deterministic, a
# read one phase or one tap off at least doubles the first, and 1.5 leaves room for another libm
MEASURED = {46341: (4.31e-3, 4.2e-7), 92682: (4.35e-3, 8.2e-4)}


@pytest.mark.parametrize("B", sorted(MEASURED))
def test_the_interpolator_against_exact_band_limited_evaluation(B):
    comps = ((200.0, 0.3, 0.1), (700.0, 0.3, 1.3), (1500.0, 0.3, 2.1))  # Hz, amplitude, phase: all below the cutoff

    def exact(pos):
        return sum(a * np.sin(2.0 * np.pi * hz * pos / 16000.0 + ph) for hz, a, ph in comps)

    x = exact(np.arange(4000, dtype=np.float64)).astype(F32)
    P = np.random.default_rng(5).integers(100 << 16, 3900 << 16, 20000, dtype=np.int64)
    xi = FR.interpolate(x, P, FR.table(B))[0].astype(np.float64)
    total, tab = np.abs(xi - exact(P / 65536.0)).max(), np.abs(xi - exact(((P >> 10) << 10) / 65536.0)).max()
    print(B, "total", total, "table", tab)
    assert total <= 1.5 * MEASURED[B][0] and tab <= 1.5 * MEASURED[B][1]
    assert total <= 2.0 * np.pi * 0.9 * (200 + 700 + 1500) / 3 / 16000.0 / 64 + tab  # the truncation's own bound


def resonant_vowel(n=16000, f0=120.0, fc=1000.0, bw=100.0, fs=16000.0):
    """An impulse train at f0 through one resonance at fc, peak 0.5."""
    x, t = np.zeros(n), 0.0
    while t < n:
        x[int(t)] = 1.0
        t += fs / f0
    r, th = np.exp(-np.pi * bw / fs), 2.0 * np.pi * fc / fs
    y, y1, y2 = np.zeros(n), 0.0, 0.0
    for i in range(n):
        y[i] = x[i] + 2.0 * r * np.cos(th) * y1 - r * r * y2
        y2, y1 = y1, y[i]
    return (y * 0.5 / np.abs(y).max()).astype(F32)


def strongest_harmonic(y, fs=16000.0):
    return float(np.argmax(np.abs(np.fft.rfft(y.astype(np.float64) * np.hanning(y.size))))) * fs / y.size


def keeps_the_period_and_moves_the_envelope(y, semis):
    """The output's period within one sample of the input's (120 Hz: 133.3), as §25 measures it, and
    its strongest harmonic within one harmonic spacing of 1000 Hz * beta."""
    lag, peak = _dominant_lag(y), strongest_harmonic(y)
    print(semis, "lag", lag, "peak", peak, "want", 1000.0 * 2.0 ** (semis / 12.0))
    return abs(lag - 16000.0 / 120.0) <= 1.0 and abs(peak - 1000.0 * 2.0 ** (semis / 12.0)) <= 120.0


@pytest.mark.parametrize("semis", [-6.0, -3.0, 3.0, 6.0])
def test_the_restatement_keeps_the_period_and_moves_the_envelope(semis):
    sh = audio.PitchShifter(evaluator=FR.evaluator)
    assert keeps_the_period_and_moves_the_envelope(sh.shift(resonant_vowel(), 0.0, semis), semis)


@pytest.mark.parametrize("chunk", [100, 277])
def test_the_stream_is_exact_over_chunks_and_composes_with_pitch(ps, chunk):
    x = np.concatenate([_small_voiced(900, period=7, seed=1), np.zeros(150, F32)])
    for pitch, formant in ((0.0, 4.0), (-5.0, 6.0), (3.0, -3.0)):
        want = ps.shift(x, pitch, formant)
        assert not np.array_equal(bits(want), bits(ps.shift(x, pitch)))
        st = ps.stream(pitch, formant)
        got, fed = [], 0
        for i in range(0, x.size, chunk):
            got.append(st.feed(x[i:i + chunk], final=i + chunk >= x.size))
            fed = min(i + chunk, x.size)
            assert fed - sum(g.size for g in got) <= st.lag or fed == x.size
        assert np.array_equal(bits(np.concatenate(got)), bits(want))
    assert type(ps.stream(2.0)) is audio.PitchStream and type(ps.stream(2.0, 0.0)) is audio.PitchStream
    assert np.array_equal(bits(ps.shift(x, 2.0, 0.0)), bits(pitch_ref.shift(x, audio.pitch_factor(2.0), **REACHY)))


@pytest.mark.parametrize("bad", [True, "3", float("nan"), float("inf"), -6.5, 6.001, 12, [3]])
def test_a_bad_formant_shift_is_a_400_and_the_pipeline_is_not_called(bad):
    p = FakePipeline()
    body = json.dumps({"text": "hello", "formant_shift": bad})
    code, payload = SV.handle_tts_json(body, p)
    assert code == 400 and payload["success"] is False and "-6.0 - 6.0" in payload["error"]
    code2, it = SV.handle_tts_stream(body, p)
    assert code2 == 400 and json.loads(b"".join(it).decode("utf-8")) == payload
    assert p.calls == []


def test_the_keyword_is_passed_only_when_set():
    p = FakePipeline()
    for body in ({"text": "x"}, {"text": "x", "formant_shift": None}, {"text": "x", "formant_shift": 0}):
        assert SV.handle_tts_json(body, p)[0] == 200 and SV.handle_tts_stream(body, p)[0] == 200
    assert [c[:2] for c in p.calls] == [("generate_speech", {}), ("stream_speech", {})] * 3
    p.calls.clear()
    assert SV.handle_tts_json({"text": "x", "formant_shift": -4, "pitch_shift": 2}, p)[0] == 200
    assert p.calls[0][1] == {"pitch_shift": 2.0, "formant_shift": -4.0} and type(p.calls[0][1]["formant_shift"]) is float


def test_the_pipeline_folds_it_into_the_pitch_stage():
    from rwkvtts.pipeline import LightweightTtsPipeline, LightweightTtsPipelineArgs
    from test_server import FakeCodec, FakeManager
    pipe = LightweightTtsPipeline(FakeManager(), FakeCodec())
    a = LightweightTtsPipelineArgs(text="hi")
    plain = pipe.generate_speech(a)
    assert np.array_equal(bits(pipe.generate_speech(a, formant_shift=0.0)), bits(plain)) and pipe._shifter is None
    for bad in (6.5, float("nan"), True):
        with pytest.raises(ValueError):
            pipe.generate_speech(a, formant_shift=bad)
        with pytest.raises(ValueError):
            pipe.stream_speech(a, formant_shift=bad)
    sh = pipe._shifter = audio.PitchShifter(evaluator=FR.evaluator)
    B = sh.formant_ratio(-4.0)
    want = FR.shift(plain, audio.pitch_factor(2.0), B, sh.formant_table(B))
    assert np.array_equal(bits(pipe.generate_speech(a, formant_shift=-4.0, pitch_shift=2.0)), bits(want))
    assert np.array_equal(bits(pipe.generate_speech_batch([a], formant_shift=-4.0, pitch_shift=2.0)[0]), bits(want))
    from rwkvtts.pipeline import audio_stages
    (_, stream), = audio_stages(None, None, None, shifter=sh, pitch_shift=2.0, formant_shift=-4.0)
    st = stream()
    parts = [st.feed(plain[i:i + 3000], final=i + 3000 >= plain.size) for i in range(0, plain.size, 3000)]
    assert type(st) is audio.FormantStream and np.array_equal(bits(np.concatenate(parts)), bits(want))
    alone = FR.shift(plain, 1.0, B, sh.formant_table(B))
    assert np.array_equal(bits(pipe.generate_speech(a, formant_shift=-4.0)), bits(alone))
