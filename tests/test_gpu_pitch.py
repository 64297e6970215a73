"""The pitch shifter's kernels (csrc/pitch.hip) against the numpy restatement of the arithmetic
contract (tests/pitch_ref.py), bit for bit: whole signals in one ragged batch with a factor per
signal, stream windows with the carried state, refusals with nothing written, ties and edges."""
import ctypes

import numpy as np
import pytest

import pitch_ref
from rwkvtts import _ffi, audio

pytestmark = pytest.mark.gpu
F32 = np.float32
SMALL = dict(hop=8, window=32, lag_min=4, lag_max=16, unvoiced=8)
FACTORS = (0.5, 2.0 ** (-3 / 12), 1.0, 2.0 ** (4 / 12), 2.0)
SEMIS = (-12.0, -3.0, 0.0, 4.0, 12.0)
assert [audio.pitch_factor(s) for s in SEMIS] == list(FACTORS)


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _cfg(p):
    return dict(hop=p.hop, window=p.window, lag_min=p.lag_min, lag_max=p.lag_max, unvoiced=p.unvoiced)


@pytest.fixture(scope="module", params=["small", "default"])
def shifter(request):
    p = audio.PitchShifter(**(SMALL if request.param == "small" else {}))
    yield p
    p.close()


@pytest.fixture(scope="module")
def small():
    p = audio.PitchShifter(**SMALL)
    yield p
    p.close()


def _signal(kind, n, period, seed=0):
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    if n == 0:
        return np.zeros(0, F32)
    if kind == "vowel":  # a decaying pulse shape every `period` samples, a little noise on top
        x = np.zeros(n)
        x[::period] = 1.0
        x = np.convolve(x, np.exp(-np.arange(3 * period) / (0.4 * period)) * np.cos(np.arange(3 * period) * 2.4 / np.sqrt(period)))[:n]
        x = 0.5 * x / max(np.abs(x).max(), 1e-9) + rng.standard_normal(n) * 0.005
    elif kind == "chirp":  # the period glides from `period` to half of it
        ph = 2.0 * np.pi * (t / period + t * t / (2.0 * period * max(n, 1)))
        x = 0.4 * np.sin(ph) + 0.1 * np.sin(2.0 * ph)
    elif kind == "noise":
        x = rng.standard_normal(n) * 0.3
    elif kind == "impulse":
        x = np.zeros(n)
        x[n // 2:n // 2 + 1] = 0.9
    elif kind == "zeros":
        x = np.zeros(n)
    else:  # "last": the last sample only
        x = np.zeros(n)
        x[n - 1:] = -0.7
    return x.astype(F32)


KINDS = ("vowel", "chirp", "noise", "impulse", "zeros", "last")


def test_a_ragged_batch_is_bitwise_the_restatement(shifter):
    p, cfg = shifter, _cfg(shifter)
    lengths = (0, 1, p.lag_min - 1, p.lag_max, p.hop, p.window, p.window + p.lag_max + 1, 3 * p.window + 17, 16000)
    period = 5 if p.lag_max == 16 else 133
    xs, ss = [], []
    for n in lengths:
        for kind in KINDS:
            x = _signal(kind, n, period, seed=n)
            for s in SEMIS:
                xs.append(x)
                ss.append(s)
    got = p.shift_batch(xs, ss)  # one call: every length, kind and factor side by side
    assert p.kernel_ms() > 0.0 and p.walk_ms() > 0.0
    voiced = 0
    for x, s, y in zip(xs, ss, got):
        if x.size == 0:
            assert y.size == 0
            continue
        want, _, _, per, _, _ = pitch_ref.window(x, 0, True, audio.pitch_factor(s), 0, 0, 0, x.size, want_marks=True, **cfg)
        voiced += int(np.any(per))
        assert y.size == x.size and np.array_equal(bits(y), bits(want)), (x.size, s)
        if not x.any():
            assert np.array_equal(bits(y), bits(x))  # silence bit for bit
    assert voiced >= 20  # the voiced path ran
    assert p.shift_batch([], []) == []


def test_windows_over_random_cuts_with_the_carried_state_are_the_whole(shifter):
    p, cfg = shifter, _cfg(shifter)
    rng = np.random.default_rng(17)
    period = 5 if p.lag_max == 16 else 133
    n = 3000 if p.lag_max == 16 else 12000
    sigs = [(_signal("vowel", n, period, 1), FACTORS[3]), (_signal("chirp", n - 77, period, 2), FACTORS[0]),
            (np.concatenate([_signal("noise", n // 2, period, 3), _signal("vowel", n // 2 + 5, period, 4)]), FACTORS[4])]
    wants = [y for y, _, _ in p.shift_windows([(x, 0, True, f, 0, 0, 0, x.size) for x, f in sigs])]
    for (x, f), w in zip(sigs, wants):
        assert np.array_equal(bits(w), bits(pitch_ref.shift(x, f, **cfg)))
    # every signal advances by a random chunk per round; all windows of a round go out in one call
    known = [0] * 3
    done = [0] * 3
    first = [0] * 3
    state = [(0, 0)] * 3
    outs = [[] for _ in sigs]
    while any(d < x.size for d, (x, _) in zip(done, sigs)):
        items, who = [], []
        for i, (x, f) in enumerate(sigs):
            if done[i] >= x.size:
                continue
            known[i] = min(x.size, known[i] + int(rng.integers(1, 2 * p.lookahead)))
            final = known[i] == x.size
            end, _ = p.plan(known[i], final, done[i], *state[i])
            items.append((x[first[i]:known[i]], first[i], final, f, done[i], state[i][0], state[i][1], max(0, end - done[i])))
            who.append(i)
        for i, it, (y, a, s) in zip(who, items, p.shift_windows(items)):
            outs[i].append(y)
            done[i] += it[-1]
            state[i] = (a, s)
            first[i] = min(p.plan(known[i], False, done[i], a, s)[1], known[i])  # the tail a stream keeps
    for o, w in zip(outs, wants):
        assert len(o) >= 3 and np.array_equal(bits(np.concatenate(o)), bits(w))


def test_the_stream_is_exact_over_chunks(small):
    x = _signal("vowel", 2500, 5, 8)
    for semis in (-7.0, 5.0):
        want = small.shift(x, semis)
        st = small.stream(semis)
        got = np.concatenate([st.feed(x[:700]), st.feed(x[700:701]), st.feed(x[701:2000]), st.feed(x[2000:], final=True)])
        assert np.array_equal(bits(got), bits(want))


def _raw(p, x, in_first, final, f, out_first, a, s, count):
    w = (_ffi.PitchWindow * 1)()
    out = np.full(max(count, 1), 7.0, F32)
    w[0].struct_size = ctypes.sizeof(_ffi.PitchWindow)
    w[0].in_, w[0].in_first, w[0].n_in, w[0].final = x.ctypes.data, in_first, x.size, final
    w[0].factor, w[0].out_first, w[0].a_prev, w[0].s_prev = f, out_first, a, s
    w[0].out_count, w[0].out, w[0].a_last, w[0].s_last = count, out.ctypes.data, -5, -6
    rc = _ffi.lib().rwkvtts_pitch_windows(p._h, w, 1)
    return rc, out, (w[0].a_last, w[0].s_last)


def test_refusals_write_nothing(small):
    p = small
    x = _signal("vowel", 1000, 5, 3)
    look, hi = p.lookahead, p.lag_max
    ok = _raw(p, x, 0, 0, 1.5, 0, 0, 0, x.size - look)
    assert ok[0] == 0 and not np.any(ok[1] == 7.0) and ok[2][0] >= 0
    a, s = ok[2]
    refused = [
        (x, 0, 0, 1.5, 0, 0, 0, x.size - look + 1),          # beyond the plan
        (x, 0, 1, 1.5, 0, 0, 0, x.size + 1),                  # past a final signal's end
        (x[50:], 50, 1, 1.5, 0, 0, 0, 100),                   # reads before the given samples
        (x, 0, 1, 1.5, 10 * hi, 0, 3, 50),                    # forged states
        (x, 0, 1, 1.5, 10 * hi, 9 * hi - hi, 9 * hi + 1, 50),
        (x, 0, 1, 1.5, 10 * hi, 8 * hi + 1, 9 * hi, 50),
        (x, 0, 1, 1.5, hi, 0, 1, 50),
        (x, 0, 1, 0.5 - 2.0 ** -54, 0, 0, 0, 50), (x, 0, 1, 2.0 + 2.0 ** -51, 0, 0, 0, 50),
        (x, 0, 1, float("nan"), 0, 0, 0, 50),
        (x, 0, 1, 1.5, 0, 0, 0, -1),
    ]
    for r in refused:
        rc, out, st = _raw(p, *r)
        assert rc == _ffi.EINVAL and np.all(out == 7.0) and st == (-5, -6), r
    # and the state the good call left is accepted where it belongs
    rc, out, _ = _raw(p, x, 0, 1, 1.5, x.size - look, a, s, look)
    assert rc == 0 and np.array_equal(bits(out), bits(pitch_ref.shift(x, 1.5, **SMALL)[x.size - look:]))
    lib = _ffi.lib()
    d1, d2 = (ctypes.c_double * 1)(0.5 - 2.0 ** -54), (ctypes.c_double * 1)(float("nan"))
    outs, ins, lens, ous = p._ragged([x], [x.size])
    outs[0][:] = 7.0
    d3 = (ctypes.c_double * 1)(2.0 + 2.0 ** -51)
    for d in (d1, d2, d3):
        assert lib.rwkvtts_pitch_batch(p._h, ins, lens, d, 1, ous) == _ffi.EINVAL and np.all(outs[0] == 7.0)


def test_ties_and_edges(small):
    p = small
    # two lags with equal d: an exactly periodic signal has d = 0 at every multiple of its period;
    # the lowest wins, which the output shows (period 5, not 10 or 15)
    x5 = np.tile(np.array([0.5, -0.25, 0.125, 0.375, -0.5], F32), 60)
    # a synthesis mark half way between two analysis marks: period 8 at factor 2 -> marks 0, 4, 8, ..
    x8 = np.tile(np.array([0.5, -0.25, 0.125, 0.375, -0.5, 0.25, 0.0625, -0.125], F32), 40)
    _, _, _, per, a, pairs = pitch_ref.window(x8, 0, True, 2.0, 0, 0, 0, x8.size, want_marks=True, **SMALL)
    assert per[0] == 8 and pairs[1] == (4, 0, 8) and pairs[3] == (12, 8, 8)
    # a partial last frame, and a signal shorter than one grain
    xp = _signal("vowel", 8 * 37 + 3, 5, 5)
    xs = [x5, x5, x8, x8, xp, xp, xp[:7]]
    ss = [4.0, -12.0, 12.0, -5.0, 3.0, -3.0, 12.0]
    for x, s, y in zip(xs, ss, p.shift_batch(xs, ss)):
        assert np.array_equal(bits(y), bits(pitch_ref.shift(x, audio.pitch_factor(s), **SMALL))), (x.size, s)


def test_a_non_finite_sample_touches_nothing_before_its_look_ahead(small):
    p = small
    x = _signal("vowel", 1200, 5, 6)
    bad = x.copy()
    bad[800] = np.nan
    bad[900] = np.inf
    clean, got = p.shift_batch([x, bad], [4.0, 4.0])
    end = p.plan(800, False)[0]
    assert got.size == x.size and np.array_equal(bits(got[:end]), bits(clean[:end]))
