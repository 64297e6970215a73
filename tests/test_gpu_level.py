"""The loudness leveller on the GPU: csrc/level.hip against the numpy restatement of its arithmetic
contract (tests/level_ref.py; include/rwkvtts.h), bit for bit -- whole signals at the
lengths where a path changes, a ragged batch with a target per signal, the peak cap and both clamps,
a bounded horizon, exact stream windows with the carried state, and windows a sample short."""
import ctypes

import numpy as np
import pytest

import level_ref
from rwkvtts import _ffi, audio

F32 = np.float32
CONFIGS = [(64, 64, 1), (64, 128, 4)]  # (B, L, A)


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


@pytest.fixture(scope="module")
def lv():
    made = {}

    def get(B=64, L=64, A=1, H=0):
        if (B, L, A, H) not in made:
            made[(B, L, A, H)] = audio.Leveller(device=0, block=B, taps=L, lookahead=A, horizon=H)
        return made[(B, L, A, H)]
    yield get
    for v in made.values():
        v.close()


def _speech(n, k, peak=0.3):
    """Harmonics under a slow envelope with a pause: loud, quiet and gated blocks."""
    rng = np.random.default_rng(2000 + k)
    t = np.arange(n, dtype=np.float64) / 16000.0
    f0 = 110.0 + 13.0 * (k % 7)
    x = sum(np.sin(2 * np.pi * f0 * h * t + rng.uniform(0, 6.28)) / h for h in range(1, 9))
    env = 0.55 + 0.45 * np.sin(2 * np.pi * (3.0 + k % 5) * t + k)
    x = x * env + 0.02 * rng.standard_normal(n)
    if n > 8:
        x[n // 3:n // 3 + n // 5] *= 1e-4  # a pause below the gate
    x = x / max(np.max(np.abs(x)), 1e-9) * peak if n else x
    return x.astype(F32)


def _ref(x, db, B, L, A, H=0):
    return level_ref.level(x, db, block=B, taps=L, lookahead=A, horizon=H)


def _lengths(B, L, A):
    return [0, 1, B - 1, B, B + 1, (A + 1) * B - 1, (A + 1) * B, (A + 1) * B + 1, 7 * B + 13, L - 5, 20 * B + 7]


@pytest.mark.gpu
@pytest.mark.parametrize("B,L,A", CONFIGS)
def test_lengths_bitwise_against_restatement(lv, B, L, A):
    """Every length of the configuration, two targets each, in one launch triple."""
    v = lv(B, L, A)
    cases = [(n, db) for n in _lengths(B, L, A) for db in (-23.0, -16.0)]
    sigs = [_speech(n, k) for k, (n, _) in enumerate(cases)]
    got = v.level_batch(sigs, [db for _, db in cases])
    for (n, db), x, y in zip(cases, sigs, got):
        want = _ref(x, db, B, L, A)
        assert y.dtype == F32 and y.size == n == want.size
        assert np.array_equal(bits(y), bits(want)), (B, L, A, n, db)
    assert v.kernel_ms() > 0.0


@pytest.mark.gpu
def test_ragged_batch_targets_silence_cap_and_clamps(lv):
    """33 ragged signals, a different target each; among them all-silence, a signal that engages the
    peak cap, a quiet one that sits on g_max and a loud one that sits on g_min."""
    B, L, A = 64, 128, 4
    v = lv(B, L, A)
    rng = np.random.default_rng(7)
    sigs = [_speech(int(rng.integers(1, 30 * B)), k, peak=float(rng.uniform(0.02, 0.9))) for k in range(33)]
    dbs = [-40.0 + 30.0 * k / 32.0 for k in range(33)]
    n = 12 * B + 5
    sigs[5] = np.zeros(n, dtype=F32)
    spike = _speech(n, 50, peak=0.01)
    spike[[70, 5 * B + 3, n - 2]] = [0.9, -0.8, 0.7]
    sigs[9], dbs[9] = spike, -16.0
    sigs[17], dbs[17] = (0.02 * np.sin(np.arange(n) * 0.4)).astype(F32), -10.0
    sigs[29], dbs[29] = (0.9 * np.sign(np.sin(np.arange(n) * 0.3))).astype(F32), -40.0
    got = v.level_batch(sigs, dbs)
    for k, (x, db, y) in enumerate(zip(sigs, dbs, got)):
        assert np.array_equal(bits(y), bits(_ref(x, db, B, L, A))), k
    assert np.array_equal(bits(got[5]), bits(sigs[5]))
    C = float(F32(0.891))
    assert 0.5 * C < np.max(np.abs(got[9])) <= C * (1 + 2.0 ** -20)        # the cap decided the spikes' level
    tail = slice((A + 4) * B, None)
    assert np.array_equal(bits(got[17][tail]), bits(sigs[17][tail] * F32(10.0)))   # g_max
    assert np.array_equal(bits(got[29][tail]), bits(sigs[29][tail] * F32(0.1)))    # g_min
    for y in got:
        assert np.max(np.abs(y), initial=0.0) <= C * (1 + 2.0 ** -20)


@pytest.mark.gpu
def test_horizon(lv):
    B, L, A = 64, 64, 1
    x = _speech(25 * B + 9, 3)
    x[: 10 * B] *= F32(0.1)  # a level change that a memory of 3 blocks forgets
    y3 = lv(B, L, A, 3).level(x, -23.0)
    y0 = lv(B, L, A, 0).level(x, -23.0)
    assert np.array_equal(bits(y3), bits(_ref(x, -23.0, B, L, A, 3)))
    assert np.array_equal(bits(y0), bits(_ref(x, -23.0, B, L, A, 0)))
    assert not np.array_equal(bits(y3), bits(y0))


@pytest.mark.gpu
@pytest.mark.parametrize("B,L,A", CONFIGS)
def test_windows_at_every_cut_offset_carry_the_state(lv, B, L, A):
    """The signal cut once at (A + 6)B - B/2 + o for every o in [0, B): the first windows in one call, then the
    final ones from the plan's tail with the state the first returned. Each pair is the one-shot."""
    v = lv(B, L, A)
    n = (A + 9) * B + 13
    x = _speech(n, 11, peak=0.5)
    x[8 * B + 5] = 0.95  # a peak the cap has to catch across the cut
    want = _ref(x, -20.0, B, L, A)
    assert np.array_equal(bits(v.level(x, -20.0)), bits(want))
    t2 = audio.level_target(-20.0)
    cuts = [(A + 6) * B - B // 2 + o for o in range(B)]
    ends = [v.plan(c, False)[0] for c in cuts]
    assert all(0 < e < n and e % B == 0 for e in ends) and len(set(ends)) == 2
    first = v.level_windows([(x[:c], 0, False, t2, 0, 0.0, 0, 1.0, e) for c, e in zip(cuts, ends)])
    second = []
    for e, (_, S, N, g) in zip(ends, first):
        a = v.plan(n, False, e // B)[1]
        assert 0 < a <= e
        second.append((x[a:], a, True, t2, e // B, S, N, g, n - e))
    for (y1, _, _, _), (y2, S, N, g) in zip(first, v.level_windows(second)):
        assert np.array_equal(bits(np.concatenate([y1, y2])), bits(want))
    # and as the stream does it
    st = v.stream(-20.0)
    parts = [st.feed(p, final=i == 4) for i, p in enumerate(np.split(x, [3, B + 1, 5 * B - 1, 9 * B + 2]))]
    assert np.array_equal(bits(np.concatenate(parts)), bits(want))


@pytest.mark.gpu
def test_a_window_a_sample_short_is_einval_and_writes_nothing(lv):
    B, L, A = 64, 128, 4
    v = lv(B, L, A)
    n = 16 * B
    x = _speech(n, 13)
    t2 = float(audio.level_target(-23.0))
    (y1, S, N, g), = v.level_windows([(x[:10 * B], 0, False, t2, 0, 0.0, 0, 1.0, (10 - A) * B)])
    c = 10 - A
    a = v.plan(n, False, c)[1]
    assert a > 0

    def call(samples, in_first, final, count):
        out = np.full(count, 7.0, dtype=F32)
        w = _ffi.LevelWindow(struct_size=ctypes.sizeof(_ffi.LevelWindow), in_=samples.ctypes.data, in_first=in_first,
                             n_in=samples.size, final=final, t2=t2, block_first=c, s_prev=float(S), n_prev=N,
                             g_prev=float(g), out_count=count, out=out.ctypes.data, s_last=-3.0, n_last=-3, g_last=-3.0)
        rc = _ffi.lib().rwkvtts_level_windows(v._h, ctypes.byref(w), 1)
        return rc, out, (w.s_last, w.n_last, w.g_last)

    good = np.ascontiguousarray(x[a:c * B + (A + 2) * B])
    rc, out, st = call(good, a, 0, 2 * B)
    assert rc == 0 and st[1] >= 0 and not np.any(out == 7.0)
    want = _ref(x, -23.0, B, L, A)
    assert np.array_equal(bits(np.concatenate([y1, out])), bits(want[:(c + 2) * B]))
    for samples, in_first in ((np.ascontiguousarray(good[:-1]), a), (np.ascontiguousarray(good[1:]), a + 1)):
        rc, out, st = call(samples, in_first, 0, 2 * B)
        assert rc == _ffi.EINVAL
        assert np.all(out == 7.0) and st == (-3.0, -3, -3.0)
    # final: a count that passes the signal's end, and one that ends inside a block
    tail = np.ascontiguousarray(x[a:])
    for count in (n - c * B + 1, B + 5):
        rc, out, st = call(tail, a, 1, count)
        assert rc == _ffi.EINVAL and np.all(out == 7.0) and st == (-3.0, -3, -3.0)
    with pytest.raises(_ffi.RwkvTtsError):  # a state no scan can have left
        v.level_windows([(tail, a, True, t2, c, 0.5, 0, 1.0, n - c * B)])


@pytest.mark.gpu
def test_defaults_three_seconds(lv):
    v = audio.Leveller(device=0)
    try:
        assert (v.block, v.taps, v.lookahead) == (1600, 1024, 4)
        x = _speech(48000 + 777, 21, peak=0.25)
        x[30000] = 0.97
        y = v.level(x, -16.0)
        assert np.array_equal(bits(y), bits(level_ref.level(x, -16.0)))
        st = v.stream(-16.0)
        parts = [st.feed(p, final=i == 3) for i, p in enumerate(np.split(x, [5120, 20480, 40000]))]
        assert np.array_equal(bits(np.concatenate(parts)), bits(y))
        assert v.kernel_ms() > 0.0
    finally:
        v.close()
