"""The join stage's contract without a GPU: properties of its numpy restatement (tests/join_ref.py),
the library's host-only entry points (ramp, capacity, the refusal of a bad description), and
audio.Joiner with the restatement standing in for the kernels."""
import ctypes

import numpy as np
import pytest

import join_ref
from rwkvtts import _ffi, audio

F32 = np.float32


def signal(n, k, lead, trail):
    rng = np.random.default_rng(k)
    x = (rng.standard_normal(n) * 0.002).clip(-0.009, 0.009).astype(F32)
    if n - trail > lead:
        x[lead:n - trail] = (rng.standard_normal(n - trail - lead) * 0.3).astype(F32)
        x[lead], x[n - trail - 1] = 0.4, -0.4
    return x


SEGS = [signal(3000, 1, 500, 700), signal(0, 2, 0, 0), signal(120, 3, 0, 0), signal(900, 4, 900, 0),
        signal(2000, 5, 10, 1980)]
GAPS = [4800, 0, 1, 960, 0]


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


@pytest.mark.parametrize("trim", [True, False])
@pytest.mark.parametrize("keep,fade", [(800, 80), (0, 0), (50, 4096), (10 ** 6, 7)])
def test_per_segment_joins_concatenate_to_the_jobs_join(trim, keep, fade):
    y, ab = join_ref.join(SEGS, GAPS, 0.01, keep, fade, trim)
    parts = [join_ref.join([s], [g], 0.01, keep, fade, trim) for s, g in zip(SEGS, GAPS)]
    assert np.array_equal(bits(y), bits(np.concatenate([p for p, _ in parts])))
    assert ab == [b[0] for _, b in parts]
    assert y.size == sum(b - a for a, b in ab) + sum(GAPS)


def test_trim_off_is_plain_concatenation_with_gaps():
    y, ab = join_ref.join(SEGS, GAPS, 0.01, 800, 80, False)
    want = np.concatenate([np.concatenate([s, np.zeros(g, F32)]) for s, g in zip(SEGS, GAPS)])
    assert np.array_equal(bits(y), bits(want))
    assert ab == [(0, s.size) for s in SEGS]


def test_silence_in_gives_only_gaps_out():
    segs = [np.zeros(1000, F32), np.full(300, 0.01, F32), np.full(7, np.nan, F32), np.zeros(0, F32)]
    y, ab = join_ref.join(segs, [100, 0, 3, 5], 0.01, 800, 80, True)
    assert ab == [(0, 0)] * 4
    assert y.size == 108 and np.array_equal(bits(y), np.zeros(108, np.uint32))  # +0.0f


def test_bounds_and_fades():
    x = signal(3000, 1, 500, 700)
    (a, b), = join_ref.join([x], [0], 0.01, 100, 16, True)[1]
    assert (a, b) == (400, 2400)
    y = join_ref.join([x], [0], 0.01, 100, 16, True)[0]
    r = join_ref.ramp(16)
    assert np.array_equal(bits(y[:16]), bits(x[400:416] * r))
    assert np.array_equal(bits(y[-16:]), bits(x[2384:2400] * r[::-1]))
    assert np.array_equal(bits(y[16:-16]), bits(x[416:2384]))
    # both edges fade whether or not a cut was made there
    z = np.full(40, 0.5, F32)
    yz, ((az, bz),) = join_ref.join([z], [0], 0.01, 0, 4, True)
    assert (az, bz) == (0, 40) and yz[0] == F32(0.5) * r4(0) and yz[39] == F32(0.5) * r4(0) and yz[4] == F32(0.5)
    # len < 2 * fade: f = len // 2, the middle sample of an odd piece is copied
    w, _ = join_ref.join([np.full(5, 0.5, F32)], [0], 0.01, 0, 64, True)
    r64 = join_ref.ramp(64)
    h = F32(0.5)
    assert np.array_equal(bits(w), bits(np.array([h * r64[0], h * r64[1], h, h * r64[1], h * r64[0]], F32)))


def r4(k):
    return join_ref.ramp(4)[k]


def test_threshold_zero_means_the_default():
    x = np.zeros(50, F32)
    x[20] = 0.005
    assert join_ref.join([x], [0], 0.0, 0, 0, True)[1] == [(0, 0)]
    assert join_ref.join([x], [0], 0.004, 0, 0, True)[1] == [(20, 21)]


# ---- the library's host-only entry points --------------------------------------------------------
def desc(threshold=0.01, keep=800, fade=80, trim=1):
    return _ffi.JoinDesc(ctypes.sizeof(_ffi.JoinDesc), threshold, keep, fade, trim)


@pytest.mark.parametrize("fade", [0, 1, 2, 3, 80, 1000, 4096])
def test_library_ramp_equals_the_python_table(fade):
    out = np.full(max(fade, 1), -1.0, dtype=F32)
    d = desc(fade=fade)
    assert _ffi.lib().rwkvtts_join_ramp(ctypes.byref(d), out.ctypes.data_as(ctypes.c_void_p)) == 0
    assert np.array_equal(bits(out[:fade]), bits(audio._join_ramp(fade)))
    assert np.array_equal(bits(audio._join_ramp(fade)), bits(join_ref.ramp(fade)))
    if fade:
        assert 0.0 < out[0] <= out[fade - 1] < 1.0 and (fade == 1 or out[0] < out[fade - 1])


@pytest.mark.parametrize("kw", [{"fade": 4097}, {"fade": -1}, {"keep": -1}, {"trim": 2}, {"trim": -1},
                                {"threshold": -1e-9}, {"threshold": float("nan")}, {"threshold": float("inf")}])
def test_bad_descriptions_are_refused(kw):
    out = np.zeros(8192, dtype=F32)
    d = desc(**kw)
    assert _ffi.lib().rwkvtts_join_ramp(ctypes.byref(d), out.ctypes.data_as(ctypes.c_void_p)) == _ffi.EINVAL
    small = desc()
    small.struct_size = 8
    assert _ffi.lib().rwkvtts_join_ramp(ctypes.byref(small), out.ctypes.data_as(ctypes.c_void_p)) == _ffi.EINVAL


def test_capacity():
    assert audio.Joiner.capacity([3, 0, 5], [1, 2, 0]) == 11
    assert audio.Joiner.capacity([], []) == 0
    for n, g in (([-1], [0]), ([1], [-1]), ([2 ** 30 + 1], [0]), ([1] * 4097, [0] * 4097)):
        with pytest.raises(_ffi.RwkvTtsError):
            audio.Joiner.capacity(n, g)
    assert audio.Joiner.capacity([2 ** 30] * 3, [0] * 3) == 3 * 2 ** 30  # 64-bit


def test_joiner_with_the_stand_in_evaluator():
    j = audio.Joiner(keep=100, fade=16, evaluator=join_ref.evaluator)
    assert j._h is None
    got = j.join_batch([(SEGS, GAPS), (SEGS[:1], [7])])
    for (segs, gaps), (y, ab) in zip([(SEGS, GAPS), (SEGS[:1], [7])], got):
        ry, rab = join_ref.join(segs, gaps, 0.01, 100, 16, True)
        assert ab == rab and np.array_equal(bits(y), bits(ry))
    y, ab = j.join(SEGS[:1], [7])
    assert np.array_equal(bits(y), bits(got[1][0]))
    with pytest.raises(ValueError):
        j.join([SEGS[0]], [1, 2])
    with pytest.raises(_ffi.RwkvTtsError):
        audio.Joiner(fade=5000, evaluator=join_ref.evaluator)
