"""The join stage on the GPU: csrc/join.hip against the numpy restatement of its arithmetic contract
(tests/join_ref.py; include/rwkvtts.h), bit for bit -- the cut bounds, the faded
edges, the gaps and the layout, for both trim values, ragged jobs in one call, and the edge cases of
the bounds (a segment's first and last sample, NaN and infinities, a sample equal to the threshold)
and of the fades (pieces shorter than two fades, no fade, no kept margin)."""
import numpy as np
import pytest

import join_ref
from rwkvtts import audio

pytestmark = pytest.mark.gpu
F32 = np.float32


def same(a, b):
    """Bitwise equality, any NaN equal to any NaN (a NaN's payload is not part of the contract)."""
    a, b = np.ascontiguousarray(a, dtype=F32), np.ascontiguousarray(b, dtype=F32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


@pytest.fixture(scope="module")
def joiners():
    made = {}

    def get(threshold=0.01, keep=800, fade=80, trim=True):
        key = (threshold, keep, fade, trim)
        if key not in made:
            made[key] = audio.Joiner(device=0, threshold=threshold, keep=keep, fade=fade, trim=trim)
        return made[key]
    yield get
    for j in made.values():
        j.close()


def speech_like(n, k, lead=None, trail=None):
    """Noise of amplitude 0.3 between a quiet head and tail (amplitude 0.003, below 0.01)."""
    rng = np.random.default_rng(500 + k)
    x = (rng.standard_normal(n) * 0.003).clip(-0.009, 0.009).astype(F32)
    lead = n // 5 if lead is None else lead
    trail = n // 7 if trail is None else trail
    if n - trail > lead:
        x[lead:n - trail] = (rng.standard_normal(n - trail - lead) * 0.3).astype(F32)
        x[lead] = 0.5       # loud for certain at both ends of the loud part
        x[n - trail - 1] = -0.5
    return x


def check(j, jobs):
    got = j.join_batch(jobs)
    assert len(got) == len(jobs)
    for (segs, gaps), (y, ab) in zip(jobs, got):
        ry, rab = join_ref.join(segs, gaps, j.threshold, j.keep, j.fade, j.trim, j.table)
        assert ab == rab
        assert same(y, ry)
    return got


LENGTHS = [0, 1, 2, 255, 256, 257, 4097]


@pytest.mark.parametrize("trim", [True, False])
def test_lengths_three_jobs_one_call(joiners, trim):
    """n_s in {0, 1, 2, 255, 256, 257, 4097}, gaps 0 and 1, three ragged jobs in one call."""
    j = joiners(keep=30, fade=16, trim=trim)
    segs = [speech_like(n, i) for i, n in enumerate(LENGTHS)]
    loud = [np.full(n, 0.25, dtype=F32) for n in LENGTHS]
    jobs = [(segs, [i % 2 for i in range(len(segs))]),
            (loud[::-1], [1] * len(loud)),
            ([segs[6], segs[0], loud[2]], [0, 0, 0])]
    got = check(j, jobs)
    if not trim:
        assert got[0][1] == [(0, n) for n in LENGTHS]
        assert same(got[0][0], np.concatenate([np.concatenate([s, np.zeros(i % 2, F32)]) for i, s in enumerate(segs)]))


def test_default_parameters_and_long_segments(joiners):
    """keep 800 / fade 80 on segments spanning several workgroups (more than 4096 samples each)."""
    j = joiners()
    segs = [speech_like(n, 20 + i) for i, n in enumerate([20000, 9001, 4096 * 3 + 5])]
    got = check(j, [(segs, [4800, 2400, 0])])
    (a0, b0) = got[0][1][0]
    assert (a0, b0) == (20000 // 5 - 800, 20000 - 20000 // 7 + 800)


def test_silent_segments_give_only_gaps(joiners):
    j = joiners(keep=10, fade=8)
    segs = [np.zeros(300, F32), np.full(257, 0.01, F32), np.full(5, -0.0099, F32), np.zeros(0, F32)]
    (y, ab), = check(j, [(segs, [3, 0, 1, 2])])
    assert ab == [(0, 0)] * 4 and y.size == 6 and not y.any()


def test_nan_inf_and_threshold_equality(joiners):
    """NaN is not loud, +-inf are; a sample equal to the threshold is not loud, the next float up is."""
    j = joiners(threshold=0.25, keep=0, fade=0)
    nan, inf = F32(np.nan), F32(np.inf)
    a = np.zeros(600, F32)
    a[[3, 599]] = nan                         # NaN alone: silent
    b = np.zeros(600, F32)
    b[[10, 300]] = [inf, -inf]
    b[[2, 500]] = nan                         # outside [lo, hi]: cut away
    c = np.zeros(600, F32)
    c[[100, 400]] = [0.25, -0.25]             # equal to the threshold: silent
    d = c.copy()
    d[200] = np.nextafter(F32(0.25), F32(1))  # just above
    d[250] = nan                              # inside a piece: copied
    (y, ab), = check(j, [([a, b, c, d], [0, 1, 0, 1])])
    assert ab == [(0, 0), (10, 301), (0, 0), (200, 201)]
    j2 = joiners(threshold=0.25, keep=100, fade=4)
    (y2, ab2), = check(j2, [([d, b], [0, 0])])
    assert ab2 == [(100, 301), (0, 401)] and np.isnan(y2).sum() == 2  # d[250]; b[2] * ramp (b[500] is cut)


def test_loud_at_first_and_last_index(joiners):
    j = joiners(keep=5, fade=4)
    x = np.zeros(1000, F32)
    x[0] = 0.5
    y = np.zeros(1000, F32)
    y[999] = -0.5
    z = np.zeros(4097, F32)
    z[[0, 4096]] = 0.5
    (out, ab), = check(j, [([x, y, z], [1, 1, 1])])
    assert ab == [(0, 6), (994, 1000), (0, 4097)]


def test_pieces_shorter_than_two_fades(joiners):
    """len_s < 2 * fade: f_s = len_s // 2, an odd piece keeps its middle sample unfaded."""
    j = joiners(keep=0, fade=64)
    segs = []
    for n in (1, 2, 3, 7, 64, 127, 128, 129):
        x = np.zeros(n + 20, F32)
        x[10:10 + n] = 0.5
        segs.append(x)
    (y, ab), = check(j, [(segs, [0] * len(segs))])
    assert [b - a for a, b in ab] == [1, 2, 3, 7, 64, 127, 128, 129]
    assert y[0] == F32(0.5)  # len 1: f = 0


@pytest.mark.parametrize("keep,fade", [(0, 0), (0, 16), (5000, 0), (5000, 4096), (2 ** 31 - 1, 3)])
def test_keep_and_fade_extremes(joiners, keep, fade):
    """fade = 0 (pure cut), keep = 0, keep > n_s (nothing cut, the edges still fade)."""
    j = joiners(keep=keep, fade=fade)
    segs = [speech_like(n, 40 + i) for i, n in enumerate([4097, 300, 257])]
    (y, ab), = check(j, [(segs, [1, 0, 1])])
    if keep >= 5000:
        assert ab == [(0, 4097), (0, 300), (0, 257)]


@pytest.mark.parametrize("n_seg", [1, 65, 300])
def test_segment_counts(joiners, n_seg):
    """The prefix over a job's segments: one lane's share, several lanes, more than 256 segments."""
    j = joiners(keep=3, fade=2)
    rng = np.random.default_rng(n_seg)
    segs = [speech_like(int(rng.integers(0, 90)), 100 + i, lead=int(rng.integers(0, 9)), trail=int(rng.integers(0, 9)))
            for i in range(n_seg)]
    gaps = [int(g) for g in rng.integers(0, 2, n_seg)]
    check(j, [(segs, gaps), (segs[::-1], gaps)])


def test_job_equals_its_segments_one_by_one(joiners):
    j = joiners(keep=40, fade=16)
    segs = [speech_like(n, 60 + i) for i, n in enumerate([900, 0, 4100, 31])]
    gaps = [5, 0, 1, 7]
    (y, ab), = j.join_batch([(segs, gaps)])
    singles = j.join_batch([([s], [g]) for s, g in zip(segs, gaps)])
    assert same(y, np.concatenate([p for p, _ in singles]))
    assert ab == [b[0] for _, b in singles]


def test_bad_calls_are_refused(joiners):
    from rwkvtts import _ffi
    for kw in ({"fade": 4097}, {"fade": -1}, {"keep": -1}, {"threshold": -0.5}, {"threshold": float("nan")},
               {"threshold": float("inf")}):
        with pytest.raises(_ffi.RwkvTtsError):
            audio.Joiner(device=0, **kw)
    j = joiners()
    with pytest.raises(_ffi.RwkvTtsError):
        j.join_batch([([np.zeros(1, F32)] * 4097, [0] * 4097)])
    with pytest.raises(_ffi.RwkvTtsError):
        j.join_batch([([np.zeros(1, F32)], [-1])])
