"""csrc/pause.hip on the GPU against its numpy restatement (tests/pause_ref.py), bitwise: named
lengths and constructed signals through one launch triple per config, a ragged batch of 33 signals
with a cap each, stream windows at every cut offset, and the refusals, which write nothing."""
import ctypes

import numpy as np
import pytest

import pause_ref
from rwkvtts import _ffi, audio

pytestmark = pytest.mark.gpu
F32 = np.float32
CONFIGS = [(16, 2, 8), (64, 1, 32)]


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


@pytest.fixture(scope="module")
def shapers():
    ps = {c: audio.PauseShaper(block=c[0], hang=c[1], fade=c[2]) for c in CONFIGS}
    yield ps
    for p in ps.values():
        p.close()


def _quiet(n, seed):
    return np.random.default_rng(seed).uniform(-0.004, 0.004, n).astype(F32)


def _with(n, seed, loud_at=(), value=0.5):
    x = _quiet(n, seed)
    for i in loud_at:
        x[i] = value if i % 2 else -value
    return x


def cases(B, H, F):
    """[(name, signal, M)]: every signal is distinct noise under the threshold with loud samples put in."""
    out = []
    M0 = 2 * F + B + 3
    # ---- lengths: all quiet, and one loud sample first (the rest is a trailing run)
    for n in (0, 1, B - 1, B, B + 1, (H + 1) * B - 1, (H + 1) * B, (H + 1) * B + 1):
        out.append((f"len_{n}_quiet", _quiet(n, n), M0))
        if n:
            out.append((f"len_{n}_loud_first", _with(n, n + 1, [0]), 2 * F))
            out.append((f"len_{n}_loud_last", _with(n, n + 2, [n - 1]), 2 * F))
    # ---- the interior rule around R = M: a run of exactly R samples between two loud blocks
    R = 6 * B
    inner = 2 * H * B + R  # quiet samples between the loud blocks: H blocks on each side stay active
    x = np.concatenate([np.full(B, 0.5, F32), _quiet(inner, 20), np.full(B, -0.5, F32)])
    for M in (R - 1, R, R + 1, R - B, 2 * F):
        out.append((f"interior_R{R}_M{M}", x, M))
    out.append(("run_of_exactly_M", x, R))
    out.append(("run_of_M_plus_one_block", np.concatenate([x[:B + inner], _quiet(B, 21), x[B + inner:]]), R))
    # ---- the leading rule around R = tl
    R = 4 * B
    x = np.concatenate([_quiet(R + H * B, 22), np.full(2 * B, 0.5, F32)])
    for M in (2 * R - 2, 2 * R - 1, 2 * R, 2 * R + 1, 2 * R + 2):
        out.append((f"leading_R{R}_M{M}", x, M))
    # ---- the trailing rule around R = hd, and hd < R <= M
    M = 2 * F + 2 * B + 1
    hd = M - M // 2
    for R in (hd - 1, hd, hd + 1, M - 1, M, M + 1, M + 3 * B):
        out.append((f"trailing_R{R}_hd{hd}_M{M}", np.concatenate([np.full(B, 0.5, F32), _quiet(H * B + R, 23 + R)]), M))
    # ---- where the loud sample sits
    n = 30 * B
    out.append(("loud_first_of_block", _with(n, 40, [14 * B]), M0))
    out.append(("loud_last_of_block", _with(n, 41, [14 * B + B - 1]), M0))
    n = max(600, 12 * B)
    out.append(("loud_below_lane_boundary", _with(n, 42, [255]), 2 * F))      # the last sample of lane 63's vector
    out.append(("loud_above_lane_boundary", _with(n, 43, [256]), 2 * F))      # the first of lane 0's next vector
    out.append(("loud_both_sides_of_lane_boundary", _with(n, 44, [255, 256]), 2 * F))
    out.append(("loud_in_every_lane_slot", _with(n, 45, [3, 4, 257, 258, 515]), 2 * F))
    # ---- the 64-block word boundary: loud bits, the dilation and a run all cross it
    n = 200 * B + 5
    out.append(("loud_block_63", _with(n, 46, [63 * B + B - 1]), M0))
    out.append(("loud_block_64", _with(n, 47, [64 * B]), M0))
    out.append(("loud_blocks_63_64_127_128", _with(n, 48, [63 * B + 1, 64 * B + 2, 127 * B, 128 * B + B - 1]), 3 * B))
    out.append(("runs_across_words", _with(n, 49, [5 * B, 60 * B, 70 * B, 126 * B, 131 * B, 199 * B]), 4 * B + 1))
    out.append(("many_short_runs", _with(n, 50, [k * B for k in range(0, 200, 2 * H + 3)]), 2 * F))
    # ---- the partial last block
    n = 20 * B + 3
    out.append(("partial_last_block_loud", _with(n, 51, [2 * B, n - 1]), M0))
    out.append(("partial_last_block_quiet", _with(n, 52, [2 * B]), M0))
    out.append(("partial_last_block_quiet_run_not_cut", _with(4 * B + 3, 53, [0]), 8 * B))
    # ---- values
    x = _with(40 * B, 54, [20 * B])
    x[3 * B + 1] = np.nan
    x[25 * B] = F32(0.01)       # exactly the threshold: not above it
    out.append(("nan_and_threshold_are_not_loud", x, M0))
    x = np.random.default_rng(55).uniform(0.02, 0.9, 9 * B + 5).astype(F32)
    out.append(("all_loud", x, 2 * F))
    return out


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "B%d_H%d_F%d" % c)
def test_named_cases_in_one_launch_triple(shapers, cfg):
    B, H, F = cfg
    ps = shapers[cfg]
    cs = cases(B, H, F)
    got = ps.shape_samples_batch([x for _, x, _ in cs], [M for _, _, M in cs])
    cuts = list(ps.cuts)
    assert ps.kernel_ms() > 0
    some_cut = 0
    for (name, x, M), y, k in zip(cs, got, cuts):
        want, wk = pause_ref.shape(x, M, B, H, F)
        assert y.size == want.size and k == wk, (name, y.size, want.size, k, wk)
        assert np.array_equal(bits(y), bits(want)), name
        some_cut += wk
    assert some_cut >= 20  # (the cases do cut)
    # and one at a time, a call of one job each
    for name, x, M in cs[::7]:
        y = ps.shape_samples_batch([x], [M])[0]
        assert np.array_equal(bits(y), bits(pause_ref.shape(x, M, B, H, F)[0])), name


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "B%d_H%d_F%d" % c)
def test_ragged_batch_of_33_signals_with_a_cap_each(shapers, cfg):
    B, H, F = cfg
    ps = shapers[cfg]
    rng = np.random.default_rng(7)
    xs, Ms = [], []
    for i in range(33):
        n = int(rng.integers(0, 90 * B)) if i else 0
        x = _quiet(n, 100 + i)
        for _ in range(int(rng.integers(0, 6))):
            a = int(rng.integers(0, max(n, 1)))
            x[a:a + int(rng.integers(1, 2 * B))] = 0.3
        xs.append(x)
        Ms.append(2 * F + i * (B // 2 + 1))  # a different M each, M = 2F among them
    assert Ms[0] == 2 * F and len(set(Ms)) == 33
    got = ps.shape_samples_batch(xs, Ms)
    assert ps.kernel_ms() > 0
    want = [pause_ref.shape(x, M, B, H, F) for x, M in zip(xs, Ms)]
    assert ps.cuts == [k for _, k in want] and sum(ps.cuts) >= 10
    for i, (y, (w, _)) in enumerate(zip(got, want)):
        assert np.array_equal(bits(y), bits(w)), i


def _stream_signal(B, H):
    return np.concatenate([_quiet(5 * B + 3, 1), np.full(B, 0.5, F32), _quiet((2 * H + 9) * B, 2), np.full(3, -0.5, F32),
                           _quiet((2 * H + 2) * B + 5, 3), np.full(B, 0.5, F32), _quiet(7 * B + 2, 4)])


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "B%d_H%d_F%d" % c)
def test_windows_at_every_cut_offset_carry_the_state(shapers, cfg):
    B, H, F = cfg
    ps = shapers[cfg]
    x = _stream_signal(B, H)
    M = 3 * B + 1
    want, cuts = pause_ref.shape(x, M, B, H, F)
    assert cuts == 3 and np.array_equal(bits(ps.shape_samples_batch([x], [M])[0]), bits(want))
    offs = list(range(0, x.size + 1))
    first = ps.shape_windows([(x[:o], 0, False, M, 0, 0, 0) for o in offs])  # every first window in one call
    second = ps.shape_windows([(x[min(need, o):], min(need, o), True, M, c, s, q)
                               for o, (_, c, s, q, need, _) in zip(offs, first)])
    carried_cut = leading = 0
    for o, a, b in zip(offs, first, second):
        ra = pause_ref.window(x[:o], 0, False, M, 0, 0, 0, B, H, F)
        assert a[1:] == ra[1:] and np.array_equal(bits(a[0]), bits(ra[0])), o
        assert np.array_equal(bits(np.concatenate([a[0], b[0]])), bits(want)), o
        assert a[5] + b[5] == cuts and o - min(a[4], o) <= ps.kept_bound(M), o
        carried_cut += a[2] == 1 and a[3] > M
        leading += a[2] == 0 and a[3] > M // 2
    assert carried_cut > 0 and leading > 0  # states inside a certain cut, after activity and before any
    # a chain of many windows through the stream object, chunks shorter than a block
    for step in (B - 3, 5 * B + 1):
        st = audio.PauseStream(ps, M)
        parts = np.split(x, np.arange(step, x.size, step))
        got = np.concatenate([st.feed(p, final=i == len(parts) - 1) for i, p in enumerate(parts)])
        assert np.array_equal(bits(got), bits(want)) and st.cuts == cuts, step


def _window(x, out, **kw):
    w = _ffi.PauseWindow(struct_size=ctypes.sizeof(_ffi.PauseWindow))
    w.in_, w.in_first, w.n_in, w.final = x.ctypes.data, 0, x.size, 0
    w.max_pause_samples, w.block_next, w.seen, w.quiet = 64, 0, 0, 0
    w.out, w.out_cap = out.ctypes.data, out.size
    w.out_count = w.n_cuts = w.block_last = w.quiet_last = w.in_first_needed = -7
    w.seen_last = -7
    for k, v in kw.items():
        setattr(w, k, v)
    return w


def test_every_einval_writes_nothing(shapers):
    B, H, F = cfg = CONFIGS[0]
    ps = shapers[cfg]
    L = _ffi.lib()
    x = _with(40 * B, 9, [0, 20 * B])
    out = np.full(x.size, 123.0, F32)
    bad = {
        "M_below_2F": dict(max_pause_samples=2 * F - 1),
        "M_above_range": dict(max_pause_samples=(1 << 30) + 1),
        "too_little_capacity": dict(out_cap=10),
        "state_seen_without_blocks": dict(seen=1),
        "state_quiet_not_a_block_multiple": dict(block_next=3, seen=1, quiet=B + 1),
        "state_quiet_reaches_an_active_block": dict(block_next=3, seen=1, quiet=3 * B),
        "state_not_seen_with_less_quiet": dict(block_next=3, seen=0, quiet=2 * B),
        "state_negative": dict(block_next=-1),
        "state_seen_2": dict(block_next=3, seen=2),
        "samples_end_before_block_next": dict(block_next=41, seen=0, quiet=41 * B),
        "samples_start_after_in_first_needed": dict(in_first=B, n_in=x.size - B, block_next=1, seen=1, quiet=0),
        "negative_n_in": dict(n_in=-1),
    }
    for name, kw in bad.items():
        w = _window(x, out, **kw)
        assert L.rwkvtts_pause_windows(ps._h, ctypes.byref(w), 1) == _ffi.EINVAL, name
        assert np.all(out == 123.0), name
        assert (w.out_count, w.n_cuts, w.block_last, w.quiet_last, w.in_first_needed, w.seen_last) == (-7,) * 6, name
    # a good window beside a bad one: nothing is launched for either
    ws = (_ffi.PauseWindow * 2)(_window(x, out), _window(x, out, max_pause_samples=1))
    assert L.rwkvtts_pause_windows(ps._h, ws, 2) == _ffi.EINVAL and np.all(out == 123.0) and ws[0].out_count == -7
    # the batch form
    n_out = (ctypes.c_int64 * 1)(-7)
    n_cuts = (ctypes.c_int64 * 1)(-7)
    P = ctypes.c_void_p * 1
    for M, n in ((2 * F - 1, x.size), (64, -1), (64, (1 << 30) + 1)):
        rc = L.rwkvtts_pause_batch(ps._h, P(x.ctypes.data), (ctypes.c_int64 * 1)(n), (ctypes.c_int64 * 1)(M), 1,
                                   P(out.ctypes.data), n_out, n_cuts)
        assert rc == _ffi.EINVAL and np.all(out == 123.0) and n_out[0] == -7 and n_cuts[0] == -7, (M, n)
    # a bad desc: no object
    h = ctypes.c_void_p()
    d = _ffi.PauseDesc(struct_size=ctypes.sizeof(_ffi.PauseDesc), block=18)
    assert L.rwkvtts_pause_create(0, ctypes.byref(d), None, ctypes.byref(h)) == _ffi.EINVAL and not h.value
    # and the good window does run
    w = _window(x, out)
    assert L.rwkvtts_pause_windows(ps._h, ctypes.byref(w), 1) == 0 and w.out_count > 0 and w.block_last == 40 - H
    ref = pause_ref.window(x, 0, False, 64, 0, 0, 0, B, H, F)
    assert np.array_equal(bits(out[:w.out_count]), bits(ref[0])) and np.all(out[w.out_count:] == 123.0)
    assert (w.block_last, w.seen_last, w.quiet_last, w.in_first_needed, w.n_cuts) == ref[1:]
