"""Exact windowed vocoder decode, host side (CPU only): the halo walk, the window plan, and the
oracle's proof that the plan's token context is enough -- and not one frame more than enough."""
import numpy as np
import pytest

from rwkvtts import _ffi, codec

T = 104
WINDOWS = [(0, 1), (1, 18), (18, 20), (20, 43), (43, 84), (84, 103), (103, 104)]


def py_halo(d):
    """Independent restatement of the walk: backwards from the samples of frame 0."""
    hop = int(np.prod(d["up_rates"][:d["n_up"]]))
    lo, hi = 0 - 3, hop - 1 + 3                      # conv_out k7
    for s, k in reversed(list(zip(d["up_rates"], d["up_kernels"]))[:d["n_up"]]):
        lo, hi = lo - 3 * (1 + 3 + 9), hi + 3 * (1 + 3 + 9)   # residual units, dilations 1, 3, 9
        p = (k - s) // 2
        lo, hi = -((-(lo + p - k + 1)) // s), (hi + p) // s   # ConvTranspose: ceil, floor
    lo, hi = lo - 3, hi + 3                          # conv_in k7
    return 3 * (d["prenet_layers"] + 1), max(-lo, hi)


def test_halo_values():
    assert codec.codec_halo(codec.CODEC_DIMS_FULL) == (39, 10)
    assert codec.codec_halo(codec.CODEC_DIMS_TINY) == (9, 10)


@pytest.mark.parametrize("layers", [0, 1, 5])
@pytest.mark.parametrize("base", ["full", "tiny", "other"])
def test_halo_agrees_with_python_walk(layers, base):
    d = dict(codec.CODEC_DIMS_FULL if base == "full" else codec.CODEC_DIMS_TINY, prenet_layers=layers)
    if base == "other":  # other rates: k = s, k = 3 s, three stages
        d.update(n_up=3, up_rates=(4, 4, 2, 1), up_kernels=(4, 12, 6, 1))
    assert codec.codec_halo(d) == py_halo(d)
    assert py_halo(d)[0] == 3 * (layers + 1)


def test_halo_rejects_bad_dims():
    for bad in (dict(n_up=0), dict(n_up=5), dict(up_kernels=(15, 11, 8, 4)), dict(up_kernels=(4, 11, 8, 4))):
        with pytest.raises(_ffi.RwkvTtsError) as e:
            codec.codec_halo(dict(codec.CODEC_DIMS_TINY, **bad))
        assert e.value.code == _ffi.EINVAL


@pytest.mark.parametrize("dims", [codec.CODEC_DIMS_FULL, codec.CODEC_DIMS_TINY])
def test_window_plan_bounds_and_clipping(dims):
    hp, hw = codec.codec_halo(dims)
    H = hp + hw
    n = 4 * H + 7
    for t0, t1 in [(0, 1), (0, n), (1, 2), (H - 1, H), (H, H + 1), (H + 1, 2 * H), (n - H - 1, n - H),
                   (n - H, n - H + 1), (n - 2, n), (n - 1, n), (hw, hw + 3), (hw + 1, n - hw - 1)]:
        for final in (True, False):
            if not final and t1 + H > n:
                with pytest.raises(_ffi.RwkvTtsError) as e:
                    codec.window_plan(dims, t0, t1, n, False)
                assert e.value.code == _ffi.EINVAL
                continue
            p = codec.window_plan(dims, t0, t1, n, final)
            (c0, c1), (w0, w1) = p["ctx"], p["wave"]
            # clipped at 0 and at n_known, otherwise exactly the halo
            assert w0 == max(0, t0 - hw) and w1 == min(n, t1 + hw)
            assert c0 == max(0, t0 - H) and c1 == min(n, t1 + H)
            assert 0 <= c0 <= w0 <= t0 < t1 <= w1 <= c1 <= n
            assert c1 - c0 <= (t1 - t0) + 2 * H          # prenet work bound
            assert w1 - w0 <= (t1 - t0) + 2 * 10         # WaveGenerator work bound
    # a plan does not depend on tokens beyond t1 + H
    assert codec.window_plan(dims, 3, 5, 5 + H, False) == codec.window_plan(dims, 3, 5, n, False)


def test_window_plan_preconditions():
    d = codec.CODEC_DIMS_TINY
    for t0, t1, n, final in [(-1, 3, 50, True), (3, 3, 50, True), (5, 3, 50, True), (0, 51, 50, True),
                             (0, 32, 50, False), (0, 1, 19, False), (0, 1, 0, True)]:
        with pytest.raises(_ffi.RwkvTtsError) as e:
            codec.window_plan(d, t0, t1, n, final)
        assert e.value.code == _ffi.EINVAL
    assert codec.window_plan(d, 0, 31, 50, False)["ctx"] == (0, 50)
    assert codec.window_plan(d, 0, 1, 20, False)["ctx"] == (0, 20)
    # struct_size too small: refused, nothing written
    p = _ffi.CodecPlan(struct_size=8, ctx0=-7)
    import ctypes
    rc = _ffi.lib().rwkvtts_codec_window_plan(ctypes.byref(codec.make_codec_dims(d)), 0, 1, 50, 1, ctypes.byref(p))
    assert rc == _ffi.EINVAL and p.ctx0 == -7


@pytest.fixture(scope="module")
def oracle_full(oracle_mod):
    d = codec.CODEC_DIMS_TINY
    w = codec.synth_codec_blob(d, seed=11)
    rs = np.random.default_rng(104)
    sem, g = rs.integers(0, 8192, T), rs.integers(0, 4096, 32)
    cd = codec.make_codec_dims(d)
    full = oracle_mod.codec_decode(cd, w, sem, g, threads=16)
    full.setflags(write=False)
    return cd, w, sem, g, full


def test_oracle_windows_bitwise_and_halo_tight(oracle_mod, oracle_full):
    """Each window decoded from the plan's token slice alone is bitwise the full decode; with one
    frame less of context some window is not (the halo is tight)."""
    cd, w, sem, g, full = oracle_full
    d = codec.CODEC_DIMS_TINY
    H = sum(codec.codec_halo(d))
    assert H == 19
    short_differs = 0
    for t0, t1 in WINDOWS:
        c0, c1 = codec.window_plan(d, t0, t1, T, True)["ctx"]
        pcm = oracle_mod.codec_decode(cd, w, sem[c0:c1], g, threads=16)
        got = pcm[(t0 - c0) * 320:(t1 - c0) * 320]
        assert np.array_equal(got, full[t0 * 320:t1 * 320]), (t0, t1)
        s0, s1 = max(0, t0 - (H - 1)), min(T, t1 + (H - 1))
        if (s0, s1) != (c0, c1):
            pcm = oracle_mod.codec_decode(cd, w, sem[s0:s1], g, threads=16)
            short_differs += int(np.count_nonzero(pcm[(t0 - s0) * 320:(t1 - s0) * 320] != full[t0 * 320:t1 * 320]))
    assert short_differs > 0
