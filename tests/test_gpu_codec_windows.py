"""Exact windowed vocoder decode on the MI355X: every window is bitwise the slice of the full GPU
decode (which tests/test_gpu_codec.py pins to the oracle). The decode accumulates each output
element in an order that depends on neither the row's position in its tile nor the launch's
length, so a window that runs the prenet on the plan's token context and the WaveGenerator on the
plan's frame range reproduces the full decode's bits, not just its values."""
import numpy as np
import pytest

import rwkvtts
from rwkvtts import _ffi, codec

pytestmark = pytest.mark.gpu

T = 104
WINDOWS = [(0, 1), (1, 18), (18, 20), (20, 43), (43, 84), (84, 103), (103, 104)]
H_TINY = 19


@pytest.fixture(scope="module")
def tiny():
    d = codec.CODEC_DIMS_TINY
    w = codec.synth_codec_blob(d, seed=11)
    rs = np.random.default_rng(104)
    g, sem = rs.integers(0, 4096, 32), rs.integers(0, 8192, T)
    decs = {"auto": codec.BiCodecDetokenizer(w, d),
            "hilo": codec.BiCodecDetokenizer(w, d, weight_path=_ffi.CODEC_WEIGHTS_HILO)}
    full = decs["auto"].decode_audio(g, sem)
    assert full.shape == (T * 320,) and full.std() > 0.05  # (a real signal: the comparisons below mean something)
    full.setflags(write=False)
    yield d, g, sem, decs, full
    for c in decs.values():
        c.close()


def _slices(full, wins):
    return [full[t0 * 320:t1 * 320] for t0, t1 in wins]


@pytest.mark.parametrize("form", ["default", "channel_last", "separate_resunit", "hilo"])
def test_tiny_windows_bitwise(tiny, form):
    d, g, sem, decs, full = tiny
    c = decs["hilo" if form == "hilo" else "auto"]
    assert c.halo() == H_TINY
    c.set_forms({"channel_last": _ffi.CODEC_FORM_CHANNEL_LAST,
                 "separate_resunit": _ffi.CODEC_FORM_SEPARATE_RESUNIT}.get(form, 0))
    try:
        # the finished utterance: every window in ONE call
        outs = c.decode_windows([(g, sem, t0, t1, True) for t0, t1 in WINDOWS])
        for (t0, t1), o, ref in zip(WINDOWS, outs, _slices(full, WINDOWS)):
            assert o.dtype == np.float32 and np.array_equal(o, ref), (form, t0, t1)
        # while the utterance is still growing: exactly t1 + H tokens known, final = 0
        inner = [(t0, t1) for t0, t1 in WINDOWS if t1 + H_TINY <= T]
        assert len(inner) >= 4
        outs = c.decode_windows([(g, sem[:t1 + H_TINY], t0, t1, False) for t0, t1 in inner])
        for (t0, t1), o, ref in zip(inner, outs, _slices(full, inner)):
            assert np.array_equal(o, ref), (form, t0, t1, "final=0")
    finally:
        c.set_forms(0)


def test_mixed_batch_equals_one_per_call(tiny):
    """Three ragged windows of different utterances (different speakers, lengths, one still growing)
    in one call == the same windows one per call == the full decodes' slices."""
    d, g, sem, decs, full = tiny
    c = decs["auto"]
    rs = np.random.default_rng(3)
    utts = [(rs.integers(0, 4096, 32), rs.integers(0, 8192, n)) for n in (61, 23, 150)]
    items = [(utts[0][0], utts[0][1], 30, 37, True), (utts[1][0], utts[1][1], 0, 23, True),
             (utts[2][0], utts[2][1][:99 + H_TINY], 64, 99, False)]
    together = c.decode_windows(items)
    for it, o in zip(items, together):
        assert np.array_equal(o, c.decode_windows([it])[0])
    for (gg, ss), it, o in zip(utts, items, together):
        assert np.array_equal(o, c.decode_audio(gg, ss)[it[2] * 320:it[3] * 320])


def test_full_dims_windows_bitwise():
    d = codec.CODEC_DIMS_FULL
    H = 49
    n = 3 * H + 47
    wins = [(0, 1), (48, 50), (50, 120), (120, n)]
    w = codec.synth_codec_blob(d)
    c = codec.BiCodecDetokenizer(w, d)
    try:
        assert c.halo() == H
        rs = np.random.default_rng(194)
        g, sem = rs.integers(0, 4096, 32), rs.integers(0, 8192, n)
        full = c.decode_audio(g, sem)
        outs = c.decode_windows([(g, sem, t0, t1, True) for t0, t1 in wins])
        for (t0, t1), o in zip(wins, outs):
            assert np.array_equal(o, full[t0 * 320:t1 * 320]), (t0, t1)
        # [48, 50) with final = 0 needs 50 + 49 tokens and no more
        o = c.decode_windows([(g, sem[:50 + H], 48, 50, False)])[0]
        assert np.array_equal(o, full[48 * 320:50 * 320])
    finally:
        c.close()


def test_precondition_violations_are_einval(tiny):
    d, g, sem, decs, full = tiny
    c = decs["auto"]
    good = (g, sem, 20, 43, True)
    bad_sem = sem.copy()
    bad_sem[30] = 8192
    bad_g = g.copy()
    bad_g[0] = 4096
    for bad in [(g, sem[:43 + H_TINY - 1], 20, 43, False),   # one token short of the look-ahead
                (g, bad_sem, 20, 43, True),                  # a code out of range inside the context
                (bad_g, sem, 20, 43, True)]:
        for items in ([bad], [good, bad]):
            outs = None
            with pytest.raises(_ffi.RwkvTtsError) as e:
                outs = c.decode_windows(items)
            assert e.value.code == _ffi.EINVAL and outs is None
    for t0, t1 in [(-1, 3), (5, 5), (7, 5), (100, 105)]:    # refused by the binding
        with pytest.raises(ValueError):
            c.decode_windows([(g, sem, t0, t1, True)])
    # a bad code outside the window's context does not matter, and the decoder still decodes
    assert np.array_equal(c.decode_windows([(g, bad_sem, 70, 80, True)])[0], full[70 * 320:80 * 320])
    assert np.array_equal(c.decode_windows([good])[0], full[20 * 320:43 * 320])
    assert np.array_equal(c.decode_audio(g, sem), full)
    # the C entry point refuses a short struct_size and t0 >= t1 itself
    import ctypes
    w = _ffi.CodecWindow(struct_size=16)
    assert _ffi.lib().rwkvtts_codec_decode_windows(c._h, ctypes.byref(w), 1) == _ffi.EINVAL
    out = np.empty(320, np.float32)
    s64, g64 = np.ascontiguousarray(sem, np.int64), np.ascontiguousarray(g, np.int64)
    w = _ffi.CodecWindow(struct_size=ctypes.sizeof(_ffi.CodecWindow), n_known=T, final=1, t0=5, t1=5,
                         semantic=s64.ctypes.data, global_=g64.ctypes.data, pcm=out.ctypes.data)
    assert _ffi.lib().rwkvtts_codec_decode_windows(c._h, ctypes.byref(w), 1) == _ffi.EINVAL
