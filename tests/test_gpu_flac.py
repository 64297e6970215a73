"""The FLAC encoder on the GPU (csrc/flac.hip, audio.FlacEncoder) against its numpy contract
(tests/flac_ref.py): bytes equal, bit for bit, on the smallest shapes that can go wrong, and the GPU's
bytes through the independent decoder (rwkvtts/flac.py) give back the quantised input. The references
are computed once per case and every group of cases goes to the GPU as one ragged batch."""
import ctypes

import numpy as np
import pytest

import flac_ref as R
from rwkvtts import _ffi, audio, flac

pytestmark = pytest.mark.gpu

BLOCKS = (256, 4096)


@pytest.fixture(scope="module")
def enc():
    e = audio.FlacEncoder(device=0)
    yield e
    e.close()


def ref_frames(x, scale, rate, B, first=0, lpc=True):
    return b"".join(R.encode_frames(R.quantise(x, scale), rate, B, first, lpc))


def check(enc, items):
    """items [(samples, scale, rate, block, first_frame, final, lpc)]: one launch pair, every window
    against the reference, sizes included."""
    got = enc.encode_windows(items)
    assert len(got) == len(items)
    for (x, s, r, B, f, fin, lpc), (data, mn, mx) in zip(items, got):
        frames = R.encode_frames(R.quantise(x, s), r, B, f, lpc)
        want = b"".join(frames)
        where = f"n={len(x)} rate={r} B={B} first={f} lpc={lpc}"
        assert len(data) == len(want), where
        assert data == want, where + f": first difference at byte {next(i for i in range(len(want)) if data[i] != want[i])}"
        sizes = [len(fr) for fr in frames] or [0]
        assert (mn, mx) == (min(sizes), max(sizes)), where
    return got


@pytest.mark.parametrize("kind", R.KINDS)
def test_every_signal_at_every_length_and_both_block_sizes(enc, kind):
    items = [(R.signal(kind, n), 1.0, R.rate_of(kind), B, 0, True, True) for B in BLOCKS for n in R.lengths(B)]
    got = check(enc, items)
    for (x, _, rate, B, _, _, _), (data, mn, mx) in zip(items, got):  # lossless through the independent decoder
        pcm, r = flac.decode(enc.header(rate, B, mn, mx, len(x)) + data)
        assert r == rate and np.array_equal(pcm, R.quantise(x))


def test_lpc_off_and_scales(enc):
    items = [(R.signal(k, 2 * 256 + 37), s, 16000, 256, 0, True, False) for k in ("vowel16", "alternating", "ramp")
             for s in (1.0, 0.37, 1.9)]
    items += [(R.signal("vowel16", 4096 + 5), s, 16000, 4096, 0, True, True) for s in (0.0, 0.001, 1.6, 7.0)]
    check(enc, items)


@pytest.mark.parametrize("first", [127, 2047, 65535, 2097151, 67108863, (1 << 31) - 3])
def test_frame_numbers_across_every_coded_length(enc, first):
    check(enc, [(R.signal("vowel16", 3 * 256), 1.0, 16000, 256, first, True, True)])


def test_all_seven_rates_and_five_block_sizes(enc):
    items = [(R.signal("vowel16", B + 100), 1.0, rate, B, 3, True, True)
             for rate, B in zip(audio.FLAC_RATES, (256, 512, 1024, 2048, 4096, 512, 1024))]
    check(enc, items)


def test_a_ragged_batch_equals_its_signals_one_by_one(enc):
    items = [(R.signal("vowel16", 1500), 1.0, 16000, 256, 0, True, True),
             (R.signal("vowel48", 4096 + 700), 0.5, 48000, 4096, 10, True, True),
             (R.signal("noise", 77), 1.0, 8000, 1024, 0, True, False),
             (R.signal("clamp", 2048), 1.3, 44100, 512, 200, False, True),
             (R.signal("ramp", 1), 1.0, 22050, 2048, 0, True, True)]
    batch = check(enc, items)
    assert batch == [enc.encode_windows([it])[0] for it in items]


def test_windows_at_every_block_boundary_equal_the_whole(enc):
    B, x = 256, R.signal("vowel16", 4 * 256 + 91)
    whole = enc.encode_windows([(x, 1.0, 16000, B, 0, True, True)])[0][0]
    assert whole == ref_frames(x, 1.0, 16000, B)
    for cut in range(1, 5):
        a, b = enc.encode_windows([(x[:cut * B], 1.0, 16000, B, 0, False, True), (x[cut * B:], 1.0, 16000, B, cut, True, True)])
        assert a[0] + b[0] == whole
    # and through the stream object, in awkward pieces
    s = enc.stream(16000, B)
    out = b"".join(s.feed(x[i:i + 333], final=i + 333 >= x.size) for i in range(0, x.size, 333))
    assert out[:42] == enc.header(16000, B) and out[42:] == whole


def test_the_file_of_encode_carries_true_totals_and_decodes(enc):
    x = R.signal("vowel48", 5000)
    data = enc.encode(x, 48000, scale=0.8)
    assert data == R.encode(x, 48000, 0.8)
    pcm, rate = flac.decode(data)
    assert rate == 48000 and np.array_equal(pcm, R.quantise(x, 0.8))
    assert enc.kernel_ms() > 0.0


def test_a_window_that_breaks_the_rules_is_einval_and_writes_nothing(enc):
    L = _ffi.lib()
    x = np.ascontiguousarray(R.signal("vowel16", 1024))

    def call(specs):
        ws = (_ffi.FlacWindow * len(specs))()
        outs = []
        for w, (n, rate, B, flags, first, cap) in zip(ws, specs):
            out = np.full(4096, 0xA5, dtype=np.uint8)
            outs.append(out)
            w.struct_size = ctypes.sizeof(_ffi.FlacWindow)
            w.in_, w.n_in, w.scale, w.sample_rate, w.block_size = x.ctypes.data, n, 1.0, rate, B
            w.flags, w.first_frame, w.out, w.out_cap = flags, first, out.ctypes.data, cap
            w.out_len, w.min_frame, w.max_frame = -7, -7, -7
        rc = L.rwkvtts_flac_encode(enc._h, ws, len(specs))
        return rc, ws, outs

    good = (512, 16000, 256, 0, 0, 4096)
    rc, ws, outs = call([good])
    assert rc == _ffi.OK and ws[0].out_len > 0 and not np.all(outs[0] == 0xA5)
    for bad in [(512, 11025, 256, 0, 0, 4096),          # an unknown rate
                (512, 16000, 300, 0, 0, 4096),          # an unknown block size
                (500, 16000, 256, 0, 0, 4096),          # misaligned and not the last
                (512, 16000, 256, 0, 0, 2 * 512 + 31),  # out_cap below the bound
                (512, 16000, 256, 1, (1 << 31) - 1, 4096)]:  # first_frame + blocks above 2^31
        rc, ws, outs = call([good, bad])
        assert rc == _ffi.EINVAL
        for w, out in zip(ws, outs):
            assert np.all(out == 0xA5) and (w.out_len, w.min_frame, w.max_frame) == (-7, -7, -7)
    assert L.rwkvtts_flac_bound(500, 256) == 2 * 500 + 32 and L.rwkvtts_flac_bound(500, 300) == -1
    rc, ws, outs = call([(500, 16000, 256, 1, (1 << 31) - 2, 2 * 500 + 32)])  # the last frame number there is
    assert rc == _ffi.OK and outs[0][:int(ws[0].out_len)].tobytes() == ref_frames(x[:500], 1.0, 16000, 256, (1 << 31) - 2)


def test_the_library_table_is_the_integer_formula(enc):
    for B in audio.FLAC_BLOCKS:
        t = np.zeros(B, dtype=np.int32)
        assert _ffi.lib().rwkvtts_flac_table(B, t.ctypes.data_as(ctypes.c_void_p)) == _ffi.OK
        assert np.array_equal(t, R.window(B))
    assert np.array_equal(enc.table, R.table())
