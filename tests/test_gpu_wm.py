"""The watermark on the GPU: csrc/wm.hip against the numpy restatement of its contract (tests/wm_ref.py;
include/rwkvtts.h). The embedder bit for bit -- whole signals at the lengths where a
path changes, silence, a ragged batch with a key, a payload and a strength per signal, exact stream
windows with the carried amplitude, a window that breaks its plan. The detector within the stated
bound of the float64 reference for every r_b and d_b, and equal in every decision, on inputs whose
reference margins dwarf that bound (asserted)."""
import ctypes

import numpy as np
import pytest

import wm_ref
from rwkvtts import _ffi, audio

F32 = np.float32
B, L, NP = 320, 129, 25600
KEY = 0x5EED0C0FFEE
SMALL = dict(bits=4, bit_len=640)  # NP = 2560


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


@pytest.fixture(scope="module")
def wm():
    made = {}

    def get(**kw):
        k = tuple(sorted(kw.items()))
        if k not in made:
            made[k] = audio.Watermarker(device=0, **kw)
        return made[k]
    yield get
    for v in made.values():
        v.close()


# ---- embed ----------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_lengths_and_silence_bitwise_against_restatement(wm):
    """The lengths where a path changes (the last wraps the period) and an all-zero signal, one launch."""
    v = wm()
    assert (v.block, v.taps, v.period) == (B, L, NP)
    lengths = [0, 1, B - 1, B, B + 1, L - 1, 3 * B + 7, NP + B + 5]
    sigs = [wm_ref.vowel(n, k) for k, n in enumerate(lengths)] + [np.zeros(5 * B + 3, dtype=F32)]
    pays = [(0x1234 + 977 * k) & 0xFFFF for k in range(len(sigs))]
    got = v.embed_batch(sigs, [KEY + k for k in range(len(sigs))], pays)
    for k, (x, p, y) in enumerate(zip(sigs, pays, got)):
        want = wm_ref.embed(x, KEY + k, p)
        assert y.dtype == F32 and y.size == x.size == want.size
        assert np.array_equal(bits(y), bits(want)), (k, x.size)
    assert np.array_equal(bits(got[-1]), bits(sigs[-1]))            # silence comes back bit for bit
    assert not np.array_equal(bits(got[-2]), bits(sigs[-2]))
    assert v.kernel_ms() > 0.0


@pytest.mark.gpu
def test_ragged_batch_keys_payloads_strengths(wm):
    v = wm()
    rng = np.random.default_rng(17)
    sigs = [wm_ref.vowel(int(n), 20 + k, peak=float(pk)) for k, (n, pk) in
            enumerate(zip(rng.integers(1, 9 * B, 5), rng.uniform(0.02, 0.9, 5)))]
    sigs[3] = wm_ref.am_noise(7 * B + 11, 3)
    keys = [0, 1, 2 ** 64 - 1, KEY, 0x0123456789ABCDEF]
    pays = [0, 0xFFFF, 0x8001, 0x00F0, 0x5A5A]
    dbs = [-26.0, -6.0, -60.0, -20.0, -33.5]
    got = v.embed_batch(sigs, keys, pays, dbs)
    for k, y in enumerate(got):
        assert np.array_equal(bits(y), bits(wm_ref.embed(sigs[k], keys[k], pays[k], dbs[k]))), k
    # the bound: |y - x| <= max a * sum|h|, with a <= s * the loudest block's RMS <= s * peak
    sum_h = float(np.sum(np.abs(v.table[:L]).astype(np.float64)))
    for x, db, y in zip(sigs, dbs, got):
        a_max = float(wm_ref.strength(db)) * float(np.max(np.abs(x)))
        assert np.max(np.abs(y.astype(np.float64) - x)) <= a_max * sum_h


@pytest.mark.gpu
def test_windows_at_every_block_boundary_carry_the_amplitude(wm):
    v = wm()
    n = 6 * B
    x = wm_ref.vowel(n, 31, peak=0.5)
    x[2 * B:3 * B] *= F32(0.05)  # a level step the ramp has to cross
    want = wm_ref.embed(x, KEY, 0xBEEF)
    s = audio.wm_strength(-26.0)
    assert np.array_equal(bits(v.embed(x, KEY, 0xBEEF)), bits(want))
    # block by block, the amplitude threaded through
    a, parts = F32(0.0), []
    for j in range(6):
        (y, a), = v.embed_windows([(x[j * B:(j + 1) * B], j * B, j == 5, s, KEY, 0xBEEF, a, j, B)])
        parts.append(y)
    assert np.array_equal(bits(np.concatenate(parts)), bits(want))
    # cut once at every boundary: the first pieces in one call, the final ones in another
    first = v.embed_windows([(x[:c * B], 0, False, s, KEY, 0xBEEF, 0.0, 0, c * B) for c in range(1, 6)])
    second = v.embed_windows([(x[c * B:], c * B, True, s, KEY, 0xBEEF, first[c - 1][1], c, n - c * B) for c in range(1, 6)])
    for (y1, _), (y2, _) in zip(first, second):
        assert np.array_equal(bits(np.concatenate([y1, y2])), bits(want))


@pytest.mark.gpu
def test_a_window_that_breaks_the_plan_is_einval_and_writes_nothing(wm):
    v = wm()
    x = wm_ref.vowel(4 * B, 33)
    s = float(audio.wm_strength(-26.0))

    def call(samples, in_first, final, block_first, count, a_prev=0.25):
        out = np.full(max(count, 1), 7.0, dtype=F32)
        w = _ffi.WmWindow(struct_size=ctypes.sizeof(_ffi.WmWindow), in_=samples.ctypes.data, in_first=in_first,
                          n_in=samples.size, final=final, strength=s, key=KEY, payload=5, a_prev=a_prev,
                          block_first=block_first, out_count=count, out=out.ctypes.data, a_last=-3.0)
        return _ffi.lib().rwkvtts_wm_embed_windows(v._h, ctypes.byref(w), 1), out, w.a_last

    rc, out, a = call(np.ascontiguousarray(x[B:3 * B]), B, 0, 1, 2 * B)
    assert rc == 0 and a >= 0.0 and not np.any(out == 7.0)
    for samples, in_first, final, bf, count in (
            (np.ascontiguousarray(x[B:3 * B - 1]), B, 0, 1, 2 * B),   # the last block a sample short
            (np.ascontiguousarray(x[B + 1:3 * B]), B + 1, 0, 1, 2 * B),  # starts after the cursor block
            (np.ascontiguousarray(x[B:]), B, 1, 1, 3 * B + 1),         # passes the signal's end
            (np.ascontiguousarray(x[B:]), B, 1, 1, B + 5)):            # ends inside a block
        rc, out, a = call(samples, in_first, final, bf, count)
        assert rc == _ffi.EINVAL and np.all(out == 7.0) and a == -3.0
    rc, out, a = call(np.ascontiguousarray(x[B:]), B, 1, 1, 3 * B, a_prev=float("nan"))
    assert rc == _ffi.EINVAL and np.all(out == 7.0) and a == -3.0


@pytest.mark.gpu
def test_stream_of_5120_sample_chunks_equals_embed(wm):
    v = wm()
    x = wm_ref.vowel(3 * 5120 + 1234, 35)
    y = v.embed(x, KEY, 0x0F0F)
    st = v.stream(KEY, 0x0F0F)
    cuts = list(range(5120, x.size, 5120))
    parts = [st.feed(p, final=i == len(cuts)) for i, p in enumerate(np.split(x, cuts))]
    assert np.array_equal(bits(np.concatenate(parts)), bits(y))
    assert np.array_equal(bits(y), bits(wm_ref.embed(x, KEY, 0x0F0F)))
    assert st.kept == 0 and all(p.size % B == 0 for p in parts[:-1])


# ---- detect ---------------------------------------------------------------------------------------
def _margins(ref):
    """The reference's own margins: the runner-up offset (outside the peak's neighbours), the threshold
    and the weakest sign must all be a relative 1e-3 away -- two orders above the f32 sums' error."""
    S, tau, n = ref["S"], ref["offset"], ref["S"].size
    other = np.ones(n, dtype=bool)
    other[[(tau - 1) % n, tau, (tau + 1) % n]] = False
    assert ref["score"] - max(S[other].max(), S[(tau - 1) % n], S[(tau + 1) % n]) > 1e-3 * ref["score"]
    assert abs(ref["score"] - ref["threshold"]) > 1e-3 * ref["threshold"]
    assert ref["min_z"] > 1e-3 or ref["seen"] == 0


def _same_decisions(got, ref):
    for k in ("detected", "offset", "payload", "seen"):
        assert got[k] == ref[k], (k, got, {q: ref[q] for q in ("detected", "offset", "payload", "seen", "score")})
    assert abs(got["score"] - ref["score"]) <= 1e-3 * max(ref["score"], 1.0)
    assert got["threshold"] == ref["threshold"]


@pytest.fixture(scope="module")
def small_clips():
    """A 1 s vowel marked under the small descriptor, and what the detect tests cut from it."""
    x = wm_ref.vowel(16000, 41)
    y = wm_ref.embed(x, KEY, 0b1010, **SMALL)
    y.setflags(write=False)
    return x, y


@pytest.mark.gpu
def test_small_r_and_d_within_the_bound_of_float64(wm, small_clips):
    v = wm(**SMALL)
    _, y = small_clips
    NB, TB = 4, 640
    got = v.detect(y, KEY, debug=True)
    ref = wm_ref.detect(y, KEY, full=True, **SMALL)
    r, d, A = wm_ref.direct_all(ref["F"], ref["F2"], KEY, NB, TB)
    u = TB * 2.0 ** -24
    er, ed = np.abs(got["r"].astype(np.float64) - r), np.abs(got["d"].astype(np.float64) - d)
    print("max |r - r64| / bound", float(np.max(er / (u * A))), " max |d - d64| / bound", float(np.max(ed / (u * d))))
    assert np.all(er <= u * A) and np.all(ed <= u * d)
    _margins(ref)
    _same_decisions(got, ref)
    assert ref["detected"] and ref["payload"] == 0b1010 and ref["offset"] == 0 and ref["seen"] == 0b1111
    assert v.kernel_ms() > 0.0


@pytest.mark.gpu
def test_small_crops_half_period_unmarked_wrong_key_and_a_ragged_batch(wm, small_clips):
    v = wm(**SMALL)
    x, y = small_clips
    P = 2560
    clips = [(y[c:], KEY) for c in (0, 1, 777, P - 1)]       # crops: the offset is the crop
    clips += [(y[:P // 2], KEY), (y[300:300 + P // 2], KEY)]  # half a period: a partial `seen`
    clips += [(x, KEY), (y, KEY + 1), (wm_ref.am_noise(9000, 5), KEY)]  # unmarked, a wrong key
    refs = [wm_ref.detect(c, k, full=True, **SMALL) for c, k in clips]
    for ref in refs:
        _margins(ref)
    for (c, k), ref in zip(clips, refs):  # one by one
        _same_decisions(v.detect(c, k), ref)
    for i, c in enumerate((0, 1, 777, P - 1)):
        assert refs[i]["detected"] and refs[i]["offset"] == c and refs[i]["payload"] == 0b1010
    assert refs[4]["seen"] == 0b0011 and refs[4]["offset"] == 0 and refs[4]["payload"] == 0b0010
    assert refs[5]["seen"] == 0b0111 and refs[5]["offset"] == 300
    assert not refs[6]["detected"] and not refs[7]["detected"] and not refs[8]["detected"]
    # one ragged batch of 4, an empty clip beside them
    pick = [0, 4, 6, 8]
    got = v.detect_batch([clips[i][0] for i in pick] + [np.zeros(0, dtype=F32)], [clips[i][1] for i in pick] + [KEY])
    for g, i in zip(got, pick):
        _same_decisions(g, refs[i])
    assert got[4]["detected"] is False and got[4]["score"] == 0.0 and got[4]["seen"] == 0


@pytest.mark.gpu
def test_defaults_four_seconds_clean_int16_cropped_and_through_8_khz(wm):
    v = wm()
    x = wm_ref.vowel(64000, 43)
    y = v.embed(x, KEY, 0xBEEF)
    assert np.array_equal(bits(y), bits(wm_ref.embed(x, KEY, 0xBEEF)))
    down, up = audio.Resampler(16000, 8000, device=0), audio.Resampler(8000, 16000, device=0)
    try:
        narrow = up.resample(down.resample(y))
    finally:
        down.close()
        up.close()
    clips = [y, (np.trunc(y * F32(32767.0)) / F32(32767.0)).astype(F32), y[7777:], narrow]
    got = v.detect_batch(clips, [KEY] * 4)
    for g, c, off in zip(got, clips, (0, 0, 7777, 0)):
        ref = wm_ref.detect(c, KEY, full=True)
        _margins(ref)
        _same_decisions(g, ref)
        assert g["detected"] and g["payload"] == 0xBEEF and g["offset"] == off and g["score"] >= 10 * g["threshold"]
