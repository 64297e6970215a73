"""The resampling kernel (csrc/resample.hip) against the arithmetic contract of include/rwkvtts.h.

The reference is the numpy restatement of that contract below: positions in float64, one operation
per step; a loop over the taps k in ascending order, each step one rounded f32 multiply and one
rounded f32 add over all outputs at once (numpy's element-wise f32 ufuncs never fuse), starting
from +0; then a + (b - a) * w1 in three rounded f32 operations. It reads the table
audio._make_sincs builds, which audio.Resampler also hands to rwkvtts_resampler_create, so kernel
and reference must agree bit for bit. tests/test_resample_cpu.py drives Resampler.stream() with the
same restatement and no GPU."""
import ctypes

import numpy as np
import pytest

from rwkvtts import _ffi, audio, codec

F32 = np.float32
PAIRS = [(16000, 48000, 1), (16000, 48000, 321), (16000, 8000, 1000), (16000, 44100, 777),
         (16000, 24000, 5120), (44100, 16000, 4410), (48000, 16000, 4801)]
ALIGNS = ["zero", "rubato"]


# ---- the contract in numpy ---------------------------------------------------------------------
def contract_positions(o, sr_in, sr_out, L, O, align):
    """(start, p0, w1) of outputs o (an int64 array)."""
    ratio = float(sr_out) / float(sr_in)
    t_ratio = 1.0 / ratio
    delay = L / 2.0 if align == "rubato" else 0.0
    idx = o.astype(np.float64) * t_ratio - delay
    start = np.floor(idx)
    pos = (idx - start) * float(O)
    p0 = np.floor(pos)
    w1 = (pos - p0).astype(F32)
    return start.astype(np.int64), p0.astype(np.int64), w1


def contract_out_len(n, sr_in, sr_out):
    return int(np.ceil(n * (float(sr_out) / float(sr_in))))


def contract_resample(x, sincs, sr_in, sr_out, align, out_first=0, out_count=None, x_first=0):
    """Outputs [out_first, out_first + out_count) of the resample of a signal of which x holds
    samples [x_first, x_first + len(x)); every other sample reads as zero. out_count None: all
    ceil(len(x) * ratio) outputs (x_first = 0)."""
    x = np.ascontiguousarray(x, dtype=F32)
    O, L = sincs.shape
    if out_count is None:
        out_count = contract_out_len(x.size, sr_in, sr_out) - out_first
    if out_count <= 0:
        return np.zeros(0, F32)
    o = np.arange(out_first, out_first + out_count, dtype=np.int64)
    start, p0, w1 = contract_positions(o, sr_in, sr_out, L, O, align)
    lo, hi = int(start[0]) - L // 2 + 1, int(start[-1]) + L // 2
    buf = np.zeros(hi - lo + 1, F32)  # signal samples [lo, hi], zero where not given
    a0, a1 = max(lo, x_first), min(hi + 1, x_first + x.size)
    if a1 > a0:
        buf[a0 - lo:a1 - lo] = x[a0 - x_first:a1 - x_first]
    r0, r1 = p0 % O, (p0 + 1) % O
    a, b = np.zeros(out_count, F32), np.zeros(out_count, F32)
    base = start - L // 2 + 1 - lo
    for k in range(L):
        xv = buf[base + k]
        a = a + xv * sincs[r0, k]
        b = b + xv * sincs[r1, k]
    return a + (b - a) * w1


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


# ---- GPU ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rs():
    """Resamplers by (sr_in, sr_out, align), created on first use, shared by the module's tests."""
    made = {}

    def get(sr_in, sr_out, align):
        key = (sr_in, sr_out, align)
        if key not in made:
            made[key] = audio.Resampler(sr_in, sr_out, device=0, align=align)
        return made[key]
    yield get
    for r in made.values():
        r.close()


def _signal(n, seed=0):
    return (np.random.default_rng(seed).standard_normal(n) * 0.3).astype(F32)


@pytest.mark.gpu
@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("sr_in,sr_out,n", PAIRS)
def test_bitwise_against_contract(rs, sr_in, sr_out, n, align):
    r = rs(sr_in, sr_out, align)
    x = _signal(n, seed=n)
    got = r.resample(x)
    ref = contract_resample(x, r.sincs, sr_in, sr_out, align)
    assert got.dtype == F32 and got.shape == ref.shape == (contract_out_len(n, sr_in, sr_out),)
    assert np.array_equal(bits(got), bits(ref))
    assert n < 300 or got.std() > 0.01  # (a real signal: the comparison means something)


@pytest.mark.gpu
@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("sr_out", [48000, 44100])
def test_impulse_names_the_table_entry(rs, sr_out, align):
    """A unit impulse at sample m: output o is s0[k] + (s1[k] - s0[k]) * w1 with k the tap that reads
    m, whatever the summation order -- start, k and the (p0 + 1) % O wrap, each on its own."""
    n, r = 600, rs(16000, sr_out, align)
    O, L = r.sincs.shape
    o = np.arange(contract_out_len(n, 16000, sr_out), dtype=np.int64)
    start, p0, w1 = contract_positions(o, 16000, sr_out, L, O, align)
    wraps = 0
    for m in (0, 299, 599):
        x = np.zeros(n, F32)
        x[m] = 1.0
        k = m - start + L // 2 - 1          # j = start + k - L/2 + 1 == m
        hit = (k >= 0) & (k < L)
        kc = np.clip(k, 0, L - 1)
        s0, s1 = r.sincs[p0 % O, kc], r.sincs[(p0 + 1) % O, kc]
        want = np.where(hit, s0 + (s1 - s0) * w1, F32(0.0)).astype(F32)
        got = r.resample(x)
        assert hit.any() and np.array_equal(bits(got), bits(want)), (sr_out, align, m)
        wraps += int(((p0 + 1 >= O) & hit).sum())
    assert sr_out != 44100 or wraps > 0   # (the wrap of the second table is exercised)


@pytest.mark.gpu
def test_ragged_batch_equals_single_calls(rs):
    r = rs(16000, 24000, "zero")
    xs = [_signal(n, seed=100 + n) for n in (0, 1, 321, 5120)]
    together = r.resample_batch(xs)
    assert [t.size for t in together] == [0, 2, 482, 7680]
    for x, t in zip(xs, together):
        assert np.array_equal(bits(t), bits(r.resample(x)))


@pytest.mark.gpu
@pytest.mark.parametrize("sr0", [24000, 8000, 44100])
def test_against_the_numpy_restatement(sr0):
    """audio.resample_audio_high_quality with device=0 against the numpy path (einsum, unspecified
    summation order): per output |d| <= 2 (L + 4) 2^-24 sum_k |x_k| (|s0_k| + |s1_k|), the standard
    forward-error bound of two f32 sums of L terms in any order (gamma_L each, the interpolation's
    three operations inside the + 4), computed here in float64."""
    n, L, O = 2400, 256, 256
    x = _signal(n, seed=sr0)
    host = audio.resample_audio_high_quality(x, sr0, 16000)
    dev = audio.resample_audio_high_quality(x, sr0, 16000, device=0)
    assert host.shape == dev.shape and dev.dtype == F32
    ratio = 16000 / sr0
    sincs = audio._make_sincs(L, O, 0.95 if ratio >= 1 else 0.95 * ratio).astype(np.float64)
    o = np.arange(host.size, dtype=np.int64)
    start, p0, _ = contract_positions(o, sr0, 16000, L, O, "rubato")
    j = start[:, None] + np.arange(L)[None, :] - L // 2 + 1
    xa = np.where((j >= 0) & (j < n), np.abs(x.astype(np.float64))[np.clip(j, 0, n - 1)], 0.0)
    bound = 2.0 * (L + 4) * 2.0 ** -24 * (xa * (np.abs(sincs[p0 % O]) + np.abs(sincs[(p0 + 1) % O]))).sum(axis=1)
    d = np.abs(host.astype(np.float64) - dev.astype(np.float64))
    print(f"sr0 {sr0}: max |d| {d.max():.3e}, max d / bound {np.max(d / np.maximum(bound, 1e-300)):.3f}")
    assert np.all(d <= bound)


def _fewest_known(r, o0, o1, first, n):
    """The fewest n_known whose out_ready_end reaches o1 (it is monotone in n_known: bisect)."""
    lo, hi = first, n
    while lo < hi:
        mid = (lo + hi) // 2
        if r.plan(mid, False, o0)[0] >= o1:
            hi = mid
        else:
            lo = mid + 1
    return lo


def _c_window(x, in_first, final, out_first, out):
    return _ffi.ResampleWindow(struct_size=ctypes.sizeof(_ffi.ResampleWindow), in_=x.ctypes.data, in_first=in_first,
                               n_in=x.size, final=1 if final else 0, out_first=out_first, out_count=out.size,
                               out=out.ctypes.data)


@pytest.mark.gpu
@pytest.mark.parametrize("align", ALIGNS)
def test_windows_bitwise_and_one_sample_short(rs, align):
    r = rs(16000, 44100, align)
    n = 5120
    x = _signal(n, seed=7)
    full = r.resample(x)
    cuts = [0, 1, 300, 301, 2048, 9000, 9001, 13000, full.size]   # output ranges of unequal size
    items = []
    for o0, o1 in zip(cuts[:-1], cuts[1:]):
        last = o1 == full.size
        # exactly the samples the plan asks for: from in_first_needed(o0) up to the fewest n_known
        # whose out_ready_end reaches o1 (all n for the last range, which is final)
        first = r.plan(n, last, o0)[1]
        known = n if last else _fewest_known(r, o0, o1, first, n)
        assert last or r.plan(known, False, o0)[0] >= o1 > r.plan(known - 1, False, o0)[0]
        items.append((np.ascontiguousarray(x[first:known]), first, last, o0, o1 - o0))
    outs = r.resample_windows(items)   # ONE call
    for (o0, o1), out in zip(zip(cuts[:-1], cuts[1:]), outs):
        assert np.array_equal(bits(out), bits(full[o0:o1])), (align, o0, o1)
    # a window one sample short, at its end or at its start, is refused -- alone or after a good
    # window in the same call -- and nothing is written
    xw, first, last, o0, cnt = items[4]
    xg, gfirst, _, go0, gcnt = items[1]
    assert not last and first > 0
    for bx, bfirst in ((np.ascontiguousarray(xw[:-1]), first), (np.ascontiguousarray(xw[1:]), first + 1)):
        canary, good_out = np.full(cnt, 7.0, F32), np.full(gcnt, 7.0, F32)
        both = (_ffi.ResampleWindow * 2)(_c_window(xg, gfirst, False, go0, good_out),
                                         _c_window(bx, bfirst, False, o0, canary))
        assert _ffi.lib().rwkvtts_resample_windows(r._h, both, 2) == _ffi.EINVAL
        assert _ffi.lib().rwkvtts_resample_windows(r._h, ctypes.byref(both[1]), 1) == _ffi.EINVAL
        assert np.all(canary == 7.0) and np.all(good_out == 7.0)
        with pytest.raises(_ffi.RwkvTtsError) as e:
            r.resample_windows([(bx, bfirst, False, o0, cnt)])
        assert e.value.code == _ffi.EINVAL
    # the good pair of the same shape goes through, and the resampler still works after a refusal
    canary, good_out = np.full(cnt, 7.0, F32), np.full(gcnt, 7.0, F32)
    both = (_ffi.ResampleWindow * 2)(_c_window(xg, gfirst, False, go0, good_out), _c_window(xw, first, False, o0, canary))
    assert _ffi.lib().rwkvtts_resample_windows(r._h, both, 2) == _ffi.OK
    assert np.array_equal(bits(canary), bits(full[o0:o0 + cnt])) and np.array_equal(bits(good_out), bits(full[go0:go0 + gcnt]))
    assert np.array_equal(bits(r.resample(x)), bits(full))


@pytest.mark.gpu
def test_handle_reuse_across_growth_shrink_and_a_refused_call():
    """A fresh resampler (its device buffers start empty): first allocation, regrowth (5120 > 40 * 1.25)
    with a zero-length member in the batch, a refused windows call that writes nothing, and reuse
    without regrowth after it."""
    r = audio.Resampler(16000, 24000, device=0, align="zero")
    try:
        def run(ns, seed):
            xs = [_signal(n, seed=seed + n) for n in ns]
            got = r.resample_batch(xs)
            for x, y in zip(xs, got):
                assert np.array_equal(bits(y), bits(contract_resample(x, r.sincs, 16000, 24000, "zero"))), (ns, x.size)
            assert r.kernel_ms() > 0.0
        run([40], 500)
        run([5120, 0, 321], 600)
        x = _signal(400, seed=9)
        end, _ = r.plan(x.size, False, 0)
        assert 0 < end < contract_out_len(x.size, 16000, 24000)
        canary = np.full(end + 1, 7.0, F32)      # one output more than the plan allows
        w = _c_window(x, 0, False, 0, canary)
        assert _ffi.lib().rwkvtts_resample_windows(r._h, ctypes.byref(w), 1) == _ffi.EINVAL
        assert np.all(canary == 7.0)
        run([40], 500)
    finally:
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("align", ALIGNS)
def test_window_far_into_a_long_signal(rs, align):
    """Sample and output indices past 2^31 (53 hours of 16 kHz audio into a stream): the plan, the
    tile descriptors and the kernel's positions are 64-bit / double throughout."""
    r = rs(16000, 44100, align)
    o0, cnt = 3 * 2 ** 31 + 12345, 700
    first = r.plan(2 ** 39, False, o0)[1]
    assert first > 2 ** 31
    known = _fewest_known(r, o0, o0 + cnt, first, first + 5000)
    x = _signal(known - first, seed=31)
    got = r.resample_windows([(x, first, False, o0, cnt)])[0]
    ref = contract_resample(x, r.sincs, 16000, 44100, align, o0, cnt, first)
    assert np.array_equal(bits(got), bits(ref)) and got.std() > 0.01
    with pytest.raises(_ffi.RwkvTtsError):
        r.resample_windows([(x[:-1], first, False, o0, cnt)])


@pytest.mark.gpu
def test_bad_descriptions_are_einval():
    for kw in (dict(sr_in=0), dict(sr_out=192001), dict(sinc_len=12), dict(sinc_len=1032), dict(oversampling=1025),
               dict(f_cutoff=1.5)):
        args = dict(sr_in=16000, sr_out=48000)
        args.update(kw)
        with pytest.raises(_ffi.RwkvTtsError) as e:
            audio.Resampler(**args)
        assert e.value.code == _ffi.EINVAL


@pytest.mark.gpu
def test_small_table_and_wide_ratio(rs):
    """Other table shapes and a ratio that narrows the tile (192 kHz -> 8 kHz: 24 inputs per output),
    with the library's own table (table == NULL) on the native side of the comparison."""
    for sr_in, sr_out, L, O, n in ((192000, 8000, 1024, 8, 30000), (8000, 192000, 8, 1024, 40), (3, 7, 64, 5, 100)):
        desc = _ffi.ResampleDesc(struct_size=ctypes.sizeof(_ffi.ResampleDesc), sr_in=sr_in, sr_out=sr_out, sinc_len=L,
                                 oversampling=O, f_cutoff=0.9, align=_ffi.RESAMPLE_ALIGN_ZERO)
        table = np.empty((O, L), F32)
        _ffi.check(_ffi.lib().rwkvtts_resample_sincs(ctypes.byref(desc), table.ctypes.data_as(ctypes.c_void_p)), "sincs")
        h = ctypes.c_void_p()
        _ffi.check(_ffi.lib().rwkvtts_resampler_create(0, ctypes.byref(desc), None, ctypes.byref(h)), "create")
        try:
            x = _signal(n, seed=L)
            m = contract_out_len(n, sr_in, sr_out)
            out = np.empty(m, F32)
            ins, outs = (ctypes.c_void_p * 1)(x.ctypes.data), (ctypes.c_void_p * 1)(out.ctypes.data)
            _ffi.check(_ffi.lib().rwkvtts_resample_batch(h, ins, (ctypes.c_int64 * 1)(n), 1, outs), "batch")
            assert np.array_equal(bits(out), bits(contract_resample(x, table, sr_in, sr_out, "zero"))), (sr_in, sr_out)
        finally:
            _ffi.lib().rwkvtts_resampler_destroy(h)


@pytest.mark.gpu
@pytest.mark.parametrize("rate", [24000, 44100])
def test_stream_behind_the_windowed_vocoder(rs, rate):
    """Tiny codec, T = 104 as tests/test_gpu_codec_windows.py: the vocoder's 16-frame windows, each fed
    to Resampler.stream(), concatenate to the resample of the full decode."""
    T, d = 104, codec.CODEC_DIMS_TINY
    c = codec.BiCodecDetokenizer(codec.synth_codec_blob(d, seed=11), d)
    try:
        g, sem = np.random.default_rng(104).integers(0, 4096, 32), np.random.default_rng(105).integers(0, 8192, T)
        full = c.decode_audio(g, sem)
        wins = [(t0, min(t0 + 16, T)) for t0 in range(0, T, 16)]
        pcm = c.decode_windows([(g, sem, t0, t1, True) for t0, t1 in wins])
    finally:
        c.close()
    r = rs(16000, rate, "zero")
    st = r.stream()
    parts = [st.feed(p, final=(t1 == T)) for (t0, t1), p in zip(wins, pcm)]
    got = np.concatenate(parts)
    assert got.size == int(np.ceil(T * 320 * rate / 16000)) and all(p.size for p in parts)
    assert np.array_equal(bits(got), bits(r.resample(full)))
    assert st.kept == 0


@pytest.mark.gpu
def test_pipeline_end_to_end():
    """stream_speech(sample_rate=24000) concatenates bitwise to generate_speech(sample_rate=24000);
    sample_rate=16000 is generate_speech(args) itself and creates no resampler."""
    import rwkvtts
    from rwkvtts import weights as W
    from rwkvtts.pipeline import LightweightTtsPipeline, LightweightTtsPipelineArgs
    from rwkvtts.tokenizer import Tokenizer
    from test_tokenizer import VOCAB
    blob = W.synth_blob(W.DIMS_TINY, seed=99)
    m = rwkvtts.DynamicBatchManager(blob, devices=[0], max_slots=4, token_chunk_size=64, tokenizer=Tokenizer(VOCAB))
    cd = codec.CODEC_DIMS_TINY
    voc = codec.BiCodecDetokenizer(codec.synth_codec_blob(cd, seed=11), cd)
    pipe = LightweightTtsPipeline(m, voc)
    try:
        args = LightweightTtsPipelineArgs(text="Hello world, this is RWKV speaking.", seed=12, max_tokens=60)
        plain = pipe.generate_speech(args)
        assert np.array_equal(bits(plain), bits(pipe.generate_speech(args, sample_rate=16000)))
        assert pipe._resamplers == {}
        one = pipe.generate_speech(args, sample_rate=24000)
        T = plain.size // 320
        assert one.size == int(np.ceil(plain.size * 1.5)) and T >= 5
        chunks = list(pipe.stream_speech(args, chunk_frames=4, sample_rate=24000))
        assert len(chunks) == (T + 3) // 4 >= 2 and chunks[-1].done and chunks[-1].t1 == T
        assert b"".join(chunks) == one.tobytes()
        assert list(pipe._resamplers) == [24000]
        ref = contract_resample(plain, pipe._resamplers[24000].sincs, 16000, 24000, "zero")
        assert np.array_equal(bits(one), bits(ref))
        # the batch form: one resample_batch call, a failed item stays empty; silence is `rate` zeros
        outs = pipe.generate_speech_batch([args, LightweightTtsPipelineArgs(text="emoji \U0001F600", seed=2)],
                                          sample_rate=24000)
        assert np.array_equal(bits(outs[0]), bits(one)) and outs[1].size == 0
        sil = pipe.generate_speech(LightweightTtsPipelineArgs(text="emoji \U0001F600"), sample_rate=24000)
        assert sil.shape == (24000,) and not sil.any()
        sil = list(pipe.stream_speech(LightweightTtsPipelineArgs(text="emoji \U0001F600"), sample_rate=24000))
        assert len(sil) == 1 and sil[0].shape == (24000,) and not sil[0].any()
    finally:
        for r in pipe._resamplers.values():
            r.close()
        m.close()
        voc.close()
