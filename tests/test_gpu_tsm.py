"""Time stretch (WSOLA) on the GPU: csrc/tsm.hip against the numpy restatement of its arithmetic
contract (tests/tsm_ref.py; include/rwkvtts.h), bit for bit -- whole signals, ragged
batches with a tempo per signal, exact stream windows with the carried start, tie-breaking, NaN, and
`tempo` through the pipeline behind the windowed vocoder."""
import ctypes

import numpy as np
import pytest

import tsm_ref
from rwkvtts import _ffi, audio, codec

F32 = np.float32
CONFIGS = [(512, 128), (64, 16), (64, 10), (32, 5)]
TEMPOS = [0.25, 0.5, 0.8, 1.0, 1.25, 1.37, 2.0, 4.0]


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def same(a, b):
    """Bitwise equality, any NaN equal to any NaN (a NaN's payload is not part of the contract)."""
    a, b = np.ascontiguousarray(a, dtype=F32), np.ascontiguousarray(b, dtype=F32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb]))


@pytest.fixture(scope="module")
def ts():
    made = {}

    def get(W=512, D=128):
        if (W, D) not in made:
            made[(W, D)] = audio.TimeStretcher(device=0, window=W, search=D)
        return made[(W, D)]
    yield get
    for t in made.values():
        t.close()


def _lengths(W):
    Hs = W // 2
    return [0, 1, Hs - 1, Hs, W, W + 1, 3 * W + 17, 20000]


def _signal(kind, n, k):
    rng = np.random.default_rng(1000 + k)
    if kind == "noise":
        return (rng.standard_normal(n) * 0.3).astype(F32)
    if kind == "chirp":
        t = np.arange(n, dtype=np.float64) / 16000.0
        return (0.6 * np.sin(2 * np.pi * (80.0 * t + 900.0 * t * t))).astype(F32)
    x = np.zeros(n, dtype=F32)
    if kind == "impulse" and n:
        x[[0, n // 3, n // 2, n - 1][k % 4]] = 1.0
    if kind == "last" and n:
        x[n - 1] = -0.75
    return x


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["noise", "chirp", "impulse", "zeros", "last"])
@pytest.mark.parametrize("W,D", CONFIGS)
def test_bitwise_against_restatement(ts, W, D, kind):
    """Every (tempo, n) of the configuration in one launch, each against the restatement."""
    t = ts(W, D)
    cases = [(tempo, n) for tempo in TEMPOS for n in _lengths(W)]
    sigs = [_signal(kind, n, k) for k, (tempo, n) in enumerate(cases)]
    got = t.stretch_batch(sigs, [tempo for tempo, _ in cases])
    for (tempo, n), x, y in zip(cases, sigs, got):
        want = tsm_ref.stretch(x, tempo, W, D)
        assert y.dtype == F32 and y.size == t.out_len(n, tempo) == want.size
        assert np.array_equal(bits(y), bits(want)), (W, D, kind, tempo, n)
        if kind == "zeros":
            assert not y.any()
    if kind == "zeros":  # every shift is 0: the last frame starts at its anchor
        Hs = W // 2
        items = [(np.zeros(20000, F32), 0, True, tempo, 0, -Hs, t.out_len(20000, tempo)) for tempo in TEMPOS]
        for tempo, (y, s_last) in zip(TEMPOS, t.stretch_windows(items)):
            M = -(-t.out_len(20000, tempo) // Hs)
            assert s_last == tsm_ref.anchor(M - 1, Hs, tempo) and not y.any()


@pytest.mark.gpu
def test_ragged_batch_with_different_tempos(ts):
    t = ts(512, 128)
    sigs = [_signal("noise", n, k) for k, n in enumerate((5000, 0, 12345, 700, 9001))]
    tempos = [0.8, 1.25, 2.0, 0.5, 1.37]
    got = t.stretch_batch(sigs, tempos)
    for x, tempo, y in zip(sigs, tempos, got):
        one = t.stretch(x, tempo)
        assert np.array_equal(bits(y), bits(one)) and np.array_equal(bits(y), bits(tsm_ref.stretch(x, tempo)))
    assert t.kernel_ms() > 0.0
    with pytest.raises(_ffi.RwkvTtsError):
        t.stretch_batch(sigs, [0.8, 1.25, 4.5, 0.5, 1.37])
    with pytest.raises(_ffi.RwkvTtsError):
        t.stretch(sigs[0], float("nan"))


def _fewest_known(t, tempo, bf, s_prev, b1, n):
    """The smallest n_known at which blocks [bf, b1) are ready (the plan is monotone in n_known)."""
    lo, hi = 0, n
    while lo < hi:
        mid = (lo + hi) // 2
        if t.plan(tempo, mid, False, bf, s_prev)[0] >= b1 * t.hop:
            hi = mid
        else:
            lo = mid + 1
    return lo


def _c_window(x, in_first, final, tempo, bf, s_prev, out):
    w = _ffi.TsmWindow()
    w.struct_size = ctypes.sizeof(_ffi.TsmWindow)
    w.in_, w.in_first, w.n_in, w.final, w.tempo = x.ctypes.data, in_first, x.size, final, tempo
    w.block_first, w.s_prev, w.out_count, w.out, w.s_last = bf, s_prev, out.size, out.ctypes.data, -12345
    return w


@pytest.mark.gpu
@pytest.mark.parametrize("W,D", [(512, 128), (64, 10)])
def test_windows_bitwise_and_one_sample_short(ts, W, D):
    t = ts(W, D)
    Hs = W // 2
    rng = np.random.default_rng(W)
    n = 40 * W
    x = _signal("noise", n, 7)
    for tempo in (0.5, 0.8, 1.0, 1.37, 4.0):
        whole, s = tsm_ref.stretch(x, tempo, W, D, return_starts=True)   # s[m + 1] = s_m
        M = len(s) - 1
        items, wants = [], []
        for _ in range(6):
            bf = int(rng.integers(0, M - 1))
            b1 = int(rng.integers(bf + 1, M + 1))
            n_known = _fewest_known(t, tempo, bf, s[bf], b1, n + 1)
            if n_known > n:      # these blocks need the end of the signal: a final window
                final, n_known, count = True, n, whole.size - bf * Hs
                b1 = M
            else:
                final, count = False, (b1 - bf) * Hs
            first = t.plan(tempo, n_known, final, bf, s[bf])[1]
            items.append((x[first:n_known], first, final, tempo, bf, s[bf], count))
            wants.append((whole[bf * Hs:bf * Hs + count], s[b1]))
        for (y, s_last), (want, s_want), it in zip(t.stretch_windows(items), wants, items):
            assert np.array_equal(bits(y), bits(want)) and s_last == s_want, (W, D, tempo, it[1:])
        # one sample short of the plan, at either end: EINVAL, nothing written
        for x_in, first, final, _, bf, s_prev, count in items:
            if final:
                continue
            out = np.full(count, 7.25, F32)
            short = np.ascontiguousarray(x_in[:-1])
            w = _c_window(short, first, 0, tempo, bf, s_prev, out)
            assert _ffi.lib().rwkvtts_tsm_windows(t._h, ctypes.byref(w), 1) == _ffi.EINVAL
            assert np.all(out == F32(7.25)) and w.s_last == -12345
            if first > 0:
                late = np.ascontiguousarray(x_in[1:])
                w = _c_window(late, first + 1, 0, tempo, bf, s_prev, out)
                assert _ffi.lib().rwkvtts_tsm_windows(t._h, ctypes.byref(w), 1) == _ffi.EINVAL
                assert np.all(out == F32(7.25)) and w.s_last == -12345
            full = np.ascontiguousarray(x_in)
            w = _c_window(full, first, 0, tempo, bf, s_prev, out)
            assert _ffi.lib().rwkvtts_tsm_windows(t._h, ctypes.byref(w), 1) == 0
            assert np.array_equal(bits(out), bits(whole[bf * Hs:bf * Hs + count]))
    # an impossible carried start, and block 0 without -Hs
    out = np.full(Hs, 7.25, F32)
    for bf, s_prev in ((0, 0), (1, 5), (3, tsm_ref.anchor(2, Hs, 1.0) + D)):
        w = _c_window(x, 0, 1, 1.0, bf, s_prev, out)
        assert _ffi.lib().rwkvtts_tsm_windows(t._h, ctypes.byref(w), 1) == _ffi.EINVAL and np.all(out == F32(7.25))


@pytest.mark.gpu
def test_handle_reuse_across_growth_shrink_and_a_refused_call():
    """A fresh stretcher (its device buffers start empty): first allocation, regrowth with a
    zero-length member in the batch, a refused windows call that writes nothing (s_last included),
    and reuse without regrowth after it."""
    W, D = 64, 10
    Hs = W // 2
    t = audio.TimeStretcher(device=0, window=W, search=D)
    try:
        def run(ns, tempos):
            xs = [_signal("noise", n, k) for k, n in enumerate(ns)]
            got = t.stretch_batch(xs, tempos)
            for x, tempo, y in zip(xs, tempos, got):
                assert np.array_equal(bits(y), bits(tsm_ref.stretch(x, tempo, W, D))), (ns, x.size, tempo)
            assert t.kernel_ms() > 0.0
        run([200], [1.25])
        run([6000, 0, 333], [0.8, 1.0, 2.0])
        x = _signal("noise", 2000, 5)
        end, _ = t.plan(1.25, x.size, False, 0, -Hs)
        assert 0 < end and end + Hs <= t.out_len(x.size, 1.25)
        out = np.full(end + Hs, 7.25, F32)       # one block more than the plan allows
        w = _c_window(x, 0, 0, 1.25, 0, -Hs, out)
        assert _ffi.lib().rwkvtts_tsm_windows(t._h, ctypes.byref(w), 1) == _ffi.EINVAL
        assert np.all(out == F32(7.25)) and w.s_last == -12345
        run([200], [1.25])
    finally:
        t.close()


def _gpu_starts(t, x, tempo):
    """[s_-1, s_0, ..] as the kernel found them: the final window cut after every block, in one launch."""
    n_out = t.out_len(x.size, tempo)
    M = -(-n_out // t.hop)
    items = [(x, 0, True, tempo, 0, -t.hop, min((k + 1) * t.hop, n_out)) for k in range(M)]
    return [-t.hop] + [s for _, s in t.stretch_windows(items)]


@pytest.mark.gpu
def test_ties_go_to_the_lowest_rank(ts):
    """A signal of exact period 8: every candidate a multiple of 8 away from the template has d = 0
    exactly; of those the one nearest to 0 wins, the negative one of a +-pair first."""
    W, D = 64, 16
    t = ts(W, D)
    Hs = W // 2
    n = 3000
    x = np.tile(np.array([0.0, 0.5, 1.0, 0.25, -0.5, -1.0, -0.125, 0.75], F32), n // 8)
    for tempo in (0.8, 1.25, 1.37):
        want, s = tsm_ref.stretch(x, tempo, W, D, return_starts=True)
        assert np.array_equal(bits(t.stretch(x, tempo)), bits(want))
        assert _gpu_starts(t, x, tempo) == s
        checked = 0
        for m in range(1, len(s) - 1):
            a = tsm_ref.anchor(m, Hs, tempo)
            if a - D < 0 or a + D + Hs > n or s[m] + 2 * Hs > n:
                continue           # (the zeros outside the signal break the period)
            r = (s[m] + Hs - a) % 8                 # shifts r, r - 8, r + 8, .. have d = 0
            best = min((d for d in range(-D, D) if (d - r) % 8 == 0), key=lambda d: -2 * d - 1 if d < 0 else 2 * d)
            assert s[m + 1] == a + best, (tempo, m)
            checked += 1
        assert checked > 20


@pytest.mark.gpu
def test_nan_neither_faults_nor_wins(ts):
    W, D = 64, 40
    t = ts(W, D)
    Hs = W // 2
    x = _signal("noise", 4000, 3)
    x[1777] = np.nan
    for tempo in (0.8, 1.0, 1.37):
        want, s = tsm_ref.stretch(x, tempo, W, D, return_starts=True)
        got = t.stretch(x, tempo)
        assert same(got, want) and np.isnan(got).any()
        gs = _gpu_starts(t, x, tempo)
        assert gs == s
        seen = 0
        for m in range(1, len(gs) - 1):
            a = tsm_ref.anchor(m, Hs, tempo)
            template_clean = not (gs[m] + Hs <= 1777 < gs[m] + 2 * Hs)
            in_span = a - D <= 1777 < a + D + Hs - 1
            if template_clean and in_span:   # 2 D = 80 candidates, at most Hs = 32 of them read the NaN
                assert not (gs[m + 1] <= 1777 < gs[m + 1] + Hs), (tempo, m)
                seen += 1
        assert seen >= 1


@pytest.mark.gpu
@pytest.mark.parametrize("W,D", [(512, 128), (64, 10)])
def test_stream_over_random_cuts(ts, W, D):
    t = ts(W, D)
    rng = np.random.default_rng(5)
    x = _signal("chirp", 30 * W + 11, 0)
    for tempo in (0.5, 1.25, 1.37):
        whole = t.stretch(x, tempo)
        st = t.stream(tempo)
        parts, pos = [], 0
        while pos < x.size:
            n = int(rng.integers(0, 6 * W))
            parts.append(st.feed(x[pos:pos + n], final=pos + n >= x.size))
            pos += n
            assert st.kept <= 2 * D + int(np.ceil(W * max(tempo, 1.0))) + 2
        assert np.array_equal(bits(np.concatenate(parts)), bits(whole)) and st.kept == 0
        with pytest.raises(ValueError):
            st.feed(x[:1])


@pytest.mark.gpu
def test_pipeline_end_to_end():
    """Behind the windowed vocoder (synthetic codec, small dims): stream_speech(tempo=1.25) concatenates
    bitwise to generate_speech(tempo=1.25), again with sample_rate=24000; tempo=1.0 is generate_speech()
    itself and creates no stretcher."""
    import rwkvtts
    from rwkvtts import weights as Wt
    from rwkvtts.pipeline import LightweightTtsPipeline, LightweightTtsPipelineArgs
    from rwkvtts.tokenizer import Tokenizer
    from test_tokenizer import VOCAB
    blob = Wt.synth_blob(Wt.DIMS_TINY, seed=99)
    m = rwkvtts.DynamicBatchManager(blob, devices=[0], max_slots=4, token_chunk_size=64, tokenizer=Tokenizer(VOCAB))
    cd = codec.CODEC_DIMS_TINY
    voc = codec.BiCodecDetokenizer(codec.synth_codec_blob(cd, seed=11), cd)
    pipe = LightweightTtsPipeline(m, voc)
    try:
        args = LightweightTtsPipelineArgs(text="Hello world, this is RWKV speaking.", seed=12, max_tokens=60)
        plain = pipe.generate_speech(args)
        assert np.array_equal(bits(plain), bits(pipe.generate_speech(args, tempo=1.0)))
        assert b"".join(pipe.stream_speech(args, chunk_frames=4, tempo=1.0)) == plain.tobytes()
        assert pipe._stretcher is None and pipe._resamplers == {}
        fast = pipe.generate_speech(args, tempo=1.25)
        assert fast.size == int(np.ceil(plain.size / 1.25)) >= 1024
        assert np.array_equal(bits(fast), bits(tsm_ref.stretch(plain, 1.25)))
        chunks = list(pipe.stream_speech(args, chunk_frames=4, tempo=1.25))
        assert len(chunks) >= 2 and chunks[-1].done and b"".join(chunks) == fast.tobytes()
        both = pipe.generate_speech(args, tempo=1.25, sample_rate=24000)
        assert both.size == int(np.ceil(fast.size * 1.5))
        assert np.array_equal(bits(both), bits(pipe._resamplers[24000].resample(fast)))
        chunks = list(pipe.stream_speech(args, chunk_frames=4, tempo=1.25, sample_rate=24000))
        assert b"".join(chunks) == both.tobytes()
        # the batch form: one stretch_batch call, a failed item stays empty; silence is not stretched
        outs = pipe.generate_speech_batch([args, LightweightTtsPipelineArgs(text="emoji \U0001F600", seed=2)], tempo=1.25)
        assert np.array_equal(bits(outs[0]), bits(fast)) and outs[1].size == 0
        sil = pipe.generate_speech(LightweightTtsPipelineArgs(text="emoji \U0001F600"), tempo=1.25)
        assert sil.shape == (16000,) and not sil.any()
        sil = list(pipe.stream_speech(LightweightTtsPipelineArgs(text="emoji \U0001F600"), tempo=1.25))
        assert len(sil) == 1 and sil[0].shape == (16000,) and not sil[0].any()
    finally:
        if pipe._stretcher is not None:
            pipe._stretcher.close()
        for r in pipe._resamplers.values():
            r.close()
        m.close()
        voc.close()
