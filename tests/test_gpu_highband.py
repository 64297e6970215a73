"""csrc/highband.hip against the numpy restatement of its contract (tests/highband_ref.py),
bit for bit, against the same chain in float64 within the bound of its sums, and through the pipeline."""
import ctypes

import numpy as np
import pytest

import highband_ref as R
import rwkvtts
from rwkvtts import _ffi, audio
from rwkvtts import codec as CC
from rwkvtts import server as SV
from rwkvtts import weights as W
from rwkvtts.pipeline import LightweightTtsPipeline, LightweightTtsPipelineArgs
from rwkvtts.tokenizer import Tokenizer
from test_tokenizer import VOCAB

pytestmark = pytest.mark.gpu
F32 = np.float32
# empty, shorter than every halo, a block edge and either side, a piece edge minus one, several pieces
LENGTHS = [0, 1, 159, 160, 161, 479, 2000]
KINDS = ["noise", "sines", "silence", "impulse", "mix"]


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _signal(kind, n):
    t = np.arange(n) / 16000.0
    noise = 0.1 * np.random.default_rng(100 + n).standard_normal(n)
    sines = 0.3 * np.sin(2 * np.pi * 1000 * t) + 0.2 * np.sin(2 * np.pi * 3000 * t)
    x = {"noise": noise, "sines": sines, "silence": np.zeros(n), "impulse": np.zeros(n),
         "mix": sines + 1.5 * noise}[kind]  # mix: blocks inside the smoothstep, gains that move
    if kind == "impulse" and n:
        x[0] = 1.0
    return x.astype(F32)


@pytest.fixture(scope="module")
def hb():
    v = audio.HighBand(device=0)
    yield v
    v.close()


@pytest.fixture(scope="module")
def cases(hb):
    """Every (kind, length) at highband 0 dB: (x, the kernels' output) from one launch pair."""
    keys = [(k, n) for k in KINDS for n in LENGTHS]
    xs = [_signal(k, n) for k, n in keys]
    return dict(zip(keys, zip(xs, hb.extend_batch(xs, [0.0] * len(xs)))))


@pytest.mark.parametrize("kind", KINDS)
def test_batch_is_bitwise_the_restatement(hb, cases, kind):
    for n in LENGTHS:
        x, y = cases[(kind, n)]
        assert y.dtype == F32 and y.size == 2 * n
        assert np.array_equal(bits(y), bits(R.highband(x, 0.0, tab=hb.table))), (kind, n)
        if kind in ("silence", "sines"):  # no high band: the input, +0 for +0, and the plain interpolation between
            assert np.array_equal(bits(y[0::2]), bits(x))
            assert np.array_equal(bits(y[1::2]), bits(R.fir(x, R.split(hb.table)[1], 16)))
    assert hb.kernel_ms() > 0.0 and (kind != "mix" or np.unique(R.highband(x, 0.0, parts=True)[3]).size > 320)  # (gains that move)


def test_a_ragged_batch_with_a_level_per_signal(hb):
    xs = [_signal("noise", 700), _signal("mix", 1283), _signal("noise", 322)]
    dbs = [-12.0, 3.5, 12.0]
    for x, db, y in zip(xs, dbs, hb.extend_batch(xs, dbs)):
        assert np.array_equal(bits(y), bits(R.highband(x, db, tab=hb.table))), db


@pytest.mark.parametrize("kind", ["noise", "mix"])
def test_within_the_bound_of_the_float64_chain(hb, cases, kind):
    """|y32 - y64| <= (31 + 32 + 63 + 2) * 2^-23 * sum|addend|, the addends of the chain's nested sums:
    |x| through |hp|, |ip| and |sh|, times the gain, plus |u|'s own."""
    x, y = cases[(kind, 2000)]
    y64, _, _, gain = R.highband(x, 0.0, tab=hb.table, dtype=np.float64, parts=True)
    hp, ip, sh, _ = (np.abs(t.astype(np.float64)) for t in R.split(hb.table))
    xa = np.abs(x.astype(np.float64))
    ab = R.fir(xa, hp, 15)
    au, av = np.zeros(4000), np.zeros(4000)
    au[0::2], au[1::2], av[0::2], av[1::2] = xa, R.fir(xa, ip, 16), ab, R.fir(ab, ip, 16)
    bound = 128 * 2.0 ** -23 * (au + gain * R.fir(av, sh, 31))
    err = np.abs(y.astype(np.float64) - y64)
    print(f"highband {kind}: max |y32 - y64| {err.max():.3e}, max err / bound {np.max(err / np.maximum(bound, 1e-30)):.4f}")
    assert np.all(err <= bound)


def test_windows_driven_by_the_plan_are_the_whole_signal(hb):
    x = _signal("mix", 2000)
    G = hb.gain(2.0)
    whole = hb.extend(x, 2.0)
    items, out_next, first = [], 0, 0
    for n_known, final in ((333, False), (777, False), (1501, False), (2000, True)):
        end = hb.plan(n_known, final, out_next)[0]
        items.append((x[first:n_known], first, final, G, out_next, end - out_next))
        out_next, first = end, hb.plan(n_known, False, end)[1]
    assert all(it[5] > 0 for it in items) and [it[1] > 0 for it in items] == [False, False, True, True]
    assert np.array_equal(bits(np.concatenate(hb.extend_windows(items))), bits(whole))
    st = hb.stream(2.0)
    parts = [st.feed(p, final=i == 3) for i, p in enumerate(np.split(x, [333, 777, 1501]))]
    assert np.array_equal(bits(np.concatenate(parts)), bits(whole))
    # one output too many, and one sample too few at the front: EINVAL, nothing written
    x2, a2, _, _, o2, c2 = items[2]
    for samples, in_first, count in ((x2, a2, c2 + 1), (np.ascontiguousarray(x2[1:]), a2 + 1, c2)):
        out = np.full(count, 7.0, dtype=F32)
        w = _ffi.HighBandWindow(struct_size=ctypes.sizeof(_ffi.HighBandWindow), in_=samples.ctypes.data, in_first=in_first,
                                n_in=samples.size, final=0, G=float(G), out_first=o2, out_count=count, out=out.ctypes.data)
        assert _ffi.lib().rwkvtts_highband_windows(hb._h, ctypes.byref(w), 1) == _ffi.EINVAL and np.all(out == 7.0)


@pytest.fixture(scope="module")
def pipe():
    m = rwkvtts.DynamicBatchManager(W.synth_blob(W.DIMS_TINY, seed=99), devices=[0], max_slots=8, token_chunk_size=128,
                                    tokenizer=Tokenizer(VOCAB))
    voc = CC.BiCodecDetokenizer(CC.synth_codec_blob(CC.CODEC_DIMS_TINY, seed=11), CC.CODEC_DIMS_TINY)
    p = LightweightTtsPipeline(m, voc)
    yield p
    m.close()
    voc.close()
    for s in list(p._resamplers.values()) + ([p._extender] if p._extender else []):
        s.close()


def test_the_pipeline_applies_it_before_a_resampler_from_32_khz(pipe, hb):
    args = lambda: LightweightTtsPipelineArgs(text="Hello world, this is RWKV speaking.", seed=12, max_tokens=80)
    plain = pipe.generate_speech(args())
    rs48 = audio.Resampler(16000, 48000, device=0, align="zero")
    rs32 = audio.Resampler(32000, 48000, device=0, align="zero")
    try:
        assert np.array_equal(bits(pipe.generate_speech(args(), highband=None)), bits(plain))
        assert np.array_equal(bits(pipe.generate_speech(args(), sample_rate=48000, highband=None)), bits(rs48.resample(plain)))
        assert pipe._extender is None and set(pipe._resamplers) == {48000}
        for rate in (24000, 16000, None):
            for call in (pipe.generate_speech, pipe.stream_speech):
                with pytest.raises(ValueError):
                    call(args(), sample_rate=rate, highband=0.0)
        with pytest.raises(ValueError):
            pipe.generate_speech(args(), sample_rate=48000, highband=12.5)
        wide = hb.extend(plain, 0.0)
        assert wide.size == 2 * plain.size and not np.array_equal(wide[1::2], R.fir(plain, R.split(hb.table)[1], 16))
        want = rs32.resample(wide)
        assert np.array_equal(bits(pipe.generate_speech(args(), sample_rate=48000, highband=0.0)), bits(want))
        chunks = list(pipe.stream_speech(args(), chunk_frames=4, sample_rate=48000, highband=0.0))
        assert len(chunks) >= 2 and chunks[-1].done and b"".join(chunks) == want.tobytes()
        assert np.array_equal(bits(pipe.generate_speech_batch([args()], sample_rate=48000, highband=0.0)[0]), bits(want))
        # at 32 kHz no resampler runs
        assert np.array_equal(bits(pipe.generate_speech(args(), sample_rate=32000, highband=3.0)), bits(hb.extend(plain, 3.0)))
        assert set(pipe._resamplers) == {48000, (32000, 48000)}
        for long_ in (pipe.generate_long_speech(args(), sample_rate=48000, highband=0.0, trim=False),
                      np.concatenate(list(pipe.stream_long_speech(args(), sample_rate=48000, highband=0.0, trim=False)))):
            assert np.asarray(long_).tobytes() == want.tobytes()
    finally:
        rs48.close()
        rs32.close()
    body = {"text": "Hello world, this is RWKV speaking.", "seed": 12, "highband": 0, "sample_rate": 48000}
    err, _, kw = SV._tts_args(body, "assets/raf")
    assert err is None and kw == {"sample_rate": 48000, "highband": 0.0}
    for bad in ({"sample_rate": 24000}, {"highband": 13}, {"highband": "3"}, {"highband": True}):
        assert SV._tts_args({**body, **bad}, "assets/raf")[0][0] == 400
    assert SV._tts_args({"text": "x", "highband": 0}, "assets/raf")[0][0] == 400
