"""csrc/limit.hip against the numpy restatement of its contract (tests/limit_ref.py), bit
for bit: a ragged batch, plan-driven windows, and through the pipeline behind the resampler."""
import ctypes

import numpy as np
import pytest

import limit_ref as R
import rwkvtts
from rwkvtts import _ffi, audio
from rwkvtts import codec as CC
from rwkvtts import weights as W
from rwkvtts.pipeline import LightweightTtsPipeline, LightweightTtsPipelineArgs
from rwkvtts.tokenizer import Tokenizer
from test_tokenizer import VOCAB

pytestmark = pytest.mark.gpu
F32, bits = np.float32, R.bits
# empty, shorter than every halo, the halo and either side, a piece edge and either side, several pieces
LENGTHS = [0, 1, 5, 69, 70, 71, 1023, 1024, 1025, 2200]
LIMITS = [0.0, -1.0, -6.0]


@pytest.fixture(scope="module")
def lim():
    v = audio.Limiter(device=0)
    yield v
    v.close()


@pytest.fixture(scope="module")
def cases(lim):
    """limit -> (signals, the contract's outputs, the kernel's outputs from one ragged launch). The last
    signal stays under every ceiling: its pieces take the kernel's copy path."""
    xs = [R.burst(n) for n in LENGTHS] + [R.burst(2200, 0.1)]
    return {db: (xs, [R.limit(x, db, tab=lim.table) for x in xs], lim.limit_batch(xs, [db] * len(xs))) for db in LIMITS}


@pytest.mark.parametrize("limit", LIMITS)
def test_a_ragged_batch_is_bitwise_the_contract_and_each_signal_alone(lim, cases, limit):
    xs, want, got = cases[limit]
    for x, w, y in zip(xs, want, got):
        assert y.dtype == F32 and y.size == x.size and (x.size == 0 or np.max(np.abs(y)) <= R.ceiling(limit))
        assert np.array_equal(bits(y), bits(w)), x.size
        assert np.array_equal(bits(lim.limit(x, limit)), bits(w)), x.size
    assert lim.kernel_ms() > 0.0 and np.array_equal(bits(got[-1]), bits(xs[-1]))
    assert sum(int(np.any(y != x)) for x, y in zip(xs, got)) == len(LENGTHS) - 1  # all but the empty one were bound
    mixed = lim.limit_batch(xs[-3:], LIMITS)  # and a ceiling per signal in one launch
    assert all(np.array_equal(bits(y), bits(cases[db][1][-3 + i])) for i, (db, y) in enumerate(zip(LIMITS, mixed)))


@pytest.mark.parametrize("chunk", [1, 160, 1500])
def test_windows_driven_by_the_plan_are_the_batch(lim, cases, chunk):
    xs, _, whole = cases[-1.0]
    c = lim.ceiling(-1.0)
    items, owner = [], []
    for s, x in enumerate(xs):
        out_next = first = 0
        for n_known in list(range(chunk, x.size, chunk)) + [x.size]:
            final = n_known == x.size
            end = lim.plan(n_known, final, out_next)[0]
            items.append((x[first:n_known], first, final, c, out_next, end - out_next))
            owner.append(s)
            out_next, first = end, lim.plan(n_known, False, end)[1]
    outs = lim.limit_windows(items)  # every window of every signal in one launch
    for s, y in enumerate(whole):
        assert np.array_equal(bits(np.concatenate([o for o, k in zip(outs, owner) if k == s] or [np.zeros(0, F32)])), bits(y))
    st, step = lim.stream(-1.0), max(chunk, 100)  # and LimiterStream on the kernel (not sample by sample: a call each)
    parts = [st.feed(xs[-2][a:a + step], final=a + step >= 2200) for a in range(0, 2200, step)]
    assert np.array_equal(bits(np.concatenate(parts)), bits(whole[-2]))


def test_a_window_that_lacks_a_sample_is_einval_and_writes_nothing(lim):
    x = R.burst(2200)
    # one output too many at the end (ready: 1000 - 70), one sample too few at the front (needed: 400 - 69)
    for samples, in_first, out_first, count in ((x[:1000], 0, 0, 931), (x[332:1000], 332, 400, 100)):
        out, samples = np.full(count, 7.0, dtype=F32), np.ascontiguousarray(samples)
        w = _ffi.LimitWindow(struct_size=ctypes.sizeof(_ffi.LimitWindow), in_=samples.ctypes.data, in_first=in_first,
                             n_in=samples.size, final=0, c=1.0, out_first=out_first, out_count=count, out=out.ctypes.data)
        assert _ffi.lib().rwkvtts_limit_windows(lim._h, ctypes.byref(w), 1) == _ffi.EINVAL and np.all(out == 7.0)


@pytest.fixture(scope="module")
def pipe():
    m = rwkvtts.DynamicBatchManager(W.synth_blob(W.DIMS_TINY, seed=99), devices=[0], max_slots=8, token_chunk_size=128,
                                    tokenizer=Tokenizer(VOCAB))
    voc = CC.BiCodecDetokenizer(CC.synth_codec_blob(CC.CODEC_DIMS_TINY, seed=11), CC.CODEC_DIMS_TINY)
    p = LightweightTtsPipeline(m, voc)
    yield p
    m.close()
    voc.close()
    for s in list(p._resamplers.values()) + list(p._levellers.values()) + ([p._limiter] if p._limiter else []):
        s.close()


def test_the_pipeline_applies_it_last_behind_the_resampler(pipe, lim):
    """The leveller's 0.891 cap against a 0.251 ceiling makes the limiter bind."""
    args = lambda: LightweightTtsPipelineArgs(text="Hello world, this is RWKV speaking.", seed=12, max_tokens=80)
    loud = pipe.generate_speech(args(), loudness=-10, sample_rate=48000)
    assert np.array_equal(bits(pipe.generate_speech(args(), loudness=-10, sample_rate=48000, limit=None)), bits(loud))
    got = pipe.generate_speech(args(), loudness=-10, limit=-12, sample_rate=48000)
    assert pipe._limiter is not None and got.size == loud.size and not np.array_equal(bits(got), bits(loud))
    assert np.array_equal(bits(got), bits(R.limit(loud, -12.0, tab=lim.table)))
    assert np.max(np.abs(got)) <= R.ceiling(-12.0) < np.max(np.abs(loud))
    chunks = list(pipe.stream_speech(args(), chunk_frames=4, loudness=-10, limit=-12, sample_rate=48000))
    assert len(chunks) >= 2 and chunks[-1].done and b"".join(chunks) == got.tobytes()
    assert np.array_equal(bits(pipe.generate_speech_batch([args()], loudness=-10, limit=-12, sample_rate=48000)[0]), bits(got))
