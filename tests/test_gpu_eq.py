"""csrc/eq.hip against the numpy restatement of its contract (tests/eq_ref.py), bit for bit:
chosen tap counts at the lengths where a piece ends, a ragged batch of designed filters, stream chunks, and
through the pipeline in front of the leveller."""
import numpy as np
import pytest

import eq_ref as R
import level_ref
import rwkvtts
from rwkvtts import audio
from rwkvtts import codec as CC
from rwkvtts import weights as W
from rwkvtts.pipeline import LightweightTtsPipeline, LightweightTtsPipelineArgs
from rwkvtts.tokenizer import Tokenizer
from test_tokenizer import VOCAB

pytestmark = pytest.mark.gpu
F32, bits = np.float32, R.bits
# one output, less than a lane's eight, a piece and either side, a piece whose span starts at sample 0, several pieces
LENGTHS = [1, 7, 2047, 2048, 2049, 2048 + 4095, 5000]
EIGHT = [("lowshelf", 120, 6, 0.7), ("peak", 400, -4, 2), ("peak", 1000, 3, 1.5), ("peak", 2000, -2, 3),
         ("peak", 3000, 5, 4), ("highshelf", 6000, -6, 0.7), ("highpass", 80, 0, 0.7071), ("lowpass", 7000, 0, 0.7071)]


def noise(n, seed):
    return (0.9 * np.random.default_rng(seed).uniform(-1.0, 1.0, n)).astype(F32)


@pytest.fixture(scope="module")
def eq():
    v = audio.Equaliser(device=0)
    yield v
    v.close()


@pytest.mark.parametrize("n_taps", [64, 192, 4096])
def test_chosen_taps_are_bitwise_the_contract_at_every_length(eq, n_taps):
    h = np.random.default_rng(n_taps).uniform(-0.2, 0.2, n_taps).astype(F32)  # passed in, not designed
    impulse = np.zeros(5000, dtype=F32)
    impulse[0] = 1.0
    xs = [noise(n, n) for n in LENGTHS] + [np.zeros(5000, dtype=F32), impulse]
    got = eq.eq_batch(xs, [0] * len(xs), table=[h])
    for x, y in zip(xs, got):
        assert y.dtype == F32 and y.size == x.size and np.array_equal(bits(y), bits(R.fir(x, h))), x.size
    assert eq.kernel_ms() > 0.0 and not bits(got[-2]).any()  # silence stays zero bits
    assert np.array_equal(bits(got[-1][:n_taps]), bits(h)) and not bits(got[-1][n_taps:]).any()  # the impulse returns the taps


def test_a_ragged_batch_of_three_filters_is_each_signal_alone(eq):
    xs = [noise(n, 10 + n) for n in (5000, 333, 2049, 4100)]
    specs = ["telephony", EIGHT, "warm", "telephony"]
    got = eq.eq_batch(xs, specs)
    assert len({eq.taps(s).size for s in specs}) == 3  # three tap counts in one launch
    for x, s, y in zip(xs, specs, got):
        assert np.array_equal(bits(y), bits(eq.eq(x, s))) and np.array_equal(bits(y), bits(R.fir(x, R.design(audio.eq_bands(s))[0])))


@pytest.mark.parametrize("chunk", [1, 319, 320, 2048, "ragged"])
def test_a_stream_is_bitwise_the_one_shot_and_returns_what_it_was_given(eq, chunk):
    x = noise(5000, 5)
    cuts = np.arange(chunk, 5000, chunk) if chunk != "ragged" else np.array([1, 2, 300, 301, 2349, 2350, 4999])
    st = eq.stream("telephony")
    pieces = np.split(x, cuts)
    parts = [st.feed(p, final=i + 1 == len(pieces)) for i, p in enumerate(pieces)]
    assert [p.size for p in parts] == [p.size for p in pieces]
    assert np.array_equal(bits(np.concatenate(parts)), bits(eq.eq(x, "telephony")))


def test_the_pipeline_applies_it_in_front_of_the_leveller():
    m = rwkvtts.DynamicBatchManager(W.synth_blob(W.DIMS_TINY, seed=99), devices=[0], max_slots=8, token_chunk_size=128,
                                    tokenizer=Tokenizer(VOCAB))
    voc = CC.BiCodecDetokenizer(CC.synth_codec_blob(CC.CODEC_DIMS_TINY, seed=11), CC.CODEC_DIMS_TINY)
    pipe = LightweightTtsPipeline(m, voc)
    try:
        args = lambda: LightweightTtsPipelineArgs(text="Hello world, this is RWKV speaking.", seed=12, max_tokens=80)
        plain = pipe.generate_speech(args())
        assert pipe._equaliser is None and np.array_equal(bits(pipe.generate_speech(args(), eq=None)), bits(plain))
        got = pipe.generate_speech(args(), eq="telephony", loudness=-20)
        want = level_ref.level(R.fir(plain, R.design(audio.eq_bands("telephony"))[0]), -20.0)
        assert got.size == plain.size and np.array_equal(bits(got), bits(want))
        chunks = list(pipe.stream_speech(args(), chunk_frames=4, eq="telephony", loudness=-20))
        assert len(chunks) >= 2 and b"".join(chunks) == got.tobytes()
    finally:
        m.close()
        voc.close()
        for s in list(pipe._levellers.values()) + ([pipe._equaliser] if pipe._equaliser else []):
            s.close()
