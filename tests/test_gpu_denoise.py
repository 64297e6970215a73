"""csrc/denoise.hip against the numpy restatement of its contract (tests/denoise_ref.py), bit for
bit: the lengths where a hop, a frame and the floor's window end, a ragged batch of three depths, stream
chunks, silence, and through the pipeline as the first stage."""
import numpy as np
import pytest

import denoise_ref as R
import rwkvtts
from rwkvtts import audio
from rwkvtts import codec as CC
from rwkvtts import weights as W
from rwkvtts.pipeline import LightweightTtsPipeline, LightweightTtsPipelineArgs
from rwkvtts.tokenizer import Tokenizer
from test_tokenizer import VOCAB

pytestmark = pytest.mark.gpu
F32, bits = np.float32, R.bits


def speechlike(n, seed):
    """A decaying 150 Hz buzz in noise: bins that the gate opens, bins it shuts, and the clamp in between."""
    t = np.arange(n) / 16000.0
    buzz = sum(np.sin(2 * np.pi * 150.0 * h * t) / h for h in range(1, 12)) * np.exp(-2.0 * t)
    return (0.2 * buzz + 0.02 * np.random.default_rng(seed).standard_normal(n)).astype(F32)


@pytest.fixture(scope="module")
def dn():
    v = audio.Denoiser(device=0)
    yield v
    v.close()


# one sample, a hop and either side, a frame and either side, and just past the floor's 125 frames
@pytest.mark.parametrize("n", [1, 127, 128, 129, 511, 512, 513, 16001])
def test_every_length_is_bitwise_the_contract(dn, n):
    x = speechlike(n, n)
    y = dn.denoise(x, 12.0)
    assert y.dtype == F32 and y.size == n and np.array_equal(bits(y), bits(R.denoise(x, 12.0)))
    assert dn.kernel_ms() > 0.0


def test_a_ragged_batch_of_three_depths_is_each_signal_alone(dn):
    xs = [speechlike(n, 10 + n) for n in (5000, 333, 16500)] + [np.zeros(0, dtype=F32)]
    depths = [3.0, 12.0, 30.0, 12.0]
    got = dn.denoise_batch(xs, depths)
    for x, d, y in zip(xs, depths, got):
        assert y.size == x.size and np.array_equal(bits(y), bits(R.denoise(x, d)))
    assert np.any(got[0] != xs[0]) and not np.array_equal(bits(got[2]), bits(R.denoise(xs[2], 12.0)))


@pytest.mark.parametrize("chunk", [1000, 333, 4097])
def test_a_stream_is_bitwise_the_one_shot(dn, chunk):
    x = speechlike(20000, 5)
    st = dn.stream(12.0)
    parts = [st.feed(x[a:a + chunk], final=a + chunk >= x.size) for a in range(0, x.size, chunk)]
    assert np.array_equal(bits(np.concatenate(parts)), bits(dn.denoise(x, 12.0)))


def test_silence_comes_back_as_zero_bits(dn):
    assert not bits(dn.denoise(np.zeros(3000, dtype=F32), 30.0)).any()


def test_the_pipeline_applies_it_first():
    m = rwkvtts.DynamicBatchManager(W.synth_blob(W.DIMS_TINY, seed=99), devices=[0], max_slots=8, token_chunk_size=128,
                                    tokenizer=Tokenizer(VOCAB))
    voc = CC.BiCodecDetokenizer(CC.synth_codec_blob(CC.CODEC_DIMS_TINY, seed=11), CC.CODEC_DIMS_TINY)
    pipe = LightweightTtsPipeline(m, voc)
    try:
        args = lambda: LightweightTtsPipelineArgs(text="Hello world, this is RWKV speaking.", seed=12, max_tokens=80)
        plain = pipe.generate_speech(args())
        assert pipe._denoiser is None and np.array_equal(bits(pipe.generate_speech(args(), denoise=None)), bits(plain))
        got = pipe.generate_speech(args(), denoise=12)
        assert got.size == plain.size and np.any(got != plain) and np.array_equal(bits(got), bits(R.denoise(plain, 12.0)))
        chunks = list(pipe.stream_speech(args(), chunk_frames=4, denoise=12))
        assert b"".join(chunks) == got.tobytes()
    finally:
        m.close()
        voc.close()
        if pipe._denoiser:
            pipe._denoiser.close()
