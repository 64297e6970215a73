"""`loudness` through the pipeline on the GPU: a tiny LM behind the native manager, a tiny codec, the
leveller's kernels between the stretch and the resampler. The stream forms concatenate bit for bit to
the one-shot forms, alone and with `tempo` and `sample_rate`; the batch form equals per-item calls;
loudness=None is today's output and creates nothing; the failed-request silence is not levelled."""
import numpy as np
import pytest

import level_ref
import rwkvtts
from rwkvtts import codec as CC
from rwkvtts import weights as W
from rwkvtts.pipeline import LightweightTtsPipeline, LightweightTtsPipelineArgs
from rwkvtts.tokenizer import Tokenizer
from test_tokenizer import VOCAB

pytestmark = pytest.mark.gpu
F32 = np.float32
LONG_TEXT = "Hello world, this is RWKV speaking. 今天天气很好。Is it fast?\nA new paragraph starts here. And the last one!"
BAD = "emoji \U0001F600"  # untokenisable: the request fails


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


@pytest.fixture(scope="module")
def pipe():
    blob = W.synth_blob(W.DIMS_TINY, seed=99)
    m = rwkvtts.DynamicBatchManager(blob, devices=[0], max_slots=8, token_chunk_size=128, tokenizer=Tokenizer(VOCAB))
    cd = CC.CODEC_DIMS_TINY
    voc = CC.BiCodecDetokenizer(CC.synth_codec_blob(cd, seed=11), cd)
    p = LightweightTtsPipeline(m, voc)
    yield p
    m.close()
    voc.close()
    for s in list(p._joiners.values()) + list(p._resamplers.values()) + list(p._levellers.values()):
        s.close()
    if p._stretcher is not None:
        p._stretcher.close()


def _args(text="Hello world, this is RWKV speaking.", seed=12, max_tokens=80):
    return LightweightTtsPipelineArgs(text=text, seed=seed, max_tokens=max_tokens)


def test_none_is_todays_output_and_creates_nothing(pipe):
    plain = pipe.generate_speech(_args())
    assert np.array_equal(bits(plain), bits(pipe.generate_speech(_args(), loudness=None)))
    assert b"".join(pipe.stream_speech(_args(), chunk_frames=4, loudness=None)) == plain.tobytes()
    assert np.array_equal(bits(pipe.generate_speech_batch([_args()], loudness=None)[0]), bits(plain))
    assert pipe._levellers == {} and pipe.leveller(None) is None
    for bad in (-41.0, -9.5, 0.0, float("nan"), True):
        with pytest.raises(ValueError):
            pipe.generate_speech(_args(), loudness=bad)
        with pytest.raises(ValueError):
            pipe.stream_speech(_args(), loudness=bad)
        with pytest.raises(ValueError):
            next(pipe.stream_long_speech(_args(), loudness=bad))
    assert pipe._levellers == {}


def test_generate_speech_is_the_restatement_of_the_vocoders_pcm(pipe):
    plain = pipe.generate_speech(_args())
    assert plain.size >= 16 * 1600  # blocks go out before the end: the stream below is a real one
    lev = pipe.generate_speech(_args(), loudness=-23.0)
    assert np.array_equal(bits(lev), bits(level_ref.level(plain, -23.0)))
    assert not np.array_equal(bits(lev), bits(plain)) and np.max(np.abs(lev)) <= float(F32(0.891)) * (1 + 2.0 ** -20)
    assert pipe.leveller(-23.0) is pipe.leveller(-16.0) is pipe._levellers[0]  # one object, the target per call
    assert pipe.leveller(-16.0, horizon=50) is pipe._levellers[50] is not pipe._levellers[0]


@pytest.mark.parametrize("kw", [{"loudness": -23.0}, {"loudness": -16.0, "tempo": 1.25, "sample_rate": 24000}],
                         ids=["alone", "tempo_rate"])
def test_stream_speech_concatenates_to_generate_speech(pipe, kw):
    whole = pipe.generate_speech(_args(), **kw)
    chunks = list(pipe.stream_speech(_args(), chunk_frames=4, **kw))
    assert len(chunks) >= 2 and chunks[-1].done and b"".join(chunks) == whole.tobytes()
    assert sum(1 for c in chunks if len(c)) >= 2  # audio left before the last chunk
    if "tempo" in kw:  # the order: stretch, level, resample
        fast = pipe.generate_speech(_args(), tempo=kw["tempo"])
        lev = pipe._levellers[0].level(fast, kw["loudness"])
        assert np.array_equal(bits(whole), bits(pipe._resamplers[24000].resample(lev)))


@pytest.mark.parametrize("kw", [{"loudness": -23.0}, {"loudness": -16.0, "tempo": 0.8, "sample_rate": 24000}],
                         ids=["alone", "tempo_rate"])
def test_long_stream_concatenates_to_long_batch(pipe, kw):
    a = _args(text=LONG_TEXT, seed=21, max_tokens=40)
    whole = pipe.generate_long_speech(a, segment_tokens=10, **kw)
    items = list(pipe.stream_long_speech(a, segment_tokens=10, **kw))
    assert len(items) == 5 and [it.segments[0] for it in items] == whole.segments
    assert whole.size > 0 and np.concatenate(items).tobytes() == np.asarray(whole).tobytes()
    if "tempo" not in kw:  # the joined signal is levelled as one
        joined = pipe.generate_long_speech(a, segment_tokens=10)
        assert np.array_equal(bits(whole), bits(pipe._levellers[0].level(np.asarray(joined), -23.0)))


def test_batch_equals_per_item_calls_and_silence_is_not_levelled(pipe):
    a, b = _args(), _args(text="Is it fast? A new paragraph starts here.", seed=3, max_tokens=50)
    outs = pipe.generate_speech_batch([a, LightweightTtsPipelineArgs(text=BAD, seed=2), b], loudness=-20.0)
    assert outs[1].size == 0  # a failed item stays empty
    assert np.array_equal(bits(outs[0]), bits(pipe.generate_speech(a, loudness=-20.0)))
    assert np.array_equal(bits(outs[2]), bits(pipe.generate_speech(b, loudness=-20.0)))
    # the failed request's second of silence never reaches the leveller
    lv, calls = pipe._levellers[0], []
    real_batch, real_stream = lv.level_batch, lv.stream
    lv.level_batch = lambda *a_, **k_: calls.append("batch") or real_batch(*a_, **k_)
    lv.stream = lambda *a_, **k_: calls.append("stream") or real_stream(*a_, **k_)
    try:
        sil = pipe.generate_speech(LightweightTtsPipelineArgs(text=BAD), loudness=-20.0)
        assert sil.shape == (16000,) and not sil.any() and calls == []
        sil = pipe.generate_speech(LightweightTtsPipelineArgs(text=BAD), loudness=-20.0, sample_rate=24000)
        assert sil.shape == (24000,) and not sil.any() and calls == []
        sil = list(pipe.stream_speech(LightweightTtsPipelineArgs(text=BAD), loudness=-20.0))
        assert len(sil) == 1 and sil[0].shape == (16000,) and not sil[0].any()
        assert "batch" not in calls  # (the stream object exists, nothing was fed to it)
        sil = pipe.generate_long_speech(LightweightTtsPipelineArgs(text=BAD), loudness=-20.0)
        assert sil.shape == (16000,) and not np.asarray(sil).any() and "batch" not in calls
    finally:
        lv.level_batch, lv.stream = real_batch, real_stream
