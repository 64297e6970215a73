"""`watermark` through the pipeline on the GPU: a tiny LM behind the native manager, a tiny codec, the
marker's kernel after the leveller and before the resampler. One-shot equals Watermarker.embed of the
unmarked result, the stream forms concatenate bit for bit to the one-shot forms, the order with
`loudness` and `sample_rate` is level -> mark -> resample, a pipeline without a key refuses before
anything is generated, and watermark=None is today's output and creates nothing."""
import numpy as np
import pytest

import rwkvtts
import wm_ref
from rwkvtts import codec as CC
from rwkvtts import weights as W
from rwkvtts.pipeline import LightweightTtsPipeline, LightweightTtsPipelineArgs
from rwkvtts.tokenizer import Tokenizer
from test_tokenizer import VOCAB

pytestmark = pytest.mark.gpu
F32 = np.float32
KEY = 0xC0FFEE0DDBA11
LONG_TEXT = "Hello world, this is RWKV speaking. 今天天气很好。Is it fast?\nA new paragraph starts here. And the last one!"
BAD = "emoji \U0001F600"  # untokenisable: the request fails


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


@pytest.fixture(scope="module")
def pipes():
    blob = W.synth_blob(W.DIMS_TINY, seed=99)
    m = rwkvtts.DynamicBatchManager(blob, devices=[0], max_slots=8, token_chunk_size=128, tokenizer=Tokenizer(VOCAB))
    cd = CC.CODEC_DIMS_TINY
    voc = CC.BiCodecDetokenizer(CC.synth_codec_blob(cd, seed=11), cd)
    p, bare = LightweightTtsPipeline(m, voc, watermark_key=KEY), LightweightTtsPipeline(m, voc)
    yield p, bare
    m.close()
    voc.close()
    for q in (p, bare):
        for s in list(q._joiners.values()) + list(q._resamplers.values()) + list(q._levellers.values()):
            s.close()
        if q._marker is not None:
            q._marker.close()


def _args(text="Hello world, this is RWKV speaking.", seed=12, max_tokens=80):
    return LightweightTtsPipelineArgs(text=text, seed=seed, max_tokens=max_tokens)


def test_none_is_todays_output_and_a_missing_key_or_a_bad_payload_raises_first(pipes):
    p, bare = pipes
    plain = bare.generate_speech(_args())
    assert np.array_equal(bits(plain), bits(p.generate_speech(_args(), watermark=None)))
    assert b"".join(p.stream_speech(_args(), chunk_frames=4, watermark=None)) == plain.tobytes()
    assert np.array_equal(bits(p.generate_speech_batch([_args()], watermark=None)[0]), bits(plain))
    assert p._marker is None and p.marker(None) is None
    calls = []
    real = bare.manager.generate_tts_batch
    bare.manager.generate_tts_batch = lambda *a, **k: calls.append(1) or real(*a, **k)
    try:
        for q, bad in ((bare, 7), (bare, 0), (p, -1), (p, 65536), (p, True), (p, 1.5), (p, "7")):
            with pytest.raises(ValueError):
                q.generate_speech(_args(), watermark=bad)
            with pytest.raises(ValueError):
                q.generate_speech_batch([_args()], watermark=bad)
            with pytest.raises(ValueError):
                q.stream_speech(_args(), watermark=bad)
            with pytest.raises(ValueError):
                q.generate_long_speech(_args(), watermark=bad)
            with pytest.raises(ValueError):
                next(q.stream_long_speech(_args(), watermark=bad))
        with pytest.raises(ValueError):
            bare.detect_watermark(plain)
    finally:
        bare.manager.generate_tts_batch = real
    assert calls == [] and bare._marker is None and p._marker is None
    with pytest.raises(ValueError):
        LightweightTtsPipeline(bare.manager, bare.codec, watermark_key=-1)


def test_generate_speech_is_embed_of_the_unmarked_result_and_reads_back(pipes):
    p, _ = pipes
    plain = p.generate_speech(_args())
    assert plain.size >= 16 * 1600
    marked = p.generate_speech(_args(), watermark=0xBEEF)
    assert np.array_equal(bits(marked), bits(p._marker.embed(plain, KEY, 0xBEEF)))
    assert np.array_equal(bits(marked), bits(wm_ref.embed(plain, KEY, 0xBEEF)))
    assert marked.size == plain.size and not np.array_equal(bits(marked), bits(plain))
    assert p.marker(1) is p.marker(65535) is p._marker  # one object, the payload per call
    got, ref = p.detect_watermark(marked), wm_ref.detect(marked, KEY)
    print("pipeline clip:", marked.size / 16000.0, "s, score", got["score"], "reference", ref["score"])
    assert got["detected"] == ref["detected"] and got["seen"] == ref["seen"] and got["threshold"] == ref["threshold"]
    # the pipeline's own detector and key on a clip that is speech-like (a tiny synthetic vocoder's PCM is not)
    clip = p._marker.embed(wm_ref.vowel(48000, 3), KEY, 0xBEEF)[5000:]
    got = p.detect_watermark(clip)
    assert got["detected"] and (got["offset"], got["payload"], got["seen"]) == (5000, 0xBEEF, 0xFFFF)
    assert not p.detect_watermark(wm_ref.vowel(48000, 3))["detected"]
    outs = p.generate_speech_batch([_args(), LightweightTtsPipelineArgs(text=BAD, seed=2)], watermark=0xBEEF)
    assert outs[1].size == 0 and np.array_equal(bits(outs[0]), bits(marked))
    sil = p.generate_speech(LightweightTtsPipelineArgs(text=BAD), watermark=0xBEEF)
    assert sil.shape == (16000,) and not sil.any()


@pytest.mark.parametrize("kw", [{"watermark": 0x1234}, {"watermark": 7, "loudness": -20.0, "sample_rate": 8000}],
                         ids=["alone", "loudness_rate"])
def test_stream_speech_concatenates_to_generate_speech(pipes, kw):
    p, _ = pipes
    whole = p.generate_speech(_args(), **kw)
    chunks = list(p.stream_speech(_args(), chunk_frames=4, **kw))
    assert len(chunks) >= 2 and chunks[-1].done and b"".join(chunks) == whole.tobytes()
    assert sum(1 for c in chunks if len(c)) >= 2  # audio left before the last chunk
    if "loudness" in kw:  # the order: level, mark, resample
        lev = p.generate_speech(_args(), loudness=kw["loudness"])
        marked = p._marker.embed(lev, KEY, kw["watermark"])
        assert np.array_equal(bits(whole), bits(p._resamplers[8000].resample(marked)))
        other = p._levellers[0].level(p._marker.embed(p.generate_speech(_args()), KEY, kw["watermark"]), kw["loudness"])
        assert not np.array_equal(bits(whole), bits(p._resamplers[8000].resample(other)))


def test_long_stream_concatenates_to_long_batch_and_marks_the_joined_signal(pipes):
    p, _ = pipes
    a = _args(text=LONG_TEXT, seed=21, max_tokens=40)
    whole = p.generate_long_speech(a, segment_tokens=10, watermark=0x00AA)
    items = list(p.stream_long_speech(a, segment_tokens=10, watermark=0x00AA))
    assert len(items) == 5 and [it.segments[0] for it in items] == whole.segments
    assert whole.size > 0 and np.concatenate(items).tobytes() == np.asarray(whole).tobytes()
    joined = p.generate_long_speech(a, segment_tokens=10)
    assert np.array_equal(bits(whole), bits(p._marker.embed(np.asarray(joined), KEY, 0x00AA)))  # one continuous sequence
