"""generate_long_speech / stream_long_speech end to end on the GPU: a tiny LM behind the native
manager, a tiny codec, the join kernels. Five segments: each segment's tokens are those of its
request run alone (segment 0 normal, the others pinned to its 32 global tokens), the PCM is the
numpy join (tests/join_ref.py) of the per-segment decode_audio, and the stream concatenates to the
batch result bit for bit, also behind the time stretch and the resampler."""
import dataclasses

import numpy as np
import pytest

import join_ref
import rwkvtts
from rwkvtts import codec as CC
from rwkvtts import weights as W
from rwkvtts.pipeline import LightweightTtsPipeline, LightweightTtsPipelineArgs, LongSpeech
from rwkvtts.segment import split_text
from rwkvtts.tokenizer import Tokenizer
from test_tokenizer import VOCAB

pytestmark = pytest.mark.gpu
TEXT = "Hello world, this is RWKV speaking. 今天天气很好。Is it fast?\nA new paragraph starts here. And the last one!"
SEG_TOKENS = 10


@pytest.fixture(scope="module")
def stack():
    blob = W.synth_blob(W.DIMS_TINY, seed=99)
    tok = Tokenizer(VOCAB)
    m = rwkvtts.DynamicBatchManager(blob, devices=[0], max_slots=8, token_chunk_size=128, tokenizer=tok)
    cd = CC.CODEC_DIMS_TINY
    voc = CC.BiCodecDetokenizer(CC.synth_codec_blob(cd, seed=11), cd)
    pipe = LightweightTtsPipeline(m, voc)
    yield pipe, m, voc, tok
    m.close()
    voc.close()
    for j in pipe._joiners.values():
        j.close()
    for r in pipe._resamplers.values():
        r.close()
    if pipe._stretcher is not None:
        pipe._stretcher.close()


def args_of(**kw):
    return LightweightTtsPipelineArgs(text=TEXT, seed=21, max_tokens=40, emotion="HAPPY", **kw)


@pytest.fixture(scope="module")
def alone(stack):
    """Each segment's request run alone: segment 0 as generate_speech builds it, the others pinned."""
    pipe, m, voc, tok = stack
    segs = split_text(TEXT, tok.encode, SEG_TOKENS)
    assert len(segs) == 5 and "".join(s.text for s in segs) == TEXT
    first = pipe._request(dataclasses.replace(args_of(), text=segs[0].text.strip()))
    g0, s0 = m.generate_tts_batch([first])[0]
    assert len(g0) == 32 and m.last_status == [0]
    out = [(g0, s0)]
    for i in range(1, 5):
        r = pipe._request(dataclasses.replace(args_of(), text=segs[i].text.strip(), seed=21 + i, voice_global_tokens=g0,
                                              pin_voice=True))
        assert r.pinned_voice and r.property_tokens == first.property_tokens
        out.append(m.generate_tts_batch([r])[0])
        assert m.last_status == [0]
    return segs, out


def test_long_speech_is_the_join_of_the_segments_run_alone(stack, alone):
    pipe, m, voc, tok = stack
    segs, tokens = alone
    out = pipe.generate_long_speech(args_of(), segment_tokens=SEG_TOKENS)
    assert isinstance(out, LongSpeech) and len(out.segments) == 5
    g0 = tokens[0][0]
    assert out.global_tokens == g0 and all(g == g0 for g, _ in tokens)  # every segment carries segment 0's globals
    assert [s["n_semantic"] for s in out.segments] == [len(s) for _, s in tokens]
    assert [s["text"] for s in out.segments] == [s.text for s in segs]
    assert [s["status"] for s in out.segments] == [0] * 5
    assert [s["truncated"] for s in out.segments] == [len(s) == 40 for _, s in tokens]
    assert sum(len(s) for _, s in tokens) > 0
    pcm = [voc.decode_audio(g, s) if s else np.zeros(0, np.float32) for g, s in tokens]
    gaps = [s.pause_ms * 16 for s in segs]
    assert gaps[-1] == 0 and 9600 in gaps and 4800 in gaps
    want, ab = join_ref.join(pcm, gaps, 0.01, 800, 80, True)
    assert [(s["a"], s["b"]) for s in out.segments] == ab
    assert np.asarray(out).tobytes() == want.tobytes()
    # other join parameters reach the kernels
    raw = pipe.generate_long_speech(args_of(), segment_tokens=SEG_TOKENS, trim=False)
    assert np.asarray(raw).tobytes() == join_ref.join(pcm, gaps, trim=False)[0].tobytes()


@pytest.mark.parametrize("kw", [{}, {"tempo": 0.8, "sample_rate": 24000}], ids=["plain", "tempo_rate"])
def test_stream_equals_batch(stack, kw):
    pipe, m, voc, tok = stack
    whole = pipe.generate_long_speech(args_of(), segment_tokens=SEG_TOKENS, **kw)
    items = list(pipe.stream_long_speech(args_of(), segment_tokens=SEG_TOKENS, **kw))
    assert len(items) == 5 and [it.segments[0] for it in items] == whole.segments
    assert np.concatenate(items).tobytes() == np.asarray(whole).tobytes()
    assert whole.size > 0 and all(it.global_tokens == whole.global_tokens for it in items)


def test_pinned_start_and_one_segment(stack, alone):
    pipe, m, voc, tok = stack
    segs, tokens = alone
    g0 = tokens[0][0]
    # pin_voice with the same voice and seed: segment 0 pinned gives what it gave unpinned
    pinned = pipe.generate_long_speech(args_of(voice_global_tokens=g0, pin_voice=True), segment_tokens=SEG_TOKENS)
    plain = pipe.generate_long_speech(args_of(), segment_tokens=SEG_TOKENS)
    assert np.asarray(pinned).tobytes() == np.asarray(plain).tobytes() and pinned.global_tokens == g0
    # one segment without trim is generate_speech
    one = LightweightTtsPipelineArgs(text="Hello world.", seed=5, max_tokens=30)
    assert np.asarray(pipe.generate_long_speech(one, trim=False)).tobytes() == pipe.generate_speech(one).tobytes()
