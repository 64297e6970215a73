"""`pitch_shift` through the pipeline on the GPU: a tiny LM behind the native manager, a tiny codec,
the shifter's kernels first of the stages. The one-shot form is shift_batch of the plain PCM; the
stream forms concatenate bit for bit to the one-shot forms, alone and with `tempo`, `loudness` and
`sample_rate`; pitch_shift=None is today's output and creates nothing; both HTTP routes return the
pipeline call's samples."""
import base64

import numpy as np
import pytest

import rwkvtts
from rwkvtts import codec as CC
from rwkvtts import server as SV
from rwkvtts import weights as W
from rwkvtts.pipeline import LightweightTtsPipeline, LightweightTtsPipelineArgs
from rwkvtts.tokenizer import Tokenizer
from test_tokenizer import VOCAB

pytestmark = pytest.mark.gpu
F32 = np.float32
LONG_TEXT = "Hello world, this is RWKV speaking. 今天天气很好。Is it fast?\nA new paragraph starts here. And the last one!"
ALL = {"pitch_shift": -3.0, "tempo": 1.25, "loudness": -16.0, "sample_rate": 24000}


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
    for s in (p._stretcher, p._shifter):
        if s is not None:
            s.close()


def _args(text="Hello world, this is RWKV speaking.", seed=12, max_tokens=80):
    return LightweightTtsPipelineArgs(text=text, seed=seed, max_tokens=max_tokens)


def test_none_is_todays_output_and_creates_nothing(pipe):
    plain = pipe.generate_speech(_args())
    for s in (None, 0, 0.0):
        assert np.array_equal(bits(plain), bits(pipe.generate_speech(_args(), pitch_shift=s)))
        assert b"".join(pipe.stream_speech(_args(), chunk_frames=4, pitch_shift=s)) == plain.tobytes()
        assert np.array_equal(bits(pipe.generate_speech_batch([_args()], pitch_shift=s)[0]), bits(plain))
        assert pipe.shifter(s) is None
    for bad in (-12.5, 12.5, float("nan"), True):
        with pytest.raises(ValueError):
            pipe.generate_speech(_args(), pitch_shift=bad)
        with pytest.raises(ValueError):
            pipe.stream_speech(_args(), pitch_shift=bad)
        with pytest.raises(ValueError):
            next(pipe.stream_long_speech(_args(), pitch_shift=bad))
    assert pipe._shifter is None


def test_generate_speech_is_shift_batch_of_the_vocoders_pcm(pipe):
    plain = pipe.generate_speech(_args())
    assert plain.size >= 4 * 1600  # outputs go out before the end: the stream below is a real one
    up = pipe.generate_speech(_args(), pitch_shift=4.0)
    assert up.size == plain.size and pipe.shifter(4.0) is pipe.shifter(-3.0) is pipe._shifter
    assert np.array_equal(bits(up), bits(pipe._shifter.shift_batch([plain], [4.0])[0]))
    a, b = _args(), _args(text="Is it fast? A new paragraph starts here.", seed=3, max_tokens=50)
    outs = pipe.generate_speech_batch([a, LightweightTtsPipelineArgs(text="emoji \U0001F600", seed=2), b], pitch_shift=4.0)
    assert outs[1].size == 0 and np.array_equal(bits(outs[0]), bits(up))
    assert np.array_equal(bits(outs[2]), bits(pipe.generate_speech(b, pitch_shift=4.0)))


@pytest.mark.parametrize("kw", [{"pitch_shift": 4.0}, ALL], ids=["alone", "all"])
def test_stream_speech_concatenates_to_generate_speech(pipe, kw):
    whole = pipe.generate_speech(_args(), **kw)
    chunks = list(pipe.stream_speech(_args(), chunk_frames=4, **kw))
    assert len(chunks) >= 2 and chunks[-1].done and b"".join(chunks) == whole.tobytes()
    assert sum(1 for c in chunks if len(c)) >= 2  # audio left before the last chunk
    if "tempo" in kw:  # the order: shift, stretch, level, resample
        x = pipe._shifter.shift(pipe.generate_speech(_args()), kw["pitch_shift"])
        x = pipe._levellers[0].level(pipe._stretcher.stretch(x, kw["tempo"]), kw["loudness"])
        assert np.array_equal(bits(whole), bits(pipe._resamplers[24000].resample(x)))


@pytest.mark.parametrize("kw", [{"pitch_shift": 4.0}, ALL], ids=["alone", "all"])
def test_long_stream_concatenates_to_long_batch(pipe, kw):
    a = _args(text=LONG_TEXT, seed=21, max_tokens=40)
    whole = pipe.generate_long_speech(a, segment_tokens=10, **kw)
    items = list(pipe.stream_long_speech(a, segment_tokens=10, **kw))
    assert len(items) == 5 and [it.segments[0] for it in items] == whole.segments
    assert whole.size > 0 and np.concatenate(items).tobytes() == np.asarray(whole).tobytes()
    if "tempo" not in kw:  # the joined signal is shifted as one, after the join
        joined = pipe.generate_long_speech(a, segment_tokens=10)
        assert np.array_equal(bits(whole), bits(pipe._shifter.shift(np.asarray(joined), 4.0)))


def test_both_http_routes_return_the_pipeline_calls_samples(pipe):
    body = {"text": "Hello world.", "seed": 7, "pitch_shift": -5, "pitch": "high"}
    err, args, kw = SV._tts_args(body, "assets/raf")
    assert err is None and kw == {"pitch_shift": -5.0}
    want = pipe.generate_speech(args, **kw)
    assert not np.array_equal(bits(want), bits(pipe.generate_speech(args)))
    code, payload = SV.handle_tts_json(body, pipe)
    assert code == 200 and base64.standard_b64decode(payload["audio_base64"]) == SV.convert_samples_to_wav(want, 16000)
    code, it = SV.handle_tts_stream(body, pipe, chunk_frames=8)
    parts = list(it)
    assert code == 200 and parts[0] == SV.streaming_wav_header(16000)
    assert b"".join(parts[1:]) == SV.samples_to_pcm16(want)
