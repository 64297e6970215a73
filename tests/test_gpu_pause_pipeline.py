"""`max_pause` through the pipeline on the GPU: a tiny LM behind the native manager, a tiny codec, the
pause kernels in front of every other stage. generate_speech equals the numpy restatement applied to
the vocoder's PCM, the stream forms concatenate bit for bit to the one-shot forms, alone and with
`tempo` and `sample_rate` in the stated order; long form shapes per segment before the join, whose
gaps survive; both routes carry the keyword; max_pause=None is today's output and creates nothing.

The synthetic vocoder emits noise, so a fixed threshold finds no silence and every comparison would
pass with nothing cut. Each case therefore takes its threshold from its own unshaped PCM
(`_threshold`) and asserts that the restatement cuts. The median block peak would not do: with half
of the blocks loud and a hang of 5 blocks, no block of noise is left non-active. The threshold here
lies between the third and the fourth largest block peak instead: three loud blocks make at most 33
blocks active and four runs, and the PCM has more than 33 + 4 * 2 blocks, so at M = 320 samples (two
blocks) a run longer than M exists whatever the noise looks like."""
import base64

import numpy as np
import pytest

import pause_ref
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
BAD = "emoji \U0001F600"  # untokenisable: the request fails
MS = 20           # the cap of every case, in ms
M = MS * 16       # and in samples


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
    for s in list(p._joiners.values()) + list(p._resamplers.values()) + list(p._shapers.values()):
        s.close()
    if p._stretcher is not None:
        p._stretcher.close()


def _args(text="Hello world, this is RWKV speaking.", seed=12, max_tokens=80):
    return LightweightTtsPipelineArgs(text=text, seed=seed, max_tokens=max_tokens)


def _threshold(pcm, k=3):
    """Between the k-th and the (k + 1)-th largest peak of the 160-sample blocks: exactly k loud blocks."""
    x = np.asarray(pcm, dtype=F32)
    nb = x.size // 160
    assert nb > 11 * k + 2 * (k + 1)
    peaks = np.sort(np.abs(x[:nb * 160]).reshape(nb, 160).max(axis=1))[::-1]
    assert peaks[k - 1] > peaks[k] > 0
    return float(F32((float(peaks[k - 1]) + float(peaks[k])) / 2.0))


def _want(pcm, thr):
    """The restatement at the pipeline's defaults; a case without a cut fails."""
    y, cuts = pause_ref.shape(pcm, M, 160, 5, 80, thr)
    assert cuts >= 1 and y.size < np.asarray(pcm).size, "the case cuts nothing: it would pass vacuously"
    return y


def test_none_is_todays_output_and_creates_nothing(pipe):
    plain = pipe.generate_speech(_args())
    assert np.array_equal(bits(plain), bits(pipe.generate_speech(_args(), max_pause=None)))
    assert b"".join(pipe.stream_speech(_args(), chunk_frames=4, max_pause=None)) == plain.tobytes()
    assert np.array_equal(bits(pipe.generate_speech_batch([_args()], max_pause=None)[0]), bits(plain))
    assert pipe._shapers == {} and pipe.pause_shaper(None) is None
    for bad in (19, 5001, 0, 300.5, float("nan"), True):
        with pytest.raises(ValueError):
            pipe.generate_speech(_args(), max_pause=bad)
        with pytest.raises(ValueError):
            pipe.stream_speech(_args(), max_pause=bad)
        with pytest.raises(ValueError):
            pipe.generate_speech_batch([_args()], max_pause=bad)
        with pytest.raises(ValueError):
            pipe.generate_long_speech(_args(), max_pause=bad)
        with pytest.raises(ValueError):
            next(pipe.stream_long_speech(_args(), max_pause=bad))
    assert pipe._shapers == {}


def test_generate_speech_is_the_restatement_of_the_vocoders_pcm(pipe):
    plain = pipe.generate_speech(_args())
    thr = _threshold(plain)
    ps = pipe.pause_shaper(MS, threshold=thr)
    assert ps is pipe.pause_shaper(300) and ps.threshold == thr  # one object, the cap per call
    want = _want(plain, thr)
    got = pipe.generate_speech(_args(), max_pause=MS)
    assert np.array_equal(bits(got), bits(want)) and ps.cuts == [pause_ref.shape(plain, M, 160, 5, 80, thr)[1]]
    # a cap nothing reaches changes nothing
    assert np.array_equal(bits(pipe.generate_speech(_args(), max_pause=5000)), bits(pause_ref.shape(plain, 80000, 160, 5, 80, thr)[0]))
    # the batch form: one call, a failed item stays empty
    b = _args(text="Is it fast? A new paragraph starts here.", seed=3, max_tokens=50)
    outs = pipe.generate_speech_batch([_args(), LightweightTtsPipelineArgs(text=BAD, seed=2), b], max_pause=MS)
    assert outs[1].size == 0 and np.array_equal(bits(outs[0]), bits(want))
    assert np.array_equal(bits(outs[2]), bits(pause_ref.shape(pipe.generate_speech(b), M, 160, 5, 80, thr)[0]))
    # the failed request's second of silence is not shaped (shaped, it would be empty)
    sil = pipe.generate_speech(LightweightTtsPipelineArgs(text=BAD), max_pause=MS)
    assert sil.shape == (16000,) and not sil.any()
    sil = list(pipe.stream_speech(LightweightTtsPipelineArgs(text=BAD), max_pause=MS))
    assert len(sil) == 1 and sil[0].shape == (16000,) and not sil[0].any()


@pytest.mark.parametrize("kw", [{}, {"tempo": 1.25, "sample_rate": 24000}], ids=["alone", "tempo_rate"])
def test_stream_speech_concatenates_to_generate_speech(pipe, kw):
    plain = pipe.generate_speech(_args())
    thr = _threshold(plain)
    pipe.pause_shaper(MS, threshold=thr)
    want = _want(plain, thr)
    whole = pipe.generate_speech(_args(), max_pause=MS, **kw)
    chunks = list(pipe.stream_speech(_args(), chunk_frames=4, max_pause=MS, **kw))
    assert len(chunks) >= 2 and chunks[-1].done and b"".join(chunks) == whole.tobytes()
    if kw:  # the order: pause, stretch, resample
        fast = pipe._stretcher.stretch(want, kw["tempo"])
        assert np.array_equal(bits(whole), bits(pipe._resamplers[24000].resample(fast)))
    else:
        assert np.array_equal(bits(whole), bits(want))
        # t0, t1 stay the vocoder's frames; the lengths no longer follow from them
        unshaped = list(pipe.stream_speech(_args(), chunk_frames=4))
        assert [(c.t0, c.t1) for c in chunks] == [(c.t0, c.t1) for c in unshaped]
        assert sum(len(c) for c in chunks) < sum(len(c) for c in unshaped) == plain.size


def test_long_form_shapes_per_segment_and_the_gaps_survive(pipe):
    a = _args(text=LONG_TEXT, seed=21, max_tokens=40)
    seen = []
    real = pipe.codec.decode_audio_batch
    pipe.codec.decode_audio_batch = lambda res: seen.append(real(res)) or seen[-1]
    try:
        plain = pipe.generate_long_speech(a, segment_tokens=10)
        segs = [np.array(x, dtype=F32) for x in seen[0]]
        assert len(segs) == 5
        thr = _threshold(np.concatenate(segs))
        pipe.pause_shaper(MS, threshold=thr)
        whole = pipe.generate_long_speech(a, segment_tokens=10, max_pause=MS)
        items = list(pipe.stream_long_speech(a, segment_tokens=10, max_pause=MS))
    finally:
        pipe.codec.decode_audio_batch = real
    shaped = [pause_ref.shape(x, M, 160, 5, 80, thr) for x in segs]
    assert sum(k for _, k in shaped) >= 1 and sum(y.size for y, _ in shaped) < sum(x.size for x in segs)
    gaps = [r["pause_ms"] * 16 for r in plain.segments]
    assert any(gaps)
    want, ab = pipe.joiner().join([y for y, _ in shaped], gaps)
    assert np.array_equal(bits(np.asarray(whole)), bits(want))
    assert [r["cut"] for r in whole.segments] == [x.size - y.size for x, (y, _) in zip(segs, shaped)]
    assert [(r["a"], r["b"]) for r in whole.segments] == ab and all("cut" not in r for r in plain.segments)
    # the join's pauses are still there, whole: after each piece, gap_s zeros
    pos = 0
    for (a_, b_), g in zip(ab, gaps):
        pos += b_ - a_
        assert not np.asarray(whole)[pos:pos + g].any()
        pos += g
    assert pos == whole.size
    assert len(items) == 5 and [it.segments[0] for it in items] == whole.segments
    assert np.concatenate(items).tobytes() == np.asarray(whole).tobytes()


def test_both_http_routes_return_the_pipeline_calls_samples(pipe):
    body = {"text": "Hello world, this is RWKV speaking.", "seed": 7, "max_pause": MS}
    err, args, kw = SV._tts_args(body, "assets/raf")
    assert err is None and kw == {"max_pause": MS}
    plain = pipe.generate_speech(args)
    thr = _threshold(plain)
    pipe.pause_shaper(MS, threshold=thr)
    want = _want(plain, thr)
    assert np.array_equal(bits(pipe.generate_speech(args, **kw)), bits(want))
    code, payload = SV.handle_tts_json(body, pipe)
    assert code == 200 and base64.standard_b64decode(payload["audio_base64"]) == SV.convert_samples_to_wav(want, 16000)
    code, it = SV.handle_tts_stream(body, pipe, chunk_frames=8)
    parts = list(it)
    assert code == 200 and parts[0] == SV.streaming_wav_header(16000)
    assert b"".join(parts[1:]) == SV.samples_to_pcm16(want)
