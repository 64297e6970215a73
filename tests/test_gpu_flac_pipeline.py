"""`format: "flac"` through both TTS routes on the GPU: a tiny LM behind the native manager, a tiny
codec, the pipeline's FlacEncoder on the finished PCM. The FLAC of /api/tts decodes to the data bytes
of the WAV the same body gets without `format`, the items of /api/tts/stream concatenate to a file that
decodes to the bytes the PCM stream sends, long-form bodies too, and a watermarked FLAC goes through
the detect route. The decoder (rwkvtts/flac.py) shares no code with the encoder."""
import base64
import os

import numpy as np
import pytest

import rwkvtts
import wm_ref
from rwkvtts import codec as CC
from rwkvtts import flac
from rwkvtts import server as SV
from rwkvtts import weights as W
from rwkvtts.pipeline import LightweightTtsPipeline
from rwkvtts.tokenizer import Tokenizer
from test_tokenizer import VOCAB

pytestmark = pytest.mark.gpu
KEY = 0xC0FFEE0DDBA11
LONG_TEXT = "Hello world, this is RWKV speaking. 今天天气很好。Is it fast?\nA new paragraph starts here. And the last one!"


@pytest.fixture(scope="module")
def pipe():
    blob = W.synth_blob(W.DIMS_TINY, seed=99)
    m = rwkvtts.DynamicBatchManager(blob, devices=[0], max_slots=8, token_chunk_size=128, tokenizer=Tokenizer(VOCAB))
    cd = CC.CODEC_DIMS_TINY
    voc = CC.BiCodecDetokenizer(CC.synth_codec_blob(cd, seed=11), cd)
    p = LightweightTtsPipeline(m, voc, watermark_key=KEY)
    yield p
    m.close()
    voc.close()
    for s in list(p._joiners.values()) + list(p._resamplers.values()) + list(p._levellers.values()):
        s.close()
    for s in (p._marker, p._encoder):
        if s is not None:
            s.close()


def wav_data(payload):
    return base64.standard_b64decode(payload["audio_base64"])[48:]


@pytest.mark.parametrize("extra", [{}, {"loudness": -20}, {"sample_rate": 48000, "tempo": 1.25}],
                         ids=["peak_rule", "loudness", "rate_tempo"])
def test_api_tts_flac_decodes_to_the_wav_routes_data_bytes(pipe, extra):
    body = dict({"text": "Hello world.", "seed": 7}, **extra)
    code, wav = SV.handle_tts_json(body, pipe)
    assert code == 200 and "format" not in wav
    code, out = SV.handle_tts_json(dict(body, format="flac"), pipe)
    assert code == 200 and out["format"] == "flac"
    data = base64.standard_b64decode(out["audio_base64"])
    pcm, rate = flac.decode(data)  # (the CRCs, the sample count and the MD5 hold)
    assert rate == extra.get("sample_rate", 16000) and pcm.size > 1000
    assert pcm.astype("<i2").tobytes() == wav_data(wav)
    print(f"{extra}: {len(data)} bytes of FLAC for {2 * pcm.size} of PCM")


@pytest.mark.parametrize("extra", [{}, {"loudness": -20, "sample_rate": 24000}], ids=["plain", "loudness_rate"])
def test_api_tts_stream_flac_concatenates_to_a_file_of_the_pcm_routes_bytes(pipe, extra):
    body = dict({"text": "Hello world, this is RWKV speaking.", "seed": 12}, **extra)
    code, it = SV.handle_tts_stream(body, pipe, chunk_frames=4)
    want = b"".join(list(it)[1:])
    code, it = SV.handle_tts_stream(dict(body, format="flac"), pipe, chunk_frames=4)
    items = list(it)
    rate = extra.get("sample_rate", 16000)
    assert code == 200 and items[0] == pipe.encoder().header(rate, 1024) and all(len(i) for i in items)
    assert len(items) >= 3  # frames left before the end
    pcm, r = flac.decode(b"".join(items))
    assert r == rate and pcm.astype("<i2").tobytes() == want
    if "loudness" in extra:  # then /api/tts sends the same samples: the same frames
        file = base64.standard_b64decode(SV.handle_tts_json(dict(body, format="flac"), pipe)[1]["audio_base64"])
        assert file[42:] == b"".join(items[1:])


def test_a_long_form_body_in_both_routes(pipe):
    body = {"text": LONG_TEXT, "seed": 21, "long_form": True, "segment_tokens": 10}
    code, wav = SV.handle_tts_json(body, pipe)
    code2, out = SV.handle_tts_json(dict(body, format="flac"), pipe)
    assert code == code2 == 200 and out["format"] == "flac" and out["segments"] == wav["segments"]
    pcm, _ = flac.decode(base64.standard_b64decode(out["audio_base64"]))
    assert pcm.size > 0 and pcm.astype("<i2").tobytes() == wav_data(wav)
    code, it = SV.handle_tts_stream(body, pipe)
    want = b"".join(list(it)[1:])
    code, it = SV.handle_tts_stream(dict(body, format="flac"), pipe)
    pcm, _ = flac.decode(b"".join(it))
    assert code == 200 and pcm.astype("<i2").tobytes() == want


def test_a_watermarked_flac_goes_through_the_detect_route(pipe, tmp_path):
    # a speech-like clip (a tiny synthetic vocoder's PCM is not), marked and encoded by the pipeline's own stages
    clip = pipe.marker(0).embed(wm_ref.vowel(48000, 3), KEY, 0xBEEF)
    data = pipe.encoder().encode(clip, 16000, scale=float(SV.peak_scale(clip)))
    path = os.path.join(tmp_path, "upload.flac")
    with open(path, "wb") as f:
        f.write(data)
    code, out = SV.handle_watermark_detect(path, pipe)
    assert code == 200 and out["detected"] is True and out["payload"] == 0xBEEF and out["seen_bits"] == 0xFFFF
    # and the route's own FLAC with `watermark`: it decodes to the marked WAV's bytes
    body = {"text": "Hello world.", "seed": 7, "watermark": 0x1234}
    wav = SV.handle_tts_json(body, pipe)[1]
    out = SV.handle_tts_json(dict(body, format="flac"), pipe)[1]
    assert flac.decode(base64.standard_b64decode(out["audio_base64"]))[0].astype("<i2").tobytes() == wav_data(wav)
