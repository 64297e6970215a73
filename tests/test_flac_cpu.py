"""FLAC without a GPU: the numpy contract of the encoder (tests/flac_ref.py) through the independent
decoder (rwkvtts/flac.py), hand-assembled frames for what the encoder never emits, hand-worked encoder
cases, FlacStream over the reference, and `format` in the server's handlers with a stand-in pipeline."""
import base64
import json
import os

import numpy as np
import pytest

import flac_ref as R
import wm_ref
from rwkvtts import audio, flac
from rwkvtts import server as SV
from rwkvtts.pipeline import SpeechChunk


# ---- the reference through the decoder -----------------------------------------------------------
@pytest.mark.parametrize("kind", R.KINDS)
def test_the_reference_decodes_to_its_input(kind):
    """Every signal of the GPU test, at every length and both block sizes: sync, both CRCs, the totals
    and the MD5 hold, and the samples are the quantised input."""
    for B in (256, 4096):
        for n in R.lengths(B):
            x = R.signal(kind, n)
            pcm, rate = flac.decode(R.encode(x, R.rate_of(kind), 1.0, B))
            assert rate == R.rate_of(kind) and pcm.dtype == np.int16 and np.array_equal(pcm, R.quantise(x)), (B, n)


def test_the_vowels_pick_lpc_and_noise_comes_out_verbatim():
    for kind in ("vowel16", "vowel48"):
        for B in (256, 4096):
            q = R.quantise(R.signal(kind, 2 * B)).astype(np.int64)
            assert [R.choose(q[i:i + B])[0][0] for i in (0, B)] == ["lpc", "lpc"], (kind, B)
    q = R.quantise(R.signal("noise", 4096)).astype(np.int64)
    assert R.choose(q)[0] == ("verbatim",) and R.choose(q[:256])[0] == ("verbatim",)
    # the widest FIXED residuals: k = 14 somewhere in the clamp signal
    sub = R.choose(R.quantise(R.signal("clamp", 256)).astype(np.int64))[0]
    assert sub[0] == "fixed" and max(sub[-1]) == 14


def test_the_size_properties_of_the_reference():
    x = R.signal("vowel16", 8192)
    assert len(R.encode(x, 16000)) < 2 * x.size                # smaller than PCM on the vowel
    for B in (256, 4096):
        for n in (1, 255, 256, 4095, 2 * B + 37):              # never above the bound, on noise
            frames = R.encode_frames(R.quantise(R.signal("noise", n)), 16000, B)
            assert sum(len(f) for f in frames) <= R.bound(n, B) == audio.FlacEncoder.bound(n, B)
            assert all(len(f) <= 2 * min(B, n - i * B) + 16 for i, f in enumerate(frames))


def test_quantise_is_the_servers_pcm16():
    x = np.concatenate([R.signal("clamp", 3000), R.signal("vowel16", 3000)])
    assert R.quantise(x).astype("<i2").tobytes() == SV.samples_to_pcm16(x)
    assert R.quantise(x, SV.peak_scale(x)).astype("<i2").tobytes() == SV.convert_samples_to_wav(x)[48:]


# ---- hand-assembled frames -----------------------------------------------------------------------
def bits_of(*fields):
    return "".join(format(v & ((1 << n) - 1), f"0{n}b") if n else "" for v, n in fields)


def coded(v):
    """The UTF-8-like coding, up to 36 bits (7 bytes)."""
    if v < 0x80:
        return bytes([v])
    n = next(k for k in range(2, 8) if v < 1 << (5 * k + 1))
    return bytes([((0xFF << (8 - n)) & 0xFF) | (v >> (6 * (n - 1)))] + [0x80 | ((v >> (6 * j)) & 0x3F)
                                                                      for j in range(n - 2, -1, -1)])


def crc(data, poly, width):
    c, top, mask = 0, 1 << (width - 1), (1 << width) - 1
    for b in data:
        c ^= b << (width - 8)
        for _ in range(8):
            c = ((c << 1) ^ poly) & mask if c & top else (c << 1) & mask
    return c


def frame(n, sub, number=0, variable=False, bs_code=None, rate_code=5):
    """A frame of n samples around the subframe's bit string."""
    if bs_code is None:
        bs_code = 6 if n <= 256 else 7
    hdr = bytes([0xFF, 0xF9 if variable else 0xF8, (bs_code << 4) | rate_code, 0x08]) + coded(number)
    hdr += bytes([n - 1]) if bs_code == 6 else (n - 1).to_bytes(2, "big") if bs_code == 7 else b""
    hdr += bytes([crc(hdr, 0x07, 8)])
    sub += "0" * (-len(sub) % 8)
    body = hdr + int(sub, 2).to_bytes(len(sub) // 8, "big")
    return body + crc(body, 0x8005, 16).to_bytes(2, "big")


def stream(frames, rate=16000, B=4096):
    return R.streaminfo(rate, B) + b"".join(frames)


def rice(values, k):
    out = ""
    for v in values:
        zz = (v << 1) ^ (v >> 63)
        out += "0" * (zz >> k) + "1" + (format(zz & ((1 << k) - 1), f"0{k}b") if k else "")
    return out


def test_an_escape_partition_and_the_five_bit_parameters():
    v = [3, -4, 100, -101, 0, 7, -1, 2]
    # FIXED order 0; 4-bit parameters; partition order 1: an escape partition of 8-bit samples, a Rice one
    sub = bits_of((0b0001000, 7), (0, 1), (0, 2), (1, 4), (15, 4), (8, 5)) + bits_of(*[(x, 8) for x in v[:4]])
    sub += bits_of((2, 4)) + rice(v[4:], 2)
    assert flac.decode(stream([frame(8, sub)]))[0].tolist() == v
    # the same with 5-bit parameters (RICE2): k = 17 never fits 4 bits; then its escape code 31 with 0 bits
    big = [30000, -30000, 12345, -1]
    sub = bits_of((0b0001000, 7), (0, 1), (1, 2), (1, 4), (17, 5)) + rice(big[:2], 17) + bits_of((3, 5)) + rice(big[2:], 3)
    assert flac.decode(stream([frame(4, sub)]))[0].tolist() == big
    sub = bits_of((0b0001001, 7), (0, 1), (5, 16), (1, 2), (0, 4), (31, 5), (0, 5))  # FIXED 1, residual all zero
    assert flac.decode(stream([frame(6, sub)]))[0].tolist() == [5] * 6
    # an LPC subframe by hand: order 2, precision 5, shift 2, coefficients (7, -3)
    s = [10, 12]
    res = [1, -2, 0, 3]
    for r in res:
        s.append(r + ((7 * s[-1] - 3 * s[-2]) >> 2))
    sub = bits_of((0b0100001, 7), (0, 1), (10, 16), (12, 16), (4, 4), (2, 5), (7, 5), (-3, 5), (0, 2), (0, 4), (1, 4)) + rice(res, 1)
    assert flac.decode(stream([frame(6, sub)]))[0].tolist() == s
    # wasted bits: a VERBATIM subframe of 14-bit samples shifted up by 2
    sub = bits_of((0b0000001, 7), (1, 1), (0b01, 2)) + bits_of(*[(x, 14) for x in (5, -6, 7)])
    assert flac.decode(stream([frame(3, sub)]))[0].tolist() == [20, -24, 28]


def test_explicit_block_sizes_and_every_coded_number_length():
    const = lambda v: bits_of((0, 8), (v, 16))
    frames = [frame(300, const(-7), number=0)]                       # 16-bit explicit block size
    frames += [frame(256, const(i), number=v) for i, v in enumerate((0x7F, 0x80, 0x7FF, 0x800, 0xFFFF, 0x10000, 0x1FFFFF,
                                                                     0x200000, 0x3FFFFFF, 0x4000000, 0x7FFFFFFF))]
    frames += [frame(16, const(99), number=(1 << 36) - 1, variable=True)]   # 7 bytes: a sample number
    frames += [frame(192, const(1), bs_code=1), frame(1152, const(2), bs_code=3), frame(512, const(3), bs_code=9)]
    pcm, rate = flac.decode(stream(frames))
    want = [-7] * 300 + sum(([i] * 256 for i in range(11)), []) + [99] * 16 + [1] * 192 + [2] * 1152 + [3] * 512
    assert rate == 16000 and pcm.tolist() == want


def test_what_the_decoder_refuses():
    good = frame(4, bits_of((0, 8), (1, 16)))
    assert flac.decode(stream([good]))[0].tolist() == [1] * 4
    for i in range(len(good)):  # any corrupted byte fails the sync, a reserved code or a CRC
        bad = bytearray(good)
        bad[i] ^= 0x10
        with pytest.raises(ValueError):
            flac.decode(stream([bytes(bad)]))
    with pytest.raises(ValueError, match="fLaC"):
        flac.decode(b"RIFF" + good)
    with pytest.raises(ValueError, match="mono 16-bit"):
        info = bytearray(R.streaminfo(16000, 4096))
        info[20] |= 0x02  # two channels
        flac.decode(bytes(info) + good)
    with pytest.raises(ValueError, match="truncated"):
        flac.decode(stream([good])[:-3])
    with pytest.raises(ValueError, match="MD5"):
        flac.decode(R.streaminfo(16000, 4096, md5=b"\1" * 16) + good)
    with pytest.raises(ValueError, match="promises"):
        flac.decode(R.streaminfo(16000, 4096, total=5) + good)
    with pytest.raises(ValueError, match="reserved subframe"):
        flac.decode(stream([frame(4, bits_of((0b0000100, 7), (0, 1), (1, 16)))]))


# ---- hand-worked encoder cases -------------------------------------------------------------------
def test_a_ramp_is_fixed_order_2_with_an_all_zero_residual():
    q = (3 * np.arange(256) - 100).astype(np.int16)
    sub, nbits = R.choose(q.astype(np.int64))
    assert sub[:2] == ("fixed", 2) and not sub[2].any() and sub[3] == 0 and sub[4].tolist() == [0]
    assert nbits == 8 + 32 + 6 + 4 + 254
    want = frame(256, bits_of((0b0001010, 7), (0, 1), (-100, 16), (-97, 16), (0, 2), (0, 4), (0, 4)) + "1" * 254,
                 number=9, bs_code=8)
    assert R.encode_frame(q, 9, 16000, 256) == want
    assert R.encode_frame(R.quantise(R.signal("ramp", 256)), 0, 16000, 256)[6] == 0x14  # the GPU test's ramp too


def test_silence_is_constant_and_a_corrupted_byte_fails_a_crc():
    data = R.encode(np.zeros(300, dtype=np.float32), 24000, block=256)
    f0 = frame(256, bits_of((0, 8), (0, 16)), number=0, bs_code=8, rate_code=7)
    f1 = frame(44, bits_of((0, 8), (0, 16)), number=1, rate_code=7)
    assert data[42:] == f0 + f1 and len(f0) == 11
    assert flac.decode(data)[0].tolist() == [0] * 300
    bad = bytearray(data)
    bad[42 + 7] ^= 1  # the constant's value: the header CRC-8 holds, the frame's CRC-16 does not
    with pytest.raises(ValueError, match="CRC-16"):
        flac.decode(bytes(bad))
    bad = bytearray(data)
    bad[42 + 4] ^= 1  # the frame number
    with pytest.raises(ValueError, match="CRC-8"):
        flac.decode(bytes(bad))


def test_the_stream_header_of_the_library_is_the_references():
    md5 = bytes(range(16))
    assert audio.FlacEncoder.header(44100, 2048, 14, 4100, 123456789, md5) == R.streaminfo(44100, 2048, 14, 4100, 123456789, md5)
    assert audio.FlacEncoder.header(8000, 256) == R.streaminfo(8000, 256)
    assert [audio.flac_default_block(r) for r in audio.FLAC_RATES] == [1024] * 4 + [2048] * 3
    assert np.array_equal(audio._flac_table(), R.table())


# ---- FlacStream over the reference ---------------------------------------------------------------
def test_flacstream_gives_the_same_frames_in_any_chunking():
    enc = audio.FlacEncoder(evaluator=R.evaluator)
    x = np.tile(R.signal("vowel16", 2000), 3)[:5120 + 3 * 256 + 37]
    whole = enc.encode(x, 16000, block=256)
    assert whole == R.encode(x, 16000, 1.0, 256)
    for chunk in (1, 160, 5120, x.size):
        s = audio.FlacStream(enc, 16000, 256)
        parts = [s.feed(x[i:i + chunk], final=i + chunk >= x.size) for i in range(0, x.size, chunk)]
        assert parts[0][:42] == R.streaminfo(16000, 256)  # unknown totals
        assert b"".join(parts)[42:] == whole[42:], chunk
        assert np.array_equal(flac.decode(b"".join(parts))[0], R.quantise(x))
        with pytest.raises(ValueError):
            s.feed(x[:1])
    with pytest.raises(_ffi_error()):
        enc.encode_windows([(x[:100], 1.0, 16000, 256, 0, False, True)])  # misaligned and not the last


def _ffi_error():
    from rwkvtts import _ffi
    return _ffi.RwkvTtsError


# ---- the server's handlers with a stand-in pipeline ----------------------------------------------
KEY = 0xABCDEF0123456789


class FakePipeline:
    def __init__(self, pcm, key=KEY):
        self.pcm, self.calls, self.watermark_key = np.asarray(pcm, dtype=np.float32), [], key
        self.marker = audio.Watermarker(evaluator=wm_ref.evaluator, detector=wm_ref.detector)
        self._encoder = audio.FlacEncoder(evaluator=R.evaluator)

    def encoder(self):
        return self._encoder

    def _pcm(self, kw):
        x = self.pcm.copy() if kw.get("watermark") is None else self.marker.embed(self.pcm, self.watermark_key, kw["watermark"])
        return x * np.float32(0.5) if "loudness" in kw else x

    def generate_speech(self, args, **kw):
        self.calls.append(("generate_speech", kw))
        return self._pcm(kw)

    def stream_speech(self, args, chunk_frames=16, **kw):
        self.calls.append(("stream_speech", kw))
        parts = np.array_split(self._pcm(kw), 7)
        yield SpeechChunk.make(np.zeros(0, dtype=np.float32), 0, 0, 0, False)
        for i, c in enumerate(parts):
            yield SpeechChunk.make(c, 0, 0, 0, i == len(parts) - 1)

    def detect_watermark(self, pcm):
        return self.marker.detect(pcm, self.watermark_key)


@pytest.mark.parametrize("bad", [True, 1, "mp3", "FLAC", "", ["flac"], {"type": "flac"}, 1.5])
def test_a_bad_format_is_a_400_and_the_pipeline_is_not_called(bad):
    p = FakePipeline(np.zeros(100))
    body = json.dumps({"text": "hello", "format": bad})
    code, payload = SV.handle_tts_json(body, p)
    assert code == 400 and payload["success"] is False and isinstance(payload["error"], str)
    code2, it = SV.handle_tts_stream(body, p)
    assert code2 == 400 and json.loads(b"".join(it).decode("utf-8")) == payload
    assert p.calls == []


def test_without_format_the_bodies_are_todays():
    x = R.signal("vowel16", 3000)
    p = FakePipeline(x)
    for body in ({"text": "x"}, {"text": "x", "format": None}, {"text": "x", "format": "wav"}):
        code, out = SV.handle_tts_json(body, p)
        assert code == 200 and set(out) == {"success", "message", "audio_base64", "duration_ms", "rtf"}
        assert base64.standard_b64decode(out["audio_base64"]) == SV.convert_samples_to_wav(x, 16000)
        code, it = SV.handle_tts_stream(body, p)
        items = list(it)
        assert code == 200 and items[0] == SV.streaming_wav_header(16000) and b"".join(items[1:]) == SV.samples_to_pcm16(x)
        assert SV.tts_stream_media_type(json.dumps(body)) == "audio/wav"
    assert p.calls == [("generate_speech", {}), ("stream_speech", {})] * 3  # `format` never reaches the pipeline


@pytest.mark.parametrize("extra", [{}, {"loudness": -20}, {"sample_rate": 48000}])
def test_flac_of_api_tts_decodes_to_the_wav_routes_data_bytes(extra):
    x = R.signal("vowel16", 5000) * np.float32(1.7)  # (past 1.0: the peak rule scales down)
    p = FakePipeline(x)
    body = dict({"text": "x"}, **extra)
    wav = base64.standard_b64decode(SV.handle_tts_json(body, p)[1]["audio_base64"])
    code, out = SV.handle_tts_json(dict(body, format="flac"), p)
    assert code == 200 and out["format"] == "flac" and out["success"] is True
    data = base64.standard_b64decode(out["audio_base64"])
    pcm, rate = flac.decode(data)
    assert rate == extra.get("sample_rate", 16000) and pcm.astype("<i2").tobytes() == wav[48:]
    assert len(data) < len(wav)
    assert [c[1] for c in p.calls] == [{k: float(v) if k == "loudness" else v for k, v in extra.items()}] * 2


def test_the_flac_stream_sends_the_header_first_then_frames():
    x = R.signal("vowel16", 5000)
    p = FakePipeline(x)
    body = {"text": "x", "format": "flac"}
    code, it = SV.handle_tts_stream(body, p)
    items = list(it)
    assert code == 200 and SV.tts_stream_media_type(json.dumps(body)) == "audio/flac"
    assert items[0] == R.streaminfo(16000, 1024) and all(len(i) for i in items)
    assert items[1][:2] == b"\xff\xf8" and b"".join(items)[42:] == R.encode(x, 16000)[42:]
    pcm, rate = flac.decode(b"".join(items))
    assert rate == 16000 and pcm.astype("<i2").tobytes() == SV.samples_to_pcm16(x)
    assert p.calls == [("stream_speech", {})]


def test_the_detect_route_takes_a_flac_upload(tmp_path):
    p = FakePipeline(wm_ref.vowel(3 * 16000, 5, peak=0.4))
    code, out = SV.handle_tts_json({"text": "hello", "watermark": 0xC0DE, "format": "flac"}, p)
    assert code == 200
    path = os.path.join(tmp_path, "marked.wav")  # (whatever the name says: the content decides)
    with open(path, "wb") as f:
        f.write(base64.standard_b64decode(out["audio_base64"]))
    code, out = SV.handle_watermark_detect(path, p)
    assert code == 200 and out["detected"] is True and out["payload"] == 0xC0DE and abs(out["seconds"] - 3.0) < 0.05
    with open(path, "wb") as f:
        f.write(b"fLaC but not a stream")
    code, out = SV.handle_watermark_detect(path, p)
    assert code == 400 and out["success"] is False


def test_the_routes_are_wired():
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient
    x = R.signal("vowel16", 3000)
    c = TestClient(SV.create_app(FakePipeline(x)))
    r = c.post("/api/tts/stream", json={"text": "hello", "format": "flac"})
    assert r.status_code == 200 and r.headers["content-type"] == "audio/flac"
    assert flac.decode(r.content)[0].astype("<i2").tobytes() == SV.samples_to_pcm16(x)
    r = c.post("/api/tts/stream", json={"text": "hello"})
    assert r.status_code == 200 and r.headers["content-type"] == "audio/wav" and r.content[44:] == SV.samples_to_pcm16(x)
    r = c.post("/api/tts", json={"text": "hello", "format": "ogg"})
    assert r.status_code == 400 and r.json()["success"] is False
    upload = base64.standard_b64decode(c.post("/api/tts", json={"text": "hello", "format": "flac"}).json()["audio_base64"])
    r = c.post("/api/watermark/detect", content=upload, headers={"content-type": "audio/flac"})
    assert r.status_code == 200 and r.json()["detected"] is False  # (read, and nothing marked it)
