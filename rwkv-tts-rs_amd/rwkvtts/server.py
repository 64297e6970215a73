"""The reference's HTTP API surface for the TTS path (bin/server.rs), over LightweightTtsPipeline.

* `convert_samples_to_wav` (:98-148): peak rule (max|x| > 1 -> 1/max, else min(0.8/max, 10),
  silence -> 1), f32 arithmetic, clamp to [-1, 1], x 32767 truncated to i16, 16 kHz mono WAV.
  The reference writes the data-chunk size as a usize (8 little-endian bytes on 64-bit) and
  declares RIFF size 36 + 2n; both are reproduced so the bytes match.
* `calculate_rtf` (:151-159), the speed / pitch string mapping of `handle_tts_json` (:528-584,
  including SURVEY B4: the pitch is remapped to names PITCH_MAP does not contain, so the pitch
  token is always 7), the voice lookup by voice_id (:481-515, a RAF JSON under `voice_dir`).
* `handle_tts_json(body, pipeline, voice_dir)` returns (HTTP status, JSON dict) exactly as the
  handler renders them; `create_app` wires it to POST /api/tts with FastAPI when installed.
* The voice-clone routes (:777-979, routes :1448-1450) over the RAF store (`voices.py`,
  VoiceFeatureManager): `handle_voice_list`, `handle_voice_delete`, `handle_voice_extract`
  (multipart voice_name / prompt_text / audio_file; the feature extraction needs the
  BiCodecTokenize + wav2vec2 encoders, whose graphs are absent: a pipeline may supply
  `reference_tokenizer`, otherwise the route answers the reference's extraction-failure body).
* `sample_rate` in the body of both TTS routes (no reference counterpart: the reference emits
  16 kHz only): one of SAMPLE_RATES, anything else a 400; the PCM is resampled on the GPU
  (audio.Resampler) and the WAV header carries the rate. Without the field the routes are unchanged.
* `tempo` in the body of both TTS routes (no reference counterpart): a JSON number in
  [TEMPO_MIN, TEMPO_MAX] = [0.5, 2.0], anything else a 400; above 1 is faster speech. It is not
  `speed`: `speed` keeps the reference's meaning, the model's five-bucket property token, which
  changes how the model speaks and which a request with a `voice_id` does not get at all
  (pipeline.generate_property_tokens returns no property tokens for a cloned voice); `tempo` is a
  continuous rate applied to the finished 16 kHz PCM by a pitch-preserving time stretch on the GPU
  (audio.TimeStretcher), before any resampling, and works for every voice. Without the field (or
  with 1.0) the routes are unchanged.
* `global_sampling` / `semantic_sampling` in the body of both TTS routes (no reference
  counterpart): each an object with any of `temperature` (0.1 .. 4.0), `top_p` (0 .. 1) and `top_k`
  (an integer >= 0, 0: no top-k) for that phase of the token generator (runtime.PhaseSampling; a
  key left out keeps the phase's own 1.0 / 0.95 / 20 global, 80 semantic); anything else a 400. The
  top-level `temperature` and `top_p` keep doing nothing, as in the reference, which parses them
  and then samples with fixed values (normal_mode_inference.rs:114-127).
* `penalties` in the body of both TTS routes (the reference's sampler_manager.rs has the three
  penalties, its TTS path never calls them): an object with any of `repetition` (0.25 .. 4.0),
  `frequency` (-8 .. 8), `presence` (-8 .. 8) and `window` (an integer 0 .. 2048, 0: the whole
  history) over the request's own semantic tokens (runtime.Penalties; a key left out keeps its
  neutral 1 / 0 / 0 / 0); anything else a 400. With `long_form` every segment gets the same
  penalties over its own history. Without the key the routes are unchanged.
* `mirostat` in the body of both TTS routes (the reference's ai00 server has the sampler, its TTS
  path never calls it): an object with any of `tau` (0.5 .. 10, default 3.0) and `rate`
  (0.001 .. 1, default 0.1) (runtime.Mirostat); it replaces the semantic phase's top-k, top-p and
  temperature, so together with `semantic_sampling` it is a 400, as is anything else. With
  `long_form` every segment gets the same values and a threshold of its own. Without the key the
  routes are unchanged.
* `long_form`, `segment_tokens` and `voice_tokens` in the body of both TTS routes (no reference
  counterpart: a request of the reference ends at 2048 semantic tokens, 41 s of audio, without an
  error). `long_form`: a JSON bool; true routes the request to pipeline.generate_long_speech /
  stream_long_speech, which cut the text into segments, synthesise them side by side with one voice
  and join them. `segment_tokens`: an integer in [SEGMENT_TOKENS_MIN, SEGMENT_TOKENS_MAX] =
  [8, 256], the segmenter's budget; it needs `long_form`. `voice_tokens`: 32 integers in [0, 4096),
  the global tokens of a voice heard before (a `long_form` response returns them): the request
  speaks with that voice and keeps its property tokens (pin_voice), with or without `long_form`; it
  excludes `voice_id`. Anything else is a 400. A `long_form` JSON response adds `voice_tokens` and
  `segments` (text, status, n_semantic, truncated, pause_ms, a, b per segment). Without the keys the
  routes are unchanged.
* `loudness` in the body of both TTS routes (no reference counterpart: the reference peak-normalises
  the finished WAV to 0.8, which sets no loudness and which a stream cannot do): a JSON number in
  [LOUDNESS_MIN, LOUDNESS_MAX] = [-40, -10] dB, anything else a 400. The 16 kHz PCM is levelled on the
  GPU to that K-weighted loudness under a peak ceiling (audio.Leveller), after the stretch and before
  the resampler. /api/tts then writes its WAV at scale 1.0 (`levelled_samples_to_wav`: no peak rule,
  which would undo the target), so its samples are byte for byte the PCM /api/tts/stream sends for
  the same body and seed. Without the field the routes are unchanged.
* `pitch_shift` in the body of both TTS routes (no reference counterpart): a JSON number in
  [PITCH_SHIFT_MIN, PITCH_SHIFT_MAX] = [-12, 12] semitones, anything else a 400; above 0 is a higher
  voice. It is not `pitch`: `pitch` keeps the reference's meaning, the model's five-class property
  token, which a request with a `voice_id` does not get at all; `pitch_shift` is a continuous shift
  of the finished 16 kHz PCM's fundamental on the GPU that keeps the spectral envelope and the
  length (audio.PitchShifter), before the stretch, and works for every voice. Without the field (or
  with 0) the routes are unchanged.
* `watermark` in the body of both TTS routes (no reference counterpart: the reference marks nothing):
  a JSON integer in [WATERMARK_MIN, WATERMARK_MAX] = [0, 65535], anything else a 400, and a 400 too on
  a server whose pipeline has no `watermark_key`. The payload is embedded in the 16 kHz PCM under the
  pipeline's key as a spread-spectrum mark (audio.Watermarker), after the leveller and before the
  resampler. Without the field the routes are unchanged.
* `max_pause` in the body of both TTS routes (no reference counterpart: the reference sends whatever
  silence the semantic model chose): a JSON integer in [MAX_PAUSE_MIN, MAX_PAUSE_MAX] = [20, 5000]
  milliseconds, anything else a 400. No silence inside the audio is longer than it and none at either
  end longer than half of it (audio.PauseShaper), capped on the 16 kHz PCM on the GPU before every
  other stage; with `long_form` per segment, before the join, whose own pauses stay. On the stream
  route a request that is all leading silence so far sends nothing yet. Without the field the routes
  are unchanged.
* `handle_watermark_detect(path, pipeline)`, POST /api/watermark/detect (no reference counterpart): an
  uploaded WAV at any supported rate, brought to 16 kHz by `load_audio(..., device=)` without volume
  normalisation, read back under the pipeline's key -> {detected, score, threshold, payload,
  seen_bits, offset, seconds}.
* `handle_tts_stream(body, pipeline, voice_dir)` (no reference counterpart): the same request as a
  WAV stream, POST /api/tts/stream -- audio while the request is still decoding, at a fixed scale
  (no peak normalisation: that needs the whole utterance).
* `format` in the body of both TTS routes (no reference counterpart: the reference sends WAV only):
  "wav" (the default; the field absent is the same) or "flac", anything else a 400. With "flac" the
  same int16 samples go out losslessly compressed by the GPU's FLAC encoder (audio.FlacEncoder):
  /api/tts puts the FLAC file into `audio_base64` and adds `"format": "flac"` to the response, at the
  peak rule's scale (1.0 with `loudness`), so rwkvtts.flac.decode of it gives the WAV's data bytes;
  /api/tts/stream answers audio/flac -- the stream header (STREAMINFO with unknown totals), then frames
  as blocks complete (1024 samples up to 24 kHz, 2048 above), the short last block at the end.
  /api/watermark/detect takes a FLAC upload too (load_audio reads it through rwkvtts.flac.decode).
  Without the field the routes are unchanged.
The embedded web UI and model download are out of scope.
"""
import base64
import json
import os
import time
from typing import Optional, Tuple

import numpy as np

from .pipeline import LightweightTtsPipelineArgs
from .runtime import Mirostat, Penalties, PhaseSampling


def peak_scale(samples) -> np.float32:
    """The peak rule of convert_samples_to_wav (:98-148): max|x| > 1 -> 1 / max, else min(0.8 / max, 10);
    silence -> 1. f32."""
    x = np.asarray(samples, dtype=np.float32)
    max_abs = np.float32(np.max(np.abs(x))) if x.size else np.float32(0.0)
    if max_abs > 0.0:
        scale = np.float32(1.0) / max_abs if max_abs > 1.0 else min(np.float32(0.8) / max_abs, np.float32(10.0))
    else:
        scale = np.float32(1.0)
    return np.float32(scale)


def convert_samples_to_wav(samples, sample_rate: int = 16000) -> bytes:
    x = np.asarray(samples, dtype=np.float32)
    scale = peak_scale(x)
    y = np.clip(x * scale, np.float32(-1.0), np.float32(1.0)) * np.float32(32767.0)
    pcm = np.trunc(y).astype("<i2")  # Rust `as i16`: truncation toward zero
    return _wav_header(x.size, sample_rate) + pcm.tobytes()


def _wav_header(n: int, sample_rate: int) -> bytes:
    hdr = b"RIFF" + int(36 + n * 2).to_bytes(4, "little", signed=False) + b"WAVE"
    hdr += b"fmt " + (16).to_bytes(4, "little") + (1).to_bytes(2, "little") + (1).to_bytes(2, "little")
    hdr += int(sample_rate).to_bytes(4, "little") + int(sample_rate * 2).to_bytes(4, "little")
    hdr += (2).to_bytes(2, "little") + (16).to_bytes(2, "little")
    return hdr + b"data" + int(n * 2).to_bytes(8, "little")  # (samples.len() * 2).to_le_bytes(): usize


def levelled_samples_to_wav(samples, sample_rate: int = 16000) -> bytes:
    """convert_samples_to_wav's header over samples_to_pcm16: scale 1.0, no peak rule. For PCM that
    the leveller has already set to a loudness under its own peak ceiling: the peak rule would undo
    the target. The data bytes are what /api/tts/stream sends for the same body and seed."""
    x = np.asarray(samples, dtype=np.float32)
    return _wav_header(x.size, sample_rate) + samples_to_pcm16(x)


def calculate_rtf(audio, processing_seconds: float, sample_rate: int = 16000) -> float:
    dur = len(audio) / float(sample_rate)
    return processing_seconds / dur if dur > 0 else 0.0


# `sample_rate` of the /api/tts and /api/tts/stream bodies (no reference counterpart: the reference
# emits 16 kHz only): telephony, the vocoder's own rate, and what browsers / Opus / audio tools take
SAMPLE_RATES = (8000, 16000, 22050, 24000, 32000, 44100, 48000)
# `tempo` of the same bodies (no reference counterpart): the range in which the time stretch still
# sounds like speech; the kernel itself takes 0.25 .. 4.0
TEMPO_MIN, TEMPO_MAX = 0.5, 2.0
# `segment_tokens` of the same bodies (no reference counterpart): text tokens per segment of a
# `long_form` request; the default, 64, is pipeline.generate_long_speech's
SEGMENT_TOKENS_MIN, SEGMENT_TOKENS_MAX = 8, 256
# `loudness` of the same bodies (no reference counterpart): the leveller's target in dB (LUFS-like:
# K-weighted, -23 broadcast, -16 streaming); the pipeline's range
LOUDNESS_MIN, LOUDNESS_MAX = -40.0, -10.0
# `pitch_shift` of the same bodies (no reference counterpart): semitones, an octave either way -- the
# kernel's own range
PITCH_SHIFT_MIN, PITCH_SHIFT_MAX = -12.0, 12.0
# `format` of the same bodies (no reference counterpart): the container of the audio that goes out
FORMATS = ("wav", "flac")
# `watermark` of the same bodies (no reference counterpart): the payload of the provenance mark, 16
# bits at the marker's defaults -- a tenant or deployment number, not a secret (the key is the secret)
WATERMARK_MIN, WATERMARK_MAX = 0, 65535
# `max_pause` of the same bodies (no reference counterpart): the longest silence inside the result, in
# milliseconds (half of it at either end) -- the pipeline's range
MAX_PAUSE_MIN, MAX_PAUSE_MAX = 20, 5000


def map_speed(speed) -> str:
    """:528-554: a known speed string passes through, other strings -> medium; numbers are
    bucketed (<=3.4 very_slow, <=4.0 slow, <=4.5 medium, <=4.8 fast, else very_fast); absent or
    unparsable -> medium (a non-number non-string parses as 4.2 -> medium)."""
    if speed is None:
        return "medium"
    if isinstance(speed, str):
        return speed if speed in ("very_slow", "slow", "medium", "fast", "very_fast") else "medium"
    try:
        v = float(np.float32(speed)) if isinstance(speed, (int, float)) and not isinstance(speed, bool) else 4.2
    except (TypeError, ValueError):
        v = 4.2
    if v <= float(np.float32(3.4)):
        return "very_slow"
    if v <= 4.0:
        return "slow"
    if v <= 4.5:
        return "medium"
    if v <= float(np.float32(4.8)):
        return "fast"
    return "very_fast"


def map_pitch(pitch: Optional[str]) -> str:
    """:570-576 (these names miss PITCH_MAP, so the pitch token is always 7)."""
    return {"low_pitch": "low", "medium_pitch": "medium", "high_pitch": "high",
            "very_high_pitch": "very_high"}.get(pitch, "medium")


_MANAGERS = {}


def voice_manager(voice_dir: str):
    """One VoiceFeatureManager per RAF directory (the server's AppState.voice_manager)."""
    from .voices import VoiceFeatureManager
    m = _MANAGERS.get(voice_dir)
    if m is None:
        m = _MANAGERS[voice_dir] = VoiceFeatureManager(voice_dir)
    return m


def load_voice_feature(voice_dir: str, voice_id: str) -> dict:
    """VoiceFeatureManager::load_voice_feature (checksum verified, cached)."""
    vf = voice_manager(voice_dir).load_voice_feature(voice_id)
    return dict(vf.__dict__)


def _tts_args(body, voice_dir: str):
    """The request body of /api/tts -> (None, LightweightTtsPipelineArgs, keywords), or
    ((status, payload), None, None) for a body the handler refuses. keywords: what the pipeline call
    takes beyond the args, each only when the body sets it to something other than its default --
    sample_rate (one of SAMPLE_RATES, not 16000), tempo (TEMPO_MIN .. TEMPO_MAX, not 1.0), loudness
    (LOUDNESS_MIN .. LOUDNESS_MAX; there is no default value that means "off" but its absence) and
    pitch_shift (PITCH_SHIFT_MIN .. PITCH_SHIFT_MAX, not 0), and max_pause (an integer MAX_PAUSE_MIN ..
    MAX_PAUSE_MAX ms; absent is off) -- so a
    body without them makes exactly the call it always made. A true `long_form` adds
    long_form=True, which the handler takes out and answers by calling the long-form entry point,
    and segment_tokens when the body sets it."""
    if isinstance(body, (bytes, str)):
        try:
            body = json.loads(body)
        except ValueError as e:
            return (400, {"success": False, "error": f"JSON解析失败: {e}"}), None, None
    if not isinstance(body, dict) or not isinstance(body.get("text"), str):
        return (400, {"success": False, "error": "JSON解析失败: missing field `text`"}), None, None
    rate = body.get("sample_rate")
    if rate is None:
        rate = 16000
    elif isinstance(rate, bool) or not isinstance(rate, int) or rate not in SAMPLE_RATES:
        return (400, {"success": False, "error": f"不支持的采样率: {rate} (支持: "
                                                 f"{', '.join(str(r) for r in SAMPLE_RATES)})"}), None, None
    tempo = body.get("tempo")
    if tempo is None:
        tempo = 1.0
    elif (isinstance(tempo, bool) or not isinstance(tempo, (int, float))
          or not TEMPO_MIN <= tempo <= TEMPO_MAX):  # (NaN fails the comparison)
        return (400, {"success": False, "error": f"不支持的语速倍率: {tempo} (支持: "
                                                 f"{TEMPO_MIN} - {TEMPO_MAX})"}), None, None
    loudness = body.get("loudness")
    if loudness is not None and (isinstance(loudness, bool) or not isinstance(loudness, (int, float))
                                 or not LOUDNESS_MIN <= loudness <= LOUDNESS_MAX):  # (NaN fails the comparison)
        return (400, {"success": False, "error": f"不支持的响度目标: {loudness} (支持: "
                                                 f"{LOUDNESS_MIN} - {LOUDNESS_MAX} dB)"}), None, None
    shift = body.get("pitch_shift")
    if shift is None:
        shift = 0.0
    elif (isinstance(shift, bool) or not isinstance(shift, (int, float))
          or not PITCH_SHIFT_MIN <= shift <= PITCH_SHIFT_MAX):  # (NaN fails the comparison)
        return (400, {"success": False, "error": f"不支持的音高偏移: {shift} (支持: "
                                                 f"{PITCH_SHIFT_MIN} - {PITCH_SHIFT_MAX} 半音)"}), None, None
    mark = body.get("watermark")
    if mark is not None and (isinstance(mark, bool) or not isinstance(mark, int)
                             or not WATERMARK_MIN <= mark <= WATERMARK_MAX):
        return (400, {"success": False, "error": f"不支持的水印载荷: {mark} (支持: "
                                                 f"{WATERMARK_MIN} - {WATERMARK_MAX} 的整数)"}), None, None
    max_pause = body.get("max_pause")
    if max_pause is not None and (isinstance(max_pause, bool) or not isinstance(max_pause, int)
                                  or not MAX_PAUSE_MIN <= max_pause <= MAX_PAUSE_MAX):
        return (400, {"success": False, "error": f"不支持的最大停顿: {max_pause} (支持: "
                                                 f"{MAX_PAUSE_MIN} - {MAX_PAUSE_MAX} 毫秒的整数)"}), None, None
    fmt = body.get("format")
    if fmt is None:
        fmt = "wav"
    elif not isinstance(fmt, str) or fmt not in FORMATS:
        return (400, {"success": False, "error": f"不支持的输出格式: {fmt} (支持: {', '.join(FORMATS)})"}), None, None
    sampling = {}
    for what in ("global_sampling", "semantic_sampling"):
        o = body.get(what)
        if o is None:
            continue
        try:
            if not isinstance(o, dict) or set(o) - {"temperature", "top_p", "top_k"}:
                raise ValueError(f"{what}: an object with any of temperature, top_p, top_k")
            sampling[what] = PhaseSampling(**{k: v for k, v in o.items() if v is not None}).check(what)
        except ValueError as e:
            return (400, {"success": False, "error": f"不支持的采样参数: {e}"}), None, None
    pen = body.get("penalties")
    if pen is not None:
        try:
            if not isinstance(pen, dict) or set(pen) - {"repetition", "frequency", "presence", "window"}:
                raise ValueError("penalties: an object with any of repetition, frequency, presence, window")
            sampling["penalties"] = Penalties(**{k: v for k, v in pen.items() if v is not None}).check()
        except ValueError as e:
            return (400, {"success": False, "error": f"不支持的惩罚参数: {e}"}), None, None
    miro = body.get("mirostat")
    if miro is not None:
        try:
            if not isinstance(miro, dict) or set(miro) - {"tau", "rate"}:
                raise ValueError("mirostat: an object with any of tau, rate")
            if "semantic_sampling" in sampling:
                raise ValueError("mirostat replaces the semantic phase's top-k, top-p and temperature: "
                                 "semantic_sampling excludes it")
            sampling["mirostat"] = Mirostat(**{k: v for k, v in miro.items() if v is not None}).check()
        except ValueError as e:
            return (400, {"success": False, "error": f"不支持的 Mirostat 参数: {e}"}), None, None
    long_form = body.get("long_form")
    if long_form is not None and not isinstance(long_form, bool):
        return (400, {"success": False, "error": f"不支持的长文本开关: {long_form} (支持: true, false)"}), None, None
    seg_tokens = body.get("segment_tokens")
    if seg_tokens is not None:
        if (isinstance(seg_tokens, bool) or not isinstance(seg_tokens, int)
                or not SEGMENT_TOKENS_MIN <= seg_tokens <= SEGMENT_TOKENS_MAX):
            return (400, {"success": False, "error": f"不支持的分段长度: {seg_tokens} (支持: "
                                                     f"{SEGMENT_TOKENS_MIN} - {SEGMENT_TOKENS_MAX})"}), None, None
        if not long_form:
            return (400, {"success": False, "error": "segment_tokens 需要 long_form 为 true"}), None, None
    voice_tokens = body.get("voice_tokens")
    if voice_tokens is not None:
        if (not isinstance(voice_tokens, list) or len(voice_tokens) != 32
                or any(isinstance(x, bool) or not isinstance(x, int) or not 0 <= x < 4096 for x in voice_tokens)):
            return (400, {"success": False, "error": "不支持的音色标记: voice_tokens 需要 32 个 [0, 4096) 内的整数"}), None, None
        if body.get("voice_id"):
            return (400, {"success": False, "error": "voice_tokens 与 voice_id 不能同时使用"}), None, None
    voice_id = body.get("voice_id")
    voice = None
    prompt_from_voice = None
    if voice_id:  # a non-empty voice_id loads the stored voice feature
        try:
            voice = load_voice_feature(voice_dir, voice_id)
            prompt_from_voice = voice.get("prompt_text", "")
        except (OSError, ValueError) as e:
            return (400, {"success": False, "error": f"音色ID '{voice_id}' 不存在或加载失败: {e}"}), None, None
    prompt_text = prompt_from_voice if prompt_from_voice is not None else (body.get("prompt_text") or "")
    args = LightweightTtsPipelineArgs(
        text=body["text"], ref_audio_path="", zero_shot=voice_id is not None,
        temperature=float(body.get("temperature") if body.get("temperature") is not None else 1.0),
        top_p=float(body.get("top_p") if body.get("top_p") is not None else 0.90),
        top_k=100, max_tokens=8000, seed=body.get("seed"),
        age=body.get("age") or "youth-adult", gender=body.get("gender") or "male",
        emotion=body.get("emotion") or "NEUTRAL", pitch=map_pitch(body.get("pitch")),
        speed=map_speed(body.get("speed")), prompt_text=prompt_text,
        voice_global_tokens=list(voice["global_tokens"]) if voice else voice_tokens,
        voice_semantic_tokens=list(voice["semantic_tokens"]) if voice else None,
        pin_voice=voice_tokens is not None, **sampling)
    kw = {}
    if long_form:
        kw["long_form"] = True
        if seg_tokens is not None:
            kw["segment_tokens"] = seg_tokens
    if rate != 16000:
        kw["sample_rate"] = rate
    if float(tempo) != 1.0:
        kw["tempo"] = float(tempo)
    if loudness is not None:
        kw["loudness"] = float(loudness)
    if float(shift) != 0.0:
        kw["pitch_shift"] = float(shift)
    if mark is not None:
        kw["watermark"] = int(mark)
    if max_pause is not None:
        kw["max_pause"] = int(max_pause)
    if fmt != "wav":
        kw["format"] = fmt  # (the handler's, not the pipeline's: taken out before the call, as long_form is)
    return None, args, kw


def _no_key(kw, pipeline):
    """The 400 of a `watermark` sent to a server whose pipeline has no key, else None."""
    if "watermark" in kw and getattr(pipeline, "watermark_key", None) is None:
        return 400, {"success": False, "error": "服务器未配置水印密钥 (watermark_key)，无法使用 watermark"}
    return None


def handle_tts_json(body, pipeline, voice_dir: str = "assets/raf") -> Tuple[int, dict]:
    t0 = time.perf_counter()
    err, args, kw = _tts_args(body, voice_dir)
    err = err or _no_key(kw, pipeline)
    if err:
        return err
    rate = kw.get("sample_rate", 16000)
    long_form = kw.pop("long_form", False)
    flac = kw.pop("format", "wav") == "flac"
    try:
        audio = pipeline.generate_long_speech(args, **kw) if long_form else pipeline.generate_speech(args, **kw)
    except Exception as e:  # noqa: BLE001 -- rendered as the reference's 500 body
        return 500, {"success": False, "error": f"生成TTS音频失败: {e}"}
    # (levelled PCM goes out at scale 1.0, as the stream route sends it: the peak rule would undo the target)
    if flac:  # the same samples as the WAV below: the peak rule's scale, or 1.0 for levelled PCM
        try:
            wav = pipeline.encoder().encode(audio, rate, scale=1.0 if "loudness" in kw else float(peak_scale(audio)))
        except Exception as e:  # noqa: BLE001 -- rendered as the reference's 500 body
            return 500, {"success": False, "error": f"生成TTS音频失败: {e}"}
    else:
        wav = levelled_samples_to_wav(audio, rate) if "loudness" in kw else convert_samples_to_wav(audio, rate)
    b64 =base64.standard_b64encode(wav).decode("ascii")
    total = time.perf_counter() - t0
    out = {"success": True, "message": "TTS生成成功", "audio_base64": b64,
           "duration_ms": int(total * 1000), "rtf": calculate_rtf(audio, total, rate)}
    if flac:
        out["format"] = "flac"
    if long_form:
        out["voice_tokens"] = audio.global_tokens
        out["segments"] = list(audio.segments)
    return 200, out


def streaming_wav_header(sample_rate: int = 16000) -> bytes:
    """The canonical 44-byte PCM WAV header (16-bit mono) with both sizes unknown (0xFFFFFFFF): the
    length of a stream is not known when its header goes out."""
    hdr = b"RIFF" + (0xFFFFFFFF).to_bytes(4, "little") + b"WAVE"
    hdr += b"fmt " + (16).to_bytes(4, "little") + (1).to_bytes(2, "little") + (1).to_bytes(2, "little")
    hdr += int(sample_rate).to_bytes(4, "little") + int(sample_rate * 2).to_bytes(4, "little")
    hdr += (2).to_bytes(2, "little") + (16).to_bytes(2, "little")
    return hdr + b"data" + (0xFFFFFFFF).to_bytes(4, "little")


def samples_to_pcm16(samples) -> bytes:
    """f32 -> little-endian i16 at scale 1.0: clamp to [-1, 1], x 32767, truncated toward zero, as
    convert_samples_to_wav does after its scaling."""
    x = np.asarray(samples, dtype=np.float32)
    y = np.clip(x, np.float32(-1.0), np.float32(1.0)) * np.float32(32767.0)
    return np.trunc(y).astype("<i2").tobytes()


def handle_tts_stream(body, pipeline, voice_dir: str = "assets/raf", chunk_frames: int = 16):
    """POST /api/tts/stream: the request body of /api/tts -> (HTTP status, iterator of bytes).

    200: a 44-byte WAV header with unknown-length sizes (streaming_wav_header), then the int16 PCM of
    pipeline.stream_speech's chunks as they are decoded (the first after chunk_frames + halo decode
    steps, not after the whole request). The scale is fixed at 1.0: the vocoder ends in tanh, so its
    samples already lie in (-1, 1). There is NO peak normalisation, unlike /api/tts
    (convert_samples_to_wav): the peak rule needs the whole utterance, which a stream does not have
    when its first sample goes out -- the same request is therefore quieter or louder here than in
    /api/tts's WAV, by that rule's factor, unless the body sets `loudness`: then both routes send the
    leveller's PCM at scale 1.0, byte for byte the same samples (the stream's lag 0.5 s behind the
    vocoder at the leveller's defaults). Clamping and truncation are convert_samples_to_wav's.
    An optional `sample_rate` (SAMPLE_RATES) streams that rate instead of 16 kHz: the chunks are
    resampled on the GPU by a resampler that is exact over chunks, and the header carries the rate.
    A refused body gives /api/tts's status and JSON body (as one bytes item); so does a failure
    before the first chunk (500). A failure after the first chunk can only end the stream."""
    err, args, kw = _tts_args(body, voice_dir)
    err = err or _no_key(kw, pipeline)
    if err:
        return err[0], iter([json.dumps(err[1], ensure_ascii=False).encode("utf-8")])
    rate = kw.get("sample_rate", 16000)
    flac = kw.pop("format", "wav") == "flac"
    try:
        # (created before the status line goes out: a failure is still a 500)
        fs = pipeline.encoder().stream(rate) if flac else None
        if kw.pop("long_form", False):  # one item per segment: the first audio when segment 0 is done
            chunks = pipeline.stream_long_speech(args, **kw)
        else:
            chunks = pipeline.stream_speech(args, chunk_frames=chunk_frames, **kw)
        first = next(chunks, None)  # before the status line goes out: a failure is still a 500
    except Exception as e:  # noqa: BLE001 -- rendered as the reference's 500 body
        payload = {"success": False, "error": f"生成TTS音频失败: {e}"}
        return 500, iter([json.dumps(payload, ensure_ascii=False).encode("utf-8")])

    def gen_flac():
        # the stream header (STREAMINFO with unknown totals), then frames as blocks complete, then the
        # short last block; an item without a complete block is empty and is not sent
        yield fs.feed(np.zeros(0, dtype=np.float32))
        if first is not None:
            b = fs.feed(first)
            if b:
                yield b
        for c in chunks:
            b = fs.feed(c)
            if b:
                yield b
        b = fs.feed(np.zeros(0, dtype=np.float32), final=True)
        if b:
            yield b

    def gen():
        yield streaming_wav_header(rate)
        # (with `tempo` an item may be empty, its blocks waiting for the next chunk's samples: an empty
        # body part would read as the end of a chunked response, so it is not sent)
        if first is not None and len(first):
            yield samples_to_pcm16(first)
        for c in chunks:
            if len(c):
                yield samples_to_pcm16(c)
    return 200, gen_flac() if flac else gen()


def tts_stream_media_type(body) -> str:
    """The media type of a 200 from handle_tts_stream for this body: audio/flac with `format: "flac"`,
    else audio/wav."""
    try:
        if isinstance(body, (bytes, str)):
            body = json.loads(body)
        return "audio/flac" if isinstance(body, dict) and body.get("format") == "flac" else "audio/wav"
    except ValueError:
        return "audio/wav"


def handle_watermark_detect(audio_path: Optional[str], pipeline) -> Tuple[int, dict]:
    """POST /api/watermark/detect: an uploaded WAV (or mono 16-bit FLAC) saved to a temporary path (None: no file) ->
    (HTTP status, JSON). The clip is brought to 16 kHz mono by load_audio without volume
    normalisation (on the codec's GPU when it has to be resampled; its silent edges are trimmed, which
    moves `offset` only), then read under the pipeline's key (pipeline.detect_watermark). 200:
    {success, detected, score, threshold, payload, seen_bits, offset, seconds} -- payload and offset
    mean something only where detected is true; seen_bits is the mask of payload bits the clip
    covers (a clip shorter than the mark's period misses some). The threshold is set for one false
    alarm in 10^6 clips without this key's mark; on noise-like audio a few seconds long the score can
    pass it while single payload bits are still unsure. A server without a key, a missing or
    unreadable file: 400 with {success: false, error}."""
    if getattr(pipeline, "watermark_key", None) is None:
        return 400, {"success": False, "error": "服务器未配置水印密钥 (watermark_key)，无法检测水印"}
    if not audio_path:
        return 400, {"success": False, "error": "未找到音频文件"}
    try:
        from .audio import load_audio
        pcm = load_audio(audio_path, 16000, volume_normalize=False,
                         device=getattr(getattr(pipeline, "codec", None), "device", None))
    except Exception as e:  # noqa: BLE001 -- every way a file can be unreadable is the caller's error
        return 400, {"success": False, "error": f"音频文件读取失败: {e}"}
    try:
        d = pipeline.detect_watermark(pcm)
    except Exception as e:  # noqa: BLE001 -- rendered as the reference's 500 body
        return 500, {"success": False, "error": f"水印检测失败: {e}"}
    return 200, {"success": True, "detected": bool(d["detected"]), "score": float(d["score"]),
                 "threshold": float(d["threshold"]), "payload": int(d["payload"]), "seen_bits": int(d["seen"]),
                 "offset": int(d["offset"]), "seconds": len(pcm) / 16000.0}


def handle_voice_list(voice_dir: str = "assets/raf") -> Tuple[int, dict]:
    """:920-944: {success, voices: [VoiceMetadata]} (an unreadable store: success false, [])."""
    try:
        voices = voice_manager(voice_dir).list_voices()
        return 200, {"success": True, "voices": [dict(v.__dict__) for v in voices]}
    except (OSError, ValueError, KeyError):
        return 200, {"success": False, "voices": []}


def handle_voice_delete(body, voice_dir: str = "assets/raf") -> Tuple[int, dict]:
    """:946-979: JSON {voice_id} -> {success, message}."""
    try:
        if isinstance(body, (bytes, str)):
            body = json.loads(body)
        voice_id = body["voice_id"]
        if not isinstance(voice_id, str):
            raise TypeError
    except (ValueError, KeyError, TypeError):
        return 200, {"success": False, "message": "请求格式错误"}
    try:
        voice_manager(voice_dir).delete_voice(voice_id)
        return 200, {"success": True, "message": "音色删除成功"}
    except (OSError, ValueError) as e:
        return 200, {"success": False, "message": f"删除音色失败: {e}"}


def handle_voice_extract(form: Optional[dict], audio_path: Optional[str], pipeline=None,
                         voice_dir: str = "assets/raf", is_multipart: bool = True) -> Tuple[int, dict]:
    """:777-918. form: voice_name / prompt_text; audio_path: the uploaded audio_file saved to a
    temporary path (None: no file). Extraction = pipeline.reference_tokenizer(path) ->
    (global, semantic) (the BiCodecTokenize encoders), duration / rate from the WAV itself."""
    def fail(msg):
        return 200, {"success": False, "message": msg, "voice_id": None}
    if not is_multipart:
        return fail("需要上传音频文件")
    form = form or {}
    name, prompt = form.get("voice_name") or "", form.get("prompt_text") or ""
    if not name:
        return fail("音色名称不能为空")
    if not prompt:
        return fail("提示词不能为空")
    if not audio_path:
        return fail("未找到音频文件")
    try:
        tok = getattr(pipeline, "reference_tokenizer", None)
        if tok is None:
            raise RuntimeError("ONNX模型文件不存在: assets/model/BiCodecTokenize.onnx")
        g, sem = tok(audio_path)
        from .audio import read_wav
        x, sr, ch = read_wav(audio_path)
        duration = (x.size // max(ch, 1)) / float(sr)
    except Exception as e:  # noqa: BLE001 -- the reference renders every extraction error this way
        return fail(f"音频特征提取失败: {e}")
    try:
        vid = voice_manager(voice_dir).save_voice_feature(name, prompt, list(g), list(sem), duration, sr)
    except (OSError, ValueError) as e:
        return fail(f"音色特征提取失败: {e}")
    return 200, {"success": True, "message": "音色特征提取成功", "voice_id": vid}


def create_app(pipeline, voice_dir: str = "assets/raf"):
    """FastAPI app with POST /api/tts (server.rs:1447) and POST /api/tts/stream. Serve with uvicorn."""
    from fastapi import FastAPI, Request
    from fastapi.responses import JSONResponse

    app = FastAPI(title="rwkvtts (MI355X)")

    @app.post("/api/tts")
    async def api_tts(request: Request):
        import anyio
        body = await request.body()
        code, payload = await anyio.to_thread.run_sync(handle_tts_json, body, pipeline, voice_dir)
        return JSONResponse(payload, status_code=code)

    @app.post("/api/tts/stream")
    async def api_tts_stream(request: Request):
        import anyio
        from fastapi.responses import Response, StreamingResponse
        body = await request.body()
        code, it = await anyio.to_thread.run_sync(handle_tts_stream, body, pipeline, voice_dir)
        if code != 200:
            return Response(b"".join(it), status_code=code, media_type="application/json")
        return StreamingResponse(it, media_type=tts_stream_media_type(body))  # (a sync iterator: iterated in a worker thread)

    @app.post("/api/watermark/detect")
    async def api_watermark_detect(request: Request):
        import anyio
        import tempfile
        data = None
        limit = 100 * 1024 * 1024  # load_audio's own bound, checked before the upload is read or written
        try:
            declared = int(request.headers.get("content-length", "0"))
        except ValueError:
            declared = 0
        if declared > limit:
            return JSONResponse({"success": False, "error": "音频文件超过 100 MB"}, status_code=413)
        if request.headers.get("content-type", "").startswith("multipart/"):
            up = (await request.form()).get("audio_file")
            if up is not None and not isinstance(up, str):
                data = await up.read()
        else:
            data = await request.body()  # (the WAV itself as the body)
        if data and len(data) > limit:  # (a body without a declared length)
            return JSONResponse({"success": False, "error": "音频文件超过 100 MB"}, status_code=413)
        path = None
        if data:
            fd, path = tempfile.mkstemp(suffix=".wav")
            with os.fdopen(fd, "wb") as f:
                f.write(data)
        try:
            code, payload = await anyio.to_thread.run_sync(handle_watermark_detect, path, pipeline)
        finally:
            if path and os.path.exists(path):
                os.remove(path)
        return JSONResponse(payload, status_code=code)

    @app.get("/api/voice-clone/list")
    async def api_voice_list():
        code, payload = handle_voice_list(voice_dir)
        return JSONResponse(payload, status_code=code)

    @app.post("/api/voice-clone/delete")
    async def api_voice_delete(request: Request):
        code, payload = handle_voice_delete(await request.body(), voice_dir)
        return JSONResponse(payload, status_code=code)

    @app.post("/api/voice-clone/extract")
    async def api_voice_extract(request: Request):
        import anyio
        import tempfile
        ctype = request.headers.get("content-type", "")
        if not ctype.startswith("multipart/"):
            return JSONResponse(handle_voice_extract(None, None, pipeline, voice_dir, is_multipart=False)[1])
        form = await request.form()
        fields = {k: v for k, v in form.items() if isinstance(v, str)}
        up = form.get("audio_file")
        path = None
        if up is not None and not isinstance(up, str):
            ext = os.path.splitext(up.filename or "audio")[1] or ".wav"
            tmp_dir = os.path.join(voice_dir, "temp", "upload_temp_files")
            os.makedirs(tmp_dir, exist_ok=True)
            fd, path = tempfile.mkstemp(suffix=ext, dir=tmp_dir)
            with os.fdopen(fd, "wb") as f:
                f.write(await up.read())
        try:
            code, payload = await anyio.to_thread.run_sync(handle_voice_extract, fields, path, pipeline, voice_dir)
        finally:
            if path and os.path.exists(path):
                os.remove(path)
        return JSONResponse(payload, status_code=code)

    return app
