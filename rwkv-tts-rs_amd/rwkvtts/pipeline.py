"""End-to-end text -> PCM: host mirror of `LightweightTtsPipeline` (src/lightweight_tts_pipeline.rs).

generate_speech (:733-852): text (+ attribute strings, or a voice's reference tokens) -> property
tokens (:162-193) -> DynamicBatchManager.generate_tts (which tokenises the text,
dynamic_batch_manager.rs:512-515) -> BiCodec decode (:606-622) -> f32 PCM @ 16 kHz; an empty
generation (a failed request) becomes one second of silence (:828-830).
generate_speech_batch (:855-1000): the same for a list of args through generate_tts_batch and
decode_audio_batch (a failed item decodes to an empty array there, as the reference's
spawn_blocking tasks return vec![]).
generate_speech, generate_speech_batch and stream_speech take `sample_rate` (no reference counterpart:
the reference emits 16 kHz only): None / 16000 is the vocoder's PCM as it is; any other rate is that
PCM resampled on the GPU with zero alignment (audio.Resampler), exact over stream chunks.
The same four entry points take `tempo` (no reference counterpart: the reference's only rate control
is the `speed` property token, which a cloned voice does not get): None / 1.0 leaves the PCM as it
is; any other value in 0.25 .. 4.0 (above 1 is faster speech) stretches the 16 kHz PCM on the GPU
without changing its pitch (audio.TimeStretcher), before any resampling, exact over stream chunks.
They and the long-form pair take `loudness` (no reference counterpart: the reference peak-normalises a
finished WAV): None leaves the PCM at the vocoder's scale; a target in dB, -40 .. -10, levels the
16 kHz PCM on the GPU to that K-weighted loudness under a peak ceiling (audio.Leveller, DESIGN.md
section 24), after the stretch and before the resampler, exact over stream chunks.
All five also take `pitch_shift` (no reference counterpart: the reference's only pitch control is the
`pitch` property token, which a cloned voice does not get): None / 0 leaves the PCM as it is; a shift
in semitones, -12 .. 12, moves the fundamental of the 16 kHz PCM on the GPU and keeps its spectral
envelope and its length (audio.PitchShifter), first of the stages -- before the
stretch, and in long-form after the join -- exact over stream chunks.
All five also take `watermark` (no reference counterpart: the reference marks nothing): None leaves the
PCM unmarked; a payload, an integer 0 .. 65535, embeds it as a spread-spectrum mark under the
pipeline's `watermark_key` (audio.Watermarker) on the 16 kHz PCM, after the
leveller and before the resampler -- in long-form on the joined signal, one continuous sequence --
exact over stream chunks. The key belongs to the pipeline, not to a request; without one, `watermark`
raises ValueError before anything is generated. detect_watermark reads a clip back.
All five also take `max_pause` (no reference counterpart: the reference sends whatever silence the
semantic model chose): None leaves the PCM as it is; a cap in milliseconds, an integer 20 .. 5000,
cuts every silence of the 16 kHz PCM on the GPU to at most that inside the result and half of it at
either end (audio.PauseShaper), first of the stages -- in long-form per segment,
before the join, whose own pauses stay -- exact over stream chunks. It is the one stage whose output
length depends on the data.
LightweightTtsPipelineArgs.global_sampling / semantic_sampling (no reference counterpart: the
reference carries temperature / top_p / top_k and samples with fixed values) set the token
generator's temperature, top-p and top-k per phase (runtime.PhaseSampling); a value outside its
range raises ValueError in the same four entry points before anything is generated.
LightweightTtsPipelineArgs.penalties (runtime.Penalties; no reference counterpart in the TTS path)
sets repetition, frequency and presence penalties over the request's own semantic tokens, in all
five entry points; in the long-form ones every segment gets the same penalties over its own history.
A value outside its range raises ValueError before anything is generated.
LightweightTtsPipelineArgs.mirostat (runtime.Mirostat; the reference has the sampler in its ai00
server and never calls it from its TTS path) samples the semantic phase with Mirostat in all five
entry points; in the long-form ones every segment gets the same tau and rate and a threshold of its
own. A bad value, or Mirostat together with semantic_sampling, raises ValueError before anything
is generated.

generate_long_speech / stream_long_speech (no reference counterpart: a request of the reference ends
at 2048 semantic tokens, 41 s, without an error) take a text of any length: segment.split_text cuts
it, the segments decode side by side with one voice (segment 0 a normal request, the others pinned
to its 32 global tokens: TtsBatchRequest.pinned_voice, LightweightTtsPipelineArgs.pin_voice), and
audio.Joiner joins their PCM on the GPU before the stretch and the resampler.

The voice store lookup by voice_id inside the pipeline (`VoiceFeatureManager::new("./raf")`,
:751) goes through `voices.VoiceFeatureManager` on `raf_dir` (the server passes the
tokens directly instead).
"""
import dataclasses
import os
import threading
from typing import List, Optional, Sequence

import numpy as np

from .properties import convert_standard_properties_to_tokens
from .runtime import LayeredRandomnessConfig, Mirostat, Penalties, PhaseSampling, SamplerArgs, TtsBatchRequest

SAMPLE_RATE = 16000


@dataclasses.dataclass
class LightweightTtsPipelineArgs:  # :18-65 (Default)
    text: str = ""
    prompt_text: str = ""
    ref_audio_path: str = ""
    temperature: float = 1.0
    top_p: float = 0.90
    top_k: int = 0
    max_tokens: int = 8000
    age: str = "youth-adult"
    gender: str = "female"
    emotion: str = "NEUTRAL"
    pitch: str = "medium"
    speed: str = "medium"
    zero_shot: bool = False
    validate: bool = False
    seed: Optional[int] = None
    voice_id: Optional[str] = None
    voice_global_tokens: Optional[List[int]] = None
    voice_semantic_tokens: Optional[List[int]] = None
    # no reference counterpart: the sampling of the global / semantic phase (runtime.PhaseSampling;
    # None: the reference's fixed (1.0, 0.95, 20 | 80)). temperature / top_p / top_k above stay
    # ignored, as in the reference.
    global_sampling: Optional[PhaseSampling] = None
    semantic_sampling: Optional[PhaseSampling] = None
    # repetition / frequency / presence penalties of the semantic phase (runtime.Penalties; None: none)
    penalties: Optional[Penalties] = None
    # Mirostat in the semantic phase (runtime.Mirostat; None: top-k / top-p / temperature as before)
    mirostat: Optional[Mirostat] = None
    # no reference counterpart: with voice_global_tokens set and voice_semantic_tokens None, a
    # normal-mode request whose 32 global tokens are those (rwkvtts_request.pinned_voice): the same
    # voice again, still with its property tokens. Without it that combination ignores the tokens.
    pin_voice: bool = False


def check_voice_pin(args) -> None:
    """ValueError for a pin_voice without exactly 32 voice_global_tokens in [0, 4096) or with
    voice_semantic_tokens, before anything is generated."""
    if not getattr(args, "pin_voice", False):
        return
    g = args.voice_global_tokens
    if args.voice_semantic_tokens is not None:
        raise ValueError("pin_voice: voice_semantic_tokens must be None (both token sets clone a voice)")
    if g is None or len(g) != 32 or any(isinstance(x, bool) or not isinstance(x, (int, np.integer)) or not 0 <= x < 4096
                                        for x in g):
        raise ValueError("pin_voice: voice_global_tokens must be 32 integers in [0, 4096)")


def check_sampling(args) -> None:
    """ValueError for a global_sampling / semantic_sampling (of pipeline args or SamplerArgs) outside
    the engine's ranges, before anything is generated."""
    for what in ("global_sampling", "semantic_sampling"):
        ph = getattr(args, what, None)
        if ph is None:
            continue
        if not isinstance(ph, PhaseSampling):
            raise ValueError(f"{what} must be a PhaseSampling")
        ph.check(what)
    pen = getattr(args, "penalties", None)
    if pen is not None:
        if not isinstance(pen, Penalties):
            raise ValueError("penalties must be a Penalties")
        pen.check()
    miro = getattr(args, "mirostat", None)
    if miro is not None:
        if not isinstance(miro, Mirostat):
            raise ValueError("mirostat must be a Mirostat")
        miro.check()
        if getattr(args, "semantic_sampling", None) is not None:
            raise ValueError("mirostat replaces the semantic phase's top-k, top-p and temperature: "
                             "semantic_sampling excludes it")
    check_voice_pin(args)


class SpeechChunk(np.ndarray):
    """One item of stream_speech: float32 PCM of frames [t0, t1) (an ndarray, so b"".join(chunks) and
    np.concatenate work on it), decoded when n_known semantic tokens were known; done: the request had
    finished by then. t0 and t1 are always the vocoder's frames; behind a stage that changes the
    length (tempo, sample_rate, and max_pause, which removes a data-dependent number of samples) the
    chunk's length does not follow from them."""
    t0 = t1 = n_known = 0
    done = False

    @classmethod
    def make(cls, pcm, t0, t1, n_known, done):
        c = np.ascontiguousarray(pcm, dtype=np.float32).view(cls)
        c.t0, c.t1, c.n_known, c.done = int(t0), int(t1), int(n_known), bool(done)
        return c


class LongSpeech(np.ndarray):
    """The result of generate_long_speech, and one item of stream_long_speech: float32 PCM (an
    ndarray) that also carries global_tokens (the voice every segment spoke with; None if none is
    known) and segments, one record per segment it holds: text, status, n_semantic, truncated (the
    segment emitted as many semantic tokens as its limit allows: it was probably cut off), pause_ms,
    and a, b (the samples [a, b) of the segment's 16 kHz PCM that the join kept). With max_pause a
    record also has cut (the samples the pause cap removed from the segment before the join), and a, b
    refer to the shaped segment."""
    global_tokens = None
    segments = ()

    @classmethod
    def make(cls, pcm, global_tokens, segments):
        c = np.ascontiguousarray(pcm, dtype=np.float32).view(cls)
        c.global_tokens = None if global_tokens is None else list(global_tokens)
        c.segments = list(segments)
        return c


def audio_stages(stretcher, tempo, resampler, leveller=None, loudness=None, shifter=None, pitch_shift=None,
                 marker=None, watermark=None, watermark_key=None, shaper=None, max_pause=None) -> list:
    """The stages behind the vocoder in the order they apply -- the pause cap at 16 kHz, then the pitch
    shift, then the stretch, then the leveller, then the watermark, then the resampler; None is no
    stage -- each as (batch, stream): batch([pcm]) -> [pcm] in one native call (one cap, one shift, one
    tempo, one loudness, one key and payload for the call), stream() -> an object whose feed(pcm, final)
    is exact over chunks. The pause cap removes samples, so every stage behind it does less work."""
    stages = []
    if shaper is not None:
        stages.append((lambda pcm: shaper.shape_batch(pcm, max_pause), lambda: shaper.stream(max_pause)))
    if shifter is not None:
        stages.append((lambda pcm: shifter.shift_batch(pcm, [pitch_shift] * len(pcm)), lambda: shifter.stream(pitch_shift)))
    if stretcher is not None:
        stages.append((lambda pcm: stretcher.stretch_batch(pcm, [tempo] * len(pcm)), lambda: stretcher.stream(tempo)))
    if leveller is not None:
        stages.append((lambda pcm: leveller.level_batch(pcm, [loudness] * len(pcm)), lambda: leveller.stream(loudness)))
    if marker is not None:
        stages.append((lambda pcm: marker.embed_batch(pcm, [watermark_key] * len(pcm), [watermark] * len(pcm)),
                       lambda: marker.stream(watermark_key, watermark)))
    if resampler is not None:
        stages.append((resampler.resample_batch, resampler.stream))
    return stages


def feed_stages(streams, pcm, final: bool):
    """One vocoder chunk through the stages' streams in order; each passes on what became exact."""
    for s in streams:
        pcm = s.feed(pcm, final=final)
    return pcm


class LightweightTtsPipeline:
    """manager: rwkvtts.DynamicBatchManager (with a tokenizer); codec: BiCodecDetokenizer."""

    def __init__(self, manager, codec, raf_dir: str = "./raf", reference_tokenizer=None,
                 watermark_key: Optional[int] = None):
        self.manager = manager
        self.codec = codec
        self.raf_dir = raf_dir
        # zero-shot from a reference audio file needs the BiCodecTokenize / wav2vec2 encoders,
        # whose graphs are not available; a callable (path -> (global, semantic))
        # may be supplied
        self.reference_tokenizer = reference_tokenizer
        self._resamplers = {}  # output rate -> audio.Resampler (created on first use, kept)
        self._stretcher = None  # audio.TimeStretcher (created on the first tempo other than 1.0, kept)
        self._joiners = {}  # (trim, keep, fade) -> audio.Joiner (created on first use, kept)
        self._levellers = {}  # horizon -> audio.Leveller (created on the first loudness, kept)
        self._shifter = None  # audio.PitchShifter (created on the first pitch_shift other than 0, kept)
        # no reference counterpart: the 64-bit key of this deployment's provenance mark (None: the
        # pipeline marks nothing and `watermark` is refused); it is the pipeline's, never a request's
        if watermark_key is not None and (isinstance(watermark_key, bool) or not isinstance(watermark_key, int)
                                          or not 0 <= watermark_key < 1 << 64):
            raise ValueError("watermark_key must be an integer in [0, 2^64)")
        self.watermark_key = watermark_key
        self._marker = None  # audio.Watermarker (created on the first watermark or detect_watermark, kept)
        self._encoder = None  # audio.FlacEncoder (created on the first `format: "flac"`, kept)
        self._shapers = {}  # threshold -> audio.PauseShaper (created on the first max_pause, kept)
        self._pause_threshold = None  # the loudness threshold of `max_pause` (None: audio.PauseShaper's default)
        self._stage_cache_lock = threading.Lock()  # guards all eight (the server's worker threads share the pipeline)

    # ---- output rates other than 16 kHz (no reference counterpart: the reference emits 16 kHz only)
    def resampler(self, sample_rate: Optional[int]):
        """None for None / 16000 (nothing is created: the PCM is the vocoder's); otherwise the
        pipeline's Resampler 16000 -> sample_rate with zero alignment (output o at input time
        o * 16000 / sample_rate: no delay, nothing cut), on the codec's GPU."""
        if sample_rate is None or int(sample_rate) == SAMPLE_RATE:
            return None
        rate = int(sample_rate)
        with self._stage_cache_lock:
            r = self._resamplers.get(rate)
            if r is None:
                from .audio import Resampler
                r = self._resamplers[rate] = Resampler(SAMPLE_RATE, rate, device=getattr(self.codec, "device", 0),
                                                       align="zero")
        return r

    # ---- speaking rate (no reference counterpart: the reference has the `speed` property token only)
    def stretcher(self, tempo: Optional[float]):
        """None for None / 1.0 (nothing is created: the PCM is the vocoder's); otherwise the
        pipeline's one TimeStretcher, on the codec's GPU. A tempo outside 0.25 .. 4.0 raises
        ValueError before anything is generated."""
        if tempo is None or float(tempo) == 1.0:
            return None
        if not 0.25 <= float(tempo) <= 4.0:  # (NaN fails)
            raise ValueError("tempo must be in [0.25, 4.0]")
        with self._stage_cache_lock:
            if self._stretcher is None:
                from .audio import TimeStretcher
                self._stretcher = TimeStretcher(device=getattr(self.codec, "device", 0))
        return self._stretcher

    # ---- long texts (no reference counterpart: the reference stops at 2048 semantic tokens)
    def joiner(self, trim: bool = True, keep: int = 800, fade: int = 80):
        """The pipeline's Joiner for these parameters, on the codec's GPU."""
        key = (bool(trim), int(keep), int(fade))
        with self._stage_cache_lock:
            j = self._joiners.get(key)
            if j is None:
                from .audio import Joiner
                j = self._joiners[key] = Joiner(device=getattr(self.codec, "device", 0), trim=key[0], keep=key[1],
                                                fade=key[2])
        return j

    # ---- loudness (no reference counterpart: the reference peak-normalises a finished WAV)
    def leveller(self, loudness: Optional[float], horizon: int = 0):
        """None for None (nothing is created: the PCM keeps the vocoder's scale); otherwise the
        pipeline's Leveller for this horizon (its other parameters are the untuned defaults of
        audio.Leveller), on the codec's GPU. The loudness is a target in dB per call, not a part of
        the object. A loudness outside -40 .. -10 raises ValueError before anything is generated."""
        if loudness is None:
            return None
        if isinstance(loudness, bool) or not -40.0 <= float(loudness) <= -10.0:  # (NaN fails)
            raise ValueError("loudness must be in [-40, -10] dB")
        key = int(horizon)
        with self._stage_cache_lock:
            v = self._levellers.get(key)
            if v is None:
                from .audio import Leveller
                v = self._levellers[key] = Leveller(device=getattr(self.codec, "device", 0), horizon=key)
        return v

    # ---- pitch (no reference counterpart: the reference has the `pitch` property token only)
    def shifter(self, pitch_shift: Optional[float]):
        """None for None / 0 (nothing is created: the PCM is the vocoder's); otherwise the pipeline's
        one PitchShifter (the untuned defaults of audio.PitchShifter), on the codec's GPU. The shift
        is in semitones per call, not a part of the object. A shift outside -12 .. 12 raises
        ValueError before anything is generated."""
        if pitch_shift is None:
            return None
        if isinstance(pitch_shift, bool) or not -12.0 <= float(pitch_shift) <= 12.0:  # (NaN fails)
            raise ValueError("pitch_shift must be in [-12, 12] semitones")
        if float(pitch_shift) == 0.0:
            return None
        with self._stage_cache_lock:
            if self._shifter is None:
                from .audio import PitchShifter
                self._shifter = PitchShifter(device=getattr(self.codec, "device", 0))
        return self._shifter

    # ---- provenance (no reference counterpart: the reference marks nothing)
    def marker(self, watermark: Optional[int] = 0):
        """None for None (nothing is created: the PCM is unmarked); otherwise the pipeline's one
        Watermarker (the untuned defaults of audio.Watermarker), on the codec's GPU. The payload is
        per call, the key is the pipeline's. A payload that is not an integer in 0 .. 65535, or any
        payload on a pipeline without a watermark_key, raises ValueError before anything is generated."""
        if watermark is None:
            return None
        if isinstance(watermark, bool) or not isinstance(watermark, (int, np.integer)) or not 0 <= int(watermark) <= 65535:
            raise ValueError("watermark must be an integer payload in [0, 65535]")
        if self.watermark_key is None:
            raise ValueError("watermark needs a pipeline with a watermark_key")
        with self._stage_cache_lock:
            if self._marker is None:
                from .audio import Watermarker
                self._marker = Watermarker(device=getattr(self.codec, "device", 0))
        return self._marker

    def detect_watermark(self, pcm) -> dict:
        """16 kHz PCM of any origin -> audio.Watermarker.detect under the pipeline's key: {detected,
        score, threshold, payload, seen, offset, min_z}. ValueError without a watermark_key. detected
        is score >= threshold, set for one false alarm in 10^6 clips that carry no mark under this key
        (another key's mark included); payload and offset mean something only where it is true, and a
        payload bit is as sure as min_z is large (under 1: a guess). DESIGN.md section 30."""
        return self.marker(0).detect(pcm, self.watermark_key)

    # ---- pauses (no reference counterpart: the reference sends the silence the semantic model chose)
    def pause_shaper(self, max_pause: Optional[int], threshold: Optional[float] = None):
        """None for None (nothing is created: the PCM is the vocoder's); otherwise the pipeline's
        PauseShaper (the untuned defaults of audio.PauseShaper), on the codec's GPU. The cap is an
        integer number of milliseconds per call, not a part of the object: no silence inside the
        result is longer than it, none at either end longer than half of it. A cap outside 20 .. 5000,
        a bool, a NaN or a fraction raises ValueError before anything is generated. threshold: the
        loudness threshold of the pipeline's pause stage from this call on (it belongs to the
        deployment, like the watermark key; None keeps the current one, at first the join's 0.01)."""
        if threshold is not None:
            if isinstance(threshold, bool) or not 0.0 < float(threshold) <= 3.0e38:  # (NaN fails)
                raise ValueError("the pause threshold must be finite and positive")
            self._pause_threshold = float(np.float32(threshold))
        if max_pause is None:
            return None
        if (isinstance(max_pause, bool) or not isinstance(max_pause, (int, float, np.integer, np.floating))
                or not 20 <= max_pause <= 5000 or int(max_pause) != max_pause):  # (NaN fails the comparison)
            raise ValueError("max_pause must be an integer number of milliseconds in [20, 5000]")
        key = self._pause_threshold
        with self._stage_cache_lock:
            ps = self._shapers.get(key)
            if ps is None:
                from .audio import PauseShaper
                ps = self._shapers[key] = PauseShaper(device=getattr(self.codec, "device", 0),
                                                      **({} if key is None else {"threshold": key}))
        return ps

    # ---- compressed output (no reference counterpart: the reference sends WAV only)
    def encoder(self):
        """The pipeline's one FlacEncoder, on the codec's GPU, created on first use. It is no stage of
        the PCM chain: the server's handlers run finished PCM through it for `format: "flac"`."""
        with self._stage_cache_lock:
            if self._encoder is None:
                from .audio import FlacEncoder
                self._encoder = FlacEncoder(device=getattr(self.codec, "device", 0))
        return self._encoder

    def _stages(self, sample_rate: Optional[int], tempo: Optional[float], loudness: Optional[float] = None,
                pitch_shift: Optional[float] = None, watermark: Optional[int] = None,
                max_pause: Optional[int] = None):  # -> (stages, output rate)
        rs = self.resampler(sample_rate)
        lv = self.leveller(loudness)
        sh = self.shifter(pitch_shift)
        mk = self.marker(watermark)
        ps = self.pause_shaper(max_pause)
        # (without max_pause the call is the one it always was: stand-ins of audio_stages see no new keyword)
        kw = {} if ps is None else {"shaper": ps, "max_pause": int(max_pause)}
        return (audio_stages(self.stretcher(tempo), tempo, rs, lv, None if lv is None else float(loudness),
                             sh, None if sh is None else float(pitch_shift),
                             mk, None if mk is None else int(watermark), self.watermark_key, **kw),
                rs.sr_out if rs else SAMPLE_RATE)

    # ---- text / attribute handling (:148-193)
    @staticmethod
    def process_text(text: str) -> str:
        return text

    @staticmethod
    def process_text_zero_shot(text: str, _prompt_text: str) -> str:
        """Cross-lingual cloning: the reference prompt text is ignored (:157-160)."""
        return text

    @staticmethod
    def generate_property_tokens(args: LightweightTtsPipelineArgs) -> List[int]:
        if (args.voice_global_tokens is not None and args.voice_semantic_tokens is not None) or args.zero_shot:
            return []
        return convert_standard_properties_to_tokens(args.age, args.gender, args.emotion, args.pitch, args.speed)

    def _voice_tokens(self, voice_id: str):
        """VoiceFeatureManager::new(raf_dir).get_voice_tokens (:751-760; checksum verified)."""
        from .voices import VoiceFeatureManager
        if getattr(self, "_voices", None) is None:
            self._voices = VoiceFeatureManager(self.raf_dir)
        return self._voices.get_voice_tokens(voice_id)

    def process_reference_audio(self, ref_audio_path: str):
        if not ref_audio_path or not os.path.exists(ref_audio_path):
            raise FileNotFoundError(f"reference audio not found: {ref_audio_path}")
        if self.reference_tokenizer is None:
            raise NotImplementedError("reference-audio tokenisation needs the BiCodecTokenize encoder")
        return self.reference_tokenizer(ref_audio_path)

    def _prompt_parts(self, args: LightweightTtsPipelineArgs):
        """(property tokens, ref global, ref semantic) with the reference's precedence (:747-789)."""
        have_voice = args.voice_global_tokens is not None and args.voice_semantic_tokens is not None
        if args.voice_id is not None:
            try:
                g, s = self._voice_tokens(args.voice_id)
                return [], g, s
            except (OSError, KeyError, ValueError):
                pass  # fall through to the directly supplied tokens / attributes
        if have_voice:
            return [], list(args.voice_global_tokens), list(args.voice_semantic_tokens)
        if args.zero_shot:
            g, s = self.process_reference_audio(args.ref_audio_path)
            return [], g, s
        if args.pin_voice and args.voice_global_tokens is not None:  # a pinned voice keeps its property tokens
            return self.generate_property_tokens(args), [int(x) for x in args.voice_global_tokens], None
        return self.generate_property_tokens(args), None, None

    def _request(self, args: LightweightTtsPipelineArgs) -> TtsBatchRequest:
        text = self.process_text_zero_shot(args.text, args.prompt_text) if args.zero_shot else self.process_text(args.text)
        props, rg, rs = self._prompt_parts(args)
        sargs = SamplerArgs(temperature=args.temperature, top_p=args.top_p, top_k=args.top_k,
                            max_tokens=args.max_tokens, seed=args.seed, voice_fidelity=0.8,
                            layered_randomness=LayeredRandomnessConfig(), token_chunk_size=512,
                            global_sampling=args.global_sampling, semantic_sampling=args.semantic_sampling,
                            penalties=args.penalties, mirostat=args.mirostat)
        return TtsBatchRequest(self.manager._tokens(text), props, rg, rs, sargs, args.voice_id,
                               pinned_voice=rg is not None and rs is None)

    def generate_speech(self, args: LightweightTtsPipelineArgs, sample_rate: Optional[int] = None,
                        tempo: Optional[float] = None, loudness: Optional[float] = None,
                        watermark: Optional[int] = None, max_pause: Optional[int] = None,
                        pitch_shift: Optional[float] = None) -> np.ndarray:
        """sample_rate None / 16000: the vocoder's 16 kHz PCM. Any other rate: that PCM resampled on
        the GPU (resampler()); the failed-request second of silence is sample_rate zeros.
        tempo None / 1.0: nothing. Any other: the 16 kHz PCM time-stretched on the GPU (stretcher())
        before the resampler; the failed-request second of silence is not stretched.
        loudness None: nothing. A target in dB, -40 .. -10 (-23, -16, ..): the 16 kHz PCM levelled on
        the GPU (leveller()) after the stretch and before the resampler; the failed-request second of
        silence is not levelled.
        pitch_shift None / 0: nothing. A shift in semitones, -12 .. 12: the 16 kHz PCM's fundamental
        moved on the GPU (shifter()) before the stretch, its envelope and length kept; independent of
        args.pitch, which stays the property token.
        watermark None: nothing. A payload 0 .. 65535: the 16 kHz PCM marked on the GPU (marker())
        under the pipeline's key, after the leveller and before the resampler; the failed-request
        second of silence is not marked (silence carries no mark).
        max_pause None: nothing. A cap in milliseconds, an integer 20 .. 5000: the silences of the
        16 kHz PCM capped on the GPU (pause_shaper()), first of the stages, so the result is shorter
        than the vocoder's PCM by what was cut; the failed-request second of silence is not shaped.
        args.global_sampling / semantic_sampling outside their ranges raise ValueError, like tempo."""
        check_sampling(args)
        stages, rate = self._stages(sample_rate, tempo, loudness, pitch_shift, watermark, max_pause)
        try:
            req = self._request(args)
        except ValueError:  # untokenisable text: the request fails -> empty result
            req = None
        g, s = self.manager.generate_tts_batch([req])[0] if req is not None else ([], [])
        if not g and not s:
            return np.zeros(rate, dtype=np.float32)  # :828-830
        pcm = self.codec.decode_audio(g, s)
        for batch, _ in stages:
            pcm = batch([pcm])[0]
        return pcm

    def stream_speech(self, args: LightweightTtsPipelineArgs, chunk_frames: int = 16,
                      sample_rate: Optional[int] = None, tempo: Optional[float] = None,
                      loudness: Optional[float] = None, watermark: Optional[int] = None,
                      max_pause: Optional[int] = None, pitch_shift: Optional[float] = None):
        """generate_speech as a generator of float32 PCM chunks (SpeechChunk: an ndarray that also
        carries t0, t1, n_known, done), each decoded while the request is still generating tokens.

        Chunk [t0, t1) (frames of 320 samples; chunk_frames each, the last one shorter) is decoded by
        the exact windowed vocoder as soon as t1 + H semantic tokens are known, or the request is
        done; chunks that become ready together go through one batched decode. H = codec.halo() is
        the decoder's receptive field per side -- 49 frames, 0.98 s of audio, at the full dims -- and
        that look-ahead is inherent to an exact chunk: with fewer tokens known, the chunk's last
        samples would still change. So the concatenation of the chunks is bitwise
        generate_speech(args) for the same seed, the first chunk exists after chunk_frames + H
        decode steps instead of after the whole request, and a request that fails before any chunk
        yields the same one second of zeros. A request that fails after some chunks were yielded
        ends the stream there (its last item has done = False). An item's done says that the request
        had finished when the chunk was decoded; the last chunk has done and t1 == n_known.

        tempo other than None / 1.0, sample_rate other than None / 16000: every vocoder chunk goes
        through one stream per stage (audio_stages: TimeStretcher.stream(tempo), then
        Resampler.stream()), each exact over chunks, so the concatenation is bitwise
        generate_speech(args, tempo=..., sample_rate=...). An item then holds what became exact with
        its frames: whole stretched blocks (it may be empty), resampled outputs short of the
        sinc_len / 2 = 128 input samples of look-ahead. t0, t1 and n_known stay in frames.

        loudness (a target in dB, -40 .. -10): Leveller.stream(loudness) sits between the two, and the
        concatenation is bitwise generate_speech(args, loudness=...). A levelled item lags its frames
        by up to lookahead + 1 blocks, 0.5 s at the defaults: a block goes out once the four blocks
        after it are complete.

        pitch_shift (semitones, -12 .. 12, not 0): PitchShifter.stream(pitch_shift) comes first, and
        the concatenation is bitwise generate_speech(args, pitch_shift=...). A shifted item lags its
        frames by the shifter's look-ahead, 0.1 s at the defaults.

        watermark (a payload 0 .. 65535): Watermarker.stream(key, payload) sits after the leveller, and
        the concatenation is bitwise generate_speech(args, watermark=...). A marked item lags its
        frames by less than one block, 20 ms.

        max_pause (milliseconds, 20 .. 5000): PauseShaper.stream(max_pause) comes first of all, and the
        concatenation is bitwise generate_speech(args, max_pause=...). t0 and t1 stay the vocoder's
        frames, and a chunk's length no longer follows from them: an item holds what became exact
        with its frames -- nothing while the request is still in its leading silence (which is latency
        no more), less than its frames where a silence was cut."""
        if chunk_frames < 1:
            raise ValueError("chunk_frames must be >= 1")
        check_sampling(args)
        try:
            req = self._request(args)
        except ValueError:  # untokenisable text: the request fails -> one second of silence
            req = None
        self.leveller(loudness)  # (refuses a bad loudness here, not at the first next())
        kw = {}
        if pitch_shift is not None:
            self.shifter(pitch_shift)  # (the same for a bad shift)
            kw["pitch_shift"] = pitch_shift
        if watermark is not None:
            self.marker(watermark)  # (and for a bad payload or a missing key)
            kw["watermark"] = watermark
        if max_pause is not None:
            self.pause_shaper(max_pause)  # (and for a bad cap)
            kw["max_pause"] = max_pause
        return self.stream_request(req, chunk_frames, sample_rate=sample_rate, tempo=tempo, loudness=loudness, **kw)

    def stream_request(self, req: Optional[TtsBatchRequest], chunk_frames: int = 16,
                       sample_rate: Optional[int] = None, tempo: Optional[float] = None,
                       loudness: Optional[float] = None, watermark: Optional[int] = None,
                       max_pause: Optional[int] = None, pitch_shift: Optional[float] = None):
        """stream_speech for a request that is already built (None: a request that failed before it
        was submitted)."""
        if chunk_frames < 1:
            raise ValueError("chunk_frames must be >= 1")
        if req is not None:
            check_sampling(req.args)
        stages, rate = self._stages(sample_rate, tempo, loudness, pitch_shift, watermark, max_pause)
        streams = [stream() for _, stream in stages]
        H = self.codec.halo()
        g, sem, t0, yielded, status = None, [], 0, False, 0
        it = self.manager.stream_tts(req) if req is not None else iter([(None, [], True)])
        try:
            for gi, new, done in it:
                if gi is not None:
                    g = gi
                sem.extend(new)
                n = len(sem)
                if done and req is not None:
                    status = (self.manager.last_status or [0])[0]
                if done and (status != 0 or (not g and not sem)):
                    if not yielded:
                        yield SpeechChunk.make(np.zeros(rate, dtype=np.float32), 0, 0, 0, True)  # :828-830
                    return
                if done and not sem:
                    self.codec.decode_audio(g, sem)  # (raises as generate_speech does: no semantic tokens)
                wins = []
                while g is not None and t0 < n and (done or t0 + chunk_frames + H <= n):
                    t1 = min(t0 + chunk_frames, n)
                    wins.append((t0, t1))
                    t0 = t1
                if wins:
                    pcm = self.codec.decode_windows([(g, sem, a, b, done) for a, b in wins])
                    for (a, b), p in zip(wins, pcm):
                        yielded = True
                        yield SpeechChunk.make(feed_stages(streams, p, done and b == n), a, b, n, done)
        finally:
            if hasattr(it, "close"):
                it.close()  # (a stream left early: the ticket is released once the request has finished)

    def generate_speech_batch(self, batch_args: Sequence[LightweightTtsPipelineArgs],
                              sample_rate: Optional[int] = None, tempo: Optional[float] = None,
                              loudness: Optional[float] = None, watermark: Optional[int] = None,
                              max_pause: Optional[int] = None, pitch_shift: Optional[float] = None) -> List[np.ndarray]:
        """sample_rate other than None / 16000: the whole batch is resampled in one resample_batch
        call (a failed item stays an empty array). tempo other than None / 1.0: the whole batch is
        first stretched in one stretch_batch call, one tempo for the call. loudness other than None:
        the whole batch is levelled in one level_batch call between the two, one target for the call.
        pitch_shift other than None / 0: the whole batch is shifted in one shift_batch call before
        all of them, one shift for the call. watermark other than None: the whole batch is marked in
        one embed_batch call after the leveller, one payload for the call. max_pause other than None:
        the silences of the whole batch are capped in one shape_batch call before all of them, one
        cap for the call."""
        for a in batch_args:
            check_sampling(a)
        stages, _ = self._stages(sample_rate, tempo, loudness, pitch_shift, watermark, max_pause)
        reqs, idx = [], []
        for i, a in enumerate(batch_args):
            try:
                reqs.append(self._request(a))
                idx.append(i)
            except ValueError:
                pass
        res = self.manager.generate_tts_batch(reqs) if reqs else []
        results = [([], [])] * len(batch_args)
        for i, r in zip(idx, res):
            results[i] = r
        pcm = self.codec.decode_audio_batch(results)
        for batch, _ in stages:
            pcm = batch(pcm)
        return pcm

    # ---- long-form synthesis (no reference counterpart: a request of the reference ends at 2048
    # semantic tokens, 41 s of audio, without an error) ------------------------------------------
    def _long_submit(self, args: LightweightTtsPipelineArgs, segment_tokens: int, pauses):
        """Segments the text and submits every segment. -> (segments, tickets, limit), or None for a
        text that cannot be tokenised or whose first segment failed before its voice was known
        (nothing is left in flight then). tickets[i] is None for a segment that was not submitted.

        A cloned voice (voice_id, both voice token sets, zero_shot) submits every segment at once as
        the zero-shot request _request builds; pin_voice submits every segment pinned from the
        start. Otherwise segment 0 is the request generate_speech would build, submitted as a
        stream; as soon as its 32 global tokens are known, segments 1 .. N-1 go out at once, each
        the same request with its own text, pinned to those tokens. Segment i is seeded with
        args.seed + i when args.seed is given."""
        from .segment import Pauses, Segment, split_text
        text = self.process_text_zero_shot(args.text, args.prompt_text) if args.zero_shot else self.process_text(args.text)
        try:
            segs = split_text(text, self.manager._tokens, segment_tokens, pauses or Pauses())
            if len(segs) <= 1:  # one segment is generate_speech's request, surrounding whitespace included
                segs = [Segment(text, list(self.manager._tokens(text)), 0, "end")]
            base = self._request(dataclasses.replace(args, text=""))
        except ValueError:  # untokenisable text
            return None

        def request(i, pin=None):
            r = dataclasses.replace(base, text_tokens=list(segs[i].tokens), args=dataclasses.replace(
                base.args, seed=None if args.seed is None else int(args.seed) + i))
            if pin is not None:
                r.ref_global_tokens, r.ref_semantic_tokens, r.pinned_voice = list(pin), None, True
            return r

        limit = 2048 if base.ref_semantic_tokens is not None else min(max(int(args.max_tokens), 0), 2048)
        if base.ref_global_tokens is not None:  # the voice is known: cloned (zero-shot) or pinned
            return segs, [self.manager.submit(request(i)) for i in range(len(segs))], limit
        t0 = self.manager.submit(request(0), stream=True)
        voice, have = None, 0
        try:
            while voice is None:
                voice, sem, done, status = self.manager.wait_tokens(t0, have)
                have = len(sem)
                if done:
                    break
        except BaseException:
            self.manager.wait_status(t0)
            raise
        if voice is None or len(voice) != 32:  # segment 0 failed in normal mode: no voice to go on with
            self.manager.wait_status(t0)
            return None
        return segs, [t0] + [self.manager.submit(request(i, voice)) for i in range(1, len(segs))], limit

    @staticmethod
    def _long_record(seg, result, status, limit):
        g, s = result
        return {"text": seg.text, "status": int(status), "n_semantic": len(s), "truncated": bool(s) and len(s) >= limit,
                "pause_ms": int(seg.pause_ms), "a": 0, "b": 0}

    @staticmethod
    def _long_shape(shaper, max_pause, pcm, recs):
        """The segments' PCM with their silences capped, in one call; each record gains `cut`."""
        shaped = shaper.shape_batch(pcm, int(max_pause))
        for rec, x, y in zip(recs, pcm, shaped):
            rec["cut"] = int(np.asarray(x).size - y.size)
        return shaped

    def generate_long_speech(self, args: LightweightTtsPipelineArgs, sample_rate: Optional[int] = None,
                             tempo: Optional[float] = None, segment_tokens: int = 64, pauses=None,
                             trim: bool = True, keep: int = 800, fade: int = 80,
                             loudness: Optional[float] = None, watermark: Optional[int] = None,
                             max_pause: Optional[int] = None, pitch_shift: Optional[float] = None) -> "LongSpeech":
        """generate_speech for a text of any length: the text is cut into segments of at most
        segment_tokens text tokens (segment.split_text), the segments decode side by side in the
        manager's slots and engines with one voice (_long_submit), and their PCM is joined on the
        GPU (audio.Joiner: with trim, each segment cut to `keep` samples around its audible part
        and faded over `fade` samples; pause_ms * 16 zero samples after it), then stretched and
        resampled as generate_speech does. One decode_audio_batch, one join.

        A failed segment contributes only its gap and its status. If segment 0 fails in normal mode,
        or every segment fails, the result is generate_speech's second of silence. A text of one
        segment with trim=False gives bitwise generate_speech(args, ...). segment_tokens, pauses,
        keep and fade are unmeasured defaults. loudness levels the joined
        signal as one (generate_speech), so the segments, decoded as independent requests, come out
        at one level; the second of silence is not levelled. pitch_shift shifts the joined signal as
        one, after the join and before the stretch. watermark marks the joined signal as one, so a
        job carries one continuous sequence across its segments and pauses. max_pause caps the
        silences of every segment's PCM before the join, all segments in one shape_batch call; the
        pauses the join puts between segments are deliberate and stay. A record's `cut` is what the
        cap removed from its segment, and its a, b then refer to the shaped segment. The second of
        silence is not shaped."""
        check_sampling(args)
        stages, rate = self._stages(sample_rate, tempo, loudness, pitch_shift, watermark)
        shaper = self.pause_shaper(max_pause)
        joiner = self.joiner(trim, keep, fade)
        plan = self._long_submit(args, segment_tokens, pauses)
        if plan is None:
            return LongSpeech.make(np.zeros(rate, dtype=np.float32), None, [])  # :828-830
        segs, tickets, limit = plan
        results = [self.manager.wait_status(t) for t in tickets]
        recs = [self._long_record(sg, r, st, limit) for sg, (r, st) in zip(segs, results)]
        voice = next((list(r[0]) for r, st in results if st == 0 and r[0]), None)
        if not any(st == 0 and (r[0] or r[1]) for r, st in results):
            return LongSpeech.make(np.zeros(rate, dtype=np.float32), voice, recs)
        pcm = self.codec.decode_audio_batch([r if st == 0 else ([], []) for r, st in results])
        if shaper is not None:
            pcm = self._long_shape(shaper, max_pause, pcm, recs)
        out, ab = joiner.join(pcm, [sg.pause_ms * (SAMPLE_RATE // 1000) for sg in segs])
        for rec, (a, b) in zip(recs, ab):
            rec["a"], rec["b"] = a, b
        for batch, _ in stages:
            out = batch([out])[0]
        return LongSpeech.make(out, voice, recs)

    def stream_long_speech(self, args: LightweightTtsPipelineArgs, sample_rate: Optional[int] = None,
                           tempo: Optional[float] = None, segment_tokens: int = 64, pauses=None,
                           trim: bool = True, keep: int = 800, fade: int = 80, loudness: Optional[float] = None,
                           watermark: Optional[int] = None, max_pause: Optional[int] = None,
                           pitch_shift: Optional[float] = None):
        """generate_long_speech as a generator of LongSpeech items, one per segment, in order: segment
        i is emitted once it and every segment before it are done -- decoded, joined alone with its
        gap (a piece depends on its own segment only), and fed through the stages' exact streams,
        with `final` on the last segment. The concatenation of the items is bitwise
        generate_long_speech for the same arguments and seed; the first audio arrives when segment 0
        has finished. An item may be empty (a failed segment without a gap; stretched blocks or
        resampled outputs still waiting for the next segment's samples). Failed segments before the
        first good one are held back until it arrives, so a text whose every segment fails yields
        the one second of silence alone. Streaming inside a segment is out of scope. With loudness
        an item also waits for the leveller's look-ahead (up to 0.5 s of the next segment), with
        pitch_shift for the shifter's (0.1 s), with watermark for the rest of its last block (20 ms).
        max_pause caps the silences of each segment's PCM before its join, one call per segment."""
        check_sampling(args)
        stages, rate = self._stages(sample_rate, tempo, loudness, pitch_shift, watermark)
        shaper = self.pause_shaper(max_pause)
        joiner = self.joiner(trim, keep, fade)
        plan = self._long_submit(args, segment_tokens, pauses)
        if plan is None:
            yield LongSpeech.make(np.zeros(rate, dtype=np.float32), None, [])
            return
        segs, tickets, limit = plan
        streams = [stream() for _, stream in stages]
        held, started, voice, waited = [], False, None, 0
        try:
            for i, (sg, t) in enumerate(zip(segs, tickets)):
                r, st = self.manager.wait_status(t)
                waited = i + 1
                rec = self._long_record(sg, r, st, limit)
                good = st == 0 and bool(r[0] or r[1])
                if good and voice is None and r[0]:
                    voice = list(r[0])
                pcm = self.codec.decode_audio_batch([r if st == 0 else ([], [])])[0]
                if shaper is not None:
                    pcm = self._long_shape(shaper, max_pause, [pcm], [rec])[0]
                piece, ((rec["a"], rec["b"]),) = joiner.join([pcm], [sg.pause_ms * (SAMPLE_RATE // 1000)])
                last = i + 1 == len(segs)
                if not started and not good:
                    held.append((piece, rec))
                    continue
                for k, (p, rc) in enumerate(held + [(piece, rec)]):
                    yield LongSpeech.make(feed_stages(streams, p, last and k == len(held)), voice, [rc])
                held, started = [], True
            if not started:
                yield LongSpeech.make(np.zeros(rate, dtype=np.float32), voice, [rc for _, rc in held])
        finally:
            for t in tickets[waited:]:  # (a stream left early: the tickets are released once the requests finish)
                self.manager.wait_status(t)
