"""rwkvtts -- MI355X-native RWKV-TTS hot path (host mirror of liuzl/rwkv-tts-rs's runtime,
sampler and batch-manager interfaces over the C-ABI in include/rwkvtts.h)."""
from . import _ffi  # noqa: F401
from ._ffi import (EOS_TOKEN, GLOBAL_TOKEN_OFFSET, HOP, N_GLOBAL, SAMPLE_RATE, SEMANTIC_LIMIT,  # noqa: F401
                   SPECIAL_TOKEN_OFFSET, TAG_0, TAG_1, TAG_2, RwkvTtsError)
from .properties import convert_standard_properties_to_tokens  # noqa: F401
from .runtime import (DynamicBatchConfig, DynamicBatchManager, LayeredRandomnessConfig, RnnInput,  # noqa: F401
                      Mirostat, Penalties, PhaseSampling, RnnInputBatch, RnnOption, SamplerArgs, SharedRwkvRuntime, StdRng, TtsBatchRequest,
                      sample_logits_with_top_p_k)
from . import weights  # noqa: F401
# streaming (audio during decode): BiCodecDetokenizer.halo / decode_windows, SharedRwkvRuntime.generate_batch(on_tokens=),
# DynamicBatchManager.stream_tts, LightweightTtsPipeline.stream_speech, server.handle_tts_stream
from .codec import BiCodecDetokenizer, codec_halo, window_plan  # noqa: F401
from .pipeline import LightweightTtsPipeline, LightweightTtsPipelineArgs, SpeechChunk  # noqa: F401
# long-form synthesis: TtsBatchRequest.pinned_voice, segment.split_text, audio.Joiner,
# LightweightTtsPipeline.generate_long_speech / stream_long_speech, long_form in the HTTP bodies
from .pipeline import LongSpeech  # noqa: F401
from .segment import Pauses, Segment, split_text  # noqa: F401
