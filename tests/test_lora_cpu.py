"""LoRA adapters without a GPU: weights.pack_adapter's header, mask, scale and matrix order
(include/rwkvtts.h "adapters"), and the `adapter` field of both HTTP bodies."""
import dataclasses
import json
import types

import numpy as np
import pytest

from rwkvtts import server as SV
from rwkvtts import weights as W
from rwkvtts.pipeline import SpeechChunk

DIMS = dict(W.DIMS_TINY, n_layer=2, n_embd=128, n_ffn=256)


def _sd(rank, targets):
    sd = {}
    for layer in range(DIMS["n_layer"]):
        for t in targets:
            N, K = W.adapter_target_shape(DIMS, t)
            name = f"blocks.{layer}.{W.ADAPTER_TARGETS[t]}"
            sd[name + ".lora_A"] = np.full((rank, K), 1 + layer + t / 8, np.float32)   # bf16 numbers
            sd[name + ".lora_B"] = np.full((N, rank), -(1 + layer + t / 8), np.float32)
    return sd


@pytest.mark.parametrize("rank,targets", [(16, (0, 1, 2, 3, 4, 5)), (48, (1, 5))])
def test_pack_adapter_layout(rank, targets):
    blob = W.pack_adapter(_sd(rank, targets), DIMS, alpha=24.0)
    hdr = blob[:64].view(np.uint32)
    assert hdr[:7].tolist() == [0x41524F4C, 1, 2, 128, 256, rank, sum(1 << t for t in targets)]
    assert blob[28:32].view(np.float32)[0] == np.float32(24.0 / rank) and not hdr[8:].any()
    body, at = blob[64:].view(np.uint16), 0
    for layer in range(2):
        for t in targets:
            N, K = W.adapter_target_shape(DIMS, t)
            for n, sign in ((rank * K, 1), (N * rank, -1)):
                want = W.f32_to_bf16_bits(np.float32(sign * (1 + layer + t / 8)))
                assert (body[at:at + n] == want).all(), (layer, t, sign)
                at += n
    assert at == body.size



class _Pipeline:
    """A stand-in pipeline whose manager has one adapter loaded; records the args of each call."""

    def __init__(self):
        self.manager, self.args = types.SimpleNamespace(adapters={"warm": 3}), []

    def generate_speech(self, args, **kw):
        self.args.append(args)
        return np.zeros(1600, np.float32)

    def stream_speech(self, args, chunk_frames=16, **kw):
        self.args.append(args)
        yield SpeechChunk.make(np.zeros(1600, np.float32), 0, 0, 0, True)


def test_http_bodies_carry_the_adapter():
    p = _Pipeline()
    for body in ({"text": "x", "adapter": "warm"}, {"text": "x"}):
        assert SV.handle_tts_json(dict(body), p)[0] == 200
        code, it = SV.handle_tts_stream(dict(body), p)
        assert code == 200 and len(list(it)) == 2
    assert [a.adapter for a in p.args] == ["warm", "warm", None, None]
    # without the field the args, and so the request, are what they were
    assert p.args[2] == SV._tts_args({"text": "x", "adapter": None}, "assets/raf")[1] == dataclasses.replace(p.args[0], adapter=None)
    p.args.clear()
    for bad in ("cold", "", 7):
        code, payload = SV.handle_tts_json({"text": "x", "adapter": bad}, p)
        code2, it = SV.handle_tts_stream({"text": "x", "adapter": bad}, p)
        assert code == code2 == 400 and json.loads(b"".join(it).decode("utf-8")) == payload and not payload["success"]
    assert p.args == []
