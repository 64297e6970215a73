"""LoRA adapters (include/rwkvtts.h "adapters") for the tests: a seeded adapter and the float64 model
whose six target matrices per layer have s * B @ A added."""
import numpy as np

import rwkv7_f64
from rwkvtts import weights as W

TARGET_TENSORS = (W.L_WR, W.L_WK, W.L_WV, W.L_WO, W.L_FFN_K, W.L_FFN_V)


def draw(dims, rank, seed, targets=range(6), scale=1.0):
    """(state dict for weights.pack_adapter, alpha). Every value is a bf16 number. s * B @ A has
    `scale` times the standard deviation of the synthetic base matrices (0.02): at 1 the adapter
    moves the logits by about as much as the base weights do."""
    rng = np.random.RandomState(seed)
    sd = {}
    for layer in range(dims["n_layer"]):
        for t in targets:
            N, K = W.adapter_target_shape(dims, t)
            for key, shape in (("lora_A", (rank, K)), ("lora_B", (N, rank))):
                v = (0.05 * rng.standard_normal(shape)).astype(np.float32)
                sd[f"blocks.{layer}.{W.ADAPTER_TARGETS[t]}.{key}"] = W.bf16_bits_to_f32(W.f32_to_bf16_bits(v))
    return sd, 8.0 * scale * rank ** 0.5


def model(blob, dims, sd, alpha):
    """rwkv7_f64.Model of `blob` with the adapter folded into its float64 matrices."""
    m = rwkv7_f64.Model(blob)
    for key in [k for k in sd if k.endswith("lora_A")]:
        _, layer, mod, name, _ = key.split(".")
        a = sd[key].astype(np.float64)
        b = sd[key[:-1] + "B"].astype(np.float64)
        s = float(np.float32(alpha / a.shape[0]))
        m.layers[int(layer)][TARGET_TENSORS[W.ADAPTER_TARGETS.index(f"{mod}.{name}")]] += s * (b @ a)
    return m
