"""CPU checks of the MXFP6 (E2M3, E3M2) and MXINT8 quant types: the config helpers, and one hand-worked
block per format through the numpy reference (a tie each way, a subnormal, the saturation, the e_min clamp)."""
import numpy as np
import pytest

import mx_ref
from rwkvtts import runtime
from rwkvtts import weights as W

# include/rwkvtts.h: (emax of the element, mantissa bits, smallest normal exponent, saturation, e_min)
OCP = {"mxfp6_e2m3": (2, 3, 0, 7.5, -123), "mxfp6_e3m2": (4, 2, -2, 28.0, -122), "mxint8": (0, 6, 0, 127 / 64, -120)}
mx_ref.FORMATS.update(OCP)

T = 2.0 ** -127
# per format: (block, expected) pairs. Block 0 has a power-of-two maximum (e = 0): a tie down, a tie up, the
# subnormal ties; block 1 rounds past the largest element; block 2 lies under the clamp (e = e_min).
CLAMP = ([4 * T, 2 * T, T, 3 * T], [4 * T, 2 * T, 0, 4 * T])
BLOCKS = {
    "mxfp6_e2m3": [([4, 1.0625, 1.1875, 0.0625, 0.1875, -0.3125], [4, 1, 1.25, 0, 0.25, -0.25]),
                   ([7.875, 7.75, -7.25], [7.5, 7.5, -7.0]), CLAMP],
    "mxfp6_e3m2": [([16, 1.125, 1.375, 0.03125, 0.09375, -0.15625], [16, 1, 1.5, 0, 0.125, -0.125]),
                   ([30, 31, -26], [28, 28, -24]), CLAMP],
    "mxint8": [([1, 193 / 128, 3 / 128, 1 / 128, -5 / 128, -1 / 256], [1, 1.5, 2 / 64, 0, -2 / 64, -0.0]),
               ([255 / 128, -253 / 128, 1.75], [127 / 64, -126 / 64, 1.75]), CLAMP],
}


@pytest.mark.parametrize("name,code", [("mxfp6_e2m3", 6), ("MXFP6_E3M2", 7), ("MxInt8", 8), ("mxfp6", 6)])
def test_parse(name, code):
    assert runtime.parse_quant_type(name) == code


def test_quant_config():
    assert runtime.quant_config(3, "mxint8") == (3, 8)


@pytest.mark.parametrize("fmt", list(OCP))
def test_reference_blocks(fmt):
    v = np.zeros((1, 96), np.float32)
    want = np.zeros((1, 96), np.float32)
    for i, (block, expected) in enumerate(BLOCKS[fmt]):
        v[0, 32 * i:32 * i + len(block)] = block
        want[0, 32 * i:32 * i + len(block)] = expected
    bits = W.f32_to_bf16_bits(v)
    assert (W.bf16_bits_to_f32(bits) == v).all(), "not bf16 numbers"
    got = W.bf16_bits_to_f32(mx_ref.dequantised(bits, fmt))
    assert got.tolist() == want.tolist() and (np.signbit(got) == np.signbit(want)).all()
