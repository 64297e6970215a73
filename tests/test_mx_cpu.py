"""CPU checks of the Microscaling quant types: the config helpers and the numpy reference's rounding."""
import numpy as np
import pytest

import mx_ref
from rwkvtts import _ffi, runtime
from rwkvtts import weights as W


@pytest.mark.parametrize("name,code", [("mxfp8", 4), ("MXFP4", 5), ("MxFp8", 4)])
def test_parse_mx(name, code):
    assert runtime.parse_quant_type(name) == code
    assert (_ffi.QUANT_MXFP8, _ffi.QUANT_MXFP4) == (4, 5)


def test_quant_config_mx():
    assert runtime.quant_config(12, "mxfp4") == (12, _ffi.QUANT_MXFP4)
    assert runtime.quant_config(0, "mxfp8") == (0, _ffi.QUANT_NONE)


def test_reference_rounding():
    """MXFP4, amax 5 -> e = 0: the midpoints go to the even mantissa; a block under 2^-123 clamps e."""
    v = np.zeros((1, 64), np.float32)
    v[0, :8] = [5, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, -0.25]
    v[0, 32:35] = [2.0 ** -125, 2.0 ** -126, 2.0 ** -127]
    got = W.bf16_bits_to_f32(mx_ref.dequantised(W.f32_to_bf16_bits(v), "mxfp4"))
    assert got[0, :8].tolist() == [4, 0, 1, 1, 2, 2, 4, -0.0] and np.signbit(got[0, 7])
    assert got[0, 32:35].tolist() == [2.0 ** -125, 2.0 ** -126, 0]
