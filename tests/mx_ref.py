"""OCP Microscaling weight quantisation (include/rwkvtts.h, RWKVTTS_QUANT_MXFP8 / MXFP4), restated
in numpy float64: bf16 bit patterns in, the dequantised weights' bf16 bit patterns out."""
import numpy as np

# type -> (emax of the element, mantissa bits, smallest normal exponent, saturation, e_min)
FORMATS = {"mxfp8": (8, 3, -6, 448.0, -117), "mxfp4": (2, 1, 0, 6.0, -125)}


def bf16_to_f64(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def dequantised(bits, fmt):
    """[N][K] uint16 (bf16 bits, finite, K % 32 == 0) -> [N][K] uint16: steps 1-4 of the contract."""
    emax, mbits, emin_el, sat, e_min = FORMATS[fmt]
    bits = np.asarray(bits, dtype=np.uint16)
    v = bf16_to_f64(bits).reshape(bits.shape[0], -1, 32)
    amax = np.abs(v).max(axis=2, keepdims=True)                       # 1. block maximum
    floor_log2 = np.frexp(np.where(amax > 0, amax, 1.0))[1] - 1       # amax = m 2^x, m in [.5, 1)
    e = np.where(amax > 0, np.clip(floor_log2 - emax, e_min, 127), e_min)  # 2. scale exponent
    a = np.ldexp(np.abs(v), -e)                                       # 3. |q|, exact
    ex = np.maximum(np.frexp(np.where(a > 0, a, 1.0))[1] - 1, emin_el)
    step = np.ldexp(1.0, ex - mbits)                                  # the element grid around |q|
    r = np.minimum(np.rint(a / step) * step, sat)                     # rint: ties to even (mantissa)
    w = np.copysign(np.ldexp(r, e), v).astype(np.float32)             # 4. exact: zero or a bf16 normal
    out = w.view(np.uint32).reshape(bits.shape)
    assert not (out & 0xFFFF).any()
    return (out >> 16).astype(np.uint16)


def dequantised_blob(blob, dims, fmt, n_layers):
    """A copy of a bf16 weight blob (dims: its dims dict) whose layers [0, n_layers) hold the
    dequantised r / k / v / o and FFN key / value matrices."""
    from rwkvtts import weights as W
    out = blob.copy()
    for layer, t, off, rows, cols, _ in W.layout(dims)[0]:
        if 0 <= layer < n_layers and t in (W.L_WR, W.L_WK, W.L_WV, W.L_WO, W.L_FFN_K, W.L_FFN_V):
            m = out[off:off + 2 * rows * cols].view(np.uint16).reshape(rows, cols)
            m[:] = dequantised(m, fmt)
    return out
