"""The powf of the sampler's temperature step (csrc/exact_math.h glibc_powf) is bit-identical to
glibc powf, which is what Rust's f32::powf calls on Linux (src/rwkv_sampler.rs:156-171), on the
domain the sampler presents: x in (0, 1], subnormals included, y = 1.0f / T. CPU check of the same
source via the library's host hook; the exhaustive sweep over every positive float up to 1.0 at
these y (12 x 1.07e9 values, 0 mismatches) was run once with tools/powf_sweep.c and is repeated on a
strided subset here."""
import ctypes

import numpy as np

from rwkvtts import _ffi

TEMPS = (0.1, 0.25, 0.5, 0.7, 0.8, 0.9, 1.1, 1.25, 1.5, 2, 3, 4)


def _underflow_straddle(libm_powf, y):
    """The largest x with powf(x, y) == 0 and its successor (bisection on the bit pattern: powf
    is monotone in x)."""
    lo, hi = 1, 0x3F800000  # powf(lo) == 0, powf(hi) == 1
    assert libm_powf(np.array([lo], np.uint32).view(np.float32)[0], y) == 0.0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if libm_powf(np.array([mid], np.uint32).view(np.float32)[0], y) == 0.0:
            lo = mid
        else:
            hi = mid
    return lo, hi


def test_powf_matches_glibc_strided():
    L = _ffi.lib()
    f = L.rwkvtts_debug_powf
    f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    f.restype = None
    libm = ctypes.CDLL("libm.so.6")
    libm.powf.argtypes = [ctypes.c_float, ctypes.c_float]
    libm.powf.restype = ctypes.c_float
    ref = np.frompyfunc(lambda a, b: libm.powf(a, b), 2, 1)  # the library side over whole arrays

    y10 = np.float32(1.0) / np.float32(0.1)
    lo, hi = _underflow_straddle(libm.powf, y10)
    # every 4099th positive bit pattern up to 1.0, plus edge values
    bits = np.arange(1, 0x3F800001, 4099, dtype=np.uint64).astype(np.uint32)
    edge = np.array([0x3F800000,           # 1.0
                     0x007FFFFF,           # the largest subnormal
                     0x00800000,           # the smallest normal
                     0x3F7FFFFF,           # nextafter(1, 0)
                     lo - 1, lo, hi, hi + 1,  # around the underflow threshold for y = 10
                     1], dtype=np.uint32)
    xs = np.concatenate([bits, edge]).view(np.float32)
    assert (xs > 0).all() and (xs <= 1).all()
    bad = []
    for T in TEMPS:
        y = np.float32(1.0) / np.float32(T)
        ys = np.full(xs.shape, y, dtype=np.float32)
        got = np.empty_like(xs)
        f(xs.ctypes.data_as(ctypes.c_void_p), ys.ctypes.data_as(ctypes.c_void_p), len(xs),
          got.ctypes.data_as(ctypes.c_void_p))
        want = ref(xs, ys).astype(np.float32)
        ne = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
        bad += [(T, float(xs[i]), float(got[i]), float(want[i])) for i in ne[:3]]
    assert not bad, bad[:6]
    # the straddle really straddles: results on both sides of the underflow exit were compared
    assert libm.powf(xs[len(bits) + 5], y10) == 0.0 and libm.powf(xs[len(bits) + 6], y10) > 0.0
