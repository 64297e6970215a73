"""The numpy restatement of the equaliser's arithmetic contract (include/rwkvtts.h): what
csrc/eq.hip must equal bit for bit. The design runs in Python floats (doubles), one operation at a time in
the header's order; the FIR adds tap by tap in ascending k over whole arrays, every f32 operation one numpy
f32 operation, so each is rounded once."""
import math

import numpy as np

F32 = np.float32
FS, IMPULSE, STEP, MAX_TAPS = 16000.0, 8192, 64, 4096


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def biquad(kind, freq, gain, q):
    """(b0, b1, b2, a1, a2) / a0 of one cookbook band."""
    w = 2.0 * math.pi * freq / FS
    cs, al = math.cos(w), math.sin(w) / (2.0 * q)
    if kind in ("lowpass", "highpass"):
        u = 1.0 - cs if kind == "lowpass" else 1.0 + cs
        b, a = (u / 2.0, u if kind == "lowpass" else -u, u / 2.0), (1.0 + al, -2.0 * cs, 1.0 - al)
    else:
        A = math.pow(10.0, gain / 40.0)
        if kind == "peak":
            b, a = (1.0 + al * A, -2.0 * cs, 1.0 - al * A), (1.0 + al / A, -2.0 * cs, 1.0 - al / A)
        else:
            be = 2.0 * math.sqrt(A) * al
            lo, hi = (A + 1.0) - (A - 1.0) * cs, (A + 1.0) + (A - 1.0) * cs
            if kind == "lowshelf":
                b = (A * (lo + be), 2.0 * A * ((A - 1.0) - (A + 1.0) * cs), A * (lo - be))
                a = (hi + be, -2.0 * ((A - 1.0) + (A + 1.0) * cs), hi - be)
            else:
                b = (A * (hi + be), -2.0 * A * ((A - 1.0) + (A + 1.0) * cs), A * (hi - be))
                a = (lo + be, 2.0 * ((A - 1.0) - (A + 1.0) * cs), lo - be)
    return b[0] / a[0], b[1] / a[0], b[2] / a[0], a[1] / a[0], a[2] / a[0]


def design(bands):
    """-> (taps h[0, N) in f32, sum |h64|), or ValueError if the response rings past 4096 taps."""
    v = [1.0] + [0.0] * (IMPULSE - 1)
    for band in bands:
        b0, b1, b2, a1, a2 = biquad(*band)
        y, x1, x2, y1, y2 = [], 0.0, 0.0, 0.0, 0.0
        for x in v:
            t = b0 * x
            t = t + b1 * x1
            t = t + b2 * x2
            t = t - a1 * y1
            t = t - a2 * y2
            x2, x1, y2, y1 = x1, x, y1, t
            y.append(t)
        v = y
    h64 = np.array(v, dtype=np.float64)
    tail = np.concatenate([np.cumsum(np.abs(h64)[::-1])[::-1], [0.0]])  # summed from the far end
    for n in range(STEP, MAX_TAPS + 1, STEP):
        if tail[n] <= tail[0] * 2.0 ** -24:
            return h64[:n].astype(F32), float(tail[0])
    raise ValueError("the filter rings past 4096 taps")


def fir(x, h):
    """y[n] = the sequential f32 sum of h[k] * x[n - k], ascending k from +0, x = 0 before the signal."""
    x, h = np.ascontiguousarray(x, dtype=F32).reshape(-1), np.ascontiguousarray(h, dtype=F32)
    xp = np.concatenate([np.zeros(h.size - 1, dtype=F32), x])  # xp[i] = x[i - (N - 1)]
    acc = np.zeros(x.size, dtype=F32)
    for k in range(h.size):
        acc = acc + h[k] * xp[h.size - 1 - k:h.size - 1 - k + x.size]
    return acc


def evaluator(eq, items, table):
    """Stands in for rwkvtts_eq_windows: a window's samples as a signal of their own (what lies before
    in_first is out of every wanted output's reach), after the plan's two checks."""
    out = []
    for x, in_first, final, s, out_first, count in items:
        assert out_first + count <= in_first + x.size and in_first <= max(0, out_first - (table[s].size - 1))
        out.append(fir(x, table[s])[out_first - in_first:out_first - in_first + count])
    return out
