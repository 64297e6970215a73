"""The numpy restatement of the limiter's arithmetic contract (include/rwkvtts.h): what
csrc/limit.hip must equal bit for bit. Every f32 operation below is one numpy f32 operation, so each is
rounded once; the FIRs and the box add term by term in ascending order over whole arrays; numpy's f32
divide is correctly rounded. With dtype=np.float64 the same chain runs in double over the same
(f32-rounded) table and ceiling: the high-precision reference."""
import math

import numpy as np

from rwkvtts.audio import _limit_table as table  # h_1[12], h_2[12], h_3[12]: one source, as the resampler's

F32 = np.float32
TAPS, HALF, PRE, POST = 12, 32, 69, 70   # taps per phase; reach of the minimum and of the box; the stage's reach


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def ceiling(limit_db):
    return F32(math.pow(10.0, float(limit_db) / 20.0))


def limit(x, limit_db=0.0, tab=None, dtype=F32, c=None):
    """The whole-signal result (c: a ceiling given directly, as a window carries it)."""
    x = np.ascontiguousarray(x, dtype=F32).reshape(-1).astype(dtype)
    n, dt = x.size, np.dtype(dtype).type
    c = dt(ceiling(limit_db) if c is None else F32(c))
    h = (table() if tab is None else tab).astype(dtype).reshape(3, TAPS)
    xp = np.zeros(n + TAPS - 1, dtype=dtype)   # xp[i] = x[i - 5]
    xp[5:5 + n] = x
    p = np.abs(x)
    for q in range(3):
        v = np.zeros(n, dtype=dtype)
        for k in range(TAPS):
            v = v + h[q, k] * xp[k:k + n]
        p = np.maximum(p, np.abs(v))
    rp = np.ones(n + 4 * HALF, dtype=dtype)    # rp[i] = r[i - 64], 1 outside the signal
    over = p > c
    rp[2 * HALF:2 * HALF + n][over] = c / p[over]
    m = np.ones(n + 2 * HALF, dtype=dtype)     # m[i] = the minimum at position i - 32
    for j in range(2 * HALF + 1):
        m = np.minimum(m, rp[j:j + n + 2 * HALF])
    s = np.zeros(n, dtype=dtype)
    for j in range(2 * HALF + 1):
        s = s + m[j:j + n]
    g = s / dt(2 * HALF + 1)
    return np.minimum(np.maximum(x * g, -c), c)


def evaluator(limiter, items):
    """Stands in for rwkvtts_limit_windows: a window's samples as a signal of their own (what lies before
    in_first is out of every wanted output's reach, what follows a window is unknown), after the plan's
    two checks."""
    out = []
    for x, in_first, final, c, out_first, count in items:
        end = in_first + x.size
        assert out_first + count <= (end if final else max(0, end - POST)) and in_first <= max(0, out_first - PRE)
        out.append(limit(x, c=c, tab=limiter.table)[out_first - in_first:out_first - in_first + count])
    return out


def burst(n, scale=1.0):
    """Sine bursts up to amplitude 1.6 until sample 1100 and a quiet 0.3 after it, with single-sample
    spikes at 0, n - 1, 1023 and 1024."""
    i = np.arange(n)
    amp = np.where(((i // 300) % 2 == 0) & (i < 1100), 1.6 * np.sin(np.pi * (i % 300) / 300.0) ** 2, 0.3)
    x = amp * np.sin(2.0 * np.pi * 0.11 * i + 0.3)
    for k in (0, n - 1, 1023, 1024):
        if 0 <= k < n:
            x[k] = 1.5 if k % 2 else -1.5
    return (scale * x).astype(F32)
