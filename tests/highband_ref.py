"""The numpy restatement of the high-band stage's arithmetic contract (include/rwkvtts.h, DESIGN.md
§40): what csrc/highband.hip must equal bit for bit. Every f32 operation below is one numpy f32
operation, so each is rounded once; every FIR adds tap by tap in ascending order over whole arrays;
numpy's f32 divide is correctly rounded. With dtype=np.float64 the same chain runs in double over
the same (f32-rounded) table: the float64 restatement the kernels' error is measured against."""
import math

import numpy as np

from rwkvtts.audio import _highband_table as table  # hp[31], ip[32], sh[63], r[320]: one source, as the resampler's

F32 = np.float32
HP_T, IP_T, SH_T, B = 31, 32, 63, 160   # taps of HP4, the interpolator and SH; input samples per block
DEFAULTS = dict(level_db=-6.0, r_lo=0.02, r_hi=0.2, floor=1e-6)


def split(tab):
    return tab[:HP_T], tab[HP_T:HP_T + IP_T], tab[HP_T + IP_T:HP_T + IP_T + SH_T], tab[HP_T + IP_T + SH_T:]


def gain_of(highband_db, level_db=DEFAULTS["level_db"]):
    return F32(math.pow(10.0, (float(level_db) + float(highband_db)) / 20.0))


def fir(x, h, lead):
    """y[n] = sum_k h[k] * x[n + lead - k], ascending k from +0; x outside [0, n) reads +0."""
    n, T = x.size, h.size
    xp = np.zeros(n + T - 1, dtype=x.dtype)
    xp[T - 1 - lead:T - 1 - lead + n] = x
    y = np.zeros(n, dtype=x.dtype)
    for k in range(T):
        y = y + h[k] * xp[T - 1 - k:T - 1 - k + n]
    return y


def energy(x):
    """Per block of B samples (zeros past the end): 64 partials over i = l (mod 64) ascending from +0,
    then p[l] += p[l + s] for l < s, s = 32 .. 1."""
    nb = -(-x.size // B)
    sq = np.zeros(nb * 192, dtype=x.dtype).reshape(nb, 192)
    xs = np.zeros(nb * B, dtype=x.dtype)
    xs[:x.size] = x
    sq[:, :B] = (xs * xs).reshape(nb, B)
    p = np.zeros((nb, 64), dtype=x.dtype)
    for m in range(3):
        p = p + sq[:, 64 * m:64 * m + 64]
    s = 32
    while s >= 1:
        p[:, :s] = p[:, :s] + p[:, s:2 * s]
        s //= 2
    return p[:, 0].copy()


def block_gains(x, b, G, r_lo, r_hi, floor):
    """g_j = G * s(Pb_j / Px_j) of every block, in x's dtype."""
    dt = x.dtype.type
    Pb, Px = energy(b), energy(x)
    lo, hi, three, two = dt(F32(r_lo)), dt(F32(r_hi)), dt(3.0), dt(2.0)
    g = np.zeros(Pb.size, dtype=x.dtype)
    for j in range(Pb.size):
        r = dt(0.0) if Px[j] < dt(F32(floor)) else dt(Pb[j] / Px[j])
        if r <= lo:
            s = dt(0.0)
        elif r >= hi:
            s = dt(1.0)
        else:
            t = dt(dt(r - lo) / dt(hi - lo))
            s = dt(dt(t * t) * dt(three - dt(two * t)))
        g[j] = dt(dt(G) * s)
    return g


def highband(x, highband_db=0.0, tab=None, dtype=F32, parts=False, **kw):
    """The whole-signal result: 2 * x.size samples at 32 kHz (parts: also u, w and the per-sample gain)."""
    p = dict(DEFAULTS)
    p.update(kw)
    x = np.ascontiguousarray(x, dtype=F32).reshape(-1).astype(dtype)
    n = x.size
    hp, ip, sh, ramp = (t.astype(dtype) for t in split(table() if tab is None else tab))
    with np.errstate(all="ignore"):
        b = fir(x, hp, 15)
        u = np.zeros(2 * n, dtype=dtype)
        u[0::2], u[1::2] = x, fir(x, ip, 16)
        v = np.zeros(2 * n, dtype=dtype)
        v[0::2], v[1::2] = b, -fir(b, ip, 16)
        w = fir(v, sh, 31)
        if n == 0:
            return (u, u, w, w) if parts else u
        g = block_gains(x, b, gain_of(highband_db, p["level_db"]), p["r_lo"], p["r_hi"], p["floor"])
        ga = np.concatenate([g[:1], g[:-1]])
        gain = (ga[:, None] + (g - ga)[:, None] * ramp[None, :]).reshape(-1)[:2 * n]
        y = np.where(gain == 0, u, u + gain * w)
    return (y, u, w, gain) if parts else y
