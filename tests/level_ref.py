"""The numpy restatement of the leveller's arithmetic contract (include/rwkvtts.h):
what csrc/level.hip must equal bit for bit, and the stand-in evaluator of audio.Leveller. Every f32
operation below is one numpy f32 operation, so each is rounded once; the FIR adds tap by tap in
ascending order over whole arrays; numpy's f32 divide and sqrt are correctly rounded."""
import math

import numpy as np

F32 = np.float32

DEFAULTS = dict(block=1600, taps=1024, lookahead=4, gate=1e-5, ceiling=0.891, g_min=0.1, g_max=10.0, horizon=0)


def biquads(fs):
    """((b, a) of the shelf, (b, a) of the high-pass) at rate fs, in the header's order of operations."""
    out = []
    for f0, Q, G in ((1681.974450955533, 0.7071752369554196, 3.999843853973347),
                     (38.13547087602444, 0.5003270373238773, None)):
        K = math.tan(math.pi * f0 / fs)
        KQ, KK = K / Q, K * K
        a0 = (1.0 + KQ) + KK
        if G is not None:
            Vh = math.pow(10.0, G / 20.0)
            Vb = math.pow(Vh, 0.4996667741545416)
            b = [((Vh + Vb * KQ) + KK) / a0, (2.0 * (KK - Vh)) / a0, ((Vh - Vb * KQ) + KK) / a0]
        else:
            b = [1.0, -2.0, 1.0]
        out.append((b, [1.0, (2.0 * (KK - 1.0)) / a0, ((1.0 - KQ) + KK) / a0]))
    return out


def _df1(b, a, x):
    y, x1, x2, y1, y2 = [], 0.0, 0.0, 0.0, 0.0
    for v in x:
        t = b[0] * v
        t = t + b[1] * x1
        t = t + b[2] * x2
        t = t - a[1] * y1
        t = t - a[2] * y2
        x2, x1, y2, y1 = x1, v, y1, t
        y.append(t)
    return y


def table(L, B, fs=16000.0):
    """h[0, L) then r[0, B)."""
    (sb, sa), (hb, ha) = biquads(fs)
    h = _df1(hb, ha, _df1(sb, sa, [1.0] + [0.0] * (L - 1)))
    r = (np.arange(1, B + 1, dtype=np.float64) / float(B))
    return np.concatenate([np.array(h, dtype=np.float64).astype(F32), r.astype(F32)])


def target(loudness_db):
    return F32(math.pow(10.0, (float(loudness_db) + 0.691) / 10.0))


def _read(x, lo, count):
    """x[lo : lo + count] with +0 outside [0, n)."""
    out = np.zeros(count, dtype=F32)
    a, b = max(lo, 0), min(lo + count, x.size)
    if b > a:
        out[a - lo:b - lo] = x[a:b]
    return out


def measure(x, h, B, k0, k1):
    """(E, pk) of blocks [k0, k1) of the signal x, which ends at x.size."""
    L = h.size
    cnt = (k1 - k0) * B
    xp = _read(x, k0 * B - (L - 1), cnt + L - 1)
    z = np.zeros(cnt, dtype=F32)
    with np.errstate(all="ignore"):
        for k in range(L):  # ascending taps, from +0: one rounded multiply, one rounded add each
            z = z + h[k] * xp[L - 1 - k:L - 1 - k + cnt]
        live = max(0, min(cnt, x.size - k0 * B))
        z[live:] = 0.0
        sq = (z * z).reshape(k1 - k0, B // 64, 64)
        p = np.zeros((k1 - k0, 64), dtype=F32)
        for m in range(B // 64):  # p[l]: ascending i = l (mod 64), from +0
            p = p + sq[:, m, :]
        s = 32
        while s >= 1:
            p[:, :s] = p[:, :s] + p[:, s:2 * s]
            s //= 2
    pk = np.abs(xp[L - 1:]).reshape(k1 - k0, B).max(axis=1) if cnt else np.zeros(0, dtype=F32)
    return p[:, 0].copy(), pk.astype(F32)


class Scan:
    """The gain scan's carried state (S, N) and its rules."""

    def __init__(self, t2, gate, C, g_min, g_max, H, S=0.0, N=0):
        self.t2, self.gate, self.C, self.g_min, self.g_max, self.H = F32(t2), F32(gate), F32(C), F32(g_min), F32(g_max), int(H)
        self.S, self.N = F32(S), int(N)

    def enter(self, P):
        if P >= self.gate:
            if self.H == 0 or self.N < self.H:
                self.S = F32(self.S + P)
                self.N += 1
            else:
                self.S = F32(F32(self.S - F32(self.S / F32(self.H))) + P)

    def gain(self, pk_a, pk_b):
        with np.errstate(all="ignore"):
            g = F32(1.0) if self.N == 0 else F32(np.sqrt(F32(self.t2 / F32(self.S / F32(self.N)))))
            if g < self.g_min:
                g = self.g_min
            if g > self.g_max:
                g = self.g_max
            p = pk_a if pk_a > pk_b else pk_b
            if F32(g * p) > self.C:
                g = F32(self.C / p)
        return g


def run(x, in_first, final, t2, c, S, N, g_prev, count, h, r, A, gate, C, g_min, g_max, H):
    """Blocks from c on, `count` samples, of the signal whose samples from in_first on are x:
    -> (y, S, N, g_last). Samples before in_first are never read (zeros stand in for them)."""
    B, L = r.size, h.size
    n = in_first + x.size
    full = np.concatenate([np.zeros(in_first, dtype=F32), x])
    cnt = -(-count // B)
    last = (-(-n // B) if final else n // B) - 1
    e0 = 0 if c == 0 else max(0, c + A - 3)
    p0 = 0 if c == 0 else c + A
    m1 = min(c + cnt - 1 + A, last)
    assert m1 >= c
    E = {}
    if m1 >= e0:
        Ev, _ = measure(full, h, B, e0, m1 + 1)
        E = {e0 + i: v for i, v in enumerate(Ev)}
    _, pkv = measure(full, h[:1], B, c, m1 + 1)
    pk = {c + i: v for i, v in enumerate(pkv)}
    den = F32(4 * B)
    sc = Scan(t2, gate, C, g_min, g_max, H, 0.0 if c == 0 else S, 0 if c == 0 else N)
    g = [F32(g_prev)]
    nxt = p0
    for j in range(c, c + cnt):
        while nxt <= min(j + A, last):
            s = F32(0.0)
            for d in (3, 2, 1, 0):
                s = F32(s + (E[nxt - d] if nxt - d >= 0 else F32(0.0)))
            sc.enter(F32(s / den))
            nxt += 1
        gj = sc.gain(pk[j], pk[j + 1] if j + 1 <= last else F32(0.0))
        if j == 0:
            g[0] = gj
        g.append(gj)
    g = np.array(g, dtype=F32)
    xs = _read(full, c * B, cnt * B).reshape(cnt, B)
    with np.errstate(all="ignore"):
        gi = g[:-1, None] + (g[1:, None] - g[:-1, None]) * r[None, :]
        y = (xs * gi).reshape(-1)[:count]
    return y.astype(F32), F32(sc.S), int(sc.N), F32(g[-1])


def _params(kw):
    p = dict(DEFAULTS)
    p.update({k: v for k, v in kw.items() if v})
    return p


def level(x, loudness_db, return_gains=False, **kw):
    """The whole-signal result."""
    p = _params(kw)
    x = np.ascontiguousarray(x, dtype=F32).reshape(-1)
    if x.size == 0:
        return x.copy()
    t = table(p["taps"], p["block"])
    h, r = t[:p["taps"]], t[p["taps"]:]
    y, S, N, g = run(x, 0, True, target(loudness_db), 0, 0.0, 0, 1.0, x.size, h, r, p["lookahead"], p["gate"],
                     p["ceiling"], p["g_min"], p["g_max"], p["horizon"])
    return (y, (S, N, g)) if return_gains else y


def evaluator(lv, items):
    """Leveller(evaluator=...): the native window call restated. A window must lie inside its plan
    (asserted), as the library checks before it launches anything."""
    outs = []
    h, r = lv.table[:lv.taps], lv.table[lv.taps:]
    for x, in_first, final, t2, c, S, N, g_prev, count in items:
        if count == 0:
            outs.append((np.zeros(0, dtype=F32), F32(S), int(N), F32(g_prev)))
            continue
        end, first = lv.plan(in_first + x.size, final, c)
        assert c * lv.block + count <= end and in_first <= first, "window outside its plan"
        assert count % lv.block == 0 or (final and c * lv.block + count == in_first + x.size)
        outs.append(run(x, in_first, final, t2, c, S, N, g_prev, count, h, r, lv.lookahead, lv.gate, lv.ceiling,
                        lv.g_min, lv.g_max, lv.horizon))
    return outs
