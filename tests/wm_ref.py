"""The numpy restatement of the watermark's contract (include/rwkvtts.h). The embedder
is what csrc/wm.hip must equal bit for bit: every f32 operation below is one numpy f32 operation, so
each is rounded once; the carrier adds tap by tap in ascending order over whole arrays; numpy's f32
divide and sqrt are correctly rounded. The detector is the float64 reference the kernels are held to
within the forward-error bound of their f32 sums: whitening, matched filter and fold in float64, the
search over every offset by FFT (a circular correlation per bit slot). Throughout, F2[m] = F[m]^2."""
import math

import numpy as np

F32 = np.float32
U64 = np.uint64

DEFAULTS = dict(block=320, taps=129, bits=16, bit_len=1600, band_lo=1000.0, band_hi=3400.0, strength_db=-26.0)
EPS = 2.0 ** -17   # the whitening floor
FS = 16000.0


def config(**kw):
    p = dict(DEFAULTS)
    p.update({k: v for k, v in kw.items() if v})
    p["period"] = p["bits"] * p["bit_len"]
    return p


# ---- table, strength, threshold ------------------------------------------------------------------
def table(L, B, lo, hi, fs=FS):
    """h[0, L) then r[0, B): the Blackman-windowed difference of two sincs at unit energy, the ramp."""
    k = np.arange(L, dtype=np.float64)
    t = k - float((L - 1) // 2)
    w = (0.42 - 0.5 * np.cos(2.0 * np.pi * k / float(L - 1))) + 0.08 * np.cos(4.0 * np.pi * k / float(L - 1))
    fh, fl = 2.0 * float(hi) / fs, 2.0 * float(lo) / fs
    g = w * (fh * np.sinc(fh * t) - fl * np.sinc(fl * t))
    h = g / math.sqrt(float(np.sum(g * g)))
    r = np.arange(1, B + 1, dtype=np.float64) / float(B)
    return np.concatenate([h, r]).astype(F32)


def strength(db):
    return F32(math.pow(10.0, float(db) / 20.0))


def chi2_sf(T, k):
    """Q(T; k), the upper tail of chi-square with k degrees of freedom: the closed forms."""
    x = 0.5 * T
    if k % 2 == 0:
        term, s = 1.0, 0.0
        for i in range(k // 2):
            s += term
            term *= x / (i + 1)
        return math.exp(-x) * s
    term, s = math.sqrt(x) / math.gamma(1.5), 0.0   # x^(i + 1/2) / Gamma(i + 3/2)
    for i in range((k - 1) // 2):
        s += term
        term *= x / (i + 1.5)
    return math.erfc(math.sqrt(x)) + math.exp(-x) * s


def threshold(NB, NP, alpha=1e-6):
    """The smallest T with NP * Q(T; NB) <= alpha, by bisection to a relative 1e-12."""
    lo, hi = 0.0, 1.0
    while NP * chi2_sf(hi, NB) > alpha:
        hi *= 2.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if NP * chi2_sf(mid, NB) > alpha:
            lo = mid
        else:
            hi = mid
    return hi


# ---- chips ---------------------------------------------------------------------------------------
def splitmix64(x):
    with np.errstate(over="ignore"):
        z = x + U64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
        return z ^ (z >> U64(31))


def chips(key, NP):
    """c(key, m) in {-1, +1}, m in [0, NP): +1 where the top bit of splitmix64(splitmix64(key) + m) is
    set (the inner hash keeps the sequences of neighbouring keys from being shifts of one another)."""
    with np.errstate(over="ignore"):
        top = splitmix64(splitmix64(U64(int(key) & (2 ** 64 - 1))) + np.arange(NP, dtype=U64)) >> U64(63)
    return np.where(top == 1, 1, -1).astype(np.int64)


def marked_chips(key, payload, NB, TB):
    """The chip of every phase of the period: c(key, m) times +1 / -1 for a set / clear payload bit."""
    NP = NB * TB
    data = np.array([1 if (int(payload) >> b) & 1 else -1 for b in range(NB)], dtype=np.int64)
    return chips(key, NP) * np.repeat(data, TB)


# ---- the embedder, op for op in f32 ----------------------------------------------------------------
def block_energy(xb):
    """E of whole blocks xb[blocks, B], as the leveller sums a block: 64 partials, then the tree."""
    nb, B = xb.shape
    with np.errstate(all="ignore"):
        sq = (xb * xb).reshape(nb, B // 64, 64)
        p = np.zeros((nb, 64), dtype=F32)
        for m in range(B // 64):
            p = p + sq[:, m, :]
        s = 32
        while s >= 1:
            p[:, :s] = p[:, :s] + p[:, s:2 * s]
            s //= 2
    return p[:, 0].copy()


def carrier(h, chip_period, n0, count):
    """u[n0, n0 + count): u[n] = sum_k h[k] * chip[n - k], ascending k from +0; chips periodic."""
    L, NP = h.size, chip_period.size
    idx = (np.arange(n0 - (L - 1), n0 + count, dtype=np.int64)) % NP
    c = chip_period[idx].astype(F32)
    u = np.zeros(count, dtype=F32)
    for k in range(L):
        u = u + h[k] * c[L - 1 - k:L - 1 - k + count]
    return u


def run(x, in_first, final, key, payload, s, c, a_prev, count, h, r, NB, TB):
    """Blocks from c on, `count` samples, of the signal whose samples from in_first on are x ->
    (y, a_last). Samples before in_first are never read."""
    B = r.size
    full = np.concatenate([np.zeros(in_first, dtype=F32), np.ascontiguousarray(x, dtype=F32)])
    cnt = -(-count // B)
    xb = np.zeros(cnt * B, dtype=F32)
    live = full[c * B:c * B + cnt * B]
    xb[:live.size] = live
    xb = xb.reshape(cnt, B)
    with np.errstate(all="ignore"):
        a = F32(s) * np.sqrt(block_energy(xb) / F32(B))
        prev = np.concatenate([[a[0] if c == 0 else F32(a_prev)], a[:-1]]).astype(F32)
        u = carrier(h, marked_chips(key, payload, NB, TB), c * B, cnt * B).reshape(cnt, B)
        g = prev[:, None] + (a[:, None] - prev[:, None]) * r[None, :]
        y = (xb + g * u).reshape(-1)[:count]
    return y.astype(F32), F32(a[-1])


def embed(x, key, payload, strength_db=None, **kw):
    p = config(**kw)
    x = np.ascontiguousarray(x, dtype=F32).reshape(-1)
    if x.size == 0:
        return x.copy()
    t = table(p["taps"], p["block"], p["band_lo"], p["band_hi"])
    s = strength(p["strength_db"] if strength_db is None else strength_db)
    return run(x, 0, True, key, payload, s, 0, 0.0, x.size, t[:p["taps"]], t[p["taps"]:], p["bits"], p["bit_len"])[0]


# ---- the detector, in float64 ---------------------------------------------------------------------
def prepare(x, h, B, NP):
    """Whiten, matched-filter and fold -> (F, F^2), float64."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    n = x.size
    nb = -(-n // B)
    xp = np.zeros(nb * B)
    xp[:n] = x
    q = np.sqrt(np.sum(xp.reshape(nb, B) ** 2, axis=1) / float(B)) + EPS
    w = (xp.reshape(nb, B) / q[:, None]).reshape(-1)[:n]
    v = np.correlate(np.concatenate([w, np.zeros(h.size - 1)]), h.astype(np.float64), mode="valid")  # sum_k h[k] w[n + k]
    folds = -(-n // NP)
    vp = np.zeros(folds * NP)
    vp[:n] = v
    F = vp.reshape(folds, NP).sum(axis=0)
    return F, F * F


def search(F, F2, key, NB, TB):
    """r[b, tau], d[b, tau] for every offset, by FFT: circular correlations with the slot's chips."""
    NP = NB * TB
    c = chips(key, NP).astype(np.float64)
    fF, fF2 = np.conj(np.fft.rfft(F)), np.conj(np.fft.rfft(F2))
    r, d = np.empty((NB, NP)), np.empty((NB, NP))
    for b in range(NB):
        cb = np.zeros(NP)
        cb[b * TB:(b + 1) * TB] = c[b * TB:(b + 1) * TB]
        r[b] = np.fft.irfft(fF * np.fft.rfft(cb), NP)
        r_mask = np.zeros(NP)
        r_mask[b * TB:(b + 1) * TB] = 1.0
        d[b] = np.fft.irfft(fF2 * np.fft.rfft(r_mask), NP)
    return r, d


def direct(F, F2, key, NB, TB, tau):
    """(r_b, d_b, sum |addend| of r_b) at one offset, by the definition."""
    NP = NB * TB
    c = chips(key, NP).astype(np.float64)
    idx = (np.arange(NP) - tau) % NP
    Fs, F2s = F[idx].reshape(NB, TB), F2[idx].reshape(NB, TB)
    return (Fs * c.reshape(NB, TB)).sum(axis=1), F2s.sum(axis=1), np.abs(Fs).sum(axis=1)


def direct_all(F, F2, key, NB, TB):
    """(r, d, A)[b, tau] at every offset by the definition (a dot product per offset, no FFT); A is
    the sum of |addend| of r."""
    NP = NB * TB
    c = chips(key, NP).astype(np.float64)
    view = np.lib.stride_tricks.sliding_window_view
    WF, WF2 = view(np.concatenate([F, F]), TB), view(np.concatenate([F2, F2]), TB)
    tau = np.arange(NP)
    r, d, A = np.empty((NB, NP)), np.empty((NB, NP)), np.empty((NB, NP))
    for b in range(NB):
        s = (b * TB - tau) % NP
        rows = WF[s]
        r[b], A[b], d[b] = rows @ c[b * TB:(b + 1) * TB], np.abs(rows).sum(axis=1), WF2[s].sum(axis=1)
    return r, d, A


def detect(x, key, full=False, **kw):
    p = config(**kw)
    NB, TB, NP = p["bits"], p["bit_len"], p["period"]
    h = table(p["taps"], p["block"], p["band_lo"], p["band_hi"])[:p["taps"]]
    T = threshold(NB, NP)
    x = np.asarray(x, dtype=F32).reshape(-1)
    if x.size == 0:
        out = dict(detected=False, score=0.0, offset=0, payload=0, seen=0, min_z=0.0, threshold=T)
        return out
    F, F2 = prepare(x, h, p["block"], NP)
    r, d = search(F, F2, key, NB, TB)
    # A slot the clip never covers has d = 0 by the definition, and one it covers only with the
    # filter's outermost taps has a d far below the FFT's rounding dust: both are redone by the
    # definition (a direct sum over the slot), so every z below is the float64 value of the contract.
    c = chips(key, NP).astype(np.float64)
    live = np.concatenate([[0], np.cumsum(np.tile(F2 > 0.0, 2).astype(np.int64))])  # (integers: exact)
    for b in range(NB):
        lo = (b * TB - np.arange(NP)) % NP
        never = live[lo + TB] == live[lo]
        r[b, never], d[b, never] = 0.0, 0.0
    tiny = (d != 0.0) & (d < 1e-9 * float(np.max(d)))
    for b, tau in zip(*np.nonzero(tiny)):
        idx = (np.arange(b * TB, (b + 1) * TB) - tau) % NP
        r[b, tau], d[b, tau] = float(np.dot(F[idx], c[b * TB:(b + 1) * TB])), float(np.sum(F2[idx]))
    cov = d > 0.0
    z = np.where(cov, r / np.sqrt(np.where(cov, d, 1.0)), 0.0)
    S = (z * z).sum(axis=0)
    tau = int(np.argmax(S))
    zb = z[:, tau]
    seen = int(sum(1 << b for b in range(NB) if cov[b, tau]))
    payload = int(sum(1 << b for b in range(NB) if cov[b, tau] and zb[b] > 0))
    mz = float(min((abs(zb[b]) for b in range(NB) if cov[b, tau]), default=0.0))
    out = dict(detected=bool(S[tau] >= T), score=float(S[tau]), offset=tau, payload=payload, seen=seen, min_z=mz,
               threshold=T)
    if full:
        out.update(F=F, F2=F2, r=r, d=d, S=S, z=z, cov=cov)
    return out


# ---- hosts ---------------------------------------------------------------------------------------
def vowel(n, k=0, peak=0.3, f0=110.0):
    """A 110 Hz harmonic stack (eight harmonics, 1/h) under a slow envelope, a little noise under it."""
    rng = np.random.default_rng(3000 + k)
    t = np.arange(n, dtype=np.float64) / FS
    x = sum(np.sin(2 * np.pi * f0 * h * t + rng.uniform(0, 6.28)) / h for h in range(1, 9))
    env = 0.55 + 0.45 * np.sin(2 * np.pi * (2.0 + k % 3) * t + k)
    x = x * env + 0.02 * rng.standard_normal(n)
    return (x / max(np.max(np.abs(x), initial=0.0), 1e-9) * peak).astype(F32)


def am_noise(n, k=0, peak=0.3):
    """White noise under a 3 Hz amplitude modulation."""
    rng = np.random.default_rng(4000 + k)
    t = np.arange(n, dtype=np.float64) / FS
    x = rng.standard_normal(n) * (0.55 + 0.45 * np.sin(2 * np.pi * 3.0 * t + k))
    return (x / max(np.max(np.abs(x), initial=0.0), 1e-9) * peak).astype(F32)


# ---- stand-ins for audio.Watermarker's native calls ---------------------------------------------------
def evaluator(wm, items):
    """Watermarker(evaluator=...): the native window call restated. A window must lie inside its plan
    (asserted), as the library checks before it launches anything."""
    outs = []
    h, r = wm.table[:wm.taps], wm.table[wm.taps:]
    for x, in_first, final, s, key, payload, a_prev, c, count in items:
        if count == 0:
            outs.append((np.zeros(0, dtype=F32), F32(a_prev)))
            continue
        end, first = wm.plan(in_first + x.size, final, c)
        assert c * wm.block + count <= end and in_first <= first, "window outside its plan"
        assert count % wm.block == 0 or (final and c * wm.block + count == in_first + x.size)
        outs.append(run(x, in_first, final, key, payload, s, c, a_prev, count, h, r, wm.bits, wm.bit_len))
    return outs


def detector(wm, clips, keys):
    """Watermarker(detector=...): the native detect call restated in float64."""
    kw = dict(block=wm.block, taps=wm.taps, bits=wm.bits, bit_len=wm.bit_len, band_lo=wm.band_lo, band_hi=wm.band_hi)
    return [detect(x, k, **kw) for x, k in zip(clips, keys)]
