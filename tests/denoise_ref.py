"""The numpy restatement of the noise reducer's arithmetic contract (include/rwkvtts.h): what
csrc/denoise.hip must equal bit for bit. Every f32 operation is one numpy f32 operation over whole arrays,
so each is rounded once; a window is computed as the kernels compute it, from the frames its samples
give, so the plan's claims are checked whenever a stream runs over `evaluator`."""
import math

import numpy as np

F32 = np.float32
N, HOP, BINS, BACK, AHEAD, SMOOTH = 512, 128, 257, 94, 30, 2
RC = np.array([0.0] + [1.0 / c for c in range(1, 6)], dtype=np.float64).astype(F32)  # rounded reciprocals


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def table():
    """w[512], the square root of the periodic Hann window, then cos and -sin of 2 pi t / 512, t < 256:
    in double, rounded once."""
    w = [math.sqrt(0.5 - 0.5 * math.cos(2.0 * math.pi * j / N)) for j in range(N)]
    c = [math.cos(2.0 * math.pi * t / N) for t in range(N // 2)]
    s = [-math.sin(2.0 * math.pi * t / N) for t in range(N // 2)]
    return np.array(w + c + s, dtype=np.float64).astype(F32)


def g_min(denoise):
    return F32(math.pow(10.0, -float(denoise) / 20.0))


def fft512(re, im, tab):
    """(M, 512) -> (M, 512): nine radix-2 decimation-in-frequency stages, natural order in; Z[k] = z[bitrev9(k)]."""
    M = re.shape[0]
    c, s = tab[N:N + 256], tab[N + 256:]
    for st in range(9):
        h = 256 >> st
        re, im = re.reshape(M, -1, 2, h), im.reshape(M, -1, 2, h)
        ur, ui, vr, vi = re[:, :, 0], im[:, :, 0], re[:, :, 1], im[:, :, 1]
        dr, di = ur - vr, ui - vi
        t = np.arange(h) << st
        pr, pi = dr * c[t] - di * s[t], dr * s[t] + di * c[t]
        pr, pi = np.where(t == 0, dr, np.where(t == 128, di, pr)), np.where(t == 0, di, np.where(t == 128, -dr, pi))
        re, im = np.stack([ur + vr, pr], axis=2).reshape(M, N), np.stack([ui + vi, pi], axis=2).reshape(M, N)
    rev = np.array([int(format(k, "09b")[::-1], 2) for k in range(N)])
    return re[:, rev], im[:, rev]


def frame_range(in_first, end, final):
    """-> (pa, pb, hi): the window's frames [pa, pb), whole pairs, of which [pa, hi) exist in the signal."""
    pa = 0 if in_first == 0 else -(-(in_first + 3 * HOP) // HOP)
    pa += pa & 1
    if final:
        hi = (end - 1) // HOP + 4
        return pa, hi + (hi & 1), hi
    pb = (end // HOP) & ~1
    return pa, pb, pb


def window(x, in_first, final, gmin, out_first, count, alpha=2.0, tab=None, f64=False):
    """Outputs [out_first, out_first + count) of the signal whose samples [in_first, in_first + x.size) are
    x. f64: the same rule in double on np.fft (the accuracy reference), not the contract."""
    tab = table() if tab is None else tab
    T = np.float64 if f64 else F32
    x = np.ascontiguousarray(x, dtype=F32).reshape(-1).astype(T)
    pa, pb, hi = frame_range(in_first, in_first + x.size, final)
    if count <= 0 or pb <= pa:
        return np.zeros(max(count, 0), dtype=F32)
    w = np.sqrt(0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N) / N)) if f64 else tab[:N]
    idx = HOP * np.arange(pa, pb)[:, None] - 3 * HOP + np.arange(N)[None, :] - in_first
    fr = np.where((idx >= 0) & (idx < x.size), x[np.clip(idx, 0, x.size - 1)], T(0)) * w[None, :]
    if f64:
        X = np.fft.rfft(fr, axis=1)
        Xr, Xi = X.real, X.imag
    else:
        zr, zi = fft512(fr[0::2], fr[1::2], tab)
        k = np.arange(BINS)
        m = (N - k) % N
        Xr, Xi = np.empty((pb - pa, BINS), dtype=F32), np.empty((pb - pa, BINS), dtype=F32)
        Xr[0::2], Xi[0::2] = (zr[:, k] + zr[:, m]) * F32(0.5), (zi[:, k] - zi[:, m]) * F32(0.5)
        Xr[1::2], Xi[1::2] = (zi[:, k] + zi[:, m]) * F32(0.5), (zr[:, m] - zr[:, k]) * F32(0.5)
    E = hi - pa
    P = (Xr * Xr + Xi * Xi)[:E]
    acc, cnt = np.zeros_like(P), np.zeros(E, dtype=np.int64)
    for d in range(-SMOOTH, SMOOTH + 1):
        r = np.arange(max(0, -d), min(E, E - d))
        acc[r] = acc[r] + P[r + d]
        cnt[r] += 1
    S = acc * ((1.0 / cnt) if f64 else RC[cnt])[:, None]
    pad = np.full((BACK + E + AHEAD, BINS), np.inf, dtype=T)
    pad[BACK:BACK + E] = S
    Nf = S.copy()
    for d in range(BACK + AHEAD + 1):
        Nf = np.minimum(Nf, pad[d:d + E])
    with np.errstate(divide="ignore", invalid="ignore"):
        G = np.where(S == 0, T(1), np.maximum(T(gmin), T(1) - T(alpha) * (Nf / S)))
    G = np.concatenate([G, np.ones((pb - hi, BINS), dtype=T)])  # the pair's frame past the end
    Gs = ((np.concatenate([G[:, :1], G[:, :-1]], axis=1) + T(2) * G) + np.concatenate([G[:, 1:], G[:, -1:]], axis=1)) * T(0.25)
    Yr, Yi = Gs * Xr, Gs * Xi
    if f64:
        v = np.fft.irfft(Yr + 1j * Yi, n=N, axis=1) * w[None, :]
    else:
        ar, ai, br, bi = Yr[0::2], Yi[0::2], Yr[1::2], Yi[1::2]
        mir = np.arange(BINS - 2, 0, -1)  # k = 257 .. 511 mirrors 255 .. 1
        pr = np.concatenate([ar - bi, (ar + bi)[:, mir]], axis=1)
        pi = np.concatenate([ai + br, (br - ai)[:, mir]], axis=1)
        orr, oi = fft512(pi, pr, tab)  # the forward butterflies on swapped parts are the inverse transform
        v = np.empty((pb - pa, N), dtype=F32)
        v[0::2], v[1::2] = (oi * F32(1.0 / N)) * w[None, :], (orr * F32(1.0 / N)) * w[None, :]
    i = out_first + np.arange(count)
    acc = np.zeros(count, dtype=T)
    for q in range(4):  # ascending frame order, from +0
        acc = acc + v[(i // HOP) + q - pa, (i % HOP) + (3 - q) * HOP]
    return (acc * T(0.5)).astype(F32) if not f64 else acc * 0.5


def denoise(x, db, alpha=2.0, tab=None, f64=False):
    x = np.ascontiguousarray(x, dtype=F32).reshape(-1)
    return window(x, 0, True, g_min(db), 0, x.size, alpha, tab, f64)


def evaluator(dn, items):
    """Stands in for rwkvtts_denoise_windows."""
    return [window(x, a, f, g, o, n, dn.alpha, dn.table) for x, a, f, g, o, n in items]
