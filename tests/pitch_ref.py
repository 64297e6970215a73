"""The numpy restatement of the pitch shifter's arithmetic contract (include/rwkvtts.h, DESIGN.md
§25): what csrc/pitch.hip must equal bit for bit, and the stand-in evaluator of audio.PitchShifter.
Every f32 operation below is one numpy f32 operation, so each is rounded once; the period sums add
sample by sample in ascending order over whole (frame, lag) arrays; the grains add in ascending q;
numpy's f32 divide is correctly rounded. Integer decisions are plain Python integers."""
import math

import numpy as np

F32 = np.float32

DEFAULTS = dict(hop=160, window=640, lag_min=32, lag_max=320, unvoiced=80, theta=0.2, floor=1e-3)


def config(**kw):
    c = dict(DEFAULTS)
    c.update({k: v for k, v in kw.items() if v})
    return c


def factor(semitones):
    return 2.0 ** (float(semitones) / 12.0)


def row_offset(P, lag_min):
    """Where the 2P-long row of length P starts: sum of 2p over lag_min <= p < P."""
    return (P - lag_min) * (P + lag_min - 1)


def table(lag_min, lag_max):
    """Rows P = lag_min .. lag_max back to back, w_P[i] = (float)(0.5 - 0.5 cos(2 pi (i + 0.5) / (2P)))."""
    rows = []
    for P in range(lag_min, lag_max + 1):
        i = np.arange(2 * P, dtype=np.float64)
        rows.append((0.5 - 0.5 * np.cos(2.0 * np.pi * (i + 0.5) / float(2 * P))).astype(F32))
    return np.concatenate(rows)


def _read(x, lo, count):
    """x[lo : lo + count] with +0 outside [0, n)."""
    out = np.zeros(count, dtype=F32)
    a, b = max(lo, 0), min(lo + count, x.size)
    if b > a:
        out[a - lo:b - lo] = x[a:b]
    return out


def periods(x, c, j0, j1):
    """P_j of frames [j0, j1) of the signal x (which ends at x.size): an int array, 0 = unvoiced."""
    Ha, Wc, lo, hi = c["hop"], c["window"], c["lag_min"], c["lag_max"]
    nf = j1 - j0
    if nf <= 0:
        return np.zeros(0, dtype=np.int64)
    theta, floor = F32(c["theta"]), F32(c["floor"])
    seg = _read(x, j0 * Ha, (nf - 1) * Ha + Wc + hi + 1)
    lags = np.arange(lo - 1, hi + 2)
    base = (np.arange(nf) * Ha)[:, None]
    d = np.zeros((nf, lags.size), dtype=F32)
    m = np.zeros((nf, lags.size), dtype=F32)
    for i in range(Wc):
        a = seg[base + i]                      # (nf, 1)
        b = seg[base + i + lags[None, :]]      # (nf, lags)
        t = a - b
        d = d + t * t
        m = m + (a * a + b * b)
    out = np.zeros(nf, dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        ok = ((d[:, 1:-1] <= d[:, :-2]) & (d[:, 1:-1] <= d[:, 2:]) & (d[:, 1:-1] <= theta * m[:, 1:-1])
              & (m[:, 1:-1] > floor))
    for f in range(nf):
        hit = np.flatnonzero(ok[f])
        if hit.size:
            out[f] = lo + int(hit[0])
    return out


def synthesis_step(P, f):
    return max(1, int(math.floor(float(P) / f + 0.5)))


def window(x_from, in_first, final, f, out_first, a_prev, s_prev, out_count, want_marks=False, **kw):
    """Outputs [out_first, out_first + out_count) of the whole-signal result and the state after them,
    from samples [in_first, in_first + x_from.size) alone: (y, a_last, s_last)."""
    c = config(**kw)
    Ha, lo, hi, P0 = c["hop"], c["lag_min"], c["lag_max"], c["unvoiced"]
    x = np.concatenate([np.zeros(in_first, dtype=F32), np.ascontiguousarray(x_from, dtype=F32)])
    end = out_first + out_count
    if out_count == 0:
        return (np.zeros(0, F32), a_prev, s_prev) + (((), (), ()) if want_marks else ())
    j0, j1 = a_prev // Ha, (end + 2 * hi - 1) // Ha + 1
    per = periods(x, c, j0, j1)

    def P(t):
        j = t // Ha
        return int(per[j - j0]) if j0 <= j < j1 else 0

    lim = end + hi
    a, s = [a_prev], [s_prev]
    while a[-1] < lim:
        a.append(a[-1] + (P(a[-1]) or P0))
    while s[-1] < lim:
        p = P(s[-1])
        s.append(s[-1] + (synthesis_step(p, f) if p else P0))
    tab = table(lo, hi)
    num = np.zeros(out_count, dtype=F32)
    den = np.zeros(out_count, dtype=F32)
    k = 0
    pairs = []
    for sq in s:
        while k + 1 < len(a) and abs(a[k + 1] - sq) < abs(a[k] - sq):  # the lower mark wins a tie
            k += 1
        ak, pk = a[k], (P(a[k]) or P0)
        pairs.append((sq, ak, pk))
        o0, o1 = max(sq - pk, out_first), min(sq + pk, end)
        if o1 <= o0:
            continue
        i0 = o0 - (sq - pk)
        w = tab[row_offset(pk, lo) + i0: row_offset(pk, lo) + i0 + (o1 - o0)]
        g = _read(x, ak - pk + i0, o1 - o0)
        sl = slice(o0 - out_first, o1 - out_first)
        num[sl] = num[sl] + w * g
        den[sl] = den[sl] + w
    with np.errstate(divide="ignore", invalid="ignore"):
        y = np.where(den == 0, F32(0.0), num / den).astype(F32)
    s_last = max(v for v in s if v <= max(0, end - hi))
    a_last = max(v for v in a if v <= max(0, s_last - hi))
    if want_marks:
        return y, a_last, s_last, per, a, pairs
    return y, a_last, s_last


def shift(x, f, **kw):
    x = np.ascontiguousarray(x, dtype=F32).reshape(-1)
    return window(x, 0, True, float(f), 0, 0, 0, x.size, **kw)[0]


def evaluator(shifter, items):
    """Stands in for rwkvtts_pitch_windows: audio.PitchShifter(evaluator=pitch_ref.evaluator)."""
    kw = dict(hop=shifter.hop, window=shifter.window, lag_min=shifter.lag_min, lag_max=shifter.lag_max,
              unvoiced=shifter.unvoiced, theta=shifter.theta, floor=shifter.floor)
    return [window(x, a, fin, f, o, ap, sp, cnt, **kw) for x, a, fin, f, o, ap, sp, cnt in items]
