"""The numpy restatement of the formant shift's arithmetic contract (include/rwkvtts.h, DESIGN.md
§38): what csrc/formant.hip must equal bit for bit. Periods, marks, pairing, Hann rows and the
denominator are pitch_ref's; the numerator term of a grain is its Hann weight times a 16-tap sum, in
ascending tap order, over one row of a 64-phase table around the fixed-point read position. Every f32
operation below is one numpy f32 operation; positions and phases are int64."""
import math

import numpy as np

import pitch_ref

F32 = np.float32
T, PHASES, BACK, ONE = 16, 64, 7, 65536


def ratio(semitones):
    """B = floor(2^(s / 12) * 65536 + 0.5), in double."""
    return int(math.floor(2.0 ** (float(semitones) / 12.0) * 65536.0 + 0.5))


def table(B):
    """(64, 16) f32: the windowed sinc of cutoff min(1, 65536 / B), step by step as the header states."""
    fc = 1.0 if B <= ONE else 65536.0 / float(B)
    out = np.empty((PHASES, T), dtype=F32)
    for ph in range(PHASES):
        v, total = [], 0.0
        for t in range(T):
            u = float(t - BACK) - ph / float(PHASES)
            z = fc * u
            if z == 0.0:
                s = 1.0
            elif z == math.floor(z):
                s = 0.0
            else:
                a = math.pi * z
                s = math.sin(a) / a
            k = (u + 0.5 * T) / float(T)
            w = (0.35875 - 0.48829 * math.cos(2.0 * math.pi * k) + 0.14128 * math.cos(4.0 * math.pi * k)
                 - 0.01168 * math.cos(6.0 * math.pi * k))
            v.append(s * (w * w))
            total = total + v[-1]
        out[ph] = [x / total for x in v]
    return out


def interpolate(x, P, tab):
    """xi at the int64 positions P: sum over ascending t of tab[(P & 65535) >> 10, t] * x[(P >> 16) - 7 + t]
    with +0 outside the signal. -> (xi, lowest index read, highest index read)."""
    P = np.asarray(P, dtype=np.int64)
    i0, ph = P >> 16, (P & 65535) >> 10
    acc = np.zeros(P.size, dtype=F32)
    for t in range(T):
        idx = i0 - BACK + t
        ok = (idx >= 0) & (idx < x.size)
        xv = np.zeros(P.size, dtype=F32)
        xv[ok] = x[idx[ok]]
        acc = acc + tab[ph, t] * xv
    return acc, int(i0.min()) - BACK, int(i0.max()) - BACK + T - 1


def window(x_from, in_first, final, f, B, tab, out_first, a_prev, s_prev, out_count, want_reads=False, **kw):
    """pitch_ref.window with the grains read at ratio B through tab: (y, a_last, s_last), and with
    want_reads the lowest and highest sample index a grain read."""
    c = pitch_ref.config(**kw)
    lo = c["lag_min"]
    x = np.concatenate([np.zeros(in_first, dtype=F32), np.ascontiguousarray(x_from, dtype=F32)])
    end = out_first + out_count
    _, a_last, s_last, _, _, pairs = pitch_ref.window(x_from, in_first, final, f, out_first, a_prev, s_prev, out_count,
                                                      want_marks=True, **kw)
    hann = pitch_ref.table(lo, c["lag_max"])
    num = np.zeros(out_count, dtype=F32)
    den = np.zeros(out_count, dtype=F32)
    reads = [None, None]
    for sq, ak, pk in pairs:
        o0, o1 = max(sq - pk, out_first), min(sq + pk, end)
        if o1 <= o0:
            continue
        r = np.arange(o0, o1, dtype=np.int64) - (sq - pk)
        w = hann[pitch_ref.row_offset(pk, lo) + r]
        xi, i_lo, i_hi = interpolate(x, (np.int64(ak) << 16) + (r - pk) * np.int64(B), tab)
        reads = [i_lo if reads[0] is None else min(reads[0], i_lo), i_hi if reads[1] is None else max(reads[1], i_hi)]
        sl = slice(o0 - out_first, o1 - out_first)
        num[sl] = num[sl] + w * xi
        den[sl] = den[sl] + w
    with np.errstate(divide="ignore", invalid="ignore"):
        y = np.where(den == 0, F32(0.0), num / den).astype(F32)
    return (y, a_last, s_last) + ((reads[0], reads[1]) if want_reads else ())


def shift(x, f, B, tab, **kw):
    x = np.ascontiguousarray(x, dtype=F32).reshape(-1)
    return window(x, 0, True, float(f), B, tab, 0, 0, 0, x.size, **kw)[0]


def evaluator(shifter, items, Bs=None):
    """Stands in for rwkvtts_formant_windows: audio.PitchShifter(evaluator=formant_ref.evaluator)."""
    if Bs is None:
        return pitch_ref.evaluator(shifter, items)
    kw = dict(hop=shifter.hop, window=shifter.window, lag_min=shifter.lag_min, lag_max=shifter.lag_max,
              unvoiced=shifter.unvoiced, theta=shifter.theta, floor=shifter.floor)
    return [window(x, a, fin, f, B, shifter.formant_table(B), o, ap, sp, cnt, **kw)
            for (x, a, fin, f, o, ap, sp, cnt), B in zip(items, Bs)]
