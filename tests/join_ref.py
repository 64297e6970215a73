"""The join stage's arithmetic contract (include/rwkvtts.h) restated in numpy: what
csrc/join.hip is pinned to bitwise (tests/test_gpu_join.py), and the stand-in evaluator of
audio.Joiner where no GPU is present (Joiner(evaluator=join_ref.evaluator))."""
import numpy as np

F32 = np.float32


def ramp(fade):
    """r[k] = (float)((k + 0.5) / fade), in double."""
    return ((np.arange(fade, dtype=np.float64) + 0.5) / float(max(fade, 1))).astype(F32)


def bounds(x, threshold, keep, trim):
    """(a, b) of one segment."""
    n = int(x.size)
    if not trim:
        return 0, n
    loud = np.nonzero(np.abs(x) > F32(threshold))[0]  # (false for NaN)
    if loud.size == 0:
        return 0, 0
    return max(0, int(loud[0]) - keep), min(n, int(loud[-1]) + 1 + keep)


def piece(x, a, b, fade, trim, table=None):
    """x[a:b] with both edges faded over f = min(fade, len // 2) samples (trim only): one rounded f32
    multiply per faded sample, every other sample copied."""
    p = np.array(x[a:b], dtype=F32, copy=True)
    if not trim:
        return p
    r = ramp(fade) if table is None else np.asarray(table, dtype=F32)
    n = b - a
    f = min(fade, n // 2)
    if f > 0:
        p[:f] = p[:f] * r[:f]                    # i < f: r[i]
        p[n - f:] = p[n - f:] * r[:f][::-1]      # i >= n - f: r[n - 1 - i]
    return p


def join(segments, gaps, threshold=0.01, keep=800, fade=80, trim=True, table=None):
    """-> (joined f32 PCM, [(a_s, b_s)]): each piece, then gap_s samples of +0."""
    threshold = float(F32(threshold)) or float(F32(0.01))
    parts, ab = [], []
    for x, g in zip(segments, gaps):
        x = np.ascontiguousarray(x, dtype=F32).reshape(-1)
        a, b = bounds(x, threshold, int(keep), trim)
        ab.append((a, b))
        parts.append(piece(x, a, b, int(fade), trim, table))
        parts.append(np.zeros(int(g), dtype=F32))
    return (np.concatenate(parts) if parts else np.zeros(0, dtype=F32)), ab


def evaluator(joiner, jobs):
    """audio.Joiner's stand-in: the joiner's own threshold, keep, fade, trim and table."""
    return [join(segs, gaps, joiner.threshold, joiner.keep, joiner.fade, joiner.trim, joiner.table)
            for segs, gaps in jobs]
