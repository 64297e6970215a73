"""The pause stage's arithmetic contract (include/rwkvtts.h) restated in numpy, twice:
`shape`, the whole-signal rule over explicit runs, which csrc/pause.hip is pinned to bitwise
(tests/test_gpu_pause.py), and `window`, the same rule as a block-by-block state machine over what a
stream knows -- the stand-in evaluator of audio.PauseShaper where no GPU is present
(PauseShaper(evaluator=pause_ref.evaluator)). The two share the ramp and nothing else, so
tests/test_pause_cpu.py holds one against the other."""
import numpy as np

F32 = np.float32


def ramp(fade):
    """r[k] = (float)((k + 0.5) / fade), in double: the join's."""
    return ((np.arange(fade, dtype=np.float64) + 0.5) / float(fade)).astype(F32)


def loud_blocks(x, B, threshold):
    """loud_k of every block, the last one possibly partial: an f32 compare, false for NaN."""
    n = int(x.size)
    nb = -(-n // B)
    over = np.zeros(nb * B, dtype=bool)
    with np.errstate(invalid="ignore"):
        over[:n] = np.abs(x) > F32(threshold)
    return over.reshape(nb, B).any(axis=1)


def active_blocks(loud, H):
    """active_k: loud_j for an existing j with |j - k| <= H."""
    nb = loud.size
    return np.array([bool(loud[max(0, k - H):k + H + 1].any()) for k in range(nb)], dtype=bool)


def runs(active):
    """[(k0, k1)]: the maximal runs of non-active blocks [k0, k1)."""
    out, k, nb = [], 0, active.size
    while k < nb:
        if active[k]:
            k += 1
            continue
        k0 = k
        while k < nb and not active[k]:
            k += 1
        out.append((k0, k))
    return out


def shape(x, M, B=160, H=5, F=80, threshold=0.01, table=None):
    """-> (shaped f32 PCM, cuts). M: the cap in samples, M >= 2F."""
    x = np.ascontiguousarray(x, dtype=F32).reshape(-1)
    M, B, H, F = int(M), int(B), int(H), int(F)
    assert M >= 2 * F
    n = int(x.size)
    r = ramp(F) if table is None else np.asarray(table, dtype=F32)
    hd, tl = M - M // 2, M // 2
    active = active_blocks(loud_blocks(x, B, threshold), H)
    nb = active.size
    if not active.any():
        return np.zeros(0, dtype=F32), (1 if n > 0 else 0)
    parts, pos, cuts = [], 0, 0   # x[:pos] is dealt with
    for k0, k1 in runs(active):
        s, e = k0 * B, min(k1 * B, n)
        R = e - s
        before, after = k0 > 0, k1 < nb
        if before and after:
            cut = R > M
        elif after:
            cut = R > tl
        else:
            cut = R > hd
        if not cut:
            continue
        cuts += 1
        parts.append(x[pos:s])
        if before:
            head = x[s:s + hd].copy()
            head[hd - F:] = head[hd - F:] * r[::-1]   # i in [hd - F, hd): r[hd - 1 - i]
            parts.append(head)
        if after:
            tail = x[e - tl:e].copy()
            tail[:F] = tail[:F] * r                   # j in [0, F): r[j]
            parts.append(tail)
        pos = e
    parts.append(x[pos:])
    return np.concatenate(parts).astype(F32, copy=False), cuts


def pending(M, B, F, c, seen, q):
    """p of the header: the first sample a window in state (c, seen, q) may still send."""
    hd, tl = M - M // 2, M // 2
    if q == 0:
        return c * B
    if seen:
        return c * B - tl if q > M else c * B - q + min(q, hd - F)
    return c * B - tl if q > tl else c * B - q


def first_needed(M, B, H, F, c, seen, q):
    return max(0, min(pending(M, B, F, c, seen, q), (c - H) * B))


def window(x, in_first, final, M, c, seen, q, B=160, H=5, F=80, threshold=0.01, table=None):
    """One stream window: signal samples [in_first, in_first + x.size) known, blocks [0, c) decided,
    seen: an active block lies before c, q: the samples of the quiet run that ends at c * B.
    -> (what became exact, c, seen, q, in_first_needed, cuts decided here)."""
    x = np.ascontiguousarray(x, dtype=F32).reshape(-1)
    M, B, H, F, c, q = int(M), int(B), int(H), int(F), int(c), int(q)
    n = in_first + int(x.size)
    assert M >= 2 * F and c * B <= n and in_first <= first_needed(M, B, H, F, c, seen, q)
    r = ramp(F) if table is None else np.asarray(table, dtype=F32)
    hd, tl = M - M // 2, M // 2
    nbk = -(-n // B) if final else n // B          # the blocks whose samples are all known
    kd = nbk if final else max(c, nbk - H)         # blocks [c, kd) are decided here
    memo = {}

    def sig(a, b):                                 # signal samples [a, b)
        assert in_first <= a <= b <= n
        return x[a - in_first:b - in_first]

    def loud(k):
        if k not in memo:
            with np.errstate(invalid="ignore"):
                memo[k] = bool((np.abs(sig(k * B, min((k + 1) * B, n))) > F32(threshold)).any())
        return memo[k]

    out, cuts = [], 0
    for k in range(c, kd):
        at = k * B
        if any(loud(j) for j in range(max(0, k - H), min(nbk, k + H + 1))):
            if q > 0:                              # the run [at - q, at) ends here
                if (q > M) if seen else (q > tl):
                    t = sig(at - tl, at).copy()
                    t[:F] = t[:F] * r
                    out.append(t)
                    cuts += 1
                else:
                    out.append(sig(at - q + (min(q, hd - F) if seen else 0), at))
            out.append(sig(at, min(at + B, n)))
            seen, q = 1, 0
            continue
        q0, q = q, q + (min(at + B, n) - at)
        if seen:                                   # run samples [0, hd - F) go out as they come
            s = at - q0
            if q0 < hd - F:
                out.append(sig(s + q0, s + min(q, hd - F)))
            if q0 <= M < q:                        # the cut is certain: the head's faded end
                h = sig(s + hd - F, s + hd).copy()
                out.append(h * r[::-1])
    if final and q > 0:
        s = n - q
        if not seen:
            cuts += 1                              # no active block at all: nothing goes out
        elif q > hd:
            cuts += 1
            if q <= M:
                out.append(sig(s + hd - F, s + hd) * r[::-1])
        else:
            out.append(sig(s + min(q, hd - F), n))
        q = 0                                      # (the signal has ended: no run is open)
    c = kd
    y = np.concatenate(out).astype(F32, copy=False) if out else np.zeros(0, dtype=F32)
    return y, c, int(seen), q, first_needed(M, B, H, F, c, seen, q), cuts


def stream(x, cuts_at, M, **cfg):
    """x through `window` cut at the given offsets -> (the concatenated outputs, cuts, most samples kept)."""
    x = np.ascontiguousarray(x, dtype=F32).reshape(-1)
    edges = sorted(set(int(a) for a in cuts_at if 0 < a < x.size)) + [x.size]
    first, state, parts, total, kept = 0, (0, 0, 0), [], 0, 0
    for i, e in enumerate(edges):
        y, c, s, q, need, k = window(x[first:e], first, i + 1 == len(edges), M, *state, **cfg)
        state, total = (c, s, q), total + k
        parts.append(y)
        first = min(need, e)
        kept = max(kept, e - first)
    return np.concatenate(parts), total, kept


def evaluator(shaper, items):
    """audio.PauseShaper's stand-in: the shaper's own block, hang, fade, threshold and table."""
    return [window(x, a, f, m, c, s, q, shaper.block, shaper.hang, shaper.fade, shaper.threshold, shaper.table)
            for x, a, f, m, c, s, q in items]
