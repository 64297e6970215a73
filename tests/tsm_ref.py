"""The numpy restatement of the time-stretch arithmetic contract (include/rwkvtts.h):
what csrc/tsm.hip must equal bit for bit. Every f32 operation below is one numpy f32 ufunc call, so
each is rounded once; the sum of squared differences is `np.add.accumulate` in f32, which adds in
ascending order, one rounded add per term (the first term is +0 + sq = sq exactly)."""
import math

import numpy as np

F32 = np.float32


def window(W):
    i = np.arange(W, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * i / float(W))).astype(F32)


def out_len(n, tempo):
    return 0 if n <= 0 else int(math.ceil(float(n) / float(tempo)))


def anchor(m, Hs, tempo):
    return int(math.floor(float(m * Hs) * float(tempo)))


def _read(x, lo, count):
    """x[lo : lo + count] with +0 outside [0, n)."""
    out = np.zeros(count, dtype=F32)
    a, b = max(lo, 0), min(lo + count, x.size)
    if b > a:
        out[a - lo:b - lo] = x[a:b]
    return out


def ranks(D):
    """rank k of the shifts -D .. D-1 (in that order): 0, -1, +1, -2, +2, .., -(D-1), +(D-1), -D."""
    delta = np.arange(-D, D, dtype=np.int64)
    return np.where(delta < 0, -2 * delta - 1, 2 * delta).astype(np.uint64)


def search(x, s_before, a, Hs, D):
    """The shift of one frame: template from s_before + Hs, candidates a - D .. a + D - 1."""
    t = _read(x, s_before + Hs, Hs)
    span = _read(x, a - D, 2 * D + Hs)
    cand = np.lib.stride_tricks.sliding_window_view(span, Hs)[:2 * D]  # [2D][Hs]
    with np.errstate(all="ignore"):
        e = t[None, :] - cand            # one rounded subtract
        sq = e * e                       # one rounded multiply
        d = np.add.accumulate(sq, axis=1, dtype=F32)[:, -1]  # sequential f32 sum from +0
    bits = np.where(np.isnan(d), F32(np.inf), d).astype(F32).view(np.uint32).astype(np.uint64)
    key = (bits << np.uint64(32)) | ranks(D)
    return int(np.argmin(key)) - D


def starts(x, tempo, W=512, D=128, blocks=None):
    """[s_-1, s_0, .. s_{M-1}] of the whole signal x (or of its first `blocks` blocks)."""
    x = np.ascontiguousarray(x, dtype=F32).reshape(-1)
    Hs = W // 2
    M = -(-out_len(x.size, tempo) // Hs)
    if blocks is not None:
        M = min(M, blocks)
    s = [-Hs]
    for m in range(M):
        if m == 0:
            s.append(0)
        else:
            a = anchor(m, Hs, tempo)
            s.append(a + search(x, s[-1], a, Hs, D))
    return s


def stretch(x, tempo, W=512, D=128, return_starts=False, max_out=None):
    """The whole-signal result (or its first max_out samples, max_out a multiple of Hs)."""
    x = np.ascontiguousarray(x, dtype=F32).reshape(-1)
    Hs = W // 2
    n_out = out_len(x.size, tempo)
    if max_out is not None:
        n_out = min(n_out, max_out)
    M = -(-n_out // Hs)
    s = starts(x, tempo, W, D, blocks=M)
    w = window(W)
    y = np.zeros(M * Hs, dtype=F32)
    for j in range(M):
        p = w[Hs:] * _read(x, s[j] + Hs, Hs)   # the earlier frame's product, on the left
        q = w[:Hs] * _read(x, s[j + 1], Hs)
        y[j * Hs:(j + 1) * Hs] = p + q
    y = y[:n_out].copy()
    return (y, s) if return_starts else y


def evaluator(stretcher, items):
    """TimeStretcher(evaluator=...): the native window call restated. A window's samples start at
    in_first; samples before it are never read (the plan's in_first_needed), so zeros stand in for
    them. A window that is not final is cut at out_len only through the plan, so the restatement
    runs on the given samples as if more followed: it must not read past them (asserted)."""
    outs = []
    W, D, Hs = stretcher.window, stretcher.search, stretcher.hop
    w = window(W)
    for x, in_first, final, tempo, block_first, s_prev, count in items:
        end, first = stretcher.plan(tempo, in_first + x.size, final, block_first, s_prev)
        assert block_first * Hs + count <= end and in_first <= first, "window outside its plan"
        full = np.concatenate([np.zeros(in_first, dtype=F32), x])
        n = full.size
        blocks = -(-count // Hs)
        y = np.zeros(blocks * Hs, dtype=F32)
        s_before = s_prev
        for b in range(blocks):
            m = block_first + b
            if m == 0:
                s_m = 0
            else:
                a = anchor(m, Hs, tempo)
                if not final:
                    assert max(s_before + 2 * Hs, a + D + Hs - 1) <= n, "a ready block reads past the known samples"
                s_m = a + search(full, s_before, a, Hs, D)
            lo = min(s_before + Hs, s_m)
            assert lo >= first or lo < 0 or m == 0, "a block reads before in_first_needed"
            y[b * Hs:(b + 1) * Hs] = w[Hs:] * _read(full, s_before + Hs, Hs) + w[:Hs] * _read(full, s_m, Hs)
            s_before = s_m
        outs.append((y[:count].copy(), s_before))
    return outs
