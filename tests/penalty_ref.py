"""The penalty contract of include/rwkvtts.h (rwkvtts_request::penalties) restated in numpy f32.

For one semantic step of a request that has emitted h[0, n_sem): H = h[max(0, n_sem - W), n_sem)
for a window W > 0, all of h for W == 0; cnt[t] = occurrences of t in H; x = logits[t] as the
sampler receives it, before EOS masking. Every t with cnt[t] > 0 is adjusted in this order, each
operation one f32 operation rounded to nearest:
  1. repetition != 1: cnt[t] times  x = x / repetition if x > 0 else x * repetition
     (per occurrence, as the reference's apply_repetition_penalty loops over the token list)
  2. frequency != 0:  x = x - (frequency * f32(cnt[t]))    (a multiply, then a subtract: no FMA)
  3. presence != 0:   x = x - presence
numpy float32 scalars round every operation to f32 and never fuse two."""
import collections

import numpy as np

Penalties = collections.namedtuple("Penalties", "repetition frequency presence window", defaults=(1.0, 0.0, 0.0, 0))


def window_of(history, window):
    """H: the part of the history the counts are taken over."""
    history = list(history)
    return history[max(0, len(history) - window):] if window > 0 else history


def counts(history, window):
    return collections.Counter(int(t) for t in window_of(history, window))


def apply(row, history, penalties):
    """-> the adjusted copy of `row` (float32). penalties: anything with repetition, frequency,
    presence and window attributes."""
    out = np.array(row, dtype=np.float32, copy=True)
    rep, freq, pres = (np.float32(penalties.repetition), np.float32(penalties.frequency),
                       np.float32(penalties.presence))
    if rep == np.float32(1.0) and freq == np.float32(0.0) and pres == np.float32(0.0):
        return out
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        for t, c in counts(history, penalties.window).items():
            x = out[t]
            if rep != np.float32(1.0):
                for _ in range(c):
                    y = np.float32(x / rep) if x > np.float32(0.0) else np.float32(x * rep)
                    if y.tobytes() == x.tobytes():  # a fixed point: every further pass gives x again
                        break
                    x = y
            if freq != np.float32(0.0):
                prod = np.float32(freq * np.float32(c))
                x = np.float32(x - prod)
            if pres != np.float32(0.0):
                x = np.float32(x - pres)
            out[t] = x
    return out
