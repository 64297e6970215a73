"""The Mirostat contract of include/rwkvtts.h (rwkvtts_request_ext::mirostat) restated in numpy f32.

For one semantic attempt of a slot with threshold mu, on the row as the sampler receives it (after
any penalty adjustment), every operation one f32 operation rounded to nearest:
  1. p[i] as the sampler's softmax: masked entries to -inf, the max, glibc expf(x - max), the
     sequential f32 sum in index order, the divide.
  2. c = #{i : p[i] > 0 and -lg(p[i]) <= mu}, n_pos = #{i : p[i] > 0}, K = min(c + 1, n_pos).
  3. The kept set: the first K ranks in the order (p descending, index ascending).
  4. cum[r] = the sequential f32 sum over ranks 0..r; S = cum[K-1].
  5. u = r32 * S, one rounded multiply.
  6. The token is the first rank with u <= cum[r].
  7. After the attempt whose token is emitted: s = lg(S) - lg(p_tok); e = s - tau;
     mu = mu - rate * e (a multiply, then a subtract: no FMA); mu = min(mu, 4 * tau).
Initial mu = 2 * tau.

lg is the library's own export rwkvtts_debug_lg2 (csrc/exact_math.h lg2f, the source the kernel
runs); expf is the library's glibc expf (rwkvtts_debug_expf_n; tests/test_expf_exact.py holds it to
libm). Everything else is restated here: numpy float32 scalars and np.add.accumulate round every
operation to f32, in order, and never fuse two."""
import collections
import ctypes

import numpy as np

from rwkvtts import _ffi

f32 = np.float32
Attempt = collections.namedtuple("Attempt", "token S p_tok K")


def _map(name, x):
    x = np.ascontiguousarray(x, dtype=np.float32)
    out = np.empty_like(x)
    f = getattr(_ffi.lib(), name)
    # (rwkvtts_debug_expf_n is, like rwkvtts_debug_expf, outside the header and _ffi.EXPORTS)
    f.restype, f.argtypes = None, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    f(x.ctypes.data_as(ctypes.c_void_p), x.size, out.ctypes.data_as(ctypes.c_void_p))
    return out


def lg(x):
    """lg of the contract for positive finite f32 values (an array, or a scalar -> np.float32)."""
    if np.ndim(x) == 0:
        return _map("rwkvtts_debug_lg2", np.array([x], dtype=np.float32))[0]
    return _map("rwkvtts_debug_lg2", x)


def expf(x):
    return _map("rwkvtts_debug_expf_n", x)


def softmax(row, masked=()):
    """Step 1. masked: indices set to -inf first (the forbid / EOS mask)."""
    x = np.array(row, dtype=np.float32, copy=True)
    for i in masked:
        x[i] = -np.inf
    with np.errstate(invalid="ignore"):
        e = expf(x - x.max())
    total = np.add.accumulate(e, dtype=np.float32)[-1]  # sequential, in index order
    return (e / total).astype(np.float32)


def kept(p, mu):
    """Steps 2 and 3 -> (the kept indices in rank order, K)."""
    p = np.asarray(p, dtype=np.float32)
    pos = np.flatnonzero(p > 0)
    c = int(np.count_nonzero(-lg(p[pos]) <= f32(mu))) if len(pos) else 0
    K = min(c + 1, len(pos))
    order = np.argsort(-p, kind="stable")  # p descending; a stable sort keeps equal p in index order
    return order[:K], K


def sample_p(p, mu, r32):
    """Steps 2 to 6 on given probabilities -> Attempt."""
    p = np.asarray(p, dtype=np.float32)
    idx, K = kept(p, mu)
    cum = np.add.accumulate(p[idx], dtype=np.float32)
    S = cum[-1]
    u = f32(f32(r32) * S)
    hit = np.flatnonzero(u <= cum)
    rank = int(hit[0]) if len(hit) else K - 1
    return Attempt(int(idx[rank]), S, p[idx[rank]], K)


def sample(row, mu, r32, masked=()):
    """Steps 1 to 6 on a logits row -> Attempt."""
    return sample_p(softmax(row, masked), mu, r32)


def surprise(S, p_tok):
    """s of step 7: the emitted token's surprise inside the kept set."""
    return f32(lg(S) - lg(p_tok))


def update(mu, tau, rate, S, p_tok):
    """Step 7 -> the new mu."""
    tau, rate = f32(tau), f32(rate)
    e = f32(surprise(S, p_tok) - tau)
    prod = f32(rate * e)
    return min(f32(f32(mu) - prod), f32(f32(4.0) * tau))


def initial_mu(tau):
    return f32(f32(2.0) * f32(tau))
