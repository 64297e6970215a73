"""The typical-sampling contract of include/rwkvtts.h (rwkvtts_request_ext_v2::typical, steps 1 to 8
there) restated in numpy f32. ln, expf and powf are the library's host exports of the source the kernel
runs (rwkvtts_debug_logf, held to libm by tests/test_typ_cpu.py; rwkvtts_debug_expf_n;
rwkvtts_debug_powf); everything else is restated here: numpy float32 scalars and np.add.accumulate
round every operation to f32, in order, and never fuse two."""
import collections
import ctypes

import numpy as np

import miro_ref
from rwkvtts import _ffi

f32 = np.float32
N_IDS = 8193
Params = collections.namedtuple("Params", "tau top_k temperature presence frequency decay",
                                defaults=(0.5, 128, 1.0, 0.3, 0.3, 0.99654026))


class State:  # per slot: a penalty and a seen mark for each id, empty at admission
    def __init__(self):
        self.pen, self.seen = np.zeros(N_IDS, np.float32), np.zeros(N_IDS, bool)


def powf(x, y):
    x = np.ascontiguousarray(x, dtype=np.float32)
    yy, out = np.full_like(x, y), np.empty_like(x)
    f = _ffi.lib().rwkvtts_debug_powf
    f.restype, f.argtypes = None, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    f(*[a.ctypes.data_as(ctypes.c_void_p) for a in (x, yy)], x.size, out.ctypes.data_as(ctypes.c_void_p))
    return out


def penalise(row, st):
    """Step 1."""
    x = np.array(row, dtype=np.float32, copy=True)
    x[st.seen] = x[st.seen] - st.pen[st.seen]
    return x


def kept_values(p, P):
    """Steps 3 to 6a -> (the kept ids in order, their powf(p, 1 / T))."""
    p = np.asarray(p, dtype=np.float32)
    pos = np.flatnonzero(p > 0)
    y = -miro_ref._map("rwkvtts_debug_logf", p[pos])
    ent = np.add.accumulate(p[pos] * y, dtype=np.float32)[-1]  # left to right in index order
    order = pos[np.lexsort((pos, np.abs(y - ent)))][:P.top_k]  # ascending key, then ascending id
    cum = np.add.accumulate(p[order], dtype=np.float32)
    stop = np.flatnonzero(~(np.concatenate([np.zeros(1, np.float32), cum[:-1]]) <= f32(P.tau)))
    kept = order[:int(stop[0])] if len(stop) else order
    return kept, powf(p[kept], f32(1.0) / f32(P.temperature))


def sample(row, P, r32, masked=()):
    """Steps 2 to 7 on a row that step 1 has adjusted -> (token, number kept)."""
    kept, v = kept_values(miro_ref.softmax(row, masked), P)
    with np.errstate(invalid="ignore", divide="ignore"):
        cum = np.add.accumulate(v / np.add.accumulate(v, dtype=np.float32)[-1], dtype=np.float32)
        hit = np.flatnonzero(f32(r32) <= cum)
    return int(kept[int(hit[0]) if len(hit) else 0]), len(kept)  # find_or_first


def update(st, tok, P):
    """Step 8."""
    st.pen[st.seen] = st.pen[st.seen] * f32(P.decay)
    st.pen[tok] = st.pen[tok] + f32(P.frequency) if st.seen[tok] else f32(P.presence)
    st.seen[tok] = True
