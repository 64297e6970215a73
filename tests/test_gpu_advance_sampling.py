"""The decode-step sampler with per-row sampling parameters (rwkvtts_debug_advance_ex: k_advance /
k_advance_params of csrc/sampler.hip) against the oracle sampler driven by the phase rules
restated here (normal_mode_inference.rs:237-391 / zero_shot_inference.rs:256-309), token for token.

Row families as in tests/test_gpu_advance.py (restated): near-uniform, peaked (top-p cut inside
the top-k), k-th and (k+1)-th largest logits tied and 1 ulp apart, heavy exact ties, EOS-dominated
rows (stop, zero-shot re-draw with EOS masked, window rule). Every family runs the whole grid
T in {0.7, 1.0, 1.3} x top_p in {0.5, 0.95, 1.0} x top_k in {0, 1, 50, 256, 300} -- the certified
path (T = 1, k <= 256), the exact walk plus the fast path's temperature step (T != 1, k <= 256),
the general path inside k_advance (k = 300; k = 0, whose 8193 probabilities are sorted as values
for top-p) -- in launches of 16 rows that carry different parameters, 20 launches each with draw
indices that cross 16-word ChaCha blocks, with the certified path allowed and with the exact walk
forced. Tokens, draws used and phases must equal the oracle's exactly; the default-parameter row of
each launch must equal what rwkvtts_debug_advance gives for it."""
import ctypes
import itertools

import numpy as np
import pytest

import rwkvtts
from rwkvtts import _ffi
from rwkvtts import weights as W

pytestmark = pytest.mark.gpu
EOS = 8192
LD = EOS + 1
STEPS = 20
TEMPS, TOP_PS, TOP_KS = (0.7, 1.0, 1.3), (0.5, 0.95, 1.0), (0, 1, 50, 256, 300)
GRID = list(itertools.product(TEMPS, TOP_PS, TOP_KS))  # 45 combinations: 3 launches of 15 + a default row
FAMILIES = ("near_uniform", "peaked", "kth_tied", "kth_1ulp", "quantised_ties", "eos_heavy", "eos_some")


class Row(ctypes.Structure):  # engine.h DebugAdvanceRow
    _fields_ = [("mode", ctypes.c_int32), ("phase", ctypes.c_int32), ("top_k", ctypes.c_int32),
                ("fixed", ctypes.c_int32), ("n_sem", ctypes.c_int32), ("hard_min", ctypes.c_int32),
                ("win_bits", ctypes.c_int32), ("win_len", ctypes.c_int32), ("key", ctypes.c_uint32 * 8),
                ("draw", ctypes.c_uint64)]


class RowEx(ctypes.Structure):  # engine.h DebugAdvanceRowEx
    _fields_ = [("row", Row), ("struct_size", ctypes.c_uint32), ("temperature", ctypes.c_float),
                ("top_p", ctypes.c_float), ("pad", ctypes.c_uint32)]


assert ctypes.sizeof(Row) == 72 and ctypes.sizeof(RowEx) == 88

CONFIGS = [
    dict(mode=0, phase=0, fixed=0, n_sem=0, hard_min=0, win_bits=0, win_len=0),     # global phase
    dict(mode=0, phase=2, fixed=0, n_sem=0, hard_min=0, win_bits=0, win_len=0),     # semantic, EOS stops
    dict(mode=0, phase=2, fixed=1, n_sem=5, hard_min=0, win_bits=0, win_len=0),     # EOS always masked
    dict(mode=1, phase=2, fixed=0, n_sem=3, hard_min=10, win_bits=0, win_len=0),    # zero-shot below hard_min
    dict(mode=1, phase=2, fixed=0, n_sem=40, hard_min=10, win_bits=0xFFF, win_len=12),  # window may stop
    dict(mode=1, phase=2, fixed=0, n_sem=40, hard_min=10, win_bits=0x0FF, win_len=12),  # ratio 8/12 < 0.7: re-draw
    dict(mode=1, phase=2, fixed=0, n_sem=40, hard_min=10, win_bits=0x1F, win_len=5),    # short window: re-draw
]
DRAWS = (0, 15, 16, 31, 1007)  # 20 launches from 15, 16 and 31 cross into the next ChaCha block


@pytest.fixture(scope="module")
def rt():
    blob = W.synth_blob(W.DIMS_TINY)
    r = rwkvtts.SharedRwkvRuntime(blob, max_slots=4, token_chunk_size=64, use_graphs=False)
    yield r
    r.close()


def _launch(rt, name, arr, n, logits, exact):
    f = getattr(_ffi.lib(), name)  # argtypes from _ffi.EXPORTS
    lg = np.ascontiguousarray(logits, dtype=np.float32)
    assert lg.shape == (n, LD) and n <= 16
    tok, used, ph = (np.zeros((STEPS, n), np.int32) for _ in range(3))
    rc = f(rt.handle, lg.ctypes.data_as(ctypes.c_void_p), n, ctypes.cast(arr, ctypes.c_void_p), int(exact), STEPS,
           tok.ctypes.data_as(ctypes.c_void_p), used.ctypes.data_as(ctypes.c_void_p), ph.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0, _ffi.lib().rwkvtts_last_error()
    return tok, used, ph


def _reference(oracle_mod, row_logits, c):
    """The oracle's tokens / draws / phases for STEPS launches of one row (same logits each time):
    the controller loop around oracle.sample with the row's own (T, top_p, top_k)."""
    T, P, K = c["T"], c["top_p"], c["top_k"]
    toks, useds, phases = [], [], []
    phase, n_sem, bits, wl, nglob = c["phase"], c["n_sem"], c["win_bits"], c["win_len"], 0
    rng = oracle_mod.Rng(c["seed"])
    for _ in range(c["draw"]):
        rng.gen_f32()
    for _ in range(STEPS):
        if phase == 3:
            toks.append(-1); useds.append(0); phases.append(3)
            continue
        if phase == 0:
            t = oracle_mod.sample(row_logits[:4096], T, P, K, None, rng)
            nglob += 1
            if nglob == 32:
                phase = 1
            toks.append(t); useds.append(1); phases.append(phase)
            continue
        lg = row_logits[:LD].copy()
        if c["fixed"] or (c["mode"] == 1 and n_sem < c["hard_min"]):
            lg[EOS] = -np.inf
        t = oracle_mod.sample(lg, T, P, K, None, rng)
        used, stop = 1, False
        if t == EOS:
            if c["mode"] == 0:
                stop = True
            else:
                non_eos = bin(bits & ((1 << wl) - 1)).count("1")
                ratio = np.float32(non_eos) / np.float32(wl) if wl > 0 else np.float32(0)
                if wl >= 12 and ratio >= np.float32(0.7):
                    stop = True
                else:
                    lg[EOS] = -np.inf
                    t = oracle_mod.sample(lg, T, P, K, None, rng)
                    used = 2
        if stop:
            phase = 3
            toks.append(-1); useds.append(used); phases.append(3)
            continue
        if c["mode"] == 1:
            bits = ((bits << 1) | (1 if t != EOS else 0)) & 0xFFF
            wl = min(12, wl + 1)
        n_sem += 1
        toks.append(t); useds.append(used); phases.append(phase)
    return toks, useds, phases


def _kth_tied(rs, k, ulps):
    """Near-uniform row whose k-th and (k+1)-th largest logits (over the first 4096 and over all
    8193) are equal (ulps = 0) or 1 ulp apart."""
    x = (rs.randn(LD) * 0.5).astype(np.float32)
    for n in (4096, LD):
        order = np.argsort(-x[:n], kind="stable")
        a, b = order[k - 1], order[k]
        x[b] = x[a] if ulps == 0 else np.nextafter(x[a], np.float32(-np.inf), dtype=np.float32)
    return x


def _family_row(rs, family, top_k):
    k = top_k if top_k > 0 else 50  # the tie sits at the row's own top-k boundary
    if family == "near_uniform":
        return (rs.randn(LD) * 0.3).astype(np.float32)
    if family == "peaked":
        p = rs.randn(LD).astype(np.float32)
        p[rs.randint(0, 4096, 3)] += np.float32([9.0, 7.5, 6.0])
        return p
    if family == "kth_tied":
        return _kth_tied(rs, k, 0)
    if family == "kth_1ulp":
        return _kth_tied(rs, k, 1)
    if family == "quantised_ties":
        return (np.round(rs.randn(LD) * 4) / 4).astype(np.float32)
    e = (rs.randn(LD) * 0.5).astype(np.float32)
    e[EOS] = 6.0 if family == "eos_heavy" else 3.5  # EOS carries most of the mass / is drawn on some steps
    return e


_CASES = {}


def _cases(oracle_mod, family):
    """Per family: three launches of 16 rows (15 grid combinations and one default-parameter row),
    with the oracle's expected outputs; built once, shared by the certified and the exact run."""
    if family in _CASES:
        return _CASES[family]
    rs = np.random.RandomState(4000 + FAMILIES.index(family))
    order = rs.permutation(len(GRID))  # each launch mixes temperatures, top-p and top-k values
    launches = []
    i = 0
    for l in range(3):
        combos = [GRID[j] for j in order[15 * l:15 * l + 15]] + [(1.0, 0.95, (20, 80, 20)[l])]
        logits, meta = [], []
        for T, P, K in combos:
            c = dict(CONFIGS[i % len(CONFIGS)], T=T, top_p=P, top_k=K, seed=104729 * (i + 1) + FAMILIES.index(family),
                     draw=DRAWS[i % len(DRAWS)])
            logits.append(_family_row(rs, family, K))
            meta.append(c)
            i += 1
        logits = np.stack(logits)
        want = [_reference(oracle_mod, logits[r], c) for r, c in enumerate(meta)]
        launches.append((logits, meta, want))
    _CASES[family] = launches
    return launches


def _row(oracle_mod, c):
    key = oracle_mod.Rng(c["seed"]).key
    return Row(c["mode"], c["phase"], c["top_k"], c["fixed"], c["n_sem"], c["hard_min"], c["win_bits"], c["win_len"],
               (ctypes.c_uint32 * 8)(*key), c["draw"])


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("exact", [0, 1])
def test_advance_sampling_grid_vs_oracle(rt, oracle_mod, family, exact):
    bad, any_used2, any_stop, emitted = [], False, False, 0
    for logits, meta, want in _cases(oracle_mod, family):
        n = len(meta)
        assert len({(c["T"], c["top_p"], c["top_k"]) for c in meta}) == n  # rows of one launch differ
        arr = (RowEx * n)(*[RowEx(_row(oracle_mod, c), ctypes.sizeof(RowEx), c["T"], c["top_p"], 0) for c in meta])
        tok, used, ph = _launch(rt, "rwkvtts_debug_advance_ex", arr, n, logits, exact)
        for r, c in enumerate(meta):
            wt, wu, wp = want[r]
            if list(tok[:, r]) != wt or list(used[:, r]) != wu or list(ph[:, r]) != wp:
                bad.append(({k: c[k] for k in ("T", "top_p", "top_k", "mode", "phase", "fixed", "n_sem", "win_bits", "draw")},
                            list(tok[:, r]), wt, list(used[:, r]), wu))
        any_used2 |= bool((used == 2).any())
        any_stop |= bool((ph == 3).any())
        emitted += int((tok >= 0).sum())
        # the default-parameter row: bitwise what the hook without parameters gives for it
        d = n - 1
        assert (meta[d]["T"], meta[d]["top_p"]) == (1.0, 0.95)
        one = (Row * 1)(_row(oracle_mod, meta[d]))
        t1, u1, p1 = _launch(rt, "rwkvtts_debug_advance", one, 1, logits[d:d + 1], exact)
        assert (t1[:, 0] == tok[:, d]).all() and (u1[:, 0] == used[:, d]).all() and (p1[:, 0] == ph[:, d]).all()
    assert not bad, (len(bad), bad[:3])
    assert emitted > 3 * 16 * STEPS // 2
    if family.startswith("eos"):  # the cases reach the stops and the re-draws (2 draws in one step)
        assert any_used2 and any_stop
