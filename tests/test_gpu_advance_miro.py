"""The decode-step controller with per-row Mirostat (rwkvtts_debug_advance_miro: k_advance_miro of
csrc/sampler.hip) against tests/miro_ref.py, driven by the phase rules restated as in
tests/test_gpu_advance_penalty.py, launch for launch: 96 launches on the same logits while each row's
threshold mu moves (and, on the penalised rows, its history grows).

Rows (8193 logits) are the penalty test's families: "peaked" (six tokens within 0.5 of each other,
the rest at least 12 lower), "signed" (positive and negative leaders; its zero-shot rows carry EOS
among them, so EOS is drawn and re-drawn with the same mu), "flat" (one value: K in the thousands,
the sorted-values path) and "minus_inf" (a third of the row -inf). Every launch has 16 rows: the grid
tau {0.5, 3, 8} x rate {0.1, 1} x with / without penalties (12 rows), a global-phase row with
Mirostat set (its 32 global tokens are the plain sampler's, then it turns semantic and starts from
its initial mu), two rows with Mirostat off (one with sampling values of its own, one default: they
must give what rwkvtts_debug_advance_pen gives) and a row that starts from mu = 0.25, below every
surprise. Both the certified path allowed (for the rows without Mirostat) and the exact walk forced.
Tokens, draws used, phases and every mu must equal the reference's, no exemptions; mu is the kernel's
own lg on the row's S and p_tok, so its equality is device lg == host lg bitwise on those values.

So that equality cannot hold vacuously, the reference's own sequences must reach K = 1, a K above
kFastTopK (256), the cap at 4 tau and a zero-shot re-draw on a Mirostat row (checked on the CPU)."""
import ctypes

import numpy as np
import pytest

import miro_ref
import penalty_ref
import rwkvtts
from rwkvtts import _ffi
from rwkvtts import weights as W
from test_gpu_advance_penalty import CONFIGS, DRAWS, EOS, FAMILIES, LD, RowPen, _family_row, _launch as _launch_pen
from test_gpu_advance_sampling import Row, RowEx

STEPS = 96
FAST_TOP_K = 256  # csrc/slot_ctrl.h kFastTopK
PEN = (1.3, 0.7, 1.5, 8)
NOPEN = (1.0, 0.0, 0.0, 0)
GRID = [(tau, rate, pen) for tau in (0.5, 3.0, 8.0) for rate in (0.1, 1.0) for pen in (NOPEN, PEN)]
f32 = np.float32


class RowMiro(ctypes.Structure):  # engine.h DebugAdvanceRowMiro
    _fields_ = [("pen", RowPen), ("tau", ctypes.c_float), ("rate", ctypes.c_float), ("mu", ctypes.c_float),
                ("on", ctypes.c_int32)]


assert ctypes.sizeof(RowMiro) == 120


@pytest.fixture(scope="module")
def rt():
    blob = W.synth_blob(W.DIMS_TINY)
    r = rwkvtts.SharedRwkvRuntime(blob, max_slots=4, token_chunk_size=64, use_graphs=False)
    yield r
    r.close()


def _launch(rt, arr, n, logits, exact, steps):
    lg = np.ascontiguousarray(logits, dtype=np.float32)
    assert lg.shape == (n, LD) and n <= 16
    tok, used, ph = (np.zeros((steps, n), np.int32) for _ in range(3))
    mu = np.zeros((steps, n), np.float32)
    rc = _ffi.lib().rwkvtts_debug_advance_miro(
        rt.handle, lg.ctypes.data_as(ctypes.c_void_p), n, ctypes.cast(arr, ctypes.c_void_p), int(exact), steps,
        *[a.ctypes.data_as(ctypes.c_void_p) for a in (tok, used, ph, mu)])
    assert rc == 0, _ffi.lib().rwkvtts_last_error()
    return tok, used, ph, mu


def _reference(oracle_mod, row_logits, c):
    """Tokens / draws / phases / mu of STEPS launches of one row (the same logits each time), and
    what the sequence reached: the controller loop around penalty_ref.apply and miro_ref (rows with
    Mirostat) or oracle.sample (rows without, and the global phase)."""
    T, P, K = c["T"], c["top_p"], c["top_k"]
    pen = penalty_ref.Penalties(*c["pen"])
    neutral = c["pen"][:3] == (1.0, 0.0, 0.0)
    tau, rate, mu, on = f32(c["tau"]), f32(c["rate"]), f32(c["mu"]), c["on"]
    toks, useds, phases, mus, hist = [], [], [], [], []
    reached = dict(k1=0, big=0, cap=0, redraw=0, kmax=0)
    phase, bits, wl, nglob = c["phase"], c["win_bits"], c["win_len"], 0
    cache = {}

    def stream():
        rng = oracle_mod.Rng(c["seed"])
        for _ in range(c["draw"]):
            rng.gen_f32()
        return rng
    grng, srng = stream(), stream()  # the hook starts both streams at the row's key and draw index

    def draw_token(lg, masked):
        """One attempt on the adjusted row -> (token, Attempt or None)."""
        if not on:
            x = np.array(lg, copy=True)
            if masked:
                x[EOS] = -np.inf
            return oracle_mod.sample(x, T, P, K, None, srng), None
        key = masked if neutral else None
        p = cache.get(key)
        if p is None:
            p = miro_ref.softmax(lg, masked=(EOS,) if masked else ())
            if key is not None:
                cache[key] = p
        a = miro_ref.sample_p(p, mu, srng.gen_f32())
        reached["k1"] += a.K == 1
        reached["big"] += a.K > FAST_TOP_K
        reached["kmax"] = max(reached["kmax"], a.K)
        return a.token, a

    for _ in range(STEPS):
        if phase == 3:
            toks.append(-1); useds.append(0); phases.append(3); mus.append(mu)
            continue
        if phase == 0:  # global rows: neither penalties nor Mirostat
            t = oracle_mod.sample(row_logits[:4096], T, P, K, None, grng)
            nglob += 1
            if nglob == 32:
                phase = 1
            toks.append(t); useds.append(1); phases.append(phase); mus.append(mu)
            continue
        if phase == 1:  # the step that fed g31: its logits are unused
            phase = 2
            toks.append(-1); useds.append(0); phases.append(2); mus.append(mu)
            continue
        lg = penalty_ref.apply(row_logits[:LD], hist, pen)  # before EOS masking
        masked = bool(c["fixed"] or (c["mode"] == 1 and len(hist) < c["hard_min"]))
        t, a = draw_token(lg, masked)
        used, stop = 1, False
        if t == EOS:
            if c["mode"] == 0:
                stop = True
            else:
                non_eos = bin(bits & ((1 << wl) - 1)).count("1")
                ratio = np.float32(non_eos) / np.float32(wl) if wl > 0 else np.float32(0)
                if wl >= 12 and ratio >= np.float32(0.7):
                    stop = True
                else:  # the re-draw samples the same adjusted row with EOS masked and the same mu
                    t, a = draw_token(lg, True)
                    used = 2
                    reached["redraw"] += bool(on)
        if stop:
            phase = 3
            toks.append(-1); useds.append(used); phases.append(3); mus.append(mu)
            continue
        if c["mode"] == 1:
            bits = ((bits << 1) | (1 if t != EOS else 0)) & 0xFFF
            wl = min(12, wl + 1)
        assert t != EOS  # EOS never enters the history
        if on:  # only the attempt whose token is emitted moves mu
            uncapped = f32(mu - f32(rate * f32(miro_ref.surprise(a.S, a.p_tok) - tau)))
            mu = miro_ref.update(mu, tau, rate, a.S, a.p_tok)
            reached["cap"] += bool(uncapped > mu)
        hist.append(t)
        toks.append(t); useds.append(used); phases.append(phase); mus.append(mu)
    return toks, useds, phases, [float(m) for m in mus], reached


_CASES = {}


def _cases(oracle_mod, family):
    """Per family: one launch of 16 rows with the reference's expected outputs; built once, shared
    by the certified and the exact run."""
    if family in _CASES:
        return _CASES[family]
    f = FAMILIES.index(family)
    rs = np.random.RandomState(7300 + f)
    combos = [dict(tau=tau, rate=rate, pen=pen, on=1, mu=float(miro_ref.initial_mu(tau)), T=1.0, top_k=20)
              for tau, rate, pen in GRID]
    combos.append(dict(tau=3.0, rate=0.1, pen=NOPEN, on=1, mu=6.0, T=1.0, top_k=20))   # row 12: global phase
    combos.append(dict(tau=0.0, rate=0.0, pen=PEN, on=0, mu=0.0, T=0.8, top_k=8))      # row 13: off, own sampling
    combos.append(dict(tau=0.0, rate=0.0, pen=NOPEN, on=0, mu=0.0, T=1.0, top_k=80))   # row 14: off, default
    combos.append(dict(tau=3.0, rate=0.1, pen=NOPEN, on=1, mu=0.25, T=1.0, top_k=20))  # row 15: mu below every surprise
    logits, meta = [], []
    for r, cb in enumerate(combos):
        cfg = CONFIGS[0] if r == 12 else CONFIGS[(r + f) % len(CONFIGS)]
        c = dict(cfg, phase=0 if r == 12 else 2, top_p=0.95, seed=32452843 * (16 * f + r + 1), draw=DRAWS[r % len(DRAWS)], **cb)
        logits.append(_family_row(rs, family, c["mode"] == 1))
        meta.append(c)
    logits = np.stack(logits)
    want = [_reference(oracle_mod, logits[r], c) for r, c in enumerate(meta)]
    _CASES[family] = (logits, meta, want)
    return _CASES[family]


def _rowmiro(oracle_mod, c):
    key = oracle_mod.Rng(c["seed"]).key
    row = Row(c["mode"], c["phase"], c["top_k"], c["fixed"], 0, c["hard_min"], c["win_bits"], c["win_len"],
              (ctypes.c_uint32 * 8)(*key), c["draw"])
    pen = RowPen(RowEx(row, ctypes.sizeof(RowMiro), c["T"], c["top_p"], 0), *c["pen"])
    return RowMiro(pen, c["tau"], c["rate"], c["mu"], c["on"])


def test_reference_sequences_reach_every_path(oracle_mod):
    """The conditions the equality test below relies on, on the reference alone (no GPU work)."""
    tot = dict(k1=0, big=0, cap=0, redraw=0, kmax=0)
    distinct_mu = 0
    for family in FAMILIES:
        _, meta, want = _cases(oracle_mod, family)
        for c, (_, _, _, mus, reached) in zip(meta, want):
            for k in ("k1", "big", "cap", "redraw"):
                tot[k] += reached[k]
            tot["kmax"] = max(tot["kmax"], reached["kmax"])
            if c["on"]:
                distinct_mu = max(distinct_mu, len(set(mus)))
    print("reached:", tot, "most distinct mu values in one row:", distinct_mu)
    assert tot["k1"] >= 1 and tot["big"] >= 1 and tot["cap"] >= 1 and tot["redraw"] >= 1, tot
    assert tot["kmax"] > 4096  # past the keyed sort's capacity too
    assert distinct_mu >= STEPS // 2  # lg is evaluated on many different values


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("exact", [0, 1])
def test_advance_miro_grid_vs_reference(rt, oracle_mod, family, exact):
    logits, meta, want = _cases(oracle_mod, family)
    n = len(meta)
    assert n == 16
    arr = (RowMiro * n)(*[_rowmiro(oracle_mod, c) for c in meta])
    tok, used, ph, mu = _launch(rt, arr, n, logits, exact, STEPS)
    bad = []
    for r, c in enumerate(meta):
        wt, wu, wp, wm, _ = want[r]
        got_mu = [float(x) for x in mu[:, r]]
        if list(tok[:, r]) != wt or list(used[:, r]) != wu or list(ph[:, r]) != wp or \
                np.asarray(got_mu, np.float32).tobytes() != np.asarray(wm, np.float32).tobytes():
            first = next(s for s in range(STEPS)
                         if (tok[s, r], used[s, r], ph[s, r], f32(got_mu[s]).tobytes()) != (wt[s], wu[s], wp[s], f32(wm[s]).tobytes()))
            bad.append((r, c, first, list(tok[first:first + 3, r]), wt[first:first + 3], got_mu[first:first + 3], wm[first:first + 3]))
    assert not bad, (len(bad), bad[:3])
    assert int((tok >= 0).sum()) > n * STEPS // 2
    # the rows with Mirostat off: what the hook without it gives for their first 104 bytes
    for d in (13, 14):
        assert meta[d]["on"] == 0
        pr = _rowmiro(oracle_mod, meta[d]).pen
        pr.ex.struct_size = ctypes.sizeof(RowPen)
        t1, u1, p1 = _launch_pen(rt, "rwkvtts_debug_advance_pen", (RowPen * 1)(pr), 1, logits[d:d + 1], exact, STEPS)
        assert (t1[:, 0] == tok[:, d]).all() and (u1[:, 0] == used[:, d]).all() and (p1[:, 0] == ph[:, d]).all()
        assert (mu[:, d] == 0.0).all()
    # the global row: 32 global tokens, the feed step, then semantic tokens under Mirostat from mu = 6
    g = 12
    assert (tok[:32, g] >= 0).all() and (tok[:32, g] < 4096).all() and ph[31, g] == 1 and ph[32, g] == 2
    assert (mu[:33, g] == 6.0).all() and len(set(mu[33:, g].tolist())) > 1


@pytest.mark.gpu
def test_hook_refuses_bad_rows(rt, oracle_mod):
    c = dict(CONFIGS[0], phase=2, T=1.0, top_p=0.95, top_k=80, seed=5, draw=0, pen=NOPEN, tau=3.0, rate=0.1, mu=6.0, on=1)
    lg = np.zeros((1, LD), np.float32)
    out = [np.zeros((300, 1), np.int32) for _ in range(3)] + [np.zeros((300, 1), np.float32)]

    def call(row, steps):
        return _ffi.lib().rwkvtts_debug_advance_miro(
            rt.handle, lg.ctypes.data_as(ctypes.c_void_p), 1, ctypes.cast((RowMiro * 1)(row), ctypes.c_void_p), 0, steps,
            *[o.ctypes.data_as(ctypes.c_void_p) for o in out])
    assert call(_rowmiro(oracle_mod, c), 2) == 0
    assert call(_rowmiro(oracle_mod, c), 257) != 0
    for k, v in (("tau", 0.4), ("tau", 10.5), ("tau", float("nan")), ("rate", 0.0), ("rate", 1.5), ("mu", float("inf")), ("on", 2)):
        assert call(_rowmiro(oracle_mod, dict(c, **{k: v})), 2) != 0, (k, v)
    short = _rowmiro(oracle_mod, c)
    short.pen.ex.struct_size = ctypes.sizeof(RowPen)
    assert call(short, 2) != 0
