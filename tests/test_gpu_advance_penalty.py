"""The decode-step controller with per-row penalties (rwkvtts_debug_advance_pen: k_advance_params of
csrc/sampler.hip with its penalty phase) against tests/penalty_ref.py followed by the oracle
sampler, driven by the phase rules restated as in tests/test_gpu_advance_sampling.py, token for
token: 96 launches on the same logits while each row's history grows.

Rows (8193 logits) are chosen so that tokens repeat: "peaked" (six tokens within 0.5 of each other,
the rest at least 12 lower), "signed" (positive and negative logits among the leaders: both branches
of the repetition rule; its zero-shot rows carry EOS among the leaders, so the re-draw with EOS
masked samples the adjusted row), "flat" (one value), "minus_inf" (a third of the row -inf). Every
launch has 16 rows with different parameters: 13 drawn from the grid repetition {1, 1.3, 0.8} x
frequency {0, 0.7, -0.5} x presence {0, 1.5} x window {0, 1, 8, 64} x T {1, 0.8} x top_k {1, 8, 80,
0} (a seeded shuffle of the 576 combinations, the all-neutral ones left out, dealt over the launches,
so every value of every parameter meets every family), one behavioural row (top_k 1, presence 8.0,
window 4), one row with neutral penalties, which must give what rwkvtts_debug_advance_ex gives, and
one global-phase row with penalties set, which must sample its 32 global tokens untouched (and then
turns semantic, where its penalties start from an empty history). Both the certified path allowed
and the exact walk forced. Tokens, draws used and phases must equal the reference's, no exemptions.

So that equality cannot hold vacuously, the reference's own sequences must show a count of at least
3 inside the window in the peaked rows and, at window 8, an eviction that changes a count."""
import ctypes
import itertools

import numpy as np
import pytest

import penalty_ref
import rwkvtts
from rwkvtts import _ffi
from rwkvtts import weights as W
from test_gpu_advance_sampling import Row, RowEx

EOS = 8192
LD = EOS + 1
STEPS = 96
GRID = [g for g in itertools.product((1.0, 1.3, 0.8), (0.0, 0.7, -0.5), (0.0, 1.5), (0, 1, 8, 64), (1.0, 0.8), (1, 8, 80, 0))
        if g[:3] != (1.0, 0.0, 0.0)]
FAMILIES = ("peaked", "signed", "flat", "minus_inf")
LAUNCHES = 2  # per family
DRAWS = (0, 15, 16, 31, 1007)
CONFIGS = [
    dict(mode=0, fixed=1, hard_min=0, win_bits=0, win_len=0),     # EOS always masked
    dict(mode=0, fixed=0, hard_min=0, win_bits=0, win_len=0),     # EOS would stop
    dict(mode=1, fixed=0, hard_min=10, win_bits=0, win_len=0),    # zero-shot: masked below hard_min, then re-draws
    dict(mode=1, fixed=0, hard_min=0, win_bits=0x0FF, win_len=12),  # zero-shot, ratio 8/12 < 0.7 at first: re-draw
]


class RowPen(ctypes.Structure):  # engine.h DebugAdvanceRowPen
    _fields_ = [("ex", RowEx), ("repetition", ctypes.c_float), ("frequency", ctypes.c_float),
                ("presence", ctypes.c_float), ("window", ctypes.c_int32)]


assert ctypes.sizeof(RowPen) == 104


@pytest.fixture(scope="module")
def rt():
    blob = W.synth_blob(W.DIMS_TINY)
    r = rwkvtts.SharedRwkvRuntime(blob, max_slots=4, token_chunk_size=64, use_graphs=False)
    yield r
    r.close()


def _launch(rt, name, arr, n, logits, exact, steps):
    f = getattr(_ffi.lib(), name)  # argtypes from _ffi.EXPORTS
    lg = np.ascontiguousarray(logits, dtype=np.float32)
    assert lg.shape == (n, LD) and n <= 16
    tok, used, ph = (np.zeros((steps, n), np.int32) for _ in range(3))
    rc = f(rt.handle, lg.ctypes.data_as(ctypes.c_void_p), n, ctypes.cast(arr, ctypes.c_void_p), int(exact), steps,
           tok.ctypes.data_as(ctypes.c_void_p), used.ctypes.data_as(ctypes.c_void_p), ph.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0, _ffi.lib().rwkvtts_last_error()
    return tok, used, ph


def _reference(oracle_mod, row_logits, c):
    """Tokens / draws / phases of STEPS launches of one row (the same logits each time), and the
    semantic history: the controller loop around penalty_ref.apply + oracle.sample."""
    T, P, K = c["T"], c["top_p"], c["top_k"]
    pen = penalty_ref.Penalties(c["rep"], c["freq"], c["pres"], c["window"])
    toks, useds, phases, hist = [], [], [], []
    phase, bits, wl, nglob = c["phase"], c["win_bits"], c["win_len"], 0

    def stream():
        rng = oracle_mod.Rng(c["seed"])
        for _ in range(c["draw"]):
            rng.gen_f32()
        return rng
    grng, srng = stream(), stream()  # the hook starts both streams at the row's key and draw index
    for _ in range(STEPS):
        if phase == 3:
            toks.append(-1); useds.append(0); phases.append(3)
            continue
        if phase == 0:  # global rows: penalties do nothing
            t = oracle_mod.sample(row_logits[:4096], T, P, K, None, grng)
            nglob += 1
            if nglob == 32:
                phase = 1
            toks.append(t); useds.append(1); phases.append(phase)
            continue
        if phase == 1:  # the step that fed g31: its logits are unused
            phase = 2
            toks.append(-1); useds.append(0); phases.append(2)
            continue
        lg = penalty_ref.apply(row_logits[:LD], hist, pen)  # before EOS masking
        if c["fixed"] or (c["mode"] == 1 and len(hist) < c["hard_min"]):
            lg[EOS] = -np.inf
        t = oracle_mod.sample(lg, T, P, K, None, srng)
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
                    lg[EOS] = -np.inf  # the re-draw samples the same adjusted row
                    t = oracle_mod.sample(lg, T, P, K, None, srng)
                    used = 2
        if stop:
            phase = 3
            toks.append(-1); useds.append(used); phases.append(3)
            continue
        if c["mode"] == 1:
            bits = ((bits << 1) | (1 if t != EOS else 0)) & 0xFFF
            wl = min(12, wl + 1)
        assert t != EOS  # EOS never enters the history
        hist.append(t)
        toks.append(t); useds.append(used); phases.append(phase)
    return toks, useds, phases, hist


def _family_row(rs, family, zero_shot):
    if family == "peaked":
        x = (rs.randn(LD) * 0.5 - 14.0).astype(np.float32)  # everything else >= 12 below the leaders
        x = np.minimum(x, np.float32(-12.0))
        x[rs.choice(EOS, 6, replace=False)] = (rs.rand(6) * 0.5).astype(np.float32)
        return x
    if family == "signed":
        x = (rs.randn(LD) * 0.5 - 9.0).astype(np.float32)
        lead = rs.choice(EOS, 8, replace=False)
        x[lead] = np.float32([0.9, 0.6, 0.3, 0.1, -0.1, -0.3, -0.6, -0.9])
        x[EOS] = 0.5 if zero_shot else -20.0  # zero-shot rows draw EOS on some steps and re-draw
        return x
    if family == "flat":
        x = np.full(LD, 0.25, dtype=np.float32)
        x[EOS] = -5.0
        return x
    x = rs.randn(LD).astype(np.float32)
    x[rs.choice(EOS, EOS // 3, replace=False)] = -np.inf
    x[EOS] = -np.inf if zero_shot else -30.0
    return x


_CASES = {}


def _cases(oracle_mod, family):
    """Per family: LAUNCHES launches of 16 rows with the reference's expected outputs; built once,
    shared by the certified and the exact run."""
    if family in _CASES:
        return _CASES[family]
    f = FAMILIES.index(family)
    rs = np.random.RandomState(7100 + f)
    order = np.random.RandomState(99).permutation(len(GRID))  # one deal of the grid over all launches
    launches = []
    i = 0
    for l in range(LAUNCHES):
        deal = [GRID[j] for j in order[13 * (LAUNCHES * f + l):][:13]]
        combos = [dict(rep=r, freq=fr, pres=p, window=w, T=T, top_k=k) for r, fr, p, w, T, k in deal]
        combos.append(dict(rep=1.0, freq=0.0, pres=8.0, window=4, T=1.0, top_k=1))    # row 13: behavioural
        combos.append(dict(rep=1.0, freq=0.0, pres=0.0, window=8, T=(1.0, 0.8)[l % 2], top_k=(80, 8)[l % 2]))  # 14: neutral
        combos.append(dict(rep=1.3, freq=0.7, pres=1.5, window=(0, 8)[l % 2], T=1.0, top_k=20))  # 15: global phase
        logits, meta = [], []
        for r, cb in enumerate(combos):
            cfg = CONFIGS[0] if r == 13 else CONFIGS[i % len(CONFIGS)]
            c = dict(cfg, phase=0 if r == 15 else 2, top_p=0.95, seed=15485863 * (i + 1) + f, draw=DRAWS[i % len(DRAWS)], **cb)
            if r == 15:
                c.update(CONFIGS[0])
            logits.append(_family_row(rs, family, c["mode"] == 1))
            meta.append(c)
            i += 1
        logits = np.stack(logits)
        want = [_reference(oracle_mod, logits[r], c) for r, c in enumerate(meta)]
        launches.append((logits, meta, want))
    _CASES[family] = launches
    return launches


def _rowpen(oracle_mod, c):
    key = oracle_mod.Rng(c["seed"]).key
    row = Row(c["mode"], c["phase"], c["top_k"], c["fixed"], 0, c["hard_min"], c["win_bits"], c["win_len"],
              (ctypes.c_uint32 * 8)(*key), c["draw"])
    return RowPen(RowEx(row, ctypes.sizeof(RowPen), c["T"], c["top_p"], 0), c["rep"], c["freq"], c["pres"], c["window"])


def _max_count_in_window(hist, window):
    return max((max(penalty_ref.counts(hist[:n], window).values()) for n in range(1, len(hist) + 1)), default=0)


def _evictions_that_change_a_count(hist, window):
    """Steps at which the id leaving the window differs from the id entering it."""
    return sum(1 for n in range(window, len(hist)) if hist[n - window] != hist[n])


def test_reference_sequences_exercise_counts_and_evictions(oracle_mod):
    """The conditions the equality test below relies on, on the reference alone (no GPU work)."""
    peak3, evict = 0, 0
    for family in FAMILIES:
        for _, meta, want in _cases(oracle_mod, family):
            for c, (_, _, _, hist) in zip(meta, want):
                if c["phase"] != 2:
                    continue
                if family == "peaked" and _max_count_in_window(hist, c["window"]) >= 3:
                    peak3 += 1
                if c["window"] == 8 and (c["rep"], c["freq"], c["pres"]) != (1.0, 0.0, 0.0):
                    evict += _evictions_that_change_a_count(hist, 8)
    assert peak3 >= 1 and evict >= 1, (peak3, evict)


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("exact", [0, 1])
def test_advance_penalty_grid_vs_reference(rt, oracle_mod, family, exact):
    bad, emitted, any_used2 = [], 0, False
    for logits, meta, want in _cases(oracle_mod, family):
        n = len(meta)
        assert n == 16 and len({tuple(sorted(c.items())) for c in meta}) == n  # rows of one launch differ
        arr = (RowPen * n)(*[_rowpen(oracle_mod, c) for c in meta])
        tok, used, ph = _launch(rt, "rwkvtts_debug_advance_pen", arr, n, logits, exact, STEPS)
        for r, c in enumerate(meta):
            wt, wu, wp, hist = want[r]
            if list(tok[:, r]) != wt or list(used[:, r]) != wu or list(ph[:, r]) != wp:
                first = next(s for s in range(STEPS) if (tok[s, r], used[s, r], ph[s, r]) != (wt[s], wu[s], wp[s]))
                bad.append((r, c, first, list(tok[first:first + 4, r]), wt[first:first + 4]))
        any_used2 |= bool((used == 2).any())
        emitted += int((tok >= 0).sum())
        # the behavioural row: presence 8.0 exceeds the leaders' 0.5 spread, so with top_k 1 and window
        # 4 no token equals any of the four before it
        if family == "peaked":
            t = list(tok[:, 13])
            assert all(x >= 0 for x in t)
            assert all(t[s] not in t[max(0, s - 4):s] for s in range(STEPS)), t
            assert len(set(t)) <= 6  # and it stays among the six leaders (12 below is out of reach)
        # the neutral row: what the hook without penalties gives for it (its limit is 64 launches)
        d = 14
        assert (meta[d]["rep"], meta[d]["freq"], meta[d]["pres"]) == (1.0, 0.0, 0.0)
        pr = _rowpen(oracle_mod, meta[d])
        ex = RowEx(pr.ex.row, ctypes.sizeof(RowEx), meta[d]["T"], meta[d]["top_p"], 0)
        t1, u1, p1 = _launch(rt, "rwkvtts_debug_advance_ex", (RowEx * 1)(ex), 1, logits[d:d + 1], exact, 64)
        assert (t1[:, 0] == tok[:64, d]).all() and (u1[:, 0] == used[:64, d]).all() and (p1[:, 0] == ph[:64, d]).all()
        # the global row: its 32 global tokens are the unpenalised sampler's
        g = 15
        assert (tok[:32, g] >= 0).all() and (tok[:32, g] < 4096).all() and ph[31, g] == 1 and ph[32, g] == 2
    assert not bad, (len(bad), bad[:3])
    assert emitted > LAUNCHES * 16 * STEPS // 2
    if family == "signed":  # the zero-shot rows reach the re-draw (2 draws in one step)
        assert any_used2


@pytest.mark.gpu
def test_hook_refuses_bad_rows(rt, oracle_mod):
    c = dict(CONFIGS[0], phase=2, T=1.0, top_p=0.95, top_k=80, seed=5, draw=0, rep=1.3, freq=0.0, pres=0.0, window=0)
    lg = np.zeros((1, LD), np.float32)
    f = _ffi.lib().rwkvtts_debug_advance_pen
    out = [np.zeros((300, 1), np.int32) for _ in range(3)]

    def call(row, steps):
        return f(rt.handle, lg.ctypes.data_as(ctypes.c_void_p), 1, ctypes.cast((RowPen * 1)(row), ctypes.c_void_p), 0,
                 steps, *[o.ctypes.data_as(ctypes.c_void_p) for o in out])
    assert call(_rowpen(oracle_mod, c), 2) == 0
    assert call(_rowpen(oracle_mod, c), 257) != 0
    for k, v in (("rep", 0.2), ("rep", float("nan")), ("freq", 9.0), ("pres", -9.0), ("window", -1), ("window", 2049)):
        assert call(_rowpen(oracle_mod, dict(c, **{k: v})), 2) != 0, (k, v)
    started = _rowpen(oracle_mod, c)
    started.ex.row.n_sem = 3  # a penalised row starts with an empty history
    assert call(started, 2) != 0
