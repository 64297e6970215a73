"""Typical sampling on the GPU against tests/typ_ref.py, bitwise.

The hook (rwkvtts_debug_advance_typ: k_advance_typ of csrc/sampler.hip), launch for launch: token ids and the
row's whole penalty array; every row is a semantic row of 8193 logits with EOS masked. "edges" (2 launches, so
that step 1 has something to subtract): every key equal; three logit values repeated with top_k 3000 (keys below
the threshold together with a partly taken run of equal keys); one entry kept; fewer positive probabilities than
top_k; top_k 1 and 8193; tau 0 and tau 1.5 (top_k binds); temperature 0.7 and 1.3; the draw forced to 0 and to
2.0, above the last cum (find_or_first); 64 near-equal ids at temperature 0.01, where every powf underflows and
the sum is 0 (find_or_first again); 100 finite ids and one. "sequence": 48 launches, decay 1.0 and ai00's.

End to end on the `tiny` model, engine and manager: the expected tokens come from the controller loop of
tests/test_gpu_generate_miro.py on the device's own single-slot logits, with typ_ref where miro_ref stands."""
import ctypes
import dataclasses
import functools

import numpy as np
import pytest

import miro_ref
import rwkvtts
import test_gpu_generate_miro as GM
import typ_ref
from rwkvtts import _ffi
from rwkvtts.runtime import Mirostat, Penalties, PhaseSampling, Typical
from helpers import make_request, synth_text
from test_gpu_advance_miro import RowMiro
from test_gpu_advance_penalty import RowPen
from test_gpu_advance_sampling import Row, RowEx
from test_gpu_generate_miro import engines  # noqa: F401  (the fixture: blob, 4-slot engine, 1-slot logits source)

EOS, LD, DRAW = 8192, 8193, 15
P = typ_ref.Params


class RowTyp(ctypes.Structure):  # engine.h DebugAdvanceRowTyp
    _fields_ = [("miro", RowMiro), ("tau", ctypes.c_float), ("temperature", ctypes.c_float),
                ("presence", ctypes.c_float), ("frequency", ctypes.c_float), ("decay", ctypes.c_float),
                ("top_k", ctypes.c_int32), ("on", ctypes.c_int32), ("force_r", ctypes.c_float)]


def _reference(oracle_mod, i, x, prm, forced, steps):  # -> (token, penalty array) after each launch of row i
    rng, st, out = oracle_mod.Rng(31 + i), typ_ref.State(), []
    for s in range(DRAW + steps):
        r = rng.gen_f32()  # (a forced r replaces the draw in step 7; the draw is still made)
        if s >= DRAW:
            tok = typ_ref.sample(typ_ref.penalise(x, st), prm, r if forced is None else forced, (EOS,))[0]
            typ_ref.update(st, tok, prm)
            out.append((tok, st.pen.copy()))
    return out


@functools.lru_cache(maxsize=None)
def _case(oracle_mod, name):  # -> ([(logits, Params, forced r or None)], launches, the reference's results)
    rs = np.random.RandomState(4100)
    rnd = lambda s=3.0: (rs.randn(LD) * s).astype(np.float32)
    finite = lambda n, s=3.0: np.where(np.arange(LD) < n, rnd(s), -np.inf).astype(np.float32)
    peaked = rnd()
    peaked[4000] = 40.0
    if name == "sequence":
        rows, steps = [(rnd(), P(decay=1.0)), (rnd(), P()), (rnd(), P(tau=0.9, decay=1.0))], 48
    else:
        rows, steps = [(np.zeros(LD, np.float32), P(tau=1.0)),
                       (np.repeat(np.float32([2.0, 1.0, 0.0]), LD // 3), P(top_k=3000, tau=1.0)),
                       (peaked, P()), (finite(50), P(tau=1.0)), (rnd(), P(top_k=1)), (rnd(), P(top_k=LD, tau=2.0)),
                       (rnd(), P(tau=0.0)), (rnd(), P(tau=1.5)), (rnd(), P(tau=0.9, temperature=0.7)),
                       (rnd(), P(tau=0.9, temperature=1.3)), (rnd(), P(tau=0.9), 0.0), (rnd(), P(tau=0.9), 2.0),
                       (finite(64, 0.05), P(tau=0.9, temperature=0.01)), (finite(100), P(tau=1.0)), (finite(1), P())], 2
    rows = [(x, p, f[0] if f else None) for x, p, *f in rows]
    return rows, steps, [_reference(oracle_mod, i, *r, steps) for i, r in enumerate(rows)]


def test_reference_rows_reach_what_they_are_for(oracle_mod):
    rows, _, _ = _case(oracle_mod, "edges")
    x, prm, _ = rows[12]  # the 64 near-equal ids
    for pen in (0.0, 0.3):  # both launches: no id, or any one id, penalised
        kept, v = typ_ref.kept_values(miro_ref.softmax(x - np.float32(pen) * (np.arange(LD) == 3), (EOS,)), prm)
        assert len(kept) > 8 and v.sum() == 0  # every powf underflows: no r <= cum, the fallback
    x, prm, _ = rows[1]  # the three repeated values
    kept = typ_ref.kept_values(miro_ref.softmax(x, (EOS,)), prm)[0]
    assert [int((x[kept] == v).sum()) for v in (2.0, 1.0, 0.0)] == [2731, 269, 0]  # a partly taken run
    _, steps, want = _case(oracle_mod, "sequence")
    assert all(len({t for t, _ in w}) < steps for w in want[:2])  # a token seen again: step 8's frequency branch


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["edges", "sequence"])
def test_advance_typ_vs_reference(engines, oracle_mod, name):  # noqa: F811
    rt = engines[2]  # (the hook brings its own rows: any engine serves)
    rows, steps, want = _case(oracle_mod, name)
    n, arr = len(rows), (RowTyp * len(rows))()
    for i, (_, p, forced) in enumerate(rows):
        row = Row(0, 2, 80, 1, 0, 0, 0, 0, (ctypes.c_uint32 * 8)(*oracle_mod.Rng(31 + i).key), DRAW)
        miro = RowMiro(RowPen(RowEx(row, ctypes.sizeof(RowTyp), 1.0, 0.95, 0), 1.0, 0.0, 0.0, 0), 0.0, 0.0, 0.0, 0)
        arr[i] = RowTyp(miro, p.tau, p.temperature, p.presence, p.frequency, p.decay, p.top_k,
                        1 if forced is None else 3, forced or 0.0)
    lg = np.ascontiguousarray(np.stack([r[0] for r in rows]), dtype=np.float32)
    tok, used, ph = (np.zeros((steps, n), np.int32) for _ in range(3))
    pen = np.zeros((steps, n, LD), np.float32)
    rc = _ffi.lib().rwkvtts_debug_advance_typ(
        rt.handle, lg.ctypes.data_as(ctypes.c_void_p), n, ctypes.cast(arr, ctypes.c_void_p), 0, steps,
        *[a.ctypes.data_as(ctypes.c_void_p) for a in (tok, used, ph, pen)])
    assert rc == 0, _ffi.lib().rwkvtts_last_error()
    assert (used == 1).all() and (ph == 2).all()
    for r, w in enumerate(want):
        first = next((s for s in range(steps) if (tok[s, r], pen[s, r].tobytes()) != (w[s][0], w[s][1].tobytes())), None)
        assert first is None, (r, first, tok[first, r], w[first][0], int((pen[first, r] != w[first][1]).sum()))


class _TypAsMiro:
    """typ_ref behind the three calls that loop makes: the 'threshold' is the slot's typ_ref.State."""
    def __init__(self, t):
        self.prm = P(t.tau, t.top_k, t.temperature, t.presence_penalty, t.frequency_penalty, t.penalty_decay)

    def initial_mu(self, tau):
        return typ_ref.State()

    def sample(self, row, st, r32, masked=()):  # a re-draw gets the same row and state: the same adjusted row
        tok = typ_ref.sample(typ_ref.penalise(row, st), self.prm, r32, masked)[0]
        return miro_ref.Attempt(tok, tok, 0.0, 0)

    def update(self, st, tau, rate, tok, p_tok):
        typ_ref.update(st, int(tok), self.prm)
        return st


def _req(i, seed, typical=None, n=12, **kw):
    r = make_request(synth_text(i, n=n), seed=seed, **kw)
    r.args.typical = typical
    return r


@pytest.mark.gpu
def test_generate_batch_and_manager_honour_typical(engines, oracle_mod, monkeypatch):  # noqa: F811
    blob, gen, one = engines
    defaults = [_req(800 + i, 70 + i, max_tokens=24) for i in range(3)]
    before = gen.generate_batch(defaults)  # before any typical request has run in this engine
    assert before == [GM._expected(one, oracle_mod, r) for r in defaults]
    zs = dict(n=6, props=[], fixed=20, ref_global=list(range(100, 132)), ref_semantic=list(range(40)))
    hard = Typical(tau=0.2, top_k=5, temperature=1.3, presence_penalty=2.0, frequency_penalty=1.0, penalty_decay=0.5)
    R = dict(plain_typ=_req(701, 901, Typical(), max_tokens=40), fixed=_req(711, 911, hard, fixed=30),
             zero=_req(707, 907, Typical(tau=0.9, top_k=8193, temperature=0.7, penalty_decay=1.0), **zs))
    want = {}
    for k, r in R.items():  # that loop, taking its Mirostat branch with typ_ref behind it
        with monkeypatch.context() as mp:
            mp.setattr(GM, "miro_ref", _TypAsMiro(r.args.typical))
            as_miro = dataclasses.replace(r, args=dataclasses.replace(r.args, typical=None, mirostat=Mirostat()))
            want[k] = GM._expected(one, oracle_mod, as_miro)
    assert len(want["plain_typ"][1]) > 0 and len(want["zero"][1]) == 20 and len(want["fixed"][1]) == 30
    # a bad value and the four excluded combinations: each fails alone with RWKVTTS_EINVAL
    bad = [_req(777, 5, Typical(top_k=0), max_tokens=24), _req(778, 6, Typical(), max_tokens=24, greedy=True)]
    for k, v in dict(mirostat=Mirostat(), penalties=Penalties(presence=1.0),
                     semantic_sampling=PhaseSampling(temperature=0.8)).items():
        bad.append(_req(777, 5, Typical(), max_tokens=24))
        setattr(bad[-1].args, k, v)
    # 9 + 3 requests on 4 slots: admission staggers, slots are reused, default slots ride beside typical ones
    order = ["plain_typ", "zero", None, "fixed", None, None, None, None, "plain_typ"]
    out = gen.generate_batch([R["plain_typ"], R["zero"], bad[0], R["fixed"], *bad[1:], R["plain_typ"]] + defaults)
    status = list(gen.last_status)
    for i, k in enumerate(order):
        assert (status[i], out[i]) == ((_ffi.EINVAL, ([], [])) if k is None else (0, want[k])), (i, k)
    assert out[len(order):] == before and status[len(order):] == [0] * 3  # the default slots' tokens, bit for bit
    m = rwkvtts.DynamicBatchManager(blob, devices=[0], max_slots=2, token_chunk_size=64)
    try:
        assert m.generate_tts_batch([R["fixed"], defaults[0], R["plain_typ"]]) == [want["fixed"], before[0], want["plain_typ"]]
        assert m.wait_status(m.submit(bad[2]))[1] == _ffi.EINVAL
    finally:
        m.close()
