"""The pinned voice on the GPU (rwkvtts_request.pinned_voice): a normal-mode request whose 32 global
tokens are given. The property: run A, a normal request with a seed, gives (G, S); run B, the same
request with pinned_voice and ref_global = G, gives (G, S) exactly -- B's prompt is what A fed itself
up to TAG_1, prefill and decode are bitwise the same per row, and the semantic draw counter starts
at 0 in both. So the oracle's normal-mode run is the reference of the pinned mode."""
import numpy as np
import pytest

import rwkvtts
from rwkvtts import _ffi
from rwkvtts import weights as W
from rwkvtts.runtime import PhaseSampling
from helpers import make_request, synth_text, to_struct

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=[_ffi.DTYPE_BF16, _ffi.DTYPE_F16], ids=["bf16", "f16"])
def tiny(request, oracle_mod):
    blob = W.synth_blob(W.DIMS_TINY, seed=31, dtype=request.param)
    rt = rwkvtts.SharedRwkvRuntime(blob, device=0, max_slots=8, token_chunk_size=128, use_graphs=True)
    yield rt, oracle_mod.Model(blob), blob
    rt.close()


def normal(i, **kw):
    kw.setdefault("max_tokens", 48)
    return make_request(synth_text(300 + i), seed=50 + i, **kw)


def pinned(req, g):
    """The same request with the voice pinned to g."""
    p = make_request(req.text_tokens, props=req.property_tokens, seed=req.args.seed, max_tokens=req.args.max_tokens,
                     fixed=req.fixed_semantic, ref_global=list(g))
    p.args.semantic_sampling = req.args.semantic_sampling
    p.args.global_sampling = req.args.global_sampling
    p.pinned_voice = True
    return p


def oracle_run(model, req):
    q, _keep = to_struct(req)
    g, s, _ = model.generate(q)
    return g, s


def test_pinned_returns_the_oracles_normal_run(tiny):
    rt, model, _ = tiny
    reqs = [normal(i) for i in range(3)]
    want = [oracle_run(model, r) for r in reqs]
    assert all(len(g) == 32 and 0 < len(s) <= 48 for g, s in want)
    got = rt.generate_batch([pinned(r, g) for r, (g, _) in zip(reqs, want)])
    assert rt.last_status == [0, 0, 0]
    assert got == want
    # (and the engine's own normal run, the A of the property)
    assert rt.generate_batch(reqs) == want


def test_pinned_fixed_semantic(tiny):
    rt, model, _ = tiny
    reqs = [normal(10 + i, fixed=40) for i in range(3)]
    want = [oracle_run(model, r) for r in reqs]
    assert all(len(s) == 40 for _, s in want)
    assert rt.generate_batch([pinned(r, g) for r, (g, _) in zip(reqs, want)]) == want


def test_pinned_semantic_temperature(tiny):
    """A semantic temperature of 0.8 takes k_advance_params; the oracle's loop cannot take the
    parameter, so the reference is the engine's normal run with it (pinned to the oracle by
    tests/test_gpu_generate_sampling.py)."""
    rt, _, _ = tiny
    reqs = [normal(20 + i) for i in range(3)]
    for r in reqs:
        r.args.semantic_sampling = PhaseSampling(temperature=0.8)
    want = rt.generate_batch(reqs)
    assert all(len(g) == 32 and len(s) > 0 for g, s in want)
    plain = rt.generate_batch([normal(20 + i) for i in range(3)])
    assert [g for g, _ in plain] == [g for g, _ in want] and plain != want  # the parameter reaches the sampler
    assert rt.generate_batch([pinned(r, g) for r, (g, _) in zip(reqs, want)]) == want


def mixed_batch(model):
    """Normal, pinned and zero-shot requests, with what each gives when run alone."""
    ref_g, ref_s = list(range(200, 232)), list(range(30))
    reqs, want = [], []
    for i in range(9):
        if i % 3 == 0:
            r = normal(30 + i, max_tokens=20 + i)
        elif i % 3 == 1:
            n = normal(30 + i, max_tokens=20 + i)
            r = pinned(n, oracle_run(model, n)[0])
        else:
            r = make_request(synth_text(330 + i, n=6), props=[], seed=80 + i, fixed=12 + i, ref_global=ref_g,
                             ref_semantic=ref_s)
        reqs.append(r)
    return reqs


def test_mixed_batch_equals_each_request_alone(tiny):
    """9 requests of the three kinds in 8 slots: admission staggers, head rows switch per step."""
    rt, model, _ = tiny
    reqs = mixed_batch(model)
    alone = [rt.generate_batch([r])[0] for r in reqs]
    assert rt.generate_batch(reqs) == alone
    assert rt.last_status == [0] * 9
    for i in (1, 4, 7):
        assert alone[i][0] == reqs[i].ref_global_tokens
        n = normal(30 + i, max_tokens=20 + i)
        assert alone[i] == oracle_run(model, n)


def test_pinned_prompt_spanning_two_mixed_steps(tiny, oracle_mod):
    """token_chunk_size smaller than the pinned prompt (6 + 1 + 24 + 1 + 32 + 1 = 65 rows)."""
    _, model, blob = tiny
    rt = rwkvtts.SharedRwkvRuntime(blob, device=0, max_slots=8, token_chunk_size=40, use_graphs=True)
    try:
        reqs = [normal(40 + i) for i in range(3)]
        want = [oracle_run(model, r) for r in reqs]
        assert rt.generate_batch([pinned(r, g) for r, (g, _) in zip(reqs, want)]) == want
    finally:
        rt.close()


def test_token_sink_first_call_carries_the_globals(tiny):
    rt, model, _ = tiny
    n = normal(50)
    g, s = oracle_run(model, n)
    calls = []
    out = rt.generate_batch([pinned(n, g)], on_tokens=lambda i, gl, first, new, done, status: calls.append(
        (i, gl, first, list(new), done, status)))
    assert out == [(g, s)]
    assert calls[0][1] == g and calls[0][2] == 0  # all 32 with the first call
    assert all(c[1] == g for c in calls)
    assert sum((c[3] for c in calls), []) == s and calls[-1][4] and calls[-1][5] == 0
    assert [c[4] for c in calls[:-1]] == [False] * (len(calls) - 1)


@pytest.mark.parametrize("bad", ["31", "33", "minus", "4096", "semantic", "null"])
def test_bad_pinned_request_fails_alone(tiny, bad):
    rt, model, _ = tiny
    good = [normal(60), normal(61)]
    want = [oracle_run(model, r) for r in good]
    g = list(want[0][0])
    b = pinned(good[0], g)
    if bad == "31":
        b.ref_global_tokens = g[:31]
    elif bad == "33":
        b.ref_global_tokens = g + [5]
    elif bad == "minus":
        b.ref_global_tokens = g[:7] + [-1] + g[8:]
    elif bad == "4096":
        b.ref_global_tokens = g[:31] + [4096]
    elif bad == "semantic":
        b.ref_semantic_tokens = [1, 2, 3]
    else:
        b.ref_global_tokens = None
    got = rt.generate_batch([good[0], b, pinned(good[1], want[1][0])])
    assert rt.last_status[0] == 0 and rt.last_status[2] == 0 and rt.last_status[1] == _ffi.EINVAL
    assert got[1] == ([], []) and got[0] == want[0] and got[2] == want[1]


def test_max_tokens_zero(tiny):
    rt, model, _ = tiny
    n = normal(70)
    g, _ = oracle_run(model, n)
    calls = []
    p = pinned(n, g)
    p.args.max_tokens = 0
    others = [pinned(n, g), p]
    got = rt.generate_batch(others, on_tokens=lambda *a: calls.append(a))
    assert rt.last_status == [0, 0]
    assert got[1] == (g, []) and got[0] == oracle_run(model, n)
    mine = [c for c in calls if c[0] == 1]
    assert mine == [(1, g, 0, [], True, 0)]
    # more of them than slots: none takes one
    assert rt.generate_batch([p] * 20) == [(g, [])] * 20


def test_pinned_at_the_mid_dims(oracle_mod):
    """The 0.4B width (the persistent decode launches), one request."""
    blob = W.synth_blob(W.DIMS_MID, seed=9)
    rt = rwkvtts.SharedRwkvRuntime(blob, device=0, max_slots=8, token_chunk_size=128, use_graphs=True)
    try:
        n = make_request(synth_text(90), seed=91, max_tokens=16)
        g, s = oracle_run(oracle_mod.Model(blob), n)
        assert len(g) == 32 and len(s) > 0
        assert rt.generate_batch([pinned(n, g)]) == [(g, s)]
    finally:
        rt.close()
