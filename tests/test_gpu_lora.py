"""Per-request LoRA adapters (include/rwkvtts.h "adapters", csrc/lora.hip) on the GPU.

forward_check.check_case unchanged: float64 (tests/lora_ref.py), bitwise against the segment alone and
against one token per call (the header's invariance claim). Gates are test_gpu_forward_dims.py's.
tiny: every split 1. c384: key split 3 (pre-summed slab up to 64 rows, relu^2 planes beyond). mid: the
0.4B widths and ranks (k_wkv6, four rkv slabs, the fused value staging). Rows 1 / 17 / 70: a partial
tile, a tile edge, a step past the 64-row planes threshold."""
import contextlib
import functools

import numpy as np
import pytest

import lora_ref
import mx_ref
import rwkv7_f64
import rwkvtts
from rwkvtts import weights as W
from forward_check import FULL, Reference, check_case, feed, tokens
from helpers import make_request, synth_text

pytestmark = pytest.mark.gpu

V = 8209
HEAD = 200
DIMS = {"tiny": dict(W.DIMS_TINY, n_vocab=V), "c384": dict(W.DIMS_TINY, n_embd=384, n_ffn=1536, n_vocab=V),
        "mid": dict(W.DIMS_MID, n_vocab=V)}
STATE_GATE = 1e-3
E = rwkvtts._ffi


@functools.lru_cache(maxsize=None)
def _case(name, rank, targets=tuple(range(6)), quant=None):
    """(base blob, adapter blob, Reference with the adapter, logit gate); asserts on the CPU that the
    adapter moves the float64 logits by at least 50 gates, so a delta that is dropped, bound to the
    wrong row or scaled wrongly cannot pass."""
    dims = DIMS[name]
    blob = W.synth_blob(dims, seed=123)
    ref_blob = mx_ref.dequantised_blob(blob, dims, quant, 2) if quant else blob
    # (four of six targets move the logits less: that adapter is drawn four times larger)
    sd, alpha = lora_ref.draw(dims, rank, seed=1000 + rank, targets=targets, scale=1.0 if len(targets) == 6 else 4.0)
    ref = Reference(lora_ref.model(ref_blob, dims, sd, alpha))
    probe = tokens(7, 64, V)
    with_ad = ref.get(probe, V)[0]
    gate = 2e-3 * max(1.0, float(with_ad.std()) / 1.6)
    st = (base := rwkv7_f64.Model(ref_blob)).new_state()
    moved = np.abs(with_ad - base.forward_rows(st, probe, V)).max()
    assert moved >= 50 * gate, (moved, gate)
    return blob, W.pack_adapter(sd, dims, alpha), ref, gate


def _adapter(dims, rank, seed):
    sd, alpha = lora_ref.draw(dims, rank, seed)
    return W.pack_adapter(sd, dims, alpha)


@contextlib.contextmanager
def _engine(blob, adapters=(), **kw):
    rt = rwkvtts.SharedRwkvRuntime(blob, **dict(dict(max_slots=4, token_chunk_size=128, use_graphs=False), **kw))
    try:
        for i, a in enumerate(adapters):
            rt.load_adapter(i, a)
        yield rt
    finally:
        rt.close()


@pytest.fixture(scope="module", params=list(DIMS))
def eng(request):
    """One engine per dims set with the rank-16 adapter as id 0 and the rank-64 adapter as id 1."""
    cases = [_case(request.param, r) for r in (16, 64)]
    with _engine(cases[0][0], [c[1] for c in cases]) as rt:
        yield request.param, rt, cases


@pytest.mark.parametrize("n", [1, 17, 70])
@pytest.mark.parametrize("ad", [0, 1], ids=["r16", "r64"])
def test_forward(eng, ad, n):
    name, rt, cases = eng
    _, _, ref, gate = cases[ad]
    for s in (2, 3):  # the input's slot and check_case's spare slot
        rt.set_slot_adapter(s, ad)
    check_case(rt, ref, [(tokens(200 + n, n, V), FULL, 2)], HEAD, gate, STATE_GATE, label=f"lora {name} r{16 + 48 * ad} [{n}]")


def test_mixed_ragged_step():
    """Segments of 5 / 16 / 23 / 1 rows bound to a / none / b / a in ONE step, ranks 16 and 48 resident
    together; the first and the last share a tile across the rows between them."""
    (blob, a16, ref_a, gate), (_, b48, ref_b, gate_b) = _case("c384", 16), _case("c384", 48)
    ref_0 = Reference(rwkv7_f64.Model(blob))
    with _engine(blob, [a16, b48]) as rt, _engine(blob) as plain:
        segs = [tokens(300 + i, n, V) for i, n in enumerate((5, 16, 23, 1))]
        for s, (ad, _) in enumerate(zip((0, None, 1, 0), segs)):
            rt.set_slot_adapter(s, ad)
        got, calls, _ = feed(rt, [(t, FULL, s) for s, t in enumerate(segs)], HEAD)
        assert calls == 1
        gate_0 = 2e-3 * max(1.0, float(ref_0.get(tokens(7, 64, V), V)[0].std()) / 1.6)
        for s, (g, t, (ref, gt)) in enumerate(zip(got, segs, ((ref_a, gate), (ref_0, gate_0), (ref_b, gate_b), (ref_a, gate)))):
            want, st = ref.get(t, HEAD)
            assert np.abs(g - want).max() < gt and np.abs(rt.read_slot(s) - st).max() < STATE_GATE, s
        alone, _, _ = feed(plain, [(segs[1], FULL, 1)], HEAD)
        assert np.array_equal(got[1], alone[0]) and np.array_equal(rt.read_slot(1), plain.read_slot(1))


@pytest.mark.parametrize("name,rank,targets,quant", [("tiny", 32, (0, 1, 2, 3), None), ("c384", 16, tuple(range(6)), "mxfp4")],
                         ids=["attention-only", "mxfp4-base"])
def test_masked_and_quantised(name, rank, targets, quant):
    """An adapter that carries the attention targets only; an adapter over two MXFP4 layers, against
    the float64 model of the dequantised blob."""
    blob, ad, ref, gate = _case(name, rank, targets, quant)
    with _engine(blob, [ad], **(dict(quant_layers=2, quant_type=quant) if quant else {})) as rt:
        for s in (0, 1):
            rt.set_slot_adapter(s, 0)
        check_case(rt, ref, [(tokens(400, 20, V), FULL, 0)], HEAD, gate, STATE_GATE, label=f"lora {name} {quant or 'masked'}")


def test_serve_path():
    """rwkvtts_generate_batch_ex with decode graphs: requests bound to a / b / none decode side by side."""
    dims = W.DIMS_MID
    blob = W.synth_blob(dims, seed=9)
    ads = [_adapter(dims, r, seed=r) for r in (16, 64)]
    with _engine(blob, ads, use_graphs=True) as rt, _engine(blob, use_graphs=True) as plain:
        def reqs(bind):
            out = [make_request(synth_text(500 + i), seed=700 + i, fixed=48) for i in range(3)]
            for r, ad in zip(out, bind):
                r.adapter = ad
            return out
        together = rt.generate_batch(reqs((0, 1, None)))
        assert rt.last_status == [0, 0, 0]
        for i, r in enumerate(reqs((0, 1, None))):
            assert rt.generate_batch([r]) == [together[i]], i
        base = plain.generate_batch(reqs((None, None, None)))
        assert together[2] == base[2]
        assert together[0] != base[0] and together[1] != base[1]
        rt.unload_adapter(0)  # no finished request holds an adapter
    # one request through DynamicBatchManager, its adapter by name
    with contextlib.closing(rwkvtts.DynamicBatchManager(blob, max_slots=4, token_chunk_size=128)) as mgr:
        mgr.load_adapter("b", ads[1])
        bound = reqs(("zz", "b", None))[1]
        assert mgr.generate_tts_batch([bound]) == [together[1]] and mgr.last_status == [0]
        with pytest.raises(ValueError):
            mgr.submit(reqs(("zz", None, None))[0])
        mgr.unload_adapter("b")
        assert mgr.adapters == {}


def test_refusals():
    dims = DIMS["tiny"]
    blob, good, _, _ = _case("tiny", 16)
    sd, alpha = lora_ref.draw(dims, 16, seed=1)

    def code(fn):
        with pytest.raises(E.RwkvTtsError) as e:
            fn()
        return e.value.code

    with _engine(W.synth_blob(dims, seed=1, dtype=E.DTYPE_F16)) as f16:
        assert code(lambda: f16.load_adapter(0, good)) == E.EUNSUPPORTED
    with _engine(blob) as rt:
        hdr = good.copy().view(np.uint32)
        hdr[5] = 24  # the rank
        assert code(lambda: rt.load_adapter(0, hdr.view(np.uint8))) == E.EINVAL
        assert code(lambda: rt.load_adapter(0, _adapter(dict(dims, n_embd=256), 16, seed=1))) == E.EINVAL
        nan = dict(sd)
        nan["blocks.1.ffn.value.lora_B"] = sd["blocks.1.ffn.value.lora_B"].copy()
        nan["blocks.1.ffn.value.lora_B"][-1, -1] = np.nan
        assert code(lambda: rt.load_adapter(0, W.pack_adapter(nan, dims, alpha))) == E.EINVAL
        assert code(lambda: rt.load_adapter(64, good)) == E.EINVAL
        rt.load_adapter(0, good)
        assert code(lambda: rt.load_adapter(0, good)) == E.EINVAL  # a live id
        rt.set_slot_adapter(1, 0)
        assert code(lambda: rt.unload_adapter(0)) == E.EBUSY
        rt.set_slot_adapter(1, None)
        rt.unload_adapter(0)
    # an unknown id in a request: it fails alone, its neighbour completes
    with _engine(W.synth_blob(W.DIMS_TINY, seed=7), use_graphs=True) as full:
        reqs = [make_request(synth_text(i), seed=i, fixed=8) for i in range(2)]
        reqs[0].adapter = 5
        out = full.generate_batch(reqs)
        assert full.last_status == [E.EINVAL, 0] and out[0] == ([], []) and len(out[1][1]) == 8
