"""Typical sampling without a GPU: the sampler's logf against libm, tests/typ_ref.py on rows checked by hand,
and the option from the Python surface down to the C block (runtime.Typical -> request_ext ->
_ffi.RequestExtV2, the pipeline's entry points, both HTTP bodies), after tests/test_miro_marshalling.py."""
import ctypes
import json

import numpy as np
import pytest

import typ_ref
from rwkvtts import _ffi
from rwkvtts import server as SV
from rwkvtts.pipeline import LightweightTtsPipeline, LightweightTtsPipelineArgs
from rwkvtts.runtime import Mirostat, Penalties, PhaseSampling, SamplerArgs, TtsBatchRequest, Typical, request_ext
from test_miro_marshalling import _refused_everywhere
from test_sampling_marshalling import FakeCodec, RecordingManager

P = typ_ref.Params
TWO, ONE_BIG = {3: 0.75, 9: 0.25}, {1: 0.05, 2: 0.05, 5: 0.9}
HAND_ROWS = [
    # p = (0.75, 0.25): entropy 0.562, surprises 0.288 and 1.386, so id 3 is nearer. tau 0.5 keeps id 3
    # alone (cum is 0.75 > 0.5 before id 9), tau 0.8 both; temperature 0.5 squares them to (0.9, 0.1)
    (TWO, P(), 0.99, 3, [3]), (TWO, P(tau=0.8), 0.76, 9, [3, 9]), (TWO, P(tau=0.8, top_k=1), 0.76, 3, [3]),
    (TWO, P(tau=0.8, temperature=0.5), 0.89, 3, [3, 9]), (TWO, P(tau=0.8, temperature=0.5), 0.91, 9, [3, 9]),
    # a uniform row: every key equal, ascending id decides; cum 0.25, 0.5, 0.75, 1
    (None, P(tau=1.0, top_k=4), 0.6, 2, [0, 1, 2, 3]),
    # surprises 0.105 (id 5) and 3.0 (ids 1, 2), entropy 0.394: id 5 first, and it alone exceeds tau
    (ONE_BIG, P(), 0.999, 5, [5]), (ONE_BIG, P(tau=0.97), 0.93, 1, [5, 1, 2]),
]


def test_logf_matches_glibc_on_every_float_of_its_domain():
    # csrc/exact_math.h glibc_logf against libm's logf (a function pointer) on every positive float up to 1.0,
    # subnormals included (0x3f800000 values), swept natively by the library's host hook
    ref, first_bad = ctypes.cast(ctypes.CDLL("libm.so.6").logf, ctypes.c_void_p), ctypes.c_uint32(0)
    bad = _ffi.lib().rwkvtts_debug_logf_sweep(1, 0x3F800000, 1, ref, ctypes.byref(first_bad))
    assert bad == 0, (bad, hex(first_bad.value))


@pytest.mark.parametrize("probs,prm,r,tok,kept", HAND_ROWS)
def test_restatement_on_hand_rows(probs, prm, r, tok, kept):
    row = np.zeros(typ_ref.N_IDS, np.float32)
    if probs:
        row[:] = -np.inf
        for i, v in probs.items():
            row[i] = np.log(v)
    assert list(typ_ref.kept_values(typ_ref.miro_ref.softmax(row), prm)[0]) == kept
    assert typ_ref.sample(row, prm, r) == (tok, len(kept))


BAD = [dict(tau=-0.1), dict(tau=float("nan")), dict(top_k=0), dict(top_k=8194), dict(top_k=1.5), dict(temperature=0),
       dict(temperature=float("inf")), dict(presence_penalty=float("inf")), dict(frequency_penalty="0.3"),
       dict(penalty_decay=0), dict(penalty_decay=1.01), dict(tau=True)]
EXCLUDED = dict(semantic_sampling=PhaseSampling(temperature=0.8), penalties=Penalties(presence=1.0), mirostat=Mirostat())
FIELDS = ("tau", "temperature", "presence_penalty", "frequency_penalty", "penalty_decay")
_typ = lambda x: (x.struct_size, x.typical_set, x.typical.top_k) + tuple(round(getattr(x.typical, k), 6) for k in FIELDS)  # noqa: E731


def test_typical_reaches_the_ext_block(tmp_path):
    V2 = _ffi.RequestExtV2
    assert (ctypes.sizeof(_ffi.RequestExt), ctypes.sizeof(V2), V2.typical_set.offset, V2.typical.offset) == (16, 44, 16, 20)
    r = TtsBatchRequest([1, 2, 3], args=SamplerArgs(seed=1))
    assert request_ext(r) is None
    r.args.typical = Typical()  # ai00's defaults
    assert _typ(request_ext(r)) == (44, 1, 128, 0.5, 1.0, 0.3, 0.3, 0.99654) and request_ext(r).mirostat_set == 0
    r.args.typical, r.args.mirostat = None, Mirostat()  # without typical sampling the block stays the 16-byte one
    assert request_ext(r).struct_size == 16
    m = RecordingManager()
    pipe = LightweightTtsPipeline(m, FakeCodec())
    # a bad value or an excluded combination is refused by all five entry points before anything is generated
    for kw in [dict(typical=Typical(**b)) for b in BAD] + [dict(typical={"tau": 0.5})] + \
            [dict(typical=Typical(), **{k: v}) for k, v in EXCLUDED.items()]:
        _refused_everywhere(pipe, m, LightweightTtsPipelineArgs(text="abc", **kw))
    typ = Typical(tau=0.9, top_k=8193, penalty_decay=1.0)
    args = LightweightTtsPipelineArgs(text="abc", seed=4, typical=typ, global_sampling=PhaseSampling(temperature=0.9))
    pipe.generate_speech(args)
    pipe.generate_speech_batch([args])
    list(pipe.stream_speech(args))
    assert len(m.seen) == 3 and all(q.args.typical is typ and _typ(request_ext(q))[2:4] == (8193, 0.9) for q in m.seen)
    assert pipe._request(args).args.typical is typ  # the long-form entry points derive their requests from this one

    def both(**body):
        n = len(m.seen)
        c1, _ = SV.handle_tts_json(json.dumps(dict(body, text="hi")), pipe, str(tmp_path))
        c2, it = SV.handle_tts_stream(dict(body, text="hi"), pipe, str(tmp_path))
        b"".join(it)
        return (c1, c2), [request_ext(q) for q in m.seen[n:]]

    codes, xs = both(typical={"tau": 0.25, "top_k": 64})  # a key left out keeps its default
    assert codes == (200, 200) and [_typ(x) for x in xs] == [(44, 1, 64, 0.25, 1.0, 0.3, 0.3, 0.99654)] * 2
    assert both(typical=None) == ((200, 200), [None, None])
    for bad in BAD + [{"rate": 0.1}, [0.5], 0.5, True]:
        assert both(typical=bad) == ((400, 400), []), bad
    for other in ({"semantic_sampling": {"temperature": 0.8}}, {"penalties": {"presence": 1.0}}, {"mirostat": {}}):
        assert both(typical={}, **other) == ((400, 400), []), other
