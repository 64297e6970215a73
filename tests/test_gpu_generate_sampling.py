"""Per-request temperature / top-p / top-k end to end: rwkvtts_generate_batch with staggered
admission, the Python DynamicBatchManager, LightweightTtsPipeline.generate_speech and
stream_speech.

The expected tokens come from the phase rules restated here (oracle/controller.c's loop, which
cannot take the parameters) around oracle.sample, which can. The logits it samples from are the
device's own -- rwkvtts_infer on one slot, one token per call, bitwise the batched step's logits by
the engine's batching invariance -- so forward-pass rounding cannot flip a token and equality is
exact for every request."""
import numpy as np
import pytest

import rwkvtts
from rwkvtts import codec as CC
from rwkvtts import weights as W
from rwkvtts.pipeline import LightweightTtsPipeline, LightweightTtsPipelineArgs
from rwkvtts.runtime import PhaseSampling, RnnInput, RnnInputBatch
from rwkvtts.tokenizer import Tokenizer
from helpers import make_request, synth_text
from test_tokenizer import VOCAB

pytestmark = pytest.mark.gpu
EOS = rwkvtts.EOS_TOKEN
SEM_ROWS = EOS + 1


@pytest.fixture(scope="module")
def engines():
    blob = W.synth_blob(W.DIMS_TINY, seed=99)
    gen = rwkvtts.SharedRwkvRuntime(blob, max_slots=4, token_chunk_size=64, use_graphs=True)
    one = rwkvtts.SharedRwkvRuntime(blob, max_slots=1, token_chunk_size=64, use_graphs=False)  # the logits source
    yield blob, gen, one
    gen.close()
    one.close()


def _expected(one, oracle_mod, req):
    """(global, semantic) of one request: the controller loop on the device's single-slot logits."""
    a = req.args
    zero_shot = req.ref_global_tokens is not None and req.ref_semantic_tokens is not None
    gp = a.global_sampling or PhaseSampling()
    sp = a.semantic_sampling or PhaseSampling()
    kg = 20 if gp.top_k is None else gp.top_k
    ks = 80 if sp.top_k is None else sp.top_k
    prompt = list(req.property_tokens) + [rwkvtts.TAG_2] + list(req.text_tokens) + [rwkvtts.TAG_0]
    if zero_shot:
        prompt += [min(max(g, 0), 4095) + rwkvtts.GLOBAL_TOKEN_OFFSET for g in req.ref_global_tokens] + [rwkvtts.TAG_1]
    one.reset_slot(0)

    def feed(tok):
        _, out = one.infer(RnnInput([RnnInputBatch([int(tok)])]), head_rows=SEM_ROWS, slots=[0])
        return out[0]

    for t in prompt:
        logits = feed(t)
    limit = min(max(a.max_tokens, 0), rwkvtts.SEMANTIC_LIMIT)
    if req.fixed_semantic > 0:
        limit = min(req.fixed_semantic, rwkvtts.SEMANTIC_LIMIT)
    glob, sem = [], []
    rs = oracle_mod.Rng((a.seed + 2000) & (2 ** 64 - 1))
    if not zero_shot:
        rg = oracle_mod.Rng((a.seed + 1000) & (2 ** 64 - 1))
        for i in range(rwkvtts.N_GLOBAL):
            if i > 0:
                logits = feed(glob[-1] + rwkvtts.GLOBAL_TOKEN_OFFSET)
            glob.append(oracle_mod.sample(logits[:4096], gp.temperature, gp.top_p, kg, None, rg))
        feed(glob[-1] + rwkvtts.GLOBAL_TOKEN_OFFSET)
        logits = feed(rwkvtts.TAG_1)
        for i in range(limit):
            if i > 0:
                logits = feed(sem[-1])
            row = logits.copy()
            if req.fixed_semantic > 0:
                row[EOS] = -np.inf
            t = oracle_mod.sample(row, sp.temperature, sp.top_p, ks, None, rs)
            if t == EOS:
                break
            sem.append(t)
        return glob, sem
    glob = [min(max(g, 0), 4095) for g in req.ref_global_tokens[:rwkvtts.N_GLOBAL]]
    tlen = len(req.text_tokens)
    est = int(np.ceil(np.float32(tlen) * np.float32(1.8)))
    hard_min = min(int(np.floor(np.float32(rwkvtts.SEMANTIC_LIMIT) * np.float32(0.9))), max(min(max(tlen // 4, 8), 64), est))
    zlimit = limit if req.fixed_semantic > 0 else rwkvtts.SEMANTIC_LIMIT
    window = []
    for i in range(zlimit):
        if i > 0:
            logits = feed(sem[-1])
        row = logits.copy()
        if i < hard_min or req.fixed_semantic > 0:
            row[EOS] = -np.inf
        t = oracle_mod.sample(row, sp.temperature, sp.top_p, ks, None, rs)
        if t == EOS:
            if len(window) >= 12 and np.float32(sum(window)) / np.float32(len(window)) >= np.float32(0.7):
                break
            row[EOS] = -np.inf
            t = oracle_mod.sample(row, sp.temperature, sp.top_p, ks, None, rs)
        window = (window + [int(t != EOS)])[-12:]
        sem.append(t)
    return glob, sem


def _requests():
    ref_g, ref_s = list(range(100, 132)), list(range(40))

    def normal(i, **kw):
        return make_request(synth_text(700 + i, n=12), seed=900 + i, max_tokens=24, **kw)

    def zero(i, **kw):
        return make_request(synth_text(700 + i, n=6), props=[], seed=900 + i, fixed=20, ref_global=ref_g,
                            ref_semantic=ref_s, **kw)

    reqs = [normal(0), zero(1), normal(2), normal(3), zero(4), normal(5)]
    reqs[2].args.semantic_sampling = PhaseSampling(temperature=0.8)                  # the fast path's powf
    reqs[3].args.global_sampling = PhaseSampling(temperature=1.3, top_p=0.5, top_k=0)  # general path, global rows
    reqs[4].args.semantic_sampling = PhaseSampling(temperature=0.7, top_p=1.0, top_k=300)
    reqs[4].args.global_sampling = PhaseSampling(temperature=2.0)                    # zero-shot: accepted, unused
    reqs[5].args.global_sampling = PhaseSampling(top_p=0.9, top_k=50)
    reqs[5].args.semantic_sampling = PhaseSampling(temperature=1.25, top_p=0.5, top_k=0)  # 8193 values sorted
    return reqs


def test_generate_batch_honours_sampling(engines, oracle_mod):
    blob, gen, one = engines
    reqs = _requests()
    bad = make_request(synth_text(777, n=12), seed=5, max_tokens=24)
    bad.args.semantic_sampling = PhaseSampling(temperature=9.0)
    got = gen.generate_batch(reqs[:3] + [bad] + reqs[3:])  # 7 requests on 4 slots: admission staggers
    status = list(gen.last_status)
    assert status[3] < 0 and got[3] == ([], [])  # the invalid one fails alone
    assert [s for i, s in enumerate(status) if i != 3] == [0] * 6
    got = got[:3] + got[4:]
    for i, r in enumerate(reqs):
        assert got[i] == _expected(one, oracle_mod, r), i
        assert len(got[i][0]) == 32 and 0 < len(got[i][1]) <= 24
    # the requests without sampling are untouched by their neighbours' parameters
    plain = [make_request(synth_text(800 + i, n=12), seed=70 + i, max_tokens=24) for i in range(3)]
    alone = gen.generate_batch([reqs[0], reqs[1]] + plain)
    assert alone[0] == got[0] and alone[1] == got[1]
    # and a set phase changes the tokens (the parameters reach the sampler)
    unset = _requests()[2]
    unset.args.semantic_sampling = None
    assert gen.generate_batch([unset])[0] != got[2]


@pytest.fixture(scope="module")
def stack(engines):
    blob, gen, one = engines
    tok = Tokenizer(VOCAB)
    m = rwkvtts.DynamicBatchManager(blob, devices=[0], max_slots=4, token_chunk_size=64, tokenizer=tok)
    cd = CC.CODEC_DIMS_TINY
    voc = CC.BiCodecDetokenizer(CC.synth_codec_blob(cd, seed=11), cd)
    yield LightweightTtsPipeline(m, voc), m, voc
    m.close()
    voc.close()


def test_manager_pipeline_and_stream_honour_sampling(engines, stack, oracle_mod):
    blob, gen, one = engines
    pipe, m, voc = stack
    # the Python manager
    req = make_request(synth_text(31, n=12), seed=41, max_tokens=24)
    req.args.semantic_sampling = PhaseSampling(temperature=0.8, top_k=40)
    want = _expected(one, oracle_mod, req)
    assert m.generate_tts_batch([req])[0] == want == gen.generate_batch([req])[0]
    # generate_speech and stream_speech
    args = LightweightTtsPipelineArgs(text="Hello world, this is RWKV speaking.", seed=12, max_tokens=40,
                                      semantic_sampling=PhaseSampling(temperature=0.7, top_p=0.9),
                                      global_sampling=PhaseSampling(top_k=0))
    preq = pipe._request(args)
    g, s = gen.generate_batch([preq])[0]  # the engine-level result for the same seed
    assert (g, s) == _expected(one, oracle_mod, preq) and len(s) > 0
    plain = pipe._request(LightweightTtsPipelineArgs(text=args.text, seed=12, max_tokens=40))
    assert gen.generate_batch([plain])[0] != (g, s)
    pcm = pipe.generate_speech(args)
    assert pcm.tobytes() == voc.decode_audio(g, s).tobytes()
    chunks = list(pipe.stream_speech(args, chunk_frames=8))
    assert len(chunks) >= 2 and chunks[-1].done and chunks[-1].t1 == len(s)
    assert np.concatenate(chunks).tobytes() == pcm.tobytes()
    with pytest.raises(ValueError):
        pipe.generate_speech(LightweightTtsPipelineArgs(text="x", semantic_sampling=PhaseSampling(temperature=0.01)))
