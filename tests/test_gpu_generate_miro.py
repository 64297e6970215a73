"""Mirostat end to end: rwkvtts_generate_batch_ex with staggered admission and slots reused by
requests without Mirostat and with other parameters, the Python DynamicBatchManager
(rwkvtts_manager_submit_ex), LightweightTtsPipeline.generate_speech, stream_speech and
generate_long_speech.

The expected tokens come from the controller loop of tests/test_gpu_generate_penalty.py restated
here with tests/miro_ref.py in place of oracle.sample on the semantic rows of a Mirostat request
(after tests/penalty_ref.py where the request has penalties too). The logits are the device's own --
rwkvtts_infer on one slot, one token per call, bitwise the batched step's logits by the engine's
batching invariance -- so equality is exact for every request. mu itself is not returned by the
engine; a wrong threshold, or one left over from a slot's previous owner, shows in the tokens."""
import dataclasses

import numpy as np
import pytest

import join_ref
import miro_ref
import penalty_ref
import rwkvtts
from rwkvtts import codec as CC
from rwkvtts import weights as W
from rwkvtts.pipeline import LightweightTtsPipeline, LightweightTtsPipelineArgs, LongSpeech
from rwkvtts.runtime import Mirostat, Penalties, PhaseSampling, RnnInput, RnnInputBatch
from rwkvtts.segment import split_text
from rwkvtts.tokenizer import Tokenizer
from helpers import make_request, synth_text
from test_tokenizer import VOCAB

pytestmark = pytest.mark.gpu
EOS = rwkvtts.EOS_TOKEN
SEM_ROWS = EOS + 1
NEUTRAL = Penalties()


@pytest.fixture(scope="module")
def engines():
    blob = W.synth_blob(W.DIMS_TINY, seed=99)
    gen = rwkvtts.SharedRwkvRuntime(blob, max_slots=4, token_chunk_size=64, use_graphs=True)
    one = rwkvtts.SharedRwkvRuntime(blob, max_slots=1, token_chunk_size=64, use_graphs=False)  # the logits source
    yield blob, gen, one
    gen.close()
    one.close()


def _expected(one, oracle_mod, req):
    """(global, semantic) of one request: the controller loop on the device's single-slot logits.
    A semantic row is adjusted by the request's penalties over its own history, then sampled by
    miro_ref with the request's running mu (Mirostat) or by oracle.sample (without)."""
    a = req.args
    pen = a.penalties or NEUTRAL
    miro = a.mirostat
    zero_shot = req.ref_global_tokens is not None and req.ref_semantic_tokens is not None
    pinned = bool(req.pinned_voice)
    gp = a.global_sampling or PhaseSampling()
    sp = a.semantic_sampling or PhaseSampling()
    kg = 1 if req.greedy else (20 if gp.top_k is None else gp.top_k)
    ks = 1 if req.greedy else (80 if sp.top_k is None else sp.top_k)
    prompt = list(req.property_tokens) + [rwkvtts.TAG_2] + list(req.text_tokens) + [rwkvtts.TAG_0]
    if zero_shot or pinned:
        prompt += [min(max(g, 0), 4095) + rwkvtts.GLOBAL_TOKEN_OFFSET for g in req.ref_global_tokens] + [rwkvtts.TAG_1]
    one.reset_slot(0)

    def feed(tok):
        _, out = one.infer(RnnInput([RnnInputBatch([int(tok)])]), head_rows=SEM_ROWS, slots=[0])
        return out[0]

    state = dict(mu=miro_ref.initial_mu(miro.tau) if miro else None, last=None)
    rs = oracle_mod.Rng((a.seed + 2000) & (2 ** 64 - 1))

    def draw(row, masked):
        """One attempt; a Mirostat attempt is remembered so that emit() can move mu by it."""
        if miro is None:
            x = np.array(row, copy=True)
            if masked:
                x[EOS] = -np.inf
            return oracle_mod.sample(x, sp.temperature, sp.top_p, ks, None, rs)
        state["last"] = miro_ref.sample(row, state["mu"], rs.gen_f32(), masked=(EOS,) if masked else ())
        return state["last"].token

    def emit():
        if miro is not None:
            state["mu"] = miro_ref.update(state["mu"], miro.tau, miro.rate, state["last"].S, state["last"].p_tok)

    for t in prompt:
        logits = feed(t)
    limit = min(max(a.max_tokens, 0), rwkvtts.SEMANTIC_LIMIT)
    if req.fixed_semantic > 0:
        limit = min(req.fixed_semantic, rwkvtts.SEMANTIC_LIMIT)
    glob, sem = [], []
    if not zero_shot:
        if pinned:
            glob = list(req.ref_global_tokens)
        else:
            rg = oracle_mod.Rng((a.seed + 1000) & (2 ** 64 - 1))
            for i in range(rwkvtts.N_GLOBAL):
                if i > 0:
                    logits = feed(glob[-1] + rwkvtts.GLOBAL_TOKEN_OFFSET)
                glob.append(oracle_mod.sample(logits[:4096], gp.temperature, gp.top_p, kg, None, rg))  # never Mirostat
            feed(glob[-1] + rwkvtts.GLOBAL_TOKEN_OFFSET)
            logits = feed(rwkvtts.TAG_1)
        for i in range(limit):
            if i > 0:
                logits = feed(sem[-1])
            t = draw(penalty_ref.apply(logits, sem, pen), req.fixed_semantic > 0)
            if t == EOS:
                break
            emit()
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
        row = penalty_ref.apply(logits, sem, pen)
        t = draw(row, i < hard_min or req.fixed_semantic > 0)
        if t == EOS:
            if len(window) >= 12 and np.float32(sum(window)) / np.float32(len(window)) >= np.float32(0.7):
                break
            t = draw(row, True)  # the same adjusted row, the same mu
        emit()
        window = (window + [int(t != EOS)])[-12:]
        sem.append(t)
    return glob, sem


def _requests():
    ref_g, ref_s = list(range(100, 132)), list(range(40))

    def normal(i, max_tokens=24, **kw):
        return make_request(synth_text(700 + i, n=12), seed=900 + i, max_tokens=max_tokens, **kw)

    plain_miro = normal(1, max_tokens=40)
    plain_miro.args.mirostat = Mirostat()
    zero = make_request(synth_text(707, n=6), props=[], seed=907, fixed=20, ref_global=ref_g, ref_semantic=ref_s)
    zero.args.mirostat = Mirostat(tau=0.5, rate=1.0)
    pen = normal(0)
    pen.args.mirostat = Mirostat(tau=8.0, rate=0.1)
    pen.args.penalties = Penalties(repetition=1.3, frequency=0.7, window=4)
    fixed = make_request(synth_text(711, n=12), seed=911, fixed=30)
    fixed.args.mirostat = Mirostat(tau=5.0, rate=0.5)
    fixed.args.global_sampling = PhaseSampling(temperature=0.8, top_k=10)
    plain = normal(4)
    return dict(plain_miro=plain_miro, zero=zero, pen=pen, fixed=fixed, plain=plain)


def _pinned_from(req, glob):
    return dataclasses.replace(req, args=dataclasses.replace(req.args), ref_global_tokens=list(glob),
                               ref_semantic_tokens=None, pinned_voice=True)


def test_generate_batch_honours_mirostat(engines, oracle_mod):
    blob, gen, one = engines
    # default requests before any Mirostat request has run in this engine: the parent's tokens
    defaults = [make_request(synth_text(800 + i, n=12), seed=70 + i, max_tokens=24) for i in range(5)]
    assert all(r.args.mirostat is None for r in defaults)
    before = gen.generate_batch(defaults)
    assert list(gen.last_status) == [0] * 5
    assert before == [_expected(one, oracle_mod, r) for r in defaults]

    R = _requests()
    want = {k: _expected(one, oracle_mod, r) for k, r in R.items()}
    pinned = _pinned_from(R["plain_miro"], want["plain_miro"][0])  # the normal request's voice, the same parameters
    bad = make_request(synth_text(777, n=12), seed=5, max_tokens=24)
    bad.args.mirostat = Mirostat(tau=11.0)
    excl = make_request(synth_text(778, n=12), seed=6, max_tokens=24, greedy=True)
    excl.args.mirostat = Mirostat()
    # 8 requests on 4 slots: admission staggers, and slots are reused with and without Mirostat
    order = ["plain_miro", "zero", "pen", None, "fixed", "plain", None, "pinned"]
    batch = [R["plain_miro"], R["zero"], R["pen"], bad, R["fixed"], R["plain"], excl, pinned]
    got = gen.generate_batch(batch)
    status = list(gen.last_status)
    assert status[3] < 0 and got[3] == ([], []) and status[6] < 0 and got[6] == ([], [])  # they fail alone
    assert [s for i, s in enumerate(status) if i not in (3, 6)] == [0] * 6
    for name, g in zip(order, got):
        if name in R:
            assert g == want[name], name
            assert len(g[0]) == 32 and len(g[1]) > 0
    # the pinned request: the tokens of the normal request it was pinned from, and the loop's
    assert got[7] == got[0] == _expected(one, oracle_mod, pinned)
    # the plain request equals its result when run alone
    assert gen.generate_batch([R["plain"]])[0] == got[5]
    # a Mirostat request's tokens differ from the same request without it
    for name in ("plain_miro", "zero", "pen", "fixed"):
        r = _requests()[name]
        r.args.mirostat = None
        assert gen.generate_batch([r])[0] != want[name], name
    # a slot used by a Mirostat request, then by one without, then by one with other parameters: one
    # slot only, so every request inherits the slot of the one before it
    solo = rwkvtts.SharedRwkvRuntime(blob, max_slots=1, token_chunk_size=64, use_graphs=True)
    try:
        other = _requests()["plain_miro"]
        other.args.mirostat = Mirostat(tau=1.0, rate=0.7)
        seq = [R["plain_miro"], R["plain"], other, R["fixed"], R["plain"]]
        got3 = solo.generate_batch(seq)
        assert got3[0] == want["plain_miro"] and got3[1] == want["plain"] == got3[4] and got3[3] == want["fixed"]
        assert got3[2] == _expected(one, oracle_mod, other) != want["plain_miro"]
    finally:
        solo.close()
    # default requests after the Mirostat batches: the tokens from before them
    assert gen.generate_batch(defaults) == before


@pytest.fixture(scope="module")
def stack(engines):
    blob, gen, one = engines
    tok = Tokenizer(VOCAB)
    m = rwkvtts.DynamicBatchManager(blob, devices=[0], max_slots=4, token_chunk_size=64, tokenizer=tok)
    cd = CC.CODEC_DIMS_TINY
    voc = CC.BiCodecDetokenizer(CC.synth_codec_blob(cd, seed=11), cd)
    pipe = LightweightTtsPipeline(m, voc)
    yield pipe, m, voc, tok
    m.close()
    voc.close()
    for j in pipe._joiners.values():
        j.close()


def test_manager_pipeline_and_stream_honour_mirostat(engines, stack, oracle_mod):
    blob, gen, one = engines
    pipe, m, voc, tok = stack
    # the Python manager
    req = make_request(synth_text(31, n=12), seed=41, max_tokens=24)
    req.args.mirostat = Mirostat(tau=2.0, rate=0.3)
    want = _expected(one, oracle_mod, req)
    assert m.generate_tts_batch([req])[0] == want == gen.generate_batch([req])[0]
    # generate_speech and stream_speech
    args = LightweightTtsPipelineArgs(text="Hello world, this is RWKV speaking.", seed=12, max_tokens=40, emotion="HAPPY",
                                      mirostat=Mirostat())
    preq = pipe._request(args)
    g, s = gen.generate_batch([preq])[0]  # the engine-level result for the same seed
    assert (g, s) == _expected(one, oracle_mod, preq) and len(s) > 0
    plain = pipe._request(LightweightTtsPipelineArgs(text=args.text, seed=12, max_tokens=40, emotion="HAPPY"))
    assert gen.generate_batch([plain])[0] != (g, s)
    pcm = pipe.generate_speech(args)
    assert pcm.tobytes() == voc.decode_audio(g, s).tobytes()
    chunks = list(pipe.stream_speech(args, chunk_frames=8))
    assert len(chunks) >= 2 and chunks[-1].done and chunks[-1].t1 == len(s)
    assert np.concatenate(chunks).tobytes() == pcm.tobytes()  # the chunks are bitwise the whole decode
    with pytest.raises(ValueError):
        pipe.generate_speech(LightweightTtsPipelineArgs(text="x", mirostat=Mirostat(rate=2.0)))
    with pytest.raises(ValueError):
        pipe.generate_speech(LightweightTtsPipelineArgs(text="x", mirostat=Mirostat(),
                                                        semantic_sampling=PhaseSampling(temperature=0.8)))


def test_long_speech_gives_every_segment_its_own_threshold(engines, stack, oracle_mod):
    blob, gen, one = engines
    pipe, m, voc, tok = stack
    text = "Hello world, this is RWKV speaking. Is it fast?"
    miro = Mirostat(tau=2.0, rate=0.5)
    args = LightweightTtsPipelineArgs(text=text, seed=23, max_tokens=24, emotion="HAPPY", mirostat=miro)
    segs = split_text(text, tok.encode, 10)
    assert len(segs) == 2
    # segment 0 as generate_speech builds it, segment 1 pinned to its voice and seeded seed + 1: each
    # with the same parameters and a threshold that starts at 2 tau
    first = pipe._request(dataclasses.replace(args, text=segs[0].text.strip()))
    g0, s0 = _expected(one, oracle_mod, first)
    second = pipe._request(dataclasses.replace(args, text=segs[1].text.strip(), seed=24, voice_global_tokens=g0,
                                               pin_voice=True))
    assert second.pinned_voice and second.args.mirostat is miro and first.args.mirostat is miro
    g1, s1 = _expected(one, oracle_mod, second)
    assert g1 == g0 and s0 and s1
    out = pipe.generate_long_speech(args, segment_tokens=10, trim=False)
    assert isinstance(out, LongSpeech) and len(out.segments) == 2 and out.global_tokens == g0
    assert [s["status"] for s in out.segments] == [0, 0]
    assert [s["n_semantic"] for s in out.segments] == [len(s0), len(s1)]
    # the PCM is the join of the decode of exactly those tokens
    pcm = [voc.decode_audio(g0, s0), voc.decode_audio(g0, s1)]
    wantpcm = join_ref.join(pcm, [s.pause_ms * 16 for s in segs], trim=False)[0]
    assert np.asarray(out).tobytes() == wantpcm.tobytes()
