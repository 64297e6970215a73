"""Audio during decode on the MI355X: the engine's token progress (rwkvtts_generate_batch_stream),
the manager's polling stream, and stream_speech's chunks against the non-streamed results.
Tiny model, tiny codec; the windowed vocoder itself is in tests/test_gpu_codec_windows.py."""
import json
import os
import threading

import numpy as np
import pytest

import rwkvtts
from rwkvtts import codec as CC
from rwkvtts import weights as W
from rwkvtts.pipeline import LightweightTtsPipeline, LightweightTtsPipelineArgs
from rwkvtts.tokenizer import Tokenizer
from test_tokenizer import VOCAB
from helpers import make_request, synth_text, to_struct

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
H_TINY = 19


@pytest.fixture(scope="module")
def blob():
    return W.synth_blob(W.DIMS_TINY, seed=99)


@pytest.fixture(scope="module")
def engine(blob):
    rt = rwkvtts.SharedRwkvRuntime(blob, max_slots=8, token_chunk_size=128, use_graphs=True)
    yield rt
    rt.close()


def _requests():
    raf = json.load(open(os.path.join(GOLDEN, "raf_voice_05d8f5ed.json")))
    return [make_request(synth_text(100), seed=50, max_tokens=48),            # ends by EOS or at 48
            make_request(synth_text(7), seed=1, fixed=60),                    # exactly 60
            make_request(synth_text(5, n=10), props=[], seed=77, ref_global=raf["global_tokens"],
                         ref_semantic=raf["semantic_tokens"][:50])]           # zero-shot


class Calls:
    def __init__(self, n):
        self.calls = [[] for _ in range(n)]

    def __call__(self, i, g, first, new, done, status):
        self.calls[i].append((g, first, list(new), done, status))


def test_engine_progress(engine, blob):
    import oracle
    om = oracle.Model(blob)
    reqs = _requests()
    seen = Calls(3)
    out = engine.generate_batch(reqs, on_tokens=seen)
    assert engine.last_status == [0, 0, 0]
    for i, (r, (g, s)) in enumerate(zip(reqs, out)):
        q, _keep = to_struct(r)
        og, os_, _ = om.generate(q)
        assert (g, s) == (og, os_)
        calls = seen.calls[i]
        # contiguous, in order, each token exactly once; together the returned result
        pos = 0
        for _, first, new, _, status in calls:
            assert first == pos and status == 0
            pos += len(new)
        assert [t for c in calls for t in c[2]] == s
        # done exactly once, in the last call; the global tokens with every semantic token
        assert [c[3] for c in calls] == [False] * (len(calls) - 1) + [True]
        assert all(c[0] == g for c in calls if c[2] or c[3])
        assert all(len(c[2]) > 0 for c in calls[:-1])
    assert len(out[1][1]) == 60
    # fixed = 60: the sink runs between units of at most 8 decode steps, so the first delivery
    # cannot hold all 60 tokens
    c1 = seen.calls[1]
    assert len(c1) > 1 and c1[0][1] + len(c1[0][2]) < 60
    assert max(len(c[2]) for c in c1) <= 8  # one delivery per unit, one token per decode step at most


def test_sinks_do_not_change_results(engine):
    reqs = _requests()
    plain = engine.generate_batch(reqs)
    assert engine.generate_batch(reqs, on_tokens=Calls(3)) == plain
    assert engine.generate_batch(reqs, on_tokens=[None, None, None]) == plain   # the stream entry, no sinks
    one = Calls(3)
    assert engine.generate_batch(reqs, on_tokens=[None, one, None]) == plain    # a sink on one slot only
    assert not one.calls[0] and not one.calls[2] and [t for c in one.calls[1] for t in c[2]] == plain[1][1]
    # more requests than slots: slots are reused, each request's stream is its own
    many = [make_request(synth_text(300 + i), seed=400 + i, fixed=9 + i) for i in range(11)]
    seen = Calls(11)
    out = engine.generate_batch(many, on_tokens=seen)
    assert out == engine.generate_batch(many)
    for i, (g, s) in enumerate(out):
        assert [t for c in seen.calls[i] for t in c[2]] == s and seen.calls[i][-1][3]


def test_failed_request_ends_its_stream(engine):
    bad = make_request([10 ** 6], seed=3, fixed=5)  # a text id outside the vocabulary
    seen = Calls(2)
    out = engine.generate_batch([bad, make_request(synth_text(9), seed=4, fixed=12)], on_tokens=seen)
    assert out[0] == ([], []) and engine.last_status[0] < 0 and len(out[1][1]) == 12
    assert seen.calls[0] == [(None, 0, [], True, engine.last_status[0])]
    assert seen.calls[1][-1][3] and [t for c in seen.calls[1] for t in c[2]] == out[1][1]

    def boom(i, g, first, new, done, status):
        raise KeyError("sink")
    with pytest.raises(KeyError):
        engine.generate_batch([make_request(synth_text(9), seed=4, fixed=12)], on_tokens=boom)
    assert engine.generate_batch([make_request(synth_text(9), seed=4, fixed=12)]) == [out[1]]


class FixedPipe(LightweightTtsPipeline):
    """Requests with exactly 60 semantic tokens (the benchmark mode of the request struct)."""
    def _request(self, args):
        r = super()._request(args)
        r.fixed_semantic = 60
        return r


@pytest.fixture(scope="module")
def stack(blob):
    tok = Tokenizer(VOCAB)
    # two engines on one device
    m = rwkvtts.DynamicBatchManager(blob, devices=[0, 0], max_slots=4, token_chunk_size=64, tokenizer=tok)
    cd = CC.CODEC_DIMS_TINY
    voc = CC.BiCodecDetokenizer(CC.synth_codec_blob(cd, seed=11), cd)
    yield m, voc
    m.close()
    voc.close()


def test_manager_stream_tts(stack):
    m, voc = stack
    for req in _requests():
        want = m.generate_tts_batch([req])[0]
        incs = list(m.stream_tts(req))
        assert [d for _, _, d in incs] == [False] * (len(incs) - 1) + [True] and m.last_status == [0]
        assert [t for _, new, _ in incs for t in new] == want[1]
        assert incs[-1][0] == want[0] and all(g == want[0] for g, new, _ in incs if new)
    fixed = list(m.stream_tts(_requests()[1]))
    assert len(fixed) > 1 and len(fixed[0][1]) < 60   # progress, not one lump at the end
    bad = list(m.stream_tts(make_request([10 ** 6], seed=3, fixed=5)))
    assert bad == [(None, [], True)] and m.last_status[0] < 0
    st = m.stats()
    assert st["submitted"] == st["completed"] and st["waiters"] == 0


def _check_stream(pipe, args, chunk_frames=8):
    chunks = list(pipe.stream_speech(args, chunk_frames=chunk_frames))
    want = pipe.generate_speech(args)
    assert want.size == 60 * 320
    assert b"".join(chunks) == want.tobytes()                    # bitwise
    assert [(c.t0, c.t1) for c in chunks] == [(t, min(t + chunk_frames, 60)) for t in range(0, 60, chunk_frames)]
    assert all(c.t1 + H_TINY <= c.n_known or c.done for c in chunks)
    assert all(c.dtype == np.float32 and c.size == (c.t1 - c.t0) * 320 for c in chunks)
    return chunks


def test_stream_speech_bitwise(stack):
    m, voc = stack
    pipe = FixedPipe(m, voc)
    assert voc.halo() == H_TINY
    chunks = _check_stream(pipe, LightweightTtsPipelineArgs(text="Hello world, this is RWKV speaking.", seed=12))
    # audio before the request is done: the first chunk was decoded from fewer than 60 tokens
    assert not chunks[0].done and chunks[0].n_known < 60 and chunks[-1].done and chunks[-1].n_known == 60
    _check_stream(pipe, LightweightTtsPipelineArgs(text="one two three", seed=3), chunk_frames=16)
    # untokenisable text: the same second of silence as generate_speech
    out = list(pipe.stream_speech(LightweightTtsPipelineArgs(text="emoji \U0001F600")))
    assert len(out) == 1 and out[0].tobytes() == pipe.generate_speech(LightweightTtsPipelineArgs(text="emoji \U0001F600")).tobytes()


def test_stream_speech_concurrent_through_two_engines(stack):
    """Three streams at once through the manager's two engines and one decoder (its calls
    serialise on the decoder's lock)."""
    m, voc = stack
    pipe = FixedPipe(m, voc)
    texts = ["first stream", "second stream here", "and a third"]
    got, errs = [None] * 3, []

    def run(i):
        try:
            got[i] = list(pipe.stream_speech(LightweightTtsPipelineArgs(text=texts[i], seed=20 + i), chunk_frames=8))
        except BaseException as e:  # noqa: BLE001 -- reported by the main thread
            errs.append(e)
    th = [threading.Thread(target=run, args=(i,)) for i in range(3)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    for i in range(3):
        want = pipe.generate_speech(LightweightTtsPipelineArgs(text=texts[i], seed=20 + i))
        assert b"".join(got[i]) == want.tobytes()
        assert all(c.t1 + H_TINY <= c.n_known or c.done for c in got[i])
    assert sum(m.stats()["served"]) == m.stats()["completed"]
