"""Shared driver of the forward-pass shape and dims tests -- TEST INFRASTRUCTURE.

A *case* is a list of inputs (tokens, option, slot) fed to one engine through rt.infer, every
slot starting from the zero state. check_case() makes the three assertions of those tests:

1. against tests/rwkv7_f64.py (float64): every returned logits row and every slot's final state;
2. bitwise, segment alone: each input's logits and final state equal those of the same tokens
   run as the only input of one call on a freshly reset slot;
3. bitwise, row by row: they also equal the same tokens fed one token per call.

Float64 references are cached per (model, tokens): a module computes each of them once.
"""
import numpy as np

import rwkvtts

FULL, LAST = rwkvtts.RnnOption.Full, rwkvtts.RnnOption.Last


def tokens(seed, n, n_vocab):
    """n uniform random ids below n_vocab."""
    return np.random.RandomState(seed).randint(0, n_vocab, size=n).astype(np.int64).tolist()


def feed(rt, inputs, head_rows):
    """inputs: [(tokens, option, slot)]. Calls rt.infer with ALL inputs (emptied ones included)
    until every token is consumed. Returns (logits per input [rows][head_rows], n_calls,
    consumed per call)."""
    rem = [list(t) for t, _, _ in inputs]
    slots = [s for _, _, s in inputs]
    got = [[] for _ in inputs]
    history = []
    while True:
        inp = rwkvtts.RnnInput([rwkvtts.RnnInputBatch(list(r), o) for r, (_, o, _) in zip(rem, inputs)],
                               rt.token_chunk_size)
        left, out = rt.infer(inp, head_rows=head_rows, slots=slots)
        used = [len(r) - len(b.tokens) for r, b in zip(rem, left.batches)]
        history.append(used)
        for i, (_, o, _) in enumerate(inputs):
            if o == FULL:
                assert out[i].shape == (used[i], head_rows), (i, out[i].shape, used[i])
                got[i].append(out[i])
            elif out[i].size:
                assert used[i] == len(rem[i]) > 0, "OPT_LAST logits before the input's last token"
                got[i].append(out[i][None, :])
        rem = [list(b.tokens) for b in left.batches]
        if not any(rem):
            break
        assert sum(used) > 0, "a call with pending tokens consumed none"
    return [np.vstack(g) if g else np.zeros((0, head_rows), np.float32) for g in got], len(history), history


class Reference:
    """Float64 logits and final state of a token sequence from the zero state, cached."""

    def __init__(self, model):
        self.model = model
        self._cache = {}

    def get(self, toks, head_rows):
        key = tuple(toks)
        hit = self._cache.get(key)
        if hit is None or hit[0].shape[1] < head_rows:
            st = self.model.new_state()
            hit = (self.model.forward_rows(st, toks, head_rows), st)
            self._cache[key] = hit
        return hit[0][:, :head_rows], hit[1]


def check_case(rt, ref, inputs, head_rows, logit_gate, state_gate, history=None, got=None, label=""):
    """The three assertions for one case. `inputs`: [(tokens, option, slot)], each slot starting
    from zero. `got`: logits per input when the caller already ran the case (in several calls of its
    own); otherwise the case is fed here and the tokens each call consumes must equal `history`
    (default: one call that takes everything). Returns the measured (max logit error, max state
    error) against float64 and prints them."""
    n_slots = rt.max_slots
    if got is None:
        for _, _, s in inputs:
            rt.reset_slot(s)
        got, calls, hist = feed(rt, inputs, head_rows)
        assert hist == (history or [[len(t) for t, _, _ in inputs]]), hist
    states = [rt.read_slot(s) for _, _, s in inputs]
    fails = []  # every miss of the case, so one run shows which of the three assertions hold
    lerr = serr = 0.0
    for i, (toks, opt, slot) in enumerate(inputs):
        if not toks:
            assert got[i].shape[0] == 0
            if states[i].any():
                fails.append(f"input {i}: an empty input changed its slot")
            continue
        want, st = ref.get(toks, head_rows)
        if opt == LAST:
            want = want[-1:]
        assert got[i].shape == want.shape, (i, got[i].shape, want.shape)
        le, se = np.abs(got[i] - want).max(), np.abs(states[i] - st).max()
        lerr, serr = max(lerr, le), max(serr, se)
        if not le < logit_gate:
            worst = int(np.abs(got[i] - want).max(axis=1).argmax())
            fails.append(f"input {i} ({len(toks)} rows): logits differ from float64 by {le:.3g} (row {worst})")
        if not se < state_gate:
            fails.append(f"input {i} ({len(toks)} rows): state differs from float64 by {se:.3g}")
    for i, (toks, opt, slot) in enumerate(inputs):
        if not toks:
            continue
        spare = (slot + 1) % n_slots
        # 2. the segment alone, one call, fresh slot
        rt.reset_slot(spare)
        alone, calls, _ = feed(rt, [(toks, opt, spare)], head_rows)
        assert calls == 1 or len(toks) > rt.token_chunk_size
        bad = np.flatnonzero((alone[0] != got[i]).any(axis=1))
        if bad.size:
            fails.append(f"input {i} ({len(toks)} rows): rows {bad[:8].tolist()} differ from the segment run alone")
        if not np.array_equal(rt.read_slot(spare), states[i]):
            fails.append(f"input {i} ({len(toks)} rows): state differs from the segment run alone")
        # 3. one token per call
        rt.reset_slot(spare)
        rows = []
        for t in toks:
            _, o = rt.infer(rwkvtts.RnnInput([rwkvtts.RnnInputBatch([t], FULL)], rt.token_chunk_size),
                            head_rows=head_rows, slots=[spare])
            rows.append(o[0])
        rows = np.vstack(rows)
        if opt == LAST:
            rows = rows[-1:]
        bad = np.flatnonzero((rows != got[i]).any(axis=1))
        if bad.size:
            fails.append(f"input {i} ({len(toks)} rows): rows {bad[:8].tolist()} differ from one token per call")
        if not np.array_equal(rt.read_slot(spare), states[i]):
            fails.append(f"input {i} ({len(toks)} rows): state differs from one token per call")
    print(f"FWD-ERR {label} logit {lerr:.3g} state {serr:.3g}")
    assert not fails, "\n".join(fails)
    return lerr, serr
