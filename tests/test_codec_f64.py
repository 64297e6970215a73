"""The float64 restatement of the vocoder (tests/codec_f64.py) against the f32 oracle, and what the
gates of tests/test_gpu_codec_dims.py resolve (CPU only).

  * the Python layout agrees with the library's;
  * on every utterance the GPU tests compare with float64, the f32 oracle is within a QUARTER of
    the end-to-end gates (5e-4 max abs, 1e-4 relative L2): the gates then measure the GPU, not the
    reference's own rounding; the new sets' PCM is not saturated;
  * launch() on the inputs a capture would deliver reproduces decode()'s conv outputs;
  * the random-walk gate 8 sqrt(m) 2^-23 A is adopted per launch class only where a numpy f32
    one-addend-at-a-time accumulation of the same addends stays inside it at every element;
  * every mutation of codec_f64.MUTATIONS breaks the adopted per-launch gate by >= 10x on every
    launch it applies to, and the end-to-end gates by >= 10x on every dims set.
"""
import numpy as np
import pytest

from rwkvtts import codec
import codec_f64 as F

WEIGHTS = ("bf16", "f32")
model_factor = F.model_factor


@pytest.mark.parametrize("name", ["tiny", "full", "u2", "u3", "u1"])
def test_layout_matches_library(name):
    d = F.dims_of(name)
    assert F.offset(d, -1, 0, 0) == codec.codec_blob_floats(d)
    # every tensor lies inside the blob, 64-float aligned, in layout order
    last = 64
    for g, (nidx, nt) in enumerate(((1, len(F.CD)), (d["prenet_layers"], len(F.CB)), (d["n_up"], len(F.CU)))):
        for i in range(nidx):
            for t in range(nt):
                o = F.offset(d, g, i, t)
                assert o == last and o % 64 == 0 and F.numel(d, g, i, t) > 0
                last = o + ((F.numel(d, g, i, t) + 63) & ~63)
    assert last == F.offset(d, -1, 0, 0)


def _oracle_cases():
    out = [("tiny", T, T) for T in (1, 5, 37)]
    for name in F.NEW_SETS:
        out += [(name, T, seed) for T, seed in F.gpu_cases(name)]
    return out


@pytest.mark.parametrize("wname", WEIGHTS)
@pytest.mark.parametrize("name,T,seed", _oracle_cases())
def test_oracle_within_a_quarter_of_the_gates(oracle_mod, name, T, seed, wname):
    g, s, ref = F.reference(name, wname, T, seed)
    got = oracle_mod.codec_decode(codec.make_codec_dims(F.dims_of(name)), F.blob(name, wname), s, g, threads=16)
    assert got.shape == ref.shape == (T * F.HOP,)
    ma, rl = F.pcm_errors(got, ref)
    print(f"{name} {wname} T={T}: oracle vs float64 max abs {ma:.2e} rel L2 {rl:.2e}")
    assert ma <= F.PCM_ATOL / 4 and rl <= F.PCM_RTOL_L2 / 4, (ma, rl)
    if name in F.NEW_SETS:
        assert ref.std() > 0.05 and np.abs(ref).max() < 1.0, (ref.std(), np.abs(ref).max())  # not saturated


# ---- per launch -------------------------------------------------------------------------------------
# (set, weights, forms, T): every launch of these decodes. T = 5 per set, weight path and form; the
# shipped sets at the lengths the GPU per-launch checks use (TINY 37, FULL 6) in their default form.
LAUNCH_CASES = [(n, w, f, 5) for n in ("u2", "u3", "u1", "tiny") for w in WEIGHTS for f in (0, F.FORM_SEPARATE_RESUNIT)]
LAUNCH_CASES += [("tiny", "bf16", 0, 37), ("full", "bf16", 0, 6), ("full", "f32", 0, 6)]
_launch_results = {}


def _launches(name, wname, forms, T):
    """[(rec, wt, inputs, clean launch() result)] of one decode, from the float64 decode's convs. Cached."""
    key = (name, wname, forms, T)
    if key not in _launch_results:
        d, w = F.dims_of(name), F.blob(name, wname)
        g, s = F.tokens(d, T, T)
        _, convs = F.decode(d, w, s, g)
        plan = codec.launch_plan(d, wname == "f32", forms, 1, T)
        idxs = F.plan_convs(plan)
        assert idxs[-1][-1] == len(convs) - 1, "the launch plan and the float64 decode disagree on the conv list"
        out = []
        for rec, idx in zip(plan, idxs):
            c = convs[idx[-1]]
            assert (rec["co"], rec["s"]) == (c["co"], c["s"]) and rec["ci"] == convs[idx[0]]["ci"]
            inp = F.synthetic_capture(rec, convs, idx)
            wt = F.launch_weights(d, w, rec)
            o = F.launch(rec, wt, *inp, [T])[0]
            out.append((rec, wt, inp, o, c))
        _launch_results[key] = out
    return _launch_results[key]


@pytest.mark.parametrize("name,wname,forms,T", LAUNCH_CASES)
def test_launch_reproduces_decode_and_f32_emulation_stays_inside_the_model_gate(name, wname, forms, T):
    worst = {}
    for rec, wt, (xh, xl, res, rb), o, c in _launches(name, wname, forms, T):
        # launch() sees the input through its bf16 hi + lo split (2^-16 relative per element) and, on
        # the bf16 path, the f32 weights rounded to bf16 (2^-9): against decode()'s unsplit float64
        tol = (2.0 ** -8 if wname == "f32" and not rec["wlo"] else 2.0 ** -14)
        scale = np.abs(c["y"]).max()
        assert np.abs(o["y"] - c["y"]).max() <= tol * max(scale, 1.0) * (4 if rec["kind"] == 2 else 1), F.launch_class(rec)
        acc32 = F.f32_tap_sum(rec, wt, xh[0], xl[0])
        if rec["kind"] == 2:
            exact, A, m = o["mid"] - wt["bias"], o["mid_A"], o["mid_m"]
        else:
            exact, A, m = o["v0"] - wt["bias"] - (rb[0] if rb is not None else 0.0), o["A"], o["m"]
        assert (A > 0).all()
        ratio = float((np.abs(acc32 - exact) / (2.0 ** -23 * A)).max())
        cls = F.launch_class(rec)
        worst[cls] = max(worst.get(cls, 0.0), ratio / np.sqrt(m))
        assert ratio <= model_factor(rec)(m), (cls, ratio, m)
        assert ratio <= m  # and the derived hard gate, a fortiori
    print(f"{name} {wname} forms={forms} T={T}: f32 emulation max |err| / (sqrt(m) 2^-23 A) per class: "
          + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))


def _mutation_ratio(rec, wt, inp, o, T, mut):
    """max over elements of |mutated - clean| / adopted gate, or None if the fault does not apply."""
    try:
        om = F.launch(rec, wt, *inp, [T], mutate=mut)[0]
    except ValueError:
        return None
    gy, gp = F.gates(rec, wt, o, model_factor(rec))
    r = float((np.abs(om["y"] - o["y"]) / gy).max())
    if gp is not None:
        r = max(r, float((np.abs(om["planes"] - o["planes"]) / gp).max()))
    return r


def test_mutations_break_the_per_launch_gate():
    """Every fault, on every launch it applies to, moves some element by >= 10x its adopted gate; and
    every launch class of LAUNCH_CASES has seen every fault that can apply to it (a residual, more
    than one tap)."""
    seen = {}
    for name, wname, forms, T in LAUNCH_CASES:
        if name == "full":
            continue  # (its classes are covered by the small sets; FULL is in the emulation test)
        for rec, wt, inp, o, _ in _launches(name, wname, forms, T):
            for mut in F.MUTATIONS:
                r = _mutation_ratio(rec, wt, inp, o, T, mut)
                if r is None:
                    continue
                key = (F.launch_class(rec), mut)
                seen[key] = min(seen.get(key, np.inf), r)
                assert r >= 10.0, (name, wname, forms, key, r)
    classes = {c for c, _ in seen}
    for c in classes:
        assert (c, "zero_row") in seen and (c, "neighbour_row") in seen
        if ",1," not in c:  # more than one tap
            assert (c, "drop_tap") in seen, c
        if c.startswith("convT"):
            assert (c, "drop_tap") in seen, c
    assert any(m == "skip_residual" and c.startswith("fused") for c, m in seen)
    print("per-launch mutation matrix, min |delta| / gate: " +
          "; ".join(f"{c} {m} {r:.0f}" for (c, m), r in sorted(seen.items())))


@pytest.mark.parametrize("name", ["tiny", "u2", "u3", "u1"])
def test_mutations_break_the_end_to_end_gates(name):
    """The same faults through the whole decoder at T = 5: each moves the PCM by >= 10x one of the
    end-to-end gates, at the first and last ConvTranspose, conv_in, and the first and last residual
    unit. (The weakest is a neighbouring-row read in the last stage's dilation-9 conv7, 17-42x: one
    32-channel chunk of one tap of one row.)"""
    d, w = F.dims_of(name), F.blob(name, "bf16")
    g, s = F.tokens(d, 5, 5)
    pcm, convs = F.decode(d, w, s, g, keep=False)
    plan = codec.launch_plan(d, False, F.FORM_SEPARATE_RESUNIT, 1, 5)
    names = [c["name"] for c in convs]
    last = d["n_up"] - 1
    targets = {names.index("conv_in"), names.index("convT.0"), names.index(f"convT.{last}"), names.index("res1.0.0"),
               names.index(f"res7.{last}.2"), names.index(f"res1.{last}.2")}
    applied = set()
    for i in sorted(targets):
        for mut in F.MUTATIONS:
            try:
                p2, _ = F.decode(d, w, s, g, mutate=(i, mut, 32 * plan[i]["nwv"], plan[i]["tn"]), keep=False)
            except ValueError:
                continue
            ma, rl = F.pcm_errors(p2, pcm)
            print(f"{name} {names[i]} {mut}: max abs {ma / F.PCM_ATOL:.0f}x, rel L2 {rl / F.PCM_RTOL_L2:.0f}x the gate")
            assert ma >= 10 * F.PCM_ATOL or rl >= 10 * F.PCM_RTOL_L2, (names[i], mut, ma, rl)
            applied.add(mut)
    assert applied == set(F.MUTATIONS)
