"""The vocoder on dims sets its tests never ran, against float64, end to end and launch by launch.

Three sets (tests/codec_f64.py: u2, u3, u1; what each reaches: tests/test_codec_plan_cpu.py), each
with bf16-exact weights and with f32 weights (the weight hi + lo kernels), each in the default form
and with RWKVTTS_CODEC_FORM_SEPARATE_RESUNIT, at T in (1, 5), a ragged batch, and the smallest
lengths at which the XCD-mapped grid has surplus blocks. Per case:

  1. PCM against the float64 restatement at the end-to-end gates of tests/test_gpu_codec.py (the f32
     oracle alone is within a quarter of them on these utterances: tests/test_codec_f64.py);
  2. batch == single, bitwise;
  3. EVERY k_conv launch against codec_f64.launch() on the launch's own captured inputs
     (rwkvtts_codec_debug_capture), at the per-launch gates below -- also on the shipped shapes
     (TINY at T = 37, FULL at T = 6, both weight paths);
  4. one windowed decode per set, bitwise the full decode's slice.

Per-launch gates (codec_f64.gates). The captured inputs are the bf16 planes, so every product is
exact in f32 and up to the epilogue the kernel's only error is the f32 accumulation of m addends in
some order: |gpu - f64| <= m 2^-23 A is derived (A = sum |addend|); 8 sqrt(m) 2^-23 A is the
random-walk model, adopted for every launch class because a one-addend-at-a-time f32 accumulation of
the same addends stays inside it (tests/test_codec_f64.py, which also shows that a dropped tap, a
neighbouring-row read, a zeroed row and a skipped residual each break it by >= 10x). Both are asserted.
"""
import json
import os

import numpy as np
import pytest

import rwkvtts
from rwkvtts import codec
import codec_f64 as F

pytestmark = pytest.mark.gpu
WEIGHTS = ("bf16", "f32")
FORMS = (0, F.FORM_SEPARATE_RESUNIT)
_report = {}


@pytest.fixture(scope="module")
def decoders():
    """One decoder per (set, weights), made on first use; the f32 blobs take the weight hi + lo path."""
    made = {}

    def get(name, wname):
        if (name, wname) not in made:
            made[name, wname] = codec.BiCodecDetokenizer(F.blob(name, wname), F.dims_of(name))
        return made[name, wname]
    yield get
    for c in made.values():
        c.close()
    d_rep = os.environ.get("RWKVTTS_REPORT_DIR")
    if d_rep and _report:
        os.makedirs(d_rep, exist_ok=True)
        json.dump(_report, open(os.path.join(d_rep, "codec_dims.json"), "w"), indent=1, sort_keys=True)


def _gate_pcm(got, ref, what):
    assert got.shape == ref.shape
    ma, rl = F.pcm_errors(got, ref)
    print(f"{what}: GPU vs float64 max abs {ma:.2e} rel L2 {rl:.2e}")
    r = _report.setdefault("pcm", {}).setdefault(what.split(" T=")[0], [0.0, 0.0])
    r[0], r[1] = max(r[0], ma), max(r[1], rl)
    assert ma <= F.PCM_ATOL and rl <= F.PCM_RTOL_L2, (what, ma, rl)


@pytest.mark.parametrize("forms", FORMS)
@pytest.mark.parametrize("wname", WEIGHTS)
@pytest.mark.parametrize("name", list(F.NEW_SETS))
def test_pcm_against_float64_and_batch_equals_single(decoders, name, wname, forms):
    c = decoders(name, wname)
    c.set_forms(forms)
    try:
        single = {}
        for T, seed in F.gpu_cases(name):
            g, s, ref = F.reference(name, wname, T, seed)
            single[T, seed] = c.decode_audio(g, s)
            _gate_pcm(single[T, seed], ref, f"{name} {wname} forms={forms} T={T}")
        ragged = [(T, 100 + i) for i, T in enumerate(F.RAGGED)]
        items = [F.reference(name, wname, T, seed)[:2] for T, seed in ragged]
        for key, pcm in zip(ragged, c.decode_audio_batch(items)):
            assert np.array_equal(pcm, single[key]), f"utterance {key} of the ragged batch differs from its single decode"
    finally:
        c.set_forms(0)


@pytest.mark.parametrize("name", list(F.NEW_SETS))
def test_interior_window_is_the_full_decodes_slice(decoders, name):
    """decode_windows on a window in the interior of the set's longest utterance (neither end of the
    utterance inside its halo): bitwise the full decode's samples."""
    T = max(T for T, _ in F.gpu_cases(name))
    c = decoders(name, "bf16")
    g, s, _ = F.reference(name, "bf16", T, T)
    full = c.decode_audio(g, s)
    H = c.halo()
    t0 = H + 1
    t1 = t0 + 2
    assert t1 + H < T, "the longest case must hold an interior window"
    win, = c.decode_windows([(g, s, t0, t1, False)])
    assert np.array_equal(win, full[t0 * F.HOP:t1 * F.HOP])


# ---- per launch -------------------------------------------------------------------------------------
def _where(rec, ratio):
    """The worst element of a [rows][co] ratio array in the launch's own coordinates."""
    r, ch = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    s = rec["s"] if rec["kind"] == 1 else 1
    TM, TN = 32 * rec["nwv"], rec["tn"]
    return (f"row {r} (input row {r // s}, phase {r % s}, time tile {(r // s) // TM} of {rec['gx']}), "
            f"channel {ch} (column tile {ch // TN} of {rec['co'] // TN})")


def _tiles(rec, ratio):
    """max ratio over the first / last time tile and the first / last column tile, named."""
    s = rec["s"] if rec["kind"] == 1 else 1
    TM, TN = 32 * rec["nwv"] * s, rec["tn"]
    last = ((ratio.shape[0] - 1) // TM) * TM
    return (f"first time tile {ratio[:TM].max():.3g}, last time tile {ratio[last:].max():.3g}, "
            f"first column tile {ratio[:, :TN].max():.3g}, last column tile {ratio[:, -TN:].max():.3g}")


def _check_launch(c, d, w, k, items, lens, what):
    """Launch k of the decode of `items`, captured, against codec_f64.launch at both gates. Returns
    (class, max |err| / (2^-23 A) on y, (sine error upper bound, its part beyond the split) or None)."""
    pcm, cap = c.capture_launch(k, items)
    rec = cap["rec"]
    wt = F.launch_weights(d, w, rec)
    res = None if cap["res"] is None else cap["res"].astype(np.float64)
    rb = None if cap["rbias"] is None else cap["rbias"].astype(np.float64)
    outs = F.launch(rec, wt, F.bf16_val(cap["x_hi"]), F.bf16_val(cap["x_lo"]), res, rb, lens)
    cls = F.launch_class(rec)
    worst, excess = 0.0, None
    for i, o in enumerate(outs):
        rows = o["rows"]
        for fname, fac in (("model", F.model_factor(rec)), ("hard", lambda m: float(m))):
            gy, gp = F.gates(rec, wt, o, fac)
            pairs = []
            if cap["y"] is not None:
                pairs.append(("y", cap["y"][i, :rows].astype(np.float64), o["y"], gy))
            if cap["y_hi"] is not None:
                pairs.append(("planes", F.bf16_val(cap["y_hi"][i, :rows]) + F.bf16_val(cap["y_lo"][i, :rows]),
                              o["planes"], gp))
            assert pairs
            for pname, got, ref, gate in pairs:
                ratio = np.abs(got - ref) / gate
                assert ratio.max() <= 1.0, (
                    f"{what} launch {k} {cls} utterance {i} {pname}: |gpu - f64| is {ratio.max():.3g}x the {fname} gate at "
                    f"{_where(rec, ratio)}; {_tiles(rec, ratio)}")
        if cap["y"] is not None:
            worst = max(worst, float((np.abs(cap["y"][i, :rows] - o["y"]) / (2.0 ** -23 * o["A"])).max()))
            if cap["y_hi"] is not None and wt["y_alpha"] is not None:
                # the hardware sine: the planes against the float64 Snake of the GPU's OWN f32 y. What is
                # left after the hi + lo split's 2^-16 and the f32 roundings, per unit of 2 |sin| / alpha
                v = cap["y"][i, :rows].astype(np.float64)
                a = wt["y_alpha"]
                pv = F.snake(v, a)
                got = F.bf16_val(cap["y_hi"][i, :rows]) + F.bf16_val(cap["y_lo"][i, :rows])
                sn = np.abs(np.sin(a * v))
                m = sn > 0.1
                if m.any():
                    # (raw: every error of the planes booked on the sine, an upper bound of its error;
                    # over: what the split and the roundings do not already explain)
                    unit = (2.0 * sn / (a + 0 * v + 1e-9))[m]
                    raw = float((np.abs(got - pv)[m] / unit).max())
                    over = float(((np.abs(got - pv) - (2.0 ** -16 + 8 * F.EPS24) * np.abs(pv))[m] / unit).max())
                    excess = (max(excess[0], raw), max(excess[1], over)) if excess else (raw, over)
    return cls, worst, excess


def _run_launches(decoders, name, wname, forms, Ts, ks=None):
    d, w = F.dims_of(name), F.blob(name, wname)
    c = decoders(name, wname)
    c.set_forms(forms)
    try:
        items = [F.tokens(d, T, 200 + T) for T in Ts]
        plan = codec.launch_plan(d, wname == "f32", forms, len(Ts), max(Ts))
        plain = c.decode_audio_batch(items)
        per_class = {}
        for k in (range(len(plan)) if ks is None else ks(plan)):
            cls, worst, excess = _check_launch(c, d, w, k, items, list(Ts), f"{name} {wname} forms={forms} T={Ts}")
            e = per_class.setdefault(cls, [0.0, None])
            e[0] = max(e[0], worst)
            if excess is not None:
                e[1] = excess if e[1] is None else (max(e[1][0], excess[0]), max(e[1][1], excess[1]))
        # an armed decode computes what an unarmed one does
        for a, b in zip(plain, c.decode_audio_batch(items)):
            assert np.array_equal(a, b)
        print(f"{name} {wname} forms={forms} T={Ts}: max |err| / (2^-23 A) on y per class: " +
              ", ".join(f"{k} {v[0]:.2f}" for k, v in sorted(per_class.items())))
        rep = _report.setdefault("launch", {})
        for k, v in per_class.items():
            r = rep.setdefault(k, [0.0, None])
            r[0] = max(r[0], v[0])
            if v[1] is not None:
                r[1] = v[1] if r[1] is None else (max(r[1][0], v[1][0]), max(r[1][1], v[1][1]))
        sines = [v[1] for v in per_class.values() if v[1] is not None]
        if sines:
            # the hardware sine's error, as far as the planes show it: it may not exceed SIN_DELTA beyond
            # what the hi + lo split and the f32 roundings explain
            assert max(x[1] for x in sines) <= F.SIN_DELTA, sines
            print(f"  hardware sine: |planes - Snake64(y)| alpha / (2 |sin|) <= {max(x[0] for x in sines):.2e}; "
                  f"beyond the split and roundings {max(x[1] for x in sines):.2e}")
    finally:
        c.set_forms(0)


@pytest.mark.parametrize("forms", FORMS)
@pytest.mark.parametrize("wname", WEIGHTS)
@pytest.mark.parametrize("name", list(F.NEW_SETS))
def test_every_launch_against_float64(decoders, name, wname, forms):
    """Every launch of a ragged two-utterance decode (5 and 3 frames), one armed decode per launch."""
    _run_launches(decoders, name, wname, forms, (5, 3))


@pytest.mark.parametrize("wname", WEIGHTS)
@pytest.mark.parametrize("key", list(F.XMAP_CASES))
def test_xmap_launches_with_surplus_blocks_against_float64(decoders, key, wname):
    """The launches each long length was chosen for (XCD-mapped 1-D grid, gx % 8 != 0), captured at
    that length."""
    T, forms, _, what, want = F.XMAP_CASES[key]

    def ks(plan):
        out = [k for k, r in enumerate(plan) if want(r)]
        assert out and all(plan[k]["xmap"] and plan[k]["gx"] % 8 for k in out), what
        return out
    _run_launches(decoders, key.rstrip("s"), wname, forms, (T,), ks)


@pytest.mark.parametrize("wname", WEIGHTS)
@pytest.mark.parametrize("name,T", [("tiny", 37), ("full", 6)])
def test_every_launch_of_the_shipped_shapes_against_float64(decoders, name, T, wname):
    """The shipped dims' kernels under the same scrutiny: the fused 4-wave dilation-9 unit, the (96,3)
    ConvTranspose, (48,7) among them (which: tests/golden/codec_plan_coverage.json)."""
    _run_launches(decoders, name, wname, 0, (T,))
