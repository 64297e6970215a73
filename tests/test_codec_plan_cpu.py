"""Which k_conv instantiation every vocoder launch of the GPU tests runs (CPU only).

rwkvtts_codec_debug_launch_plan is the function Codec::conv() and Codec::resunit_fused() take their
choice from (column tile, taps class, weight-lo, waves, fused, LDS bytes, grid, XCD mapping). The
tests below pin, per dims set, weight path, residual-unit form and length that a GPU test uses, the
set of (instantiation, launch kind, xmap, gx % 8) reached: tests/golden/codec_plan_coverage.json.
If a chooser change moves a GPU test off the kernel it was written for, this fails instead of the
GPU case quietly running something else. Regenerate the table, after reading the difference, with
`python tests/test_codec_plan_cpu.py --write`.
"""
import itertools
import json
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path[:0] = [os.path.join(HERE, "..", "rwkv-tts-rs_amd"), HERE]

from rwkvtts import codec  # noqa: E402
import codec_f64 as F  # noqa: E402

TABLE = os.path.join(HERE, "golden", "codec_plan_coverage.json")
SEP = F.FORM_SEPARATE_RESUNIT
# (set, weight-lo path, forms) -> lengths: what tests/test_gpu_codec_dims.py, test_gpu_codec.py and
# test_gpu_codec_windows.py decode (Tmax of each call)
LENGTHS = {}
for _n in F.NEW_SETS:
    for _w, _f in itertools.product((False, True), (0, SEP)):
        LENGTHS[_n, _w, _f] = sorted({T for T, _ in F.gpu_cases(_n)})
for _w, _f in itertools.product((False, True), (0, SEP)):
    LENGTHS["tiny", _w, _f] = [1, 2, 5, 37, 41, 129, 130]
    LENGTHS["full", _w, _f] = [5, 6, 7, 9, 24] + ([512] if not _f else [])


def entry(r):
    return f"{F.launch_class(r)} xmap={r['xmap']} gx%8={r['gx'] % 8 if r['xmap'] else '-'}"


def coverage():
    out = {}
    for (name, wlo, forms), Ts in sorted(LENGTHS.items()):
        reach = {}
        for T in Ts:
            for r in codec.launch_plan(F.dims_of(name), wlo, forms, 1, T):
                reach.setdefault(entry(r), []).append(T)
        out[f"{name} {'wlo' if wlo else 'bf16'} forms={forms}"] = {k: sorted(set(v)) for k, v in sorted(reach.items())}
    return out


def test_coverage_table():
    want = json.load(open(TABLE))
    got = coverage()
    assert sorted(got) == sorted(want)
    for k in got:
        assert got[k] == want[k], f"{k}: the launches of a GPU test moved to other kernels"


def _reached(name, wlo, forms, T=5):
    return {(F.launch_class(r), r["xmap"], r["gx"] % 8) for r in codec.launch_plan(F.dims_of(name), wlo, forms, 1, T)}


def test_new_sets_reach_what_they_were_chosen_for():
    cls = lambda name, wlo, forms=0, T=5: {c for c, _, _ in _reached(name, wlo, forms, T)}
    # u2: ConvTranspose with 5 taps (KT 7, 8 waves) and with one tap (k == s)
    assert {"convT(64,7,bf16,8)", "convT(64,1,bf16,4)"} <= cls("u2", False)
    assert {"convT(64,7,wlo,8)", "convT(64,1,wlo,4)"} <= cls("u2", True)
    # u3: phases of 4 and 3 taps in one KT 7 launch; one-tap ConvTranspose at 192 (TN 64) and 96 (TN 48)
    assert {"convT(64,7,bf16,8)", "convT(64,1,bf16,4)", "convT(48,1,bf16,4)"} <= cls("u3", False)
    assert {"convT(64,7,wlo,8)", "convT(48,1,wlo,4)"} <= cls("u3", True)
    d = F.DIMS_U3
    p, K, s = (d["up_kernels"][0] - d["up_rates"][0]) // 2, d["up_kernels"][0], d["up_rates"][0]
    assert {(K - (ph + p) % s + s - 1) // s for ph in range(s)} == {3, 4}
    # u1: 320 output phases in one launch, fused residual units (8- and 4-wave) right behind it
    plan = codec.launch_plan(F.DIMS_U1, False, 0, 1, 5)
    ct = [r for r in plan if r["kind"] == 1]
    assert len(ct) == 1 and ct[0]["gy"] == 320 * (96 // ct[0]["tn"])
    assert {"fused(96,7,bf16,8)", "fused(96,7,bf16,4)"} <= cls("u1", False)
    # gemv-jobs flush (2 jobs per AdaLN, 32 per launch), every k_dw_ln slot, a partial last slot, no block
    assert 2 * (F.DIMS_U2["prenet_layers"] + 1) > 32
    assert F.DIMS_U3["prenet_dim"] == 512 and F.DIMS_U1["prenet_dim"] % 128 == 64 and F.DIMS_U1["prenet_layers"] == 0


def test_xmap_lengths_are_the_smallest_with_surplus_blocks():
    """The long lengths of the GPU tests: the smallest T at which the named launches run the XCD-mapped
    1-D grid with gx % 8 != 0 (blocks past gx return early), on both weight paths."""
    for key, (T, forms, _wlo, what, want) in F.XMAP_CASES.items():
        d = F.NEW_SETS[key.rstrip("s")]
        for wlo in (False, True):
            assert F.xmap_length(d, wlo, forms, want) == T, (key, what, wlo)


def conv_kernels():
    """RT_CONV_KERNELS and RT_CONV_FUSED of csrc/codec.hip as launch classes of any kind."""
    src = open(os.path.join(HERE, "..", "rwkv-tts-rs_amd", "csrc", "codec.hip")).read()
    out = set()
    for macro, fused in (("RT_CONV_KERNELS", False), ("RT_CONV_FUSED", True)):
        body = re.search(r"#define " + macro + r"\(X\)((?:.*\\\n)*.*)\n", src).group(1)
        for tn, kt, wlo, nwv in re.findall(r"X\((\d+), (\d+), (true|false), (\d+)\)", body):
            out.add((int(tn), int(kt), wlo == "true", int(nwv), fused))
    return out


# instantiations that no admitted dims reach (see test_unreachable_instantiations)
UNREACHABLE = {
    (48, 3, False, 4, False), (96, 7, False, 8, False), (192, 1, False, 4, False),
    (48, 3, True, 4, False), (96, 7, True, 8, False), (48, 7, True, 4, False), (64, 7, True, 4, False), (96, 7, True, 4, False),
}


def test_unreachable_instantiations():
    """Method: dims drawn (seeded) over what Codec::init admits -- n_up 1..4, every ordered
    factorisation of 320 into n_up rates, kernels k = s + 2 j up to 7 taps per phase, last-stage width
    32 / 64 / 96, latent / prenet / inter widths in multiples of 64 (prenet <= 512), 0 or 1 ConvNeXt
    block -- 3000 draws, each planned on both weight paths and both residual-unit forms. The chooser
    does not look at T except for the grid, so T = 1. What the draws never reach, out of the 28 + 2
    instantiations csrc/codec.hip compiles, is the list above. Removing them is a follow-up."""
    def factorisations(n, parts):
        if parts == 1:
            return [(n,)]
        return [(f,) + rest for f in range(1, n + 1) if n % f == 0 for rest in factorisations(n // f, parts - 1)]
    facts = {k: factorisations(320, k) for k in (1, 2, 3, 4)}
    rs = np.random.default_rng(28)
    reached = set()
    admitted = 0
    for _ in range(3000):
        n_up = int(rs.integers(1, 5))
        rates = facts[n_up][int(rs.integers(len(facts[n_up])))]
        kernels = tuple(int(s + 2 * rs.integers(0, max(1, (6 * s) // 2 + 1))) for s in rates)
        if any((k + s - 1) // s > 7 for k, s in zip(kernels, rates)):
            continue
        L = 64 * int(rs.integers(1, 17))
        d = dict(codebook_size=8192, codebook_dim=8, latent_dim=L, n_global=32, fsq_levels=4, fsq_dims=6, spk_dim=L,
                 prenet_dim=64 * int(rs.integers(1, 9)), prenet_inter=64 * int(rs.integers(1, 33)),
                 prenet_layers=int(rs.integers(0, 2)), dec_channels=int(rs.choice([32, 64, 96])) << n_up, n_up=n_up,
                 up_rates=rates, up_kernels=kernels)
        for wlo, forms in itertools.product((False, True), (0, SEP)):
            try:
                plan = codec.launch_plan(d, wlo, forms, 1, 1)
            except RuntimeError:
                continue  # (admitted by init, but some launch has no tile that fits the LDS)
            admitted += 1
            reached |= {(r["tn"], r["kt"], bool(r["wlo"]), r["nwv"], r["kind"] == 2) for r in plan}
    assert admitted > 4000
    kernels = conv_kernels()
    assert len(kernels) == 30 and reached <= kernels
    assert kernels - reached == UNREACHABLE


if __name__ == "__main__" and "--write" in sys.argv:
    json.dump(coverage(), open(TABLE, "w"), indent=1, sort_keys=True)
    print("wrote", TABLE)
