"""The watermark without a GPU: the library's host-only entry points (table, strength, threshold,
plan) against tests/wm_ref.py, and the reference pinned to itself -- the properties of the embedder's
contract, and what the float64 detector makes of marked, attacked, unmarked and wrong-key clips on two
hosts, a synthetic vowel (a 110 Hz harmonic stack under a slow envelope) and amplitude-modulated white
noise. DESIGN.md §30 carries the figures this file prints.

The statistic divides r_b by the root of sum F^2, the exact variance of r_b under independent chips
whatever the folds of the clip share, so the null set below holds every unmarked and every wrong-key
clip of both hosts at 2 .. 8 s to the threshold, the marked vowel read under another key included
(DESIGN.md §30.2 has what a division by the folded v^2 scored there)."""
import ctypes

import numpy as np
import pytest

import wm_ref
from rwkvtts import _ffi, audio

F32 = np.float32
B, L, NB, TB, NP = 320, 129, 16, 1600, 25600
KEY = 0x5EED0C0FFEE


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _desc(**kw):
    return _ffi.WmDesc(struct_size=ctypes.sizeof(_ffi.WmDesc), **kw)


@pytest.fixture(scope="module")
def wm():
    return audio.Watermarker(evaluator=wm_ref.evaluator, detector=wm_ref.detector)


@pytest.fixture(scope="module")
def marked():
    x = wm_ref.vowel(64000, 0)
    y = wm_ref.embed(x, KEY, 0xBEEF)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


# ---- host-only entry points ---------------------------------------------------------------------
@pytest.mark.parametrize("kw", [{}, dict(block=64, taps=33, bits=4, bit_len=640), dict(band_lo=300.0, band_hi=2000.0)])
def test_the_library_table_is_pythons(kw):
    p = wm_ref.config(**kw)
    tab = np.full(p["taps"] + p["block"], -1.0, F32)
    assert _ffi.lib().rwkvtts_wm_table(ctypes.byref(_desc(**kw)), tab.ctypes.data_as(ctypes.c_void_p)) == 0
    want = wm_ref.table(p["taps"], p["block"], p["band_lo"], p["band_hi"])
    assert np.array_equal(bits(want), bits(audio._wm_table(p["taps"], p["block"], p["band_lo"], p["band_hi"])))
    # (two math libraries: a last-place difference in a cosine may move a tap by an ulp)
    assert np.max(np.abs(tab.astype(np.float64) - want)) <= 2.0 ** -23 * float(np.max(np.abs(want)))
    h = want[:p["taps"]].astype(np.float64)
    assert abs(float(np.sum(h * h)) - 1.0) < 1e-6 and np.array_equal(h, h[::-1])   # unit energy, linear phase
    if not kw:  # (the default: the lower edge is well above the Blackman window's transition width, 5.5 fs / L)
        assert abs(float(np.sum(h))) < 1e-3
    assert np.array_equal(bits(want[p["taps"]:]), bits((np.arange(1, p["block"] + 1) / float(p["block"])).astype(F32)))


def test_threshold_is_the_chi_square_tail_at_one_in_a_million_over_the_period():
    for kw, nb, n_p in (({}, 16, 25600), (dict(bits=4, bit_len=640), 4, 2560), (dict(bits=5, bit_len=640), 5, 3200)):
        t = ctypes.c_double()
        assert _ffi.lib().rwkvtts_wm_threshold(ctypes.byref(_desc(**kw)), ctypes.byref(t)) == 0
        T = wm_ref.threshold(nb, n_p)
        assert abs(t.value - T) <= 1e-9 * T
        assert n_p * wm_ref.chi2_sf(T, nb) <= 1e-6 < n_p * wm_ref.chi2_sf(T * (1 - 1e-9), nb)
    assert 80.0 < wm_ref.threshold(16, 25600) < 90.0
    for T in (1.0, 7.5, 40.0):  # the closed forms: k = 2 is the exponential, odd k lies between its neighbours
        assert abs(wm_ref.chi2_sf(T, 2) - np.exp(-T / 2)) < 1e-15
        assert wm_ref.chi2_sf(T, 4) < wm_ref.chi2_sf(T, 5) < wm_ref.chi2_sf(T, 6)
    # odd k against a numeric integral of the density x^(k/2-1) e^(-x/2) / (2^(k/2) Gamma(k/2))
    import math
    xs = np.linspace(7.5, 200.0, 400001)
    pdf = xs ** 1.5 * np.exp(-xs / 2) / (2 ** 2.5 * math.gamma(2.5))
    assert abs(float(np.sum((pdf[1:] + pdf[:-1]) * 0.5 * (xs[1] - xs[0]))) - wm_ref.chi2_sf(7.5, 5)) < 1e-8


def test_plan_strength_and_refused_descriptions(wm):
    assert wm.plan(0, False) == (0, 0) and wm.plan(B - 1, False) == (0, 0) and wm.plan(B, False) == (B, 0)
    assert wm.plan(5 * B + 7, False, 3) == (5 * B, 3 * B) and wm.plan(5 * B + 7, True, 3) == (5 * B + 7, 3 * B)
    assert (wm.block, wm.taps, wm.bits, wm.bit_len, wm.period) == (B, L, NB, TB, NP)
    assert audio.wm_strength(-26.0) == wm_ref.strength(-26.0) and audio.wm_strength(-6) == wm_ref.strength(-6)
    for bad in (-60.5, -5.9, 0.0, float("nan")):
        with pytest.raises(ValueError):
            audio.wm_strength(bad)
    for kw in (dict(block=100), dict(block=4864), dict(taps=128), dict(taps=1), dict(bits=33), dict(bits=-1),
               dict(bit_len=1000), dict(bit_len=6720), dict(band_lo=3400.0, band_hi=1000.0), dict(band_hi=8000.0),
               dict(band_lo=float("nan")), dict(strength_db=-3.0), dict(strength_db=-61.0)):
        assert _ffi.lib().rwkvtts_wm_plan(ctypes.byref(_desc(**kw)), 0, 0, 0, None, None) == _ffi.EINVAL, kw
    for bad in (-1, 65536, True, 1.0):
        with pytest.raises(ValueError):
            wm.embed(np.zeros(10, F32), KEY, bad)
    for bad in (-1, 1 << 64, None):
        with pytest.raises(ValueError):
            wm.embed(np.zeros(10, F32), bad, 1)


def test_chips_are_balanced_and_neighbouring_keys_are_not_shifts():
    a, b = wm_ref.chips(KEY, NP), wm_ref.chips(KEY + 1, NP)
    assert set(np.unique(a)) == {-1, 1} and abs(int(a.sum())) < 5 * NP ** 0.5
    xc = np.fft.irfft(np.conj(np.fft.rfft(a.astype(np.float64))) * np.fft.rfft(b.astype(np.float64)), NP)
    assert np.max(np.abs(xc)) < 6 * NP ** 0.5          # (a shifted copy would give NP at its lag)
    assert wm_ref.splitmix64(np.uint64(0)) == np.uint64(0xE220A8397B1DCDAF)   # the published test vector


# ---- the embedder's contract --------------------------------------------------------------------
def test_silence_is_unchanged_and_the_difference_stays_under_its_bound(wm, marked):
    z = np.zeros(3 * B + 17, dtype=F32)
    assert np.array_equal(bits(wm_ref.embed(z, KEY, 0xFFFF)), bits(z))
    x, y = marked
    h, s = wm.table[:L].astype(np.float64), float(wm_ref.strength(-26.0))
    nb = -(-x.size // B)
    xp = np.zeros(nb * B, dtype=F32)
    xp[:x.size] = x
    a = (F32(s) * np.sqrt(wm_ref.block_energy(xp.reshape(nb, B)) / F32(B))).astype(np.float64)
    hi = np.repeat(np.maximum(a, np.concatenate([a[:1], a[:-1]])), B)[:x.size]
    diff = np.abs(y.astype(np.float64) - x)
    assert np.all(diff <= hi * np.sum(np.abs(h))) and diff.max() > 0   # the contract's bound, no slack
    print("max |y - x| / bound:", float(np.max(diff[hi > 0] / (hi[hi > 0] * np.sum(np.abs(h))))))
    # -26 dB of the block's level, shaped by a unit-energy filter: the mark's RMS sits 26 dB under the host's
    ratio = 20 * np.log10(np.sqrt(np.mean(diff ** 2)) / np.sqrt(np.mean(x.astype(np.float64) ** 2)))
    print("mark RMS re host RMS, dB:", round(float(ratio), 2))
    assert -28.0 < ratio < -24.0


def test_a_stream_of_any_cut_is_the_one_shot_and_lags_one_block(wm):
    x = wm_ref.vowel(9 * B + 45, 7)
    want = wm_ref.embed(x, KEY, 0x1D)
    assert np.array_equal(bits(wm.embed(x, KEY, 0x1D)), bits(want))
    for cuts in ([1, 2, B, B + 1, 5 * B - 1], [3 * B], [x.size - 1], list(range(100, x.size, 100))):
        st = wm.stream(KEY, 0x1D)
        parts, fed = [], 0
        pieces = np.split(x, cuts)
        for i, p in enumerate(pieces):
            parts.append(st.feed(p, final=i == len(pieces) - 1))
            fed += p.size
            if i < len(pieces) - 1:
                assert sum(q.size for q in parts) == B * (fed // B) and st.kept == fed % B
        assert np.array_equal(bits(np.concatenate(parts)), bits(want))


# ---- what the detector makes of it ----------------------------------------------------------------
def test_the_reference_reads_every_attack_on_the_vowel(marked):
    x, y = marked
    T = wm_ref.threshold(NB, NP)
    back = audio.resample_audio_high_quality(audio.resample_audio_high_quality(y, 16000, 8000), 8000, 16000)
    attacks = {"clean": (y, 0), "cropped 7777": (y[7777:], 7777), "gain 0.3": (y * F32(0.3), 0),
               "int16": ((np.trunc(y * F32(32767.0)) / F32(32767.0)).astype(F32), 0), "8 kHz and back": (back, None)}
    for name, (clip, off) in attacks.items():
        d = wm_ref.detect(clip, KEY)
        print(f"{name}: score {d['score']:.0f}  min|z| {d['min_z']:.1f}  offset {d['offset']}  payload {d['payload']:#06x}")
        assert d["detected"] and d["payload"] == 0xBEEF and d["seen"] == 0xFFFF and d["score"] >= 10 * T, name
        assert off is None or d["offset"] == off, name


def test_no_unmarked_or_wrong_key_clip_reaches_the_threshold():
    T = wm_ref.threshold(NB, NP)
    seconds = (2, 3, 4, 5, 6, 8)
    clips = []
    for k, sec in enumerate(seconds):
        n = sec * 16000
        v, w = wm_ref.vowel(n, 10 + k), wm_ref.am_noise(n, 10 + k)
        clips += [(f"unmarked vowel {sec} s", v, KEY + k), (f"unmarked noise {sec} s", w, KEY + k),
                  (f"wrong key noise {sec} s", wm_ref.embed(w, KEY + k, 0x1234 + k), KEY + k + 100),
                  (f"wrong key vowel {sec} s", wm_ref.embed(v, KEY + k, 0x1234 + k), KEY + k + 100)]
    assert len(clips) == 24
    scores = {name: wm_ref.detect(x, key)["score"] for name, x, key in clips}
    print("null scores:", {k: round(v, 1) for k, v in scores.items()}, "T", round(T, 2))
    assert max(scores.values()) < T, max(scores, key=scores.get)


def test_a_clip_shorter_than_the_period_reports_what_it_saw(marked):
    _, y = marked
    d = wm_ref.detect(y[:12000], KEY)   # seven and a half bit slots
    assert d["detected"] and d["offset"] == 0 and d["seen"] == 0x00FF and d["payload"] == 0xBEEF & 0x00FF
    d = wm_ref.detect(y[4000:4000 + 8000], KEY)  # from the middle of slot 2 to the middle of slot 7
    assert d["offset"] == 4000 and d["seen"] == 0b11111100 and d["payload"] == 0xBEEF & 0b11111100
    assert wm_ref.detect(np.zeros(0, F32), KEY)["detected"] is False


def test_the_noise_host_is_the_hard_one():
    """White noise fills the mark's band. The scores and the weakest bit are figures for DESIGN.md and
    are not gated; that the search lands on the mark's own alignment is."""
    for sec in (2, 4):
        x = wm_ref.am_noise(sec * 16000, 1)
        d = wm_ref.detect(wm_ref.embed(x, KEY, 0xBEEF), KEY)
        print(f"noise host {sec} s: score {d['score']:.0f}  min|z| {d['min_z']:.2f}  payload ok {d['payload'] == 0xBEEF}")
        assert d["offset"] == 0 and d["seen"] == 0xFFFF
