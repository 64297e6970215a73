"""The high-band contract itself (include/rwkvtts.h) on the CPU, through tests/highband_ref.py."""
import ctypes

import numpy as np
import pytest

import highband_ref as R
from rwkvtts import _ffi

F32 = np.float32
HP, IP, SH, RAMP = R.split(R.table())


def _db(h, fs, lo, hi):
    """The largest magnitude of h's response over [lo, hi] Hz, in dB."""
    H = np.abs(np.fft.rfft(h.astype(np.float64), 1 << 14))
    f = np.arange(H.size) * fs / float(1 << 14)
    return 20.0 * np.log10(H[(f >= lo) & (f <= hi)].max())


def _interp32():
    """The interpolator as one 63-tap filter at 32 kHz: the unit tap and ip at the odd offsets."""
    g = np.zeros(63)
    g[31] = 1.0
    g[31 + 2 * (16 - np.arange(32)) - 1] = IP
    return g


def _band(y, fs, lo, hi):
    """The energy of y between lo and hi Hz per sample."""
    Y = np.abs(np.fft.rfft(y.astype(np.float64))) ** 2
    f = np.arange(Y.size) * fs / float(y.size)
    return 2.0 * Y[(f >= lo) & (f < hi)].sum() / float(y.size) ** 2


def test_table_and_what_the_filters_reject():
    lib = np.zeros(446, dtype=F32)
    desc = _ffi.HighBandDesc(struct_size=ctypes.sizeof(_ffi.HighBandDesc))
    _ffi.check(_ffi.lib().rwkvtts_highband_table(ctypes.byref(desc), lib.ctypes.data_as(ctypes.c_void_p)), "table")
    assert np.max(np.abs(lib.astype(np.float64) - R.table())) <= 1e-9  # (another libm's last bit, rounded to f32)
    # the measured figures of DESIGN.md §40, each asserted a little above itself
    assert _db(HP, 16000, 0, 3000) <= -47.0 and abs(_db(HP, 16000, 5000, 8000)) <= 0.03
    assert _db(SH, 32000, 0, 7500) <= -53.0 and _db(SH, 32000, 13500, 16000) <= -51.0
    g = _interp32() / 2.0
    H = np.abs(np.fft.rfft(g, 1 << 14))
    assert np.max(np.abs(H[:int(7000 / 32000 * (1 << 14))] - 1.0)) <= 0.003 and _db(g, 32000, 9000, 16000) <= -51.0


def test_a_voiced_signal_gets_no_high_band():
    t = np.arange(4000) / 16000.0
    x = (0.3 * np.sin(2 * np.pi * 1000 * t) + 0.2 * np.sin(2 * np.pi * 3000 * t)).astype(F32)
    for dt in (F32, np.float64):
        y, u, w, gain = R.highband(x, 12.0, dtype=dt, parts=True)
        assert not gain.any() and y.size == 8000
        assert np.array_equal(y[0::2], x.astype(dt)) and np.array_equal(y[1::2], R.fir(x.astype(dt), IP.astype(dt), 16))


@pytest.mark.parametrize("db", [0.0, -12.0, 12.0])
def test_noise_gets_the_folded_band_at_the_stated_level(db):
    """The band is measured on y - u = gain * w: u's own image leakage just above 8 kHz is the
    interpolator's, not the synthesised band's. Expected per-sample energy ratio: G^2 times the mean
    over 8-12 kHz of |SH(f) HP4(16k - f) I(16k - f)|^2 (the tilt's mean, with the two filters the band
    went through before it). Tolerance: the two energies weight the same 4000 noise bins differently; a
    weighted sum of K chi-square bins has a relative deviation below sqrt(2 / K_eff), K_eff >= 2000 for
    a weighting within 12 dB, and 4 sigma of that is 12.6 %."""
    n = 16000
    x = (0.1 * np.random.default_rng(40).standard_normal(n)).astype(F32)
    y, u, w, gain = R.highband(x, db, dtype=np.float64, parts=True)
    G = float(R.gain_of(db))
    assert np.array_equal(gain, np.full(2 * n, G))  # every block is above r_hi: s = 1 throughout
    f = 8000.0 + 4000.0 * (np.arange(2000) + 0.5) / 2000.0
    e = lambda h, c, fs, fr: np.abs(np.exp(-2j * np.pi * np.outer(fr / fs, np.arange(h.size) - c)) @ h.astype(np.float64))
    tilt = np.mean((e(SH, 31, 32000.0, f) * e(HP, 15, 16000.0, 16000.0 - f) * e(_interp32() / 2.0, 31, 32000.0, 16000.0 - f)) ** 2)
    ratio = _band(y - u, 32000, 8000, 12000) / _band(x, 16000, 4000, 8000)
    print(f"highband {db:+.0f} dB: ratio {ratio:.5f}, G^2 * tilt mean {G * G * tilt:.5f}")
    assert abs(ratio / (G * G * tilt) - 1.0) <= 4.0 * np.sqrt(2.0 / 2000.0)
    # below 7.5 kHz the output is the interpolated input up to SH's rejection of the folded signal
    b = R.fir(x.astype(np.float64), HP.astype(np.float64), 15)
    v_energy = (np.sum(b * b) + np.sum(R.fir(b, IP.astype(np.float64), 16) ** 2)) / (2.0 * n)
    assert _band(y - u, 32000, 0, 7500) <= (G * 10.0 ** (-53.0 / 20.0)) ** 2 * v_energy


def test_the_plan_is_monotone_and_what_it_calls_ready_never_changes():
    desc = _ffi.HighBandDesc(struct_size=ctypes.sizeof(_ffi.HighBandDesc))

    def plan(n_known, final, out_first=0):
        end, first = ctypes.c_int64(), ctypes.c_int64()
        _ffi.check(_ffi.lib().rwkvtts_highband_plan(ctypes.byref(desc), n_known, final, out_first, ctypes.byref(end),
                                                    ctypes.byref(first)), "plan")
        return end.value, first.value

    ends = [plan(n, 0)[0] for n in range(0, 1200)]
    firsts = [plan(5000, 0, o)[1] for o in range(0, 2400)]
    assert ends == sorted(ends) and firsts == sorted(firsts) and ends[0] == 0 and ends[-1] > 0 and firsts[-1] > 0
    assert all(plan(n, 1)[0] == 2 * n and ends[n] <= 2 * n for n in range(0, 1200))
    rng = np.random.default_rng(41)
    x = (0.1 * rng.standard_normal(1200)).astype(F32)
    for n in (174, 175, 205, 206, 207, 335, 366, 367, 1000):  # either side of both of the plan's terms
        other = np.concatenate([x[:n], (0.5 * rng.standard_normal(300)).astype(F32)])
        a, b = R.highband(x), R.highband(other)
        assert np.array_equal(a[:ends[n]].view(np.uint32), b[:ends[n]].view(np.uint32)), n
        if n in (175, 206):  # and one output more would have changed (the far taps are small: seen in double)
            a, b = R.highband(x, dtype=np.float64), R.highband(other, dtype=np.float64)
            assert np.array_equal(a[:ends[n]], b[:ends[n]]) and a[ends[n]] != b[ends[n]], n
