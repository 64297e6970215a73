"""The formant shift's kernel (csrc/formant.hip) against the numpy restatement of the arithmetic
contract (tests/formant_ref.py), bit for bit: one ragged batch with a (pitch, formant) pair per signal,
streams over chunks, and what the stage is for -- the period stays, the envelope moves."""
import numpy as np
import pytest

import formant_ref as FR
import pitch_ref
from rwkvtts import audio
from test_formant_cpu import keeps_the_period_and_moves_the_envelope, resonant_vowel
from test_pitch_cpu import _vowel, bits

pytestmark = pytest.mark.gpu
F32 = np.float32
PAIRS = ((0.0, 4.0), (0.0, -6.0), (3.0, -3.0), (-5.0, 6.0), (0.0, 0.0), (2.0, 0.0))  # (pitch, formant) semitones


def _signals():
    """0.3 .. 0.5 s: one length of whole 320-sample pieces, the others not; 50 and 500 Hz are p = Lmax and
    p = Lmin, the noise is unvoiced, the last is shorter than one frame."""
    noise = (np.random.default_rng(2).standard_normal(6400) * 0.3).astype(F32)
    return {"vowel90": _vowel(90.0, 7777), "vowel200": _vowel(200.0, 4800 + 123), "vowel50": _vowel(50.0, 8000 - 1),
            "vowel500": _vowel(500.0, 5001), "noise": noise, "silence": np.zeros(5000, F32),
            "short": _vowel(200.0, 600)[500:600].copy()}


@pytest.fixture(scope="module")
def shifter():
    p = audio.PitchShifter()
    yield p
    p.close()


@pytest.fixture(scope="module")
def batch(shifter):
    """Every signal with every pair in one launch triple -> {(name, pair): (x, y)}."""
    sig = _signals()
    keys = [(name, pair) for name in sig for pair in PAIRS]
    ys = shifter.shift_batch([sig[n] for n, _ in keys], [p[0] for _, p in keys], formant=[p[1] for _, p in keys])
    assert shifter.kernel_ms() > 0.0
    per = {n: pitch_ref.window(sig[n], 0, True, 1.0, 0, 0, 0, sig[n].size, want_marks=True)[3] for n in ("vowel50", "vowel500", "noise")}
    assert shifter.lag_max in per["vowel50"] and shifter.lag_min in per["vowel500"] and not per["noise"].any()
    return {k: (sig[k[0]], y) for k, y in zip(keys, ys)}


@pytest.mark.parametrize("name", list(_signals()))
def test_a_ragged_batch_is_bitwise_the_restatement(shifter, batch, name):
    x = batch[(name, PAIRS[0])][0]
    for pitch, formant in PAIRS:
        y = batch[(name, (pitch, formant))][1]
        B = FR.ratio(formant)
        want, _, _, lo, hi = FR.window(x, 0, True, audio.pitch_factor(pitch), B, shifter.formant_table(B), 0, 0, 0, x.size,
                                       want_reads=True)
        assert y.size == x.size and np.array_equal(bits(y), bits(want)), (name, pitch, formant)
        assert formant <= 0.0 or (lo < 0 and hi >= x.size)  # a grain read faster leaves the signal at both ends
        if not x.any():
            assert np.array_equal(bits(y), bits(x))  # silence bit for bit
    # an unshifted job inside a shifted call is the pitch path's output (k_pitch_synth), bitwise
    plain = shifter.shift_batch([x, x], [0.0, 2.0])
    assert np.array_equal(bits(batch[(name, (0.0, 0.0))][1]), bits(plain[0]))
    assert np.array_equal(bits(batch[(name, (2.0, 0.0))][1]), bits(plain[1]))


@pytest.mark.parametrize("chunk", [1600, 2777])
def test_streams_are_bitwise_the_one_shot_result(shifter, batch, chunk):
    for (name, pair), (x, want) in batch.items():
        if pair[1] == 0.0:  # (the pitch stage's own stream: tests/test_gpu_pitch.py)
            continue
        st = shifter.stream(*pair)
        got = []
        for i in range(0, x.size, chunk):
            got.append(st.feed(x[i:i + chunk], final=i + chunk >= x.size))
            fed = min(i + chunk, x.size)
            assert fed == x.size or fed - sum(g.size for g in got) <= st.lag == 1600
        assert x.size < 2 * chunk + 1600 or sum(g.size > 0 for g in got) >= 2  # the kept tail was cut and used again
        assert np.array_equal(bits(np.concatenate(got)), bits(want)), (name, pair)


def test_the_period_stays_and_the_envelope_moves(shifter):
    x, shifts = resonant_vowel(), (-6.0, -3.0, 3.0, 6.0)
    for s, y in zip(shifts, shifter.shift_batch([x] * 4, [0.0] * 4, formant=shifts)):
        assert keeps_the_period_and_moves_the_envelope(y, s), s
