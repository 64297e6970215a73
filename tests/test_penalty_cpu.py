"""tests/penalty_ref.py (the penalty contract of include/rwkvtts.h restated in numpy f32) on cases
computed by hand: powers of two, so every quotient and product below is exact and can be checked
without a calculator, plus two pinned cases with the repetition 1.3 of the GPU tests and one where
a fused multiply-add would give another answer than the contract's multiply, then subtract."""
import numpy as np

import penalty_ref as R
from penalty_ref import Penalties

f32 = np.float32
INF = f32(np.inf)


def _bits(a):
    return np.asarray(a, dtype=np.float32).tobytes()


ROW = np.array([2.0, -2.0, 0.0, -np.inf, 1.5, 3.0, -0.0], dtype=np.float32)


def test_repetition_is_per_occurrence_and_branches_on_the_sign():
    # counts 1: 2 / 2 = 1, -2 * 2 = -4; counts 3: 2 / 8 = 0.25, -2 * 8 = -16
    one = R.apply(ROW, [0, 1], Penalties(repetition=2.0))
    assert _bits(one) == _bits([1.0, -4.0, 0.0, -np.inf, 1.5, 3.0, -0.0])
    three = R.apply(ROW, [0, 1, 0, 1, 1, 0], Penalties(repetition=2.0))
    assert _bits(three) == _bits([0.25, -16.0, 0.0, -np.inf, 1.5, 3.0, -0.0])
    # repetition < 1 rewards: 2 / 0.5 = 4 three times = 16, -2 * 0.5 three times = -0.25
    rew = R.apply(ROW, [0, 0, 0, 1, 1, 1], Penalties(repetition=0.5))
    assert _bits(rew) == _bits([16.0, -0.25, 0.0, -np.inf, 1.5, 3.0, -0.0])
    # the GPU tests' 1.3 (f32 0x1.4ccccc): pinned quotients and products, each step rounded to f32
    r13 = R.apply(ROW, [0, 1], Penalties(repetition=1.3))
    assert float(r13[0]).hex() == "0x1.89d89e0000000p+0" and float(r13[1]).hex() == "-0x1.4ccccc0000000p+1"
    r13 = R.apply(ROW, [0, 0, 0, 1, 1, 1], Penalties(repetition=1.3))
    assert float(r13[0]).hex() == "0x1.d217140000000p-1" and float(r13[1]).hex() == "-0x1.19374a0000000p+2"


def test_zero_and_minus_inf():
    # logit 0 is not > 0: 0 * rep = 0 (and -0 stays -0); then 0 - 0.5 * 2 - 0.25
    z = R.apply(ROW, [2, 2, 6], Penalties(repetition=2.0))
    assert _bits(z) == _bits(ROW)
    z = R.apply(ROW, [2, 2], Penalties(2.0, 0.5, 0.25, 0))
    assert _bits(z) == _bits([2.0, -2.0, -1.25, -np.inf, 1.5, 3.0, -0.0])
    # -inf stays -inf through every step, with either sign of frequency and presence
    for p in (Penalties(2.0, 0.5, 0.25, 0), Penalties(0.5, -8.0, -8.0, 0), Penalties(4.0, 8.0, 8.0, 0)):
        assert R.apply(ROW, [3] * 7, p)[3] == -INF
    # the repetition loop reaches its fixed points without changing anything afterwards
    big = R.apply(np.array([1.0, -1.0], dtype=np.float32), [0] * 400 + [1] * 400, Penalties(repetition=0.5))
    assert big[0] == INF and big[1] == 0.0 and np.signbit(big[1])


def test_frequency_then_presence_in_order():
    # cnt 1: 2 - 0.5 = 1.5, then - 0.25 = 1.25; cnt 3: 2 - 1.5 = 0.5, then 0.25
    assert R.apply(ROW, [0], Penalties(1.0, 0.5, 0.25, 0))[0] == f32(1.25)
    assert R.apply(ROW, [0, 0, 0], Penalties(1.0, 0.5, 0.25, 0))[0] == f32(0.25)
    assert R.apply(ROW, [1, 1, 1], Penalties(1.0, 0.5, 0.25, 0))[1] == f32(-3.75)
    # all three: (2 / 2 / 2 / 2 = 0.25) - 1.5 - 0.25 = -1.5 ; (-2 * 8 = -16) - 1.5 - 0.25 = -17.75
    all3 = R.apply(ROW, [0, 1, 0, 1, 0, 1], Penalties(2.0, 0.5, 0.25, 0))
    assert all3[0] == f32(-1.5) and all3[1] == f32(-17.75)
    # negative values reward
    assert R.apply(ROW, [4, 4], Penalties(1.0, -0.5, -0.25, 0))[4] == f32(2.75)
    # tokens that do not occur are untouched, bit for bit
    assert _bits(all3[2:]) == _bits(ROW[2:])


def test_window_cuts_occurrences_off():
    h = [0, 0, 5, 0, 4]
    P = lambda w: Penalties(1.0, 0.5, 0.0, w)  # noqa: E731
    assert R.apply(ROW, h, P(0))[0] == f32(0.5)      # three occurrences
    assert R.apply(ROW, h, P(5))[0] == f32(0.5)      # window == history length
    assert R.apply(ROW, h, P(64))[0] == f32(0.5)     # window > history length
    assert R.apply(ROW, h, P(4))[0] == f32(1.0)      # h[1:]: two
    assert R.apply(ROW, h, P(2))[0] == f32(1.5)      # h[3:]: one
    assert R.apply(ROW, h, P(1))[0] == f32(2.0)      # h[4:]: none -- the last occurrence is cut off
    assert R.apply(ROW, h, P(1))[4] == f32(1.0) and R.apply(ROW, h, P(2))[5] == f32(3.0)
    assert R.counts(h, 3) == {5: 1, 0: 1, 4: 1} and R.window_of(h, 0) == h and R.window_of([], 4) == []


def test_neutral_values_return_the_row_bit_for_bit():
    rs = np.random.RandomState(3)
    row = rs.randn(8193).astype(np.float32)
    row[[7, 99]] = [-np.inf, -0.0]
    h = list(rs.randint(0, 8192, 300)) + [7, 99]
    for w in (0, 1, 8, 2048):
        out = R.apply(row, h, Penalties(1.0, 0.0, 0.0, w))
        assert out.tobytes() == row.tobytes() and out is not row
    assert R.apply(row, [], Penalties(1.3, 0.7, 1.5, 0)).tobytes() == row.tobytes()  # an empty history


def test_frequency_is_a_multiply_then_a_subtract_not_an_fma():
    # found by search: frequency f32(0.7) = 0x1.666666p-1, cnt 3. The exact product 0x1.0cccccc8p+1
    # needs 26 bits and rounds to 0x1.0cccccp+1 (error -2^-24), and for x = 2.5 the two results
    # differ: 2.5 - RN(product) = 0x1.9999ap-2 exactly, while the fused RN(2.5 - product) is
    # 0x1.99999cp-2. The contract is the first.
    f, c, x = f32(0.7), 3, f32(2.5)
    prod = f32(f * f32(c))
    assert float(prod).hex() == "0x1.0ccccc0000000p+1" and float(prod) - float(f) * c == -2.0 ** -24
    fused = f32(float(x) - float(f) * c)  # double holds the product and the difference exactly
    assert float(fused).hex() == "0x1.99999c0000000p-2"
    got = R.apply(np.array([2.5], dtype=np.float32), [0, 0, 0], Penalties(1.0, 0.7, 0.0, 0))[0]
    assert float(got).hex() == "0x1.9999a00000000p-2" and got != fused
    # and where x equals the rounded product the contract gives exactly 0, a fused operation -2^-24
    got = R.apply(np.array([prod], dtype=np.float32), [0, 0, 0], Penalties(1.0, 0.7, 0.0, 0))[0]
    assert got == 0.0 and f32(float(prod) - float(f) * c) == f32(-2.0 ** -24)
