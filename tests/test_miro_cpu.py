"""tests/miro_ref.py (the Mirostat contract of include/rwkvtts.h restated in numpy f32) on rows
computed by hand -- probabilities that are powers of two, whose surprises are integers and whose sums
are exact --, the update's multiply-then-subtract on a case where a fused operation would differ, the
cap at 4 tau, lg (the library's export, the source the kernel runs) against libm's log2f and float64
log2 on a strided sweep of (0, 1], and the behaviour the sampler is for: on a row whose entropy lies
well above tau the running surprise is pulled towards tau. The GPU is held bitwise to this reference
(tests/test_gpu_advance_miro.py), so the behavioural case covers it too."""
import ctypes
import ctypes.util

import numpy as np

import miro_ref as R

f32 = np.float32
# p = 1/2, 1/4, 1/8, 1/8: surprises 1, 2, 3, 3
P4 = np.array([0.5, 0.25, 0.125, 0.125], dtype=np.float32)


def test_lg_is_exact_on_powers_of_two():
    x = np.array([1.0, 0.5, 0.25, 0.125, 2.0 ** -126, 2.0 ** -149], dtype=np.float32)  # the last: subnormal
    assert R.lg(x).tolist() == [0.0, -1.0, -2.0, -3.0, -126.0, -149.0]
    assert R.lg(f32(0.5)) == f32(-1.0)


def test_tie_at_the_cut_keeps_the_lower_index():
    # mu = 2: c = 2 (surprises 1 and 2), K = 3: the cut falls between the two entries of 1/8, and
    # (p descending, index ascending) keeps index 2. S = 0.875.
    idx, K = R.kept(P4, 2.0)
    assert K == 3 and idx.tolist() == [0, 1, 2]
    # u = r S against cum = 0.5, 0.75, 0.875
    assert R.sample_p(P4, 2.0, 0.5) == R.Attempt(0, f32(0.875), f32(0.5), 3)      # u = 0.4375 <= 0.5
    assert R.sample_p(P4, 2.0, 0.625) == R.Attempt(1, f32(0.875), f32(0.25), 3)   # u = 0.546875
    assert R.sample_p(P4, 2.0, 0.875) == R.Attempt(2, f32(0.875), f32(0.125), 3)  # u = 0.765625
    assert R.sample_p(P4, 2.0, 1.0 - 2.0 ** -24).token == 2  # the largest draw: never index 3
    # the same values in another index order: the tie is broken by index, not by position in a sort
    q = np.array([0.125, 0.5, 0.125, 0.25], dtype=np.float32)
    assert R.kept(q, 2.0)[0].tolist() == [1, 3, 0]
    # mu = 3 admits all four: c = 4, K = min(5, 4)
    idx, K = R.kept(P4, 3.0)
    assert K == 4 and idx.tolist() == [0, 1, 2, 3] and R.sample_p(P4, 3.0, 0.9375).token == 3


def test_threshold_on_the_boundary_is_inclusive():
    # -lg(p) <= mu: mu = 1 counts the entry of surprise 1 exactly, so K = 2; just below, K = 1
    assert R.kept(P4, 1.0)[1] == 2
    assert R.kept(P4, np.nextafter(f32(1.0), f32(0.0)))[1] == 1


def test_mu_below_every_surprise_keeps_one():
    # c = 0, K = 1: the most probable token whatever the draw; its surprise inside the kept set is 0
    for r in (0.0, 0.3, 1.0 - 2.0 ** -24):
        a = R.sample_p(P4, 0.5, r)
        assert a == R.Attempt(0, f32(0.5), f32(0.5), 1)
    assert R.surprise(f32(0.5), f32(0.5)) == 0.0
    assert R.kept(P4, -3.0)[1] == 1  # a negative threshold too


def test_single_positive_entry_and_minus_inf():
    # one positive entry: c = 1, K = min(2, 1) = 1
    assert R.sample_p(np.array([0.0, 1.0, 0.0], dtype=np.float32), 6.0, 0.7) == R.Attempt(1, f32(1.0), f32(1.0), 1)
    # through the softmax: -inf logits get p = 0 and are never kept, whatever mu
    row = np.array([-np.inf, 0.0, -np.inf, 0.0, -np.inf], dtype=np.float32)
    p = R.softmax(row)
    assert p.tolist() == [0.0, 0.5, 0.0, 0.5, 0.0]
    idx, K = R.kept(p, 40.0)
    assert K == 2 and idx.tolist() == [1, 3]
    assert R.sample(row, 40.0, 0.5).token == 1 and R.sample(row, 40.0, 0.75).token == 3
    # the mask (forbid / EOS) is applied before the max: masking the leader renormalises the rest
    row = np.array([5.0, 0.0, 0.0], dtype=np.float32)
    assert R.softmax(row, masked=(0,)).tolist() == [0.0, 0.5, 0.5]
    assert R.sample(row, 40.0, 0.9, masked=(0,)).token == 2


def test_softmax_sums_sequentially_in_f32():
    # 1 + 2^-24 + 2^-24 in f32: sequentially each add rounds back to 1 (ties to even); pairwise
    # or double would give 1 + 2^-23. e = exp(0), exp(-24 ln 2)-ish values are not exact, so use
    # the accumulate itself on exact values
    e = np.array([1.0, 2.0 ** -24, 2.0 ** -24], dtype=np.float32)
    assert np.add.accumulate(e, dtype=np.float32)[-1] == f32(1.0)
    assert f32(e.astype(np.float64).sum()) == f32(1.0 + 2.0 ** -23)


def test_update_is_a_multiply_then_a_subtract_not_an_fma():
    # S = 1, p_tok = 2^-4: s = 4 exactly; tau = 1: e = 3; rate f32(0.7) = 0x1.666666p-1. The exact
    # product 0x1.0cccccc8p+1 needs 26 bits and rounds to 0x1.0cccccp+1; from mu = 2.5 the contract
    # gives 2.5 - RN(product) = 0x1.9999ap-2 exactly, a fused RN(2.5 - product) 0x1.99999cp-2.
    rate, e, mu = f32(0.7), 3, f32(2.5)
    assert R.surprise(f32(1.0), f32(2.0 ** -4)) == f32(4.0)
    prod = f32(rate * f32(e))
    assert float(prod).hex() == "0x1.0ccccc0000000p+1"
    fused = f32(float(mu) - float(rate) * e)  # double holds the product and the difference exactly
    assert float(fused).hex() == "0x1.99999c0000000p-2"
    got = R.update(mu, 1.0, rate, f32(1.0), f32(2.0 ** -4))
    assert float(got).hex() == "0x1.9999a00000000p-2" and got != fused


def test_update_moves_towards_tau_and_is_capped_at_four_tau():
    # a token less surprising than tau raises the threshold, a more surprising one lowers it
    assert R.update(6.0, 3.0, 0.5, f32(1.0), f32(0.5)) == f32(7.0)        # s = 1: mu - 0.5 (1 - 3)
    assert R.update(6.0, 3.0, 0.5, f32(1.0), f32(2.0 ** -7)) == f32(4.0)  # s = 7: mu - 0.5 (7 - 3)
    assert R.update(6.0, 3.0, 0.5, f32(1.0), f32(0.125)) == f32(6.0)      # s = tau: unchanged
    # the cap: s = 0, tau = 3, rate = 1 from 11.5 would give 14.5; 4 tau = 12
    assert R.update(11.5, 3.0, 1.0, f32(0.5), f32(0.5)) == f32(12.0)
    assert R.update(12.0, 3.0, 1.0, f32(0.5), f32(0.5)) == f32(12.0)
    assert R.update(1.5, 0.5, 1.0, f32(0.5), f32(0.5)) == f32(2.0)        # exactly 4 tau: not above
    assert R.initial_mu(3.0) == f32(6.0) and R.initial_mu(0.5) == f32(1.0)


def _ordered(a):
    i = np.asarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def test_lg_against_libm_and_float64_on_a_sweep():
    """Every 4099th f32 of (0, 1], subnormals included, and 1.0 itself: 259 907 values. Measured:
    against libm's log2f at most 1 ulp (49 values differ), against float64 log2 at most 0.50000007
    ulp of the result. The gates are those figures plus one ulp."""
    bits = np.append(np.arange(1, 0x3F800000 + 1, 4099, dtype=np.uint32), np.uint32(0x3F800000))
    x = bits.view(np.float32)
    got = R.lg(x)
    libm = ctypes.CDLL(ctypes.util.find_library("m"))
    libm.log2f.restype, libm.log2f.argtypes = ctypes.c_float, [ctypes.c_float]
    ref = np.array([libm.log2f(float(v)) for v in x], dtype=np.float32)
    d = np.abs(_ordered(got) - _ordered(ref))
    r64 = np.log2(x.astype(np.float64))
    err = np.abs(got.astype(np.float64) - r64) / np.spacing(np.abs(r64).astype(np.float32)).astype(np.float64)
    print(f"lg sweep: {len(x)} values, vs log2f max {d.max()} ulp ({int((d > 0).sum())} differ), "
          f"vs float64 max {err.max():.8f} ulp")
    assert d.max() <= 1 + 1
    assert err.max() <= 0.50000007 + 1.0


def test_running_surprise_is_pulled_towards_tau():
    """CPU reference only. A row of 8193 N(0, 1) logits has about 12.3 bits of entropy; with tau =
    3 (at least 2 bits below it, the side on which the test is valid: mu is capped, so a row with
    less entropy than tau cannot be pushed up) the mean surprise of launches 64..256 must lie closer
    to tau than the row's entropy does."""
    rs = np.random.RandomState(20)
    row = rs.randn(8193).astype(np.float32)
    tau, rate = f32(3.0), f32(0.1)
    p = R.softmax(row)
    pp = p[p > 0].astype(np.float64)
    entropy = float(-(pp * np.log2(pp)).sum())
    assert entropy >= float(tau) + 2.0
    mu, sur = R.initial_mu(tau), []
    draws = rs.randint(0, 1 << 24, 256)
    for step in range(256):
        a = R.sample_p(p, mu, f32(draws[step]) * f32(2.0 ** -24))
        sur.append(float(R.surprise(a.S, a.p_tok)))
        mu = R.update(mu, tau, rate, a.S, a.p_tok)
    mean = float(np.mean(sur[64:]))
    print(f"entropy {entropy:.3f} bits, tau {float(tau)}, mean surprise of launches 64..256 {mean:.3f}, final mu {float(mu):.3f}")
    assert abs(mean - float(tau)) < abs(entropy - float(tau))
