"""RWKVTTS_QUANT_INT8 / NF4 (include/rwkvtts.h, the comment above k_quant_pack) restated in numpy --
TEST INFRASTRUCTURE. 16-bit bit patterns (bf16 or f16) in; codes, scales and dequantised weights out.

Two forms of the same rule:

  dequantised()  vectorised, for whole matrices: numpy float32 operations (each IEEE, rounded once); the
                 two fused multiply-adds are formed in float64 and rounded once to float32. The
                 quantising fma's product-sum is exact in float64 (24 + 8 bits, and a v too small for
                 that gives code 0 either way); the dequantising one is asserted exact (TwoSum).
  exact()        element by element in fractions.Fraction, every float32 / f16 rounding made by _rne()
                 below: no numpy arithmetic at all. For the 16 x 256 edge matrix.

No dequantised weight is ever -0: Int8's q * step is >= +0 and (+0) + (-0) = +0, a sum that cancels is
+0, and nothing underflows (mn is a multiple of 2^-24, q * step of 2^-149); NF4's t[q] * s is a product
with s >= 2^-24 and |t| >= 0.079 or t = +0. exact() returns +0 for every zero.

quantised_model(): the float64 model (rwkv7_f64.Model) whose quantised layers hold these weights.
edge_matrix(): the matrix tests/test_gpu_quant.py::test_roundtrip and tests/test_quant_ref_cpu.py use.
"""
from fractions import Fraction

import numpy as np

from rwkvtts import _ffi
from rwkvtts import weights as W

# the NormalFloat-4 code table (QLoRA, Dettmers et al. 2023, appendix E), as float32
NF4 = np.array([-1.0, -0.6961928009986877, -0.5250730514526367, -0.39491748809814453, -0.28444138169288635,
                -0.18477343022823334, -0.09105003625154495, 0.0, 0.07958029955625534, 0.16093020141124725,
                0.24611230194568634, 0.33791524171829224, 0.44070982933044434, 0.5626170039176941,
                0.7229568362236023, 1.0], dtype=np.float32)
NF4_MID = (NF4[:-1] + NF4[1:]) * np.float32(0.5)  # float32: the sum rounded once, the half exact
BLOCK = {"int8": 128, "nf4": 64}
TARGETS = (W.L_WR, W.L_WK, W.L_WV, W.L_WO, W.L_FFN_K, W.L_FFN_V)


def decode(bits, dtype):
    """uint16 bit patterns -> float32 (exact)."""
    bits = np.asarray(bits, dtype=np.uint16)
    if dtype == _ffi.DTYPE_BF16:
        return (bits.astype(np.uint32) << np.uint32(16)).view(np.float32)
    return bits.view(np.float16).astype(np.float32)


def encode(x, dtype):
    """float -> uint16 bit patterns; asserts every value is exactly a number of the dtype."""
    x = np.asarray(x, dtype=np.float64)
    f = x.astype(np.float32)
    if dtype == _ffi.DTYPE_BF16:
        assert not (f.view(np.uint32) & 0xFFFF).any(), "not bf16 numbers"
        bits = (f.view(np.uint32) >> 16).astype(np.uint16)
    else:
        with np.errstate(over="ignore"):
            bits = f.astype(np.float16).view(np.uint16)
    assert (decode(bits, dtype).astype(np.float64) == x).all(), "not numbers of the dtype"
    return bits


def _f16(x):
    return np.asarray(x, dtype=np.float32).astype(np.float16).astype(np.float32)


# ---------------------------------------------------------------- vectorised
def dequantised(bits, dtype, qt):
    """[N][K] uint16 -> float64 [N][K]: the dequantised weights (float32 values)."""
    bits = np.asarray(bits, dtype=np.uint16)
    N, K = bits.shape
    x = decode(bits, dtype).reshape(N, K // BLOCK[qt], BLOCK[qt])
    with np.errstate(divide="ignore", invalid="ignore"):
        if qt == "int8":
            mn, mx = _f16(x.min(axis=2, keepdims=True)), _f16(x.max(axis=2, keepdims=True))
            d = mx - mn
            v = np.clip((x - mn) / d, np.float32(0), np.float32(1))
            q = np.floor((v.astype(np.float64) * 255.0 + 0.5).astype(np.float32))
            q = np.where(mx != mn, q, np.float32(0)).astype(np.float64)
            a, b = q * (d / np.float32(255)).astype(np.float64), mn.astype(np.float64) + 0.0 * q
            s = a + b
            bb = s - a
            assert not ((a - (s - bb)) + (b - bb)).any(), "the dequantising fma is not exact in float64 here"
            w = s.astype(np.float32)
        else:
            sc = _f16(np.abs(x).max(axis=2, keepdims=True))
            v = x / sc
            q = (v[..., None] > NF4_MID).sum(axis=-1)
            q = np.where(sc != 0, q, 7)
            w = (NF4[q].astype(np.float64) * sc.astype(np.float64)).astype(np.float32)
    w = w + np.float32(0)  # (-0 -> +0: see the module docstring)
    return w.reshape(N, K).astype(np.float64)


# ---------------------------------------------------------------- exact
def _rne(x, p, qexp):
    """Fraction -> the nearest number with p significant bits and quantum >= 2^qexp, ties to even."""
    if x == 0:
        return Fraction(0)
    a = abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    assert Fraction(2) ** e <= a < Fraction(2) ** (e + 1)
    quantum = Fraction(2) ** max(e - p + 1, qexp)
    n = a / quantum
    fl = n.numerator // n.denominator
    rem = n - fl
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and fl & 1):
        fl += 1
    return (fl * quantum) * (1 if x > 0 else -1)


def _r32(x):
    r = _rne(x, 24, -149)
    assert abs(r) < Fraction(2) ** 128
    return r


def _r16(x):
    r = _rne(x, 11, -24)
    assert abs(r) <= 65504, "outside f16's finite range"
    return r


def exact(bits, dtype, qt):
    """[N][K] uint16 -> dict of [N][K] arrays following the float32 operations one by one:
    w (float32, the dequantised weights), q (codes), v (float64: the float32 quotient BEFORE the
    clamp; NaN where the block has no quotient), and per-block lo / hi (Int8: f16 min, max; NF4:
    hi the f16 absmax), raw_lo / raw_hi (before the f16 rounding), as float64."""
    bits = np.asarray(bits, dtype=np.uint16)
    N, K = bits.shape
    B = BLOCK[qt]
    xs = decode(bits, dtype).astype(np.float64)
    out = {k: np.zeros((N, K)) for k in ("w", "q", "v", "lo", "hi", "raw_lo", "raw_hi")}
    t = [Fraction(float(z)) for z in NF4]
    mid = [_r32(t[i] + t[i + 1]) / 2 for i in range(15)]
    for n in range(N):
        for k0 in range(0, K, B):
            x = [Fraction(float(z)) for z in xs[n, k0:k0 + B]]
            sl = (n, slice(k0, k0 + B))
            if qt == "int8":
                raw_lo, raw_hi = min(x), max(x)
                mn, mx = _r16(raw_lo), _r16(raw_hi)
                d = _r32(mx - mn)
                step = _r32(d / 255)
                for i, xi in enumerate(x):
                    q, v = 0, None
                    if mx != mn:
                        v = _r32(_r32(xi - mn) / d)
                        vc = min(max(v, Fraction(0)), Fraction(1))
                        f = _r32(vc * 255 + Fraction(1, 2))
                        q = f.numerator // f.denominator
                    out["q"][n, k0 + i] = q
                    out["v"][n, k0 + i] = np.nan if v is None else float(v)
                    out["w"][n, k0 + i] = float(_r32(q * step + mn))
            else:
                raw_lo = raw_hi = max(abs(z) for z in x)
                mn = mx = _r16(raw_hi)
                for i, xi in enumerate(x):
                    q, v = 7, None
                    if mx != 0:
                        v = _r32(xi / mx)
                        q = sum(1 for m in mid if v > m)
                    out["q"][n, k0 + i] = q
                    out["v"][n, k0 + i] = np.nan if v is None else float(v)
                    out["w"][n, k0 + i] = float(_r32(t[q] * mx))
            for key, val in (("lo", mn), ("hi", mx), ("raw_lo", raw_lo), ("raw_hi", raw_hi)):
                out[key][sl] = float(val)
    out["w"] = out["w"].astype(np.float32)
    return out


# ---------------------------------------------------------------- the float64 model
def quantised_model(blob, dims, qt, n_layers):
    """rwkv7_f64.Model of `blob` whose layers [0, n_layers) hold the dequantised r / k / v / o / FFN key /
    FFN value matrices in float64."""
    import rwkv7_f64
    m = rwkv7_f64.Model(blob)
    raw = np.ascontiguousarray(blob).view(np.uint8)
    for layer, t, off, rows, cols, _ in W.layout(dims)[0]:
        if 0 <= layer < n_layers and t in TARGETS:
            m.layers[layer][t] = dequantised(raw[off:off + 2 * rows * cols].view(np.uint16).reshape(rows, cols), m.dtype, qt)
    return m


# ---------------------------------------------------------------- the edge matrix
def _nf4_neighbours(dtype):
    """Per NF4 midpoint i: the (x, s) pairs of dtype numbers (s = |x|'s block maximum, s >= |x|) whose
    float32 quotient x / s is the largest below mid[i], equal to it (None if no pair is), and the
    smallest above: the closest the dtype's numbers come to the strict `>` from either side."""
    pd, px = (8, 8) if dtype == _ffi.DTYPE_BF16 else (11, 11)
    D = np.arange(1 << (pd - 1), 1 << pd, dtype=np.float32)[:, None]  # s = D (one binade is enough)
    A = np.arange(1 << (px - 1), 1 << px, dtype=np.float32)[None, :]
    tables = []
    for j in range(0, 6):  # |x| = A 2^-j
        xa = A * np.float32(2.0 ** -j)
        tables.append((xa, (xa / D).astype(np.float64), xa <= D))
    picks = []
    for i, m in enumerate(NF4_MID):
        best = {}
        for xa, va, ok in tables:  # (a float32 quotient is odd in x)
            xs, v = np.copysign(xa, m), np.copysign(va, m)
            for name, sel, arg in (("below", ok & (v < m), np.argmax), ("equal", ok & (v == m), np.argmax),
                                   ("above", ok & (v > m), np.argmin)):
                if not sel.any():
                    continue
                score = np.where(sel, v, -np.inf if arg is np.argmax else np.inf)
                r, c = np.unravel_index(arg(score), score.shape)
                cand = (float(v[r, c]), float(np.broadcast_to(xs, v.shape)[r, c]), float(D[r, 0]))
                old = best.get(name)
                if old is None or (name == "below" and cand[0] > old[0]) or (name == "above" and cand[0] < old[0]):
                    best[name] = cand
        picks.append((i, best))
    return picks


def edge_matrix(dtype, qt):
    """(bits [16][256] uint16, edges): every value an exact number of the dtype inside f16's finite
    range. `edges` maps an edge's name to the (row, block) pairs built to hold it; assert_edges()
    checks through exact() that each is really there."""
    bf = dtype == _ffi.DTYPE_BF16
    B = BLOCK[qt]
    nb = 256 // B
    u = 2.0 ** -24  # f16's quantum
    over = (1 + 2.0 ** -7) * 2.0 ** -20  # a bf16 number; f16 rounds it (quantum 2^-24) to 2^-20
    rng = np.random.RandomState(5)
    blocks, names = [], []

    def add(name, vals):
        b = np.zeros(B)
        b[:len(vals)] = vals
        blocks.append(b)
        names.append(name)

    grid = np.arange(-100, 101) / 128.0  # 8 significant bits: numbers of both dtypes
    if qt == "int8":
        add("constant", [0.375] * B)
        add("constant", [-3.0] * B)
        add("zero", [0.0] * B)
        add("zero", [-0.0] * B)
        add("single", [0.0] * 17 + [0.4375])
        add("single", [0.0] * 90 + [-0.8125])             # zeros get code 255: fma(255, step, mn) for a zero
        add("half", [0.0, 1.0, 0.5] + [k / 256.0 for k in range(1, 120)])        # v = .5: v * 255 = 127.5
        add("half_above", [-u, 1.0, 0.5] + [k / 256.0 for k in range(1, 120)])   # d = r32(1 + 2^-24) = 1; v = .5 + 2^-24
        add("half_below", [u, 2.0, 1.0] + [k / 128.0 for k in range(1, 126)])    # d = r32(2 - 2^-24) = 2; v = .5 - 2^-25
        add("negzero", [-0.0, 0.25, -0.25, 0.0, -0.0, 0.125])
        add("negzero", [-0.0, 0.0, 0.5, -0.0])
        add("subnormal", [k * u for k in range(3, 41)] * 3)  # range 37 * 2^-24, min and max f16 subnormals
        add("subnormal", [-k * u for k in range(0, 128)])
        if bf:
            add("clamp", [-over, over, -2.0 ** -20, 2.0 ** -20] + [k * u for k in range(-15, 16)])
            add("clamp", [2 * over] + [k * 2.0 ** -27 + over for k in range(0, 127)])  # the maximum alone rounds (down)
        while len(blocks) < 16 * nb:
            add("random", rng.choice(grid, B) * 2.0 ** rng.randint(-6, 3))
    else:
        add("zero", [0.0] * B)
        add("zero", [0.0, -0.0] * (B // 2))
        for i, best in _nf4_neighbours(dtype):
            for side in ("below", "equal", "above"):
                if side in best:
                    _, x, s = best[side]
                    add(f"mid_{side}_{i}", [s, x, -s, -x, 0.0, -0.0] + [s * 2.0 ** -k for k in range(1, 8)] + [-s * 2.0 ** -k for k in range(1, 8)])
        add("absmax", [-1.5, 1.5, 0.75, -0.75])
        add("absmax", [-96.0] + [0.5 * k for k in range(60)])
        add("subnormal", [k * u for k in range(-31, 32)])      # absmax 31 * 2^-24
        add("subnormal", [u, -u, 0.0])                         # absmax the smallest f16 number
        if bf:
            add("absmax_rounds", [over, -over, 2.0 ** -20, -2.0 ** -20] + [k * u for k in range(-15, 16)])
            add("absmax_rounds", [-(1 + 2.0 ** -5 + 2.0 ** -6) * 2.0 ** -20] + [k * u for k in range(1, 17)])  # 16.75 * 2^-24: up, to 17
        assert len(blocks) <= 16 * nb, len(blocks)
        while len(blocks) < 16 * nb:
            add("random", rng.choice(grid, B) * 2.0 ** rng.randint(-6, 3))
    m = np.array(blocks[:16 * nb]).reshape(16, 256)
    edges = {}
    for j, name in enumerate(names[:16 * nb]):
        edges.setdefault(name, []).append((j // nb, j % nb))
    return encode(m, dtype), edges


def assert_edges(bits, dtype, qt, edges, ex):
    """Every edge of the issue's list is present in the matrix, judged by exact()'s intermediates."""
    bf = dtype == _ffi.DTYPE_BF16
    B = BLOCK[qt]

    def blk(name, key):
        return [ex[key][r, b * B:(b + 1) * B] for r, b in edges[name]]

    def inp(name):
        return [bits[r, b * B:(b + 1) * B] for r, b in edges[name]]

    if qt == "int8":
        assert any(lo[0] == hi[0] != 0 for lo, hi in zip(blk("constant", "lo"), blk("constant", "hi")))
        assert any(lo[0] == hi[0] == 0 for lo, hi in zip(blk("zero", "lo"), blk("zero", "hi")))
        assert all(np.isnan(v).all() for v in blk("constant", "v") + blk("zero", "v"))  # the mx == mn branch
        assert all((decode(b, dtype) != 0).sum() == 1 for b in inp("single"))
        assert any((w[q == 255] != 0).any() and (decode(b, dtype)[q == 255] == 0).all()  # a zero that does not come back as zero
                   for w, q, b in zip(blk("single", "w"), blk("single", "q"), inp("single")))
        half, up, dn = 0.5, float(np.nextafter(np.float32(0.5), np.float32(1))), float(np.nextafter(np.float32(0.5), np.float32(0)))
        for name, want, code in (("half", half, 128), ("half_above", up, 128), ("half_below", dn, 127)):
            v, q = blk(name, "v")[0], blk(name, "q")[0]
            assert (v == want).any() and (q[v == want] == code).all(), (name, want)
        assert Fraction(half) * 255 == Fraction(255, 2)  # n + 0.5 exactly; the only float32 v for which it is
        assert all((b == 0x8000).any() for b in inp("negzero")) and any((b == 0x8000).any() and (b == 0).any() for b in inp("negzero"))
        assert all(0 < (hi[0] - lo[0]) < 2.0 ** -14 for lo, hi in zip(blk("subnormal", "lo"), blk("subnormal", "hi")))
        clamped_lo = clamped_hi = False
        for name in edges:
            for v, lo, hi, rl, rh in zip(*(blk(name, k) for k in ("v", "lo", "hi", "raw_lo", "raw_hi"))):
                if name == "clamp":
                    assert lo[0] > rl[0] or hi[0] < rh[0]
                    clamped_lo |= bool(lo[0] > rl[0] and (v < 0).any())
                    clamped_hi |= bool(hi[0] < rh[0] and (v > 1).any())
                else:  # f16 rounding of min / max acts in the clamp blocks only
                    assert lo[0] == rl[0] and hi[0] == rh[0] and not ((v < 0) | (v > 1)).any(), name
        # (an f16 matrix cannot hold the edge: min and max are f16 numbers already)
        assert (clamped_lo and clamped_hi) if bf else "clamp" not in edges
    else:
        assert all((hi == 0).all() and (q == 7).all() and (w == 0).all()
                   for hi, q, w in zip(blk("zero", "hi"), blk("zero", "q"), blk("zero", "w")))
        assert any((b == 0x8000).any() for b in inp("zero"))
        sides = {s: [i for i in range(15) if f"mid_{s}_{i}" in edges] for s in ("below", "equal", "above")}
        assert sides["below"] == list(range(15)) and sides["above"] == list(range(15)), sides
        for s, idx in sides.items():
            for i in idx:
                v, q = blk(f"mid_{s}_{i}", "v")[0], blk(f"mid_{s}_{i}", "q")[0]
                m = float(NF4_MID[i])
                hit = (v < m) & (v > m - 2e-3) if s == "below" else v == m if s == "equal" else (v > m) & (v < m + 2e-3)
                assert hit.any() and (q[hit] == (i + 1 if s == "above" else i)).all(), (s, i)
        vs, qs = np.concatenate(blk("absmax", "v")), np.concatenate(blk("absmax", "q"))
        assert ((vs == 1) & (qs == 15)).any() and ((vs == -1) & (qs == 0)).any()
        assert all(0 < hi[0] < 2.0 ** -14 for hi in blk("subnormal", "hi"))
        for name in edges:
            for hi, rh in zip(blk(name, "hi"), blk(name, "raw_hi")):
                assert (hi[0] != rh[0]) == (name == "absmax_rounds"), name
        assert ("absmax_rounds" in edges) == bf  # (an f16 matrix cannot hold the edge)
        if bf:
            his, raws = blk("absmax_rounds", "hi"), blk("absmax_rounds", "raw_hi")
            assert any(h[0] < r[0] for h, r in zip(his, raws)) and any(h[0] > r[0] for h, r in zip(his, raws))
