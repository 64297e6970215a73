"""The FLAC encoder's contract (include/rwkvtts.h) restated in numpy: every bit
of csrc/flac.hip's output is defined here. Integer arithmetic throughout, except the quantisation (three
rounded f32 operations per sample) and the Levinson-Durbin recursion (Python floats: IEEE f64, one
rounded operation at a time). Vectorised over a block's samples; Python-level loops run over blocks,
candidates, partition orders and the recursion's scalars only. No code is shared with the decoder
(rwkvtts/flac.py)."""
import hashlib

import numpy as np

RATE_CODES = {8000: 4, 16000: 5, 22050: 6, 24000: 7, 32000: 8, 44100: 9, 48000: 10}
BLOCK_CODES = {256: 8, 512: 9, 1024: 10, 2048: 11, 4096: 12}
MAX_LPC, PRECISION, MAX_K, MAX_PORDER = 12, 12, 14, 8
I64 = np.int64


def quantise(x, scale=1.0):
    """q = trunc(clamp(x * scale, -1, 1) * 32767), each operation rounded to f32 on its own."""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    y = np.clip(x * np.float32(scale), np.float32(-1.0), np.float32(1.0)) * np.float32(32767.0)
    return np.trunc(y).astype(np.int16)


def window(n):
    """The Q15 Welch window of an n-sample block: w[i] = 32768 - floor(32768 d^2 / D^2), d = 2i - n + 1,
    D = n + 1 (1 .. 32768; symmetric)."""
    d = 2 * np.arange(n, dtype=I64) - n + 1
    return 32768 - (32768 * d * d) // ((n + 1) * (n + 1))


def table():
    """The stage's table: the windows of the five block sizes back to back, int32."""
    return np.concatenate([window(b) for b in sorted(BLOCK_CODES)]).astype(np.int32)


def autocorrelation(q, max_lag):
    """v = (q * w) >> 10 (arithmetic); R[l] = sum_{i >= l} v[i] v[i - l], l = 0 .. max_lag, in int64
    (|v| <= 2^20 and n <= 4096: |R| <= 2^52, so the sum is exact and its f64 value too)."""
    q = np.asarray(q, dtype=I64)
    v = (q * window(q.size)) >> 10
    return [int(np.sum(v[l:] * v[:q.size - l])) for l in range(max_lag + 1)]


def levinson(R, m):
    """-> the predictors of orders 1 .. (as far as the recursion goes, at most m): a[j] multiplies
    s[i - 1 - j]. The recursion stops before an order whose error E is not > 0."""
    a, E, out = [], float(R[0]), []
    for i in range(m):
        if not E > 0.0:
            break
        acc = float(R[i + 1])
        for j in range(i):
            acc = acc - a[j] * float(R[i - j])
        k = acc / E
        a = [a[j] - k * a[i - 1 - j] for j in range(i)] + [k]
        E = E * (1.0 - k * k)
        out.append(list(a))
    return out


def quantise_coefficients(a):
    """-> (12-bit integers, shift) or None. With 2^(e-1) <= max|a| < 2^e: shift = min(11 - e, 15), the
    order is dropped if that is negative or max|a| is zero or not finite; c = clamp(rint(a * 2^shift),
    -2048, 2047), rint to even."""
    a = np.asarray(a, dtype=np.float64)
    if not np.all(np.isfinite(a)):
        return None
    cmax = float(np.max(np.abs(a)))
    if not cmax > 0.0:
        return None
    shift = min(11 - int(np.frexp(cmax)[1]), 15)
    if shift < 0:
        return None
    c = np.clip(np.rint(a * float(1 << shift)), -2048.0, 2047.0).astype(I64)
    return c, shift


def fixed_residual(s, order):
    return np.diff(s, order) if order else s.copy()


def lpc_residual(s, c, shift):
    p, n = len(c), s.size
    pred = np.zeros(n - p, dtype=I64)
    for j in range(p):
        pred += int(c[j]) * s[p - 1 - j:n - 1 - j]
    return s[p:] - (pred >> shift)


def max_partition_order(n, order):
    o = 0
    while o < MAX_PORDER and n % (2 << o) == 0 and (n >> (o + 1)) > order:
        o += 1
    return o


def rice_plan(res, n, order):
    """-> (bits of the partitioned residual without its 6 header bits, partition order, k per partition):
    the exact count for every partition order, the best k per partition (the lowest on a tie), the
    lowest order on a tie."""
    r = np.asarray(res, dtype=I64)
    zz = np.zeros(n, dtype=I64)
    zz[order:] = (r << 1) ^ (r >> 63)
    ks = np.arange(MAX_K + 1, dtype=I64)[:, None]
    best = None
    for o in range(max_partition_order(n, order) + 1):
        S = (zz[None, :] >> ks).reshape(MAX_K + 1, 1 << o, n >> o).sum(axis=2)
        cnt = np.full(1 << o, n >> o, dtype=I64)
        cnt[0] -= order
        bits = S + (ks + 1) * cnt[None, :]
        k = np.argmin(bits, axis=0)
        total = int(np.sum(4 + bits[k, np.arange(1 << o)]))
        if best is None or total < best[0]:
            best = (total, o, k)
    return best


# ---- bits ------------------------------------------------------------------------------------
def _place(bits, pos, vals, nbits):
    """bits[pos[i] ...] = the nbits[i] low bits of vals[i], most significant first."""
    pos, vals, nbits = (np.asarray(v, dtype=I64) for v in (pos, vals, nbits))
    idx = np.repeat(np.arange(pos.size), nbits)
    off = np.arange(int(nbits.sum())) - np.repeat(np.cumsum(nbits) - nbits, nbits)
    bits[pos[idx] + off] = (vals[idx] >> (nbits[idx] - 1 - off)) & 1


def _fields(fields):
    vals = np.array([v & ((1 << b) - 1) for v, b in fields], dtype=I64)
    nb = np.array([b for _, b in fields], dtype=I64)
    bits = np.zeros(int(nb.sum()), dtype=np.uint8)
    _place(bits, np.cumsum(nb) - nb, vals, nb)
    return bits


def _rice_bits(res, n, order, o, k):
    plen = n >> o
    i = np.arange(order, n)
    part = i // plen
    kk = k[part].astype(I64)
    r = np.asarray(res, dtype=I64)
    zz = (r << 1) ^ (r >> 63)
    first = np.zeros(i.size, dtype=I64)          # a partition's first residual carries its 4-bit k
    first[np.concatenate([[0], np.arange(1, 1 << o) * plen - order])] = 4
    length = first + (zz >> kk) + 1 + kk
    start = np.cumsum(length) - length
    bits = np.zeros(int(length.sum()), dtype=np.uint8)
    head = first > 0
    _place(bits, start[head], kk[head], first[head])
    _place(bits, start + first + (zz >> kk), (1 << kk) | (zz & ((1 << kk) - 1)), kk + 1)
    return bits


def utf8(v):
    if v < 0x80:
        return bytes([v])
    n = next(k for k in range(2, 7) if v < 1 << (5 * k + 1))
    out = [((0xFF << (8 - n)) & 0xFF) | (v >> (6 * (n - 1)))]
    return bytes(out + [0x80 | ((v >> (6 * j)) & 0x3F) for j in range(n - 2, -1, -1)])


def crc8(data):
    c = 0
    for b in data:
        c ^= b
        for _ in range(8):
            c = ((c << 1) ^ 0x07) & 0xFF if c & 0x80 else (c << 1) & 0xFF
    return c


def _mul16(a, b):
    """a * b mod x^16 + x^15 + x^2 + 1 over GF(2), elementwise (a an array, b an int)."""
    a = np.asarray(a, dtype=I64)
    out = np.zeros_like(a)
    for bit in range(15, -1, -1):
        out = ((out << 1) ^ np.where(out & 0x8000, 0x18005, 0)) & 0xFFFF
        if (b >> bit) & 1:
            out ^= a
    return out


def crc16(data):
    """CRC-16, polynomial 0x8005, initial value 0, by halving: zero bytes in front change nothing, and
    CRC(A || B) = CRC(A) * x^(8 |B|) + CRC(B)."""
    d = np.frombuffer(bytes(data), dtype=np.uint8).astype(I64)
    if d.size == 0:
        return 0
    size = 1 << (d.size - 1).bit_length()
    c = _crc_bytes(np.concatenate([np.zeros(size - d.size, dtype=I64), d]))
    xp = 0x0100  # x^8: what a chunk's CRC is multiplied by when one byte follows it
    while c.size > 1:
        c = _mul16(c[0::2], xp) ^ c[1::2]
        xp = int(_mul16(np.array([xp]), xp)[0])
    return int(c[0])


def _crc_bytes(b):
    """The CRC of each one-byte message."""
    c = np.asarray(b, dtype=I64) << 8
    for _ in range(8):
        c = ((c << 1) ^ np.where(c & 0x8000, 0x18005, 0)) & 0xFFFF
    return c


# ---- frames ----------------------------------------------------------------------------------
def choose(s, lpc=True):
    """The block's subframe: ("constant",) | ("verbatim",) | ("fixed", order, res, o, k) |
    ("lpc", order, c, shift, res, o, k), and its size in bits."""
    n = s.size
    if np.all(s == s[0]):
        return ("constant",), 24
    best, best_bits = ("verbatim",), 8 + 16 * n
    cands = [("fixed", p, fixed_residual(s, p)) for p in range(min(5, n))]
    if lpc:
        m = min(MAX_LPC, n - 1)
        for a in (levinson(autocorrelation(s, m), m) if m > 0 else []):
            qc = quantise_coefficients(a)
            if qc is not None:
                cands.append(("lpc", len(a), qc[0], qc[1], lpc_residual(s, qc[0], qc[1])))
    found = None
    for cand in cands:
        p, res = cand[1], cand[-1]
        rice, o, k = rice_plan(res, n, p)
        bits = 8 + 16 * p + 6 + rice + (9 + PRECISION * p if cand[0] == "lpc" else 0)
        if found is None or bits < found[1]:
            found = (cand + (o, k), bits)
    if found is not None and found[1] < best_bits:
        best, best_bits = found
    return best, best_bits


def encode_frame(q, frame_number, rate, B, lpc=True):
    """One frame: q the block's int16 samples (len(q) == B, or 1 .. B - 1 for a signal's last)."""
    s = np.asarray(q, dtype=I64)
    n = s.size
    assert 1 <= n <= B and 0 <= frame_number < 1 << 31
    bs = BLOCK_CODES[B] if n == B else (6 if n <= 256 else 7)
    hdr = bytes([0xFF, 0xF8, (bs << 4) | RATE_CODES[rate], 0x08]) + utf8(frame_number)
    if bs == 6:
        hdr += bytes([n - 1])
    elif bs == 7:
        hdr += bytes([(n - 1) >> 8, (n - 1) & 0xFF])
    hdr += bytes([crc8(hdr)])
    sub, _ = choose(s, lpc)
    smp = lambda a: [(int(v), 16) for v in a]
    if sub[0] == "constant":
        bits = _fields([(0x00, 8), (int(s[0]), 16)])
    elif sub[0] == "verbatim":
        bits = _fields([(0x02, 8)] + smp(s))
    elif sub[0] == "fixed":
        _, p, res, o, k = sub
        bits = np.concatenate([_fields([((8 | p) << 1, 8)] + smp(s[:p]) + [(0, 2), (o, 4)]), _rice_bits(res, n, p, o, k)])
    else:
        _, p, c, shift, res, o, k = sub
        head = [((32 | (p - 1)) << 1, 8)] + smp(s[:p]) + [(PRECISION - 1, 4), (shift, 5)]
        head += [(int(v), PRECISION) for v in c] + [(0, 2), (o, 4)]
        bits = np.concatenate([_fields(head), _rice_bits(res, n, p, o, k)])
    body = hdr + np.packbits(bits).tobytes()
    c = crc16(body)
    return body + bytes([c >> 8, c & 0xFF])


def streaminfo(rate, B, min_frame=0, max_frame=0, total=0, md5=b"\0" * 16):
    """"fLaC" and the one (last) STREAMINFO block: 42 bytes."""
    v = (rate << 44) | (0 << 41) | (15 << 36) | total
    return (b"fLaC" + bytes([0x80, 0, 0, 34]) + B.to_bytes(2, "big") + B.to_bytes(2, "big") +
            min_frame.to_bytes(3, "big") + max_frame.to_bytes(3, "big") + v.to_bytes(8, "big") + bytes(md5))


def encode_frames(q, rate, B, first_frame=0, lpc=True):
    q = np.asarray(q, dtype=np.int16)
    return [encode_frame(q[i:i + B], first_frame + i // B, rate, B, lpc) for i in range(0, q.size, B)]


def default_block(rate):
    return 1024 if rate <= 24000 else 2048


def bound(n, B):
    """The largest byte count n samples can give: 2 n + 16 per frame."""
    return 2 * n + 16 * (-(-n // B))


def encode(x, rate, scale=1.0, block=None, lpc=True):
    """A whole signal -> the FLAC file."""
    B = block or default_block(rate)
    q = quantise(x, scale)
    frames = encode_frames(q, rate, B, 0, lpc)
    sizes = [len(f) for f in frames] or [0]
    md5 = hashlib.md5(q.astype("<i2").tobytes()).digest()
    return streaminfo(rate, B, min(sizes), max(sizes), q.size, md5) + b"".join(frames)


def evaluator(encoder, items):
    """Stands in for the native call of audio.FlacEncoder: items [(pcm, scale, rate, block, first_frame,
    final, lpc)] -> [(bytes, min_frame, max_frame)]."""
    out = []
    for x, scale, rate, B, first, final, lpc in items:
        frames = encode_frames(quantise(x, scale), rate, B, first, lpc)
        sizes = [len(f) for f in frames] or [0]
        out.append((b"".join(frames), min(sizes), max(sizes)))
    return out


def vowel(n, rate=16000, f0=120.0, peak=0.5, seed=3, breath=0.05):
    """A synthetic vowel: a pulse train at f0 plus breath noise through four formant resonators in parallel."""
    rng = np.random.RandomState(seed)
    t = np.arange(n)
    period = rate / f0
    e = np.zeros(n)
    e[(np.arange(int(n / period) + 1) * period).astype(int).clip(0, n - 1)] = 1.0
    e += breath * rng.randn(n)
    y = np.zeros(n)
    for f, bw in ((700.0, 90.0), (1200.0, 110.0), (2600.0, 160.0), (5200.0, 400.0)):  # parallel: a bright spectrum
        r = np.exp(-np.pi * bw / rate)
        a1, a2 = 2.0 * r * np.cos(2.0 * np.pi * f / rate), -r * r
        out = np.zeros(n)
        y1 = y2 = 0.0
        for i in range(n):
            v = e[i] + a1 * y1 + a2 * y2
            out[i] = v
            y2, y1 = y1, v
        y = y + out
    return (y * (peak / np.max(np.abs(y)))).astype(np.float32)


# ---- the signals both test files use ---------------------------------------------------------
KINDS = ("silence", "dc", "ramp", "alternating", "noise", "impulse", "clamp", "vowel16", "vowel48")
_LONGEST = 2 * 4096 + 37
_cache = {}


def lengths(B):
    """The short last block, an order above the length, odd lengths (partition order 0 only), every
    padding of 0 .. 7 bits, more than one block."""
    return (1, 12, 13, 255, 256, 257, 4095, 2 * B + 37)


def rate_of(kind):
    return 48000 if kind == "vowel48" else 16000


def signal(kind, n):
    """The first n samples of the kind's signal (f32)."""
    if kind not in _cache:
        N, rng = _LONGEST, np.random.RandomState(KINDS.index(kind))
        if kind == "silence":
            x = np.zeros(N)
        elif kind == "dc":
            x = np.full(N, 0.25)
        elif kind == "ramp":          # q = 3 i (mod 30000): second differences all zero inside a block
            x = ((3 * np.arange(N)) % 30000 + 0.5) / 32767.0
        elif kind == "alternating":   # +-32767: the widest FIXED residuals
            x = np.where(np.arange(N) % 2, -1.0, 1.0)
        elif kind == "noise":         # full scale and white: nothing beats VERBATIM
            x = rng.uniform(-1.0, 1.0, N)
        elif kind == "impulse":
            x = np.zeros(N)
            x[5] = 0.9
        elif kind == "clamp":         # beyond +-1 and on the clamp's edge, between small values
            edge = np.array([-3.0, -1.0, -1.0000001, -0.99999994, 0.99999994, 1.0, 1.0000001, 2.5, 1e30, -1e30])
            x = np.where(rng.rand(N) < 0.2, edge[rng.randint(0, edge.size, N)], 0.01 * rng.randn(N))
        elif kind == "vowel16":
            x = vowel(N, 16000)
        else:                         # the same vowel resampled to 48 kHz
            from rwkvtts.audio import resample_audio_high_quality
            x = resample_audio_high_quality(vowel(N // 3 + 300, 16000), 16000, 48000)[400:400 + N]
        _cache[kind] = np.asarray(x, dtype=np.float32)
    return _cache[kind][:n]
