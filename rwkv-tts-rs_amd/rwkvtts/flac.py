"""A FLAC decoder for mono 16-bit streams, written from RFC 9639 (host only, numpy).

`decode(data) -> (int16 samples, sample_rate)`. It is the independent reader of what the GPU encoder
(csrc/flac.hip, audio.FlacEncoder) writes -- it shares no code with the encoder or with the encoder's
numpy contract (tests/flac_ref.py) -- and it is how POST /api/watermark/detect takes a FLAC upload. It
reads any mono 16-bit stream: fixed or variable block size, every block-size and sample-rate code,
CONSTANT, VERBATIM, FIXED and LPC subframes with wasted bits, both Rice codings (4- and 5-bit
parameters) and their escape code, metadata blocks other than STREAMINFO skipped. It checks the frame
sync code, the header CRC-8, the frame CRC-16, the sample count and the MD5 of STREAMINFO where those
are not zero ("unknown"), and raises ValueError on anything else: more channels, another sample size,
a reserved code, a truncated frame. Unverified against libFLAC: no third-party FLAC implementation
was at hand when this was written.
"""
import hashlib

import numpy as np

_RATES = {1: 88200, 2: 176400, 3: 192000, 4: 8000, 5: 16000, 6: 22050, 7: 24000, 8: 32000, 9: 44100, 10: 48000,
          11: 96000}
_FIXED = {0: [], 1: [1], 2: [2, -1], 3: [3, -3, 1], 4: [4, -6, 4, -1]}


def _table(poly, width):
    top, mask, out = 1 << (width - 1), (1 << width) - 1, []
    for b in range(256):
        c = b << (width - 8)
        for _ in range(8):
            c = ((c << 1) ^ poly) & mask if c & top else (c << 1) & mask
        out.append(c)
    return out


_T8, _T16 = _table(0x07, 8), _table(0x8005, 16)


def _crc8(data):
    c = 0
    for b in data:
        c = _T8[c ^ b]
    return c


def _crc16(data):
    c = 0
    for b in data:
        c = ((c << 8) & 0xFFFF) ^ _T16[(c >> 8) ^ b]
    return c


class _Short(ValueError):
    """The bits ran out: the frame is truncated, or longer than the window that was unpacked for it."""


class _Bits:
    """A window of the stream as bits: w[i] the 32 bits from bit i on, nxt[i] the first set bit at or
    after i."""

    def __init__(self, data):
        b = np.frombuffer(data, dtype=np.uint8)
        self.nbits = 8 * b.size
        p = np.concatenate([b, np.zeros(8, dtype=np.uint8)]).astype(np.int64)
        w40 = (p[:-4] << 32) | (p[1:-3] << 24) | (p[2:-2] << 16) | (p[3:-1] << 8) | p[4:]
        i = np.arange(self.nbits + 8, dtype=np.int64)
        self.w_np = (w40[i >> 3] >> (8 - (i & 7))) & 0xFFFFFFFF
        self.w = self.w_np.tolist()
        bits = np.unpackbits(b)
        idx = np.where(bits == 1, np.arange(bits.size), self.nbits + 64)
        self.nxt = np.concatenate([np.minimum.accumulate(idx[::-1])[::-1], [self.nbits + 64] * 8]).tolist()
        self.pos = 0

    def need(self, n):
        if self.pos + n > self.nbits:
            raise _Short("FLAC: truncated frame")

    def u(self, n):
        if n == 0:
            return 0
        self.need(n)
        v = self.w[self.pos] >> (32 - n)
        self.pos += n
        return v

    def s(self, n):
        v = self.u(n)
        return v - (1 << n) if n and v >> (n - 1) else v

    def unary(self):
        e = self.nxt[self.pos]
        if e >= self.nbits:
            raise _Short("FLAC: truncated frame")
        q, self.pos = e - self.pos, e + 1
        return q

    def array(self, count, n, signed=True):
        """count fields of n bits (n <= 32) -> int64."""
        if n == 0 or count == 0:
            return np.zeros(count, dtype=np.int64)
        self.need(count * n)
        v = self.w_np[self.pos + n * np.arange(count, dtype=np.int64)] >> (32 - n)
        self.pos += count * n
        return np.where(v >> (n - 1), v - (1 << n), v) if signed else v


def _coded_number(data, pos):
    """The UTF-8-like number at data[pos] -> (value, next pos)."""
    if pos >= len(data):
        raise ValueError("FLAC: truncated frame header")
    b0 = data[pos]
    if b0 < 0x80:
        return b0, pos + 1
    n = 8 - (b0 ^ 0xFF).bit_length()  # leading ones
    if n < 2 or n > 7 or pos + n > len(data):
        raise ValueError("FLAC: bad coded number")
    v = b0 & (0x7F >> n)
    for b in data[pos + 1:pos + n]:
        if b & 0xC0 != 0x80:
            raise ValueError("FLAC: bad coded number")
        v = (v << 6) | (b & 0x3F)
    return v, pos + n


def _residual(br, n, order):
    method = br.u(2)
    if method > 1:
        raise ValueError("FLAC: reserved residual coding method")
    pbits, esc = (4, 15) if method == 0 else (5, 31)
    po = br.u(4)
    if n % (1 << po) or (n >> po) < order:
        raise ValueError("FLAC: bad partition order")
    out = []
    w, nxt, nbits = br.w, br.nxt, br.nbits
    for p in range(1 << po):
        cnt = (n >> po) - (order if p == 0 else 0)
        k = br.u(pbits)
        if k == esc:
            out.extend(br.array(cnt, br.u(5)).tolist())
            continue
        pos, sh = br.pos, 32 - k
        for _ in range(cnt):
            e = nxt[pos]
            if e + k >= nbits:
                raise _Short("FLAC: truncated frame")
            zz = (((e - pos) << k) | (w[e + 1] >> sh)) if k else e - pos
            pos = e + 1 + k
            out.append((zz >> 1) ^ -(zz & 1))
        br.pos = pos
    return out


def _predict(warm, res, coefs, shift):
    out = [int(v) for v in warm]
    p = len(coefs)
    if p == 0:
        return out + res
    rc = coefs[::-1]
    for r in res:
        acc = 0
        for c, v in zip(rc, out[-p:]):
            acc += c * v
        out.append(r + (acc >> shift))
    return out


def _subframe(br, n, bps):
    if br.u(1):
        raise ValueError("FLAC: subframe padding bit set")
    kind = br.u(6)
    wasted = 0
    if br.u(1):
        wasted = br.unary() + 1
        bps -= wasted
        if bps <= 0:
            raise ValueError("FLAC: too many wasted bits")
    if kind == 0:
        out = [br.s(bps)] * n
    elif kind == 1:
        out = br.array(n, bps).tolist()
    elif 8 <= kind <= 12:
        order = kind - 8
        if order > n:
            raise ValueError("FLAC: predictor order above the block size")
        warm = br.array(order, bps).tolist()
        out = _predict(warm, _residual(br, n, order), _FIXED[order], 0)
    elif kind >= 32:
        order = kind - 31
        if order > n:
            raise ValueError("FLAC: predictor order above the block size")
        warm = br.array(order, bps).tolist()
        prec = br.u(4) + 1
        if prec == 16:
            raise ValueError("FLAC: reserved coefficient precision")
        shift = br.s(5)
        if shift < 0:
            raise ValueError("FLAC: negative predictor shift")
        coefs = [br.s(prec) for _ in range(order)]
        out = _predict(warm, _residual(br, n, order), coefs, shift)
    else:
        raise ValueError("FLAC: reserved subframe type")
    return [v << wasted for v in out] if wasted else out


def decode(data):
    """A FLAC file (or a stream whose STREAMINFO leaves the totals unknown) -> (int16 samples, rate)."""
    data = bytes(data)
    if data[:4] != b"fLaC":
        raise ValueError("FLAC: no fLaC marker")
    pos, info = 4, None
    while True:
        if pos + 4 > len(data):
            raise ValueError("FLAC: truncated metadata")
        last, kind, size = data[pos] >> 7, data[pos] & 0x7F, int.from_bytes(data[pos + 1:pos + 4], "big")
        body = data[pos + 4:pos + 4 + size]
        if len(body) != size or kind == 127:
            raise ValueError("FLAC: bad metadata block")
        if kind == 0:
            if info is not None or pos != 4 or size != 34:
                raise ValueError("FLAC: bad STREAMINFO")
            info = body
        pos += 4 + size
        if last:
            break
    if info is None:
        raise ValueError("FLAC: no STREAMINFO")
    v = int.from_bytes(info[10:18], "big")
    rate, channels, bps, total = v >> 44, ((v >> 41) & 7) + 1, ((v >> 36) & 31) + 1, v & ((1 << 36) - 1)
    md5 = info[18:34]
    if channels != 1 or bps != 16:
        raise ValueError(f"FLAC: only mono 16-bit streams are read (this one: {channels} channels, {bps} bits)")
    if rate == 0:
        raise ValueError("FLAC: sample rate 0")
    samples = []
    count = 0
    while pos < len(data):
        start = pos
        if len(data) - pos < 6 or data[pos] != 0xFF or data[pos + 1] & 0xFE != 0xF8:
            raise ValueError("FLAC: lost frame sync")
        bs_code, sr_code = data[pos + 2] >> 4, data[pos + 2] & 15
        ch_code, ss_code, reserved = data[pos + 3] >> 4, (data[pos + 3] >> 1) & 7, data[pos + 3] & 1
        if reserved or bs_code == 0 or sr_code == 15:
            raise ValueError("FLAC: reserved code in a frame header")
        if ch_code != 0:
            raise ValueError("FLAC: only mono frames are read")
        if ss_code not in (0, 4):
            raise ValueError("FLAC: only 16-bit frames are read")
        _, pos = _coded_number(data, pos + 4)
        extra = (1 if bs_code == 6 else 2 if bs_code == 7 else 0) + (1 if sr_code == 12 else 2 if sr_code in (13, 14) else 0)
        if pos + extra + 1 > len(data):
            raise ValueError("FLAC: truncated frame header")
        if bs_code == 1:
            n = 192
        elif bs_code <= 5:
            n = 576 << (bs_code - 2)
        elif bs_code == 6:
            n, pos = data[pos] + 1, pos + 1
        elif bs_code == 7:
            n, pos = int.from_bytes(data[pos:pos + 2], "big") + 1, pos + 2
        else:
            n = 256 << (bs_code - 8)
        if sr_code == 0:
            frame_rate = rate
        elif sr_code <= 11:
            frame_rate = _RATES[sr_code]
        elif sr_code == 12:
            frame_rate, pos = data[pos] * 1000, pos + 1
        else:
            frame_rate, pos = int.from_bytes(data[pos:pos + 2], "big") * (1 if sr_code == 13 else 10), pos + 2
        if frame_rate != rate:
            raise ValueError("FLAC: a frame's sample rate differs from STREAMINFO's")
        if _crc8(data[start:pos]) != data[pos]:
            raise ValueError("FLAC: frame header CRC-8 mismatch")
        pos += 1
        window = 4 * n + 64  # bytes unpacked for the subframe: enough for any frame near 16 bits a sample
        while True:
            br = _Bits(data[pos:pos + window])
            try:
                out = _subframe(br, n, 16)
                break
            except _Short:
                if pos + window >= len(data):
                    raise
                window *= 8
        if len(out) != n:
            raise ValueError("FLAC: subframe length mismatch")
        pos += (br.pos + 7) // 8
        if pos + 2 > len(data):
            raise ValueError("FLAC: truncated frame")
        if _crc16(data[start:pos]) != int.from_bytes(data[pos:pos + 2], "big"):
            raise ValueError("FLAC: frame CRC-16 mismatch")
        pos += 2
        samples.append(np.asarray(out, dtype=np.int64))
        count += n
    x = np.concatenate(samples) if samples else np.zeros(0, dtype=np.int64)
    if x.size and (x.min() < -32768 or x.max() > 32767):
        raise ValueError("FLAC: a decoded sample does not fit 16 bits")
    pcm = x.astype(np.int16)
    if total and total != pcm.size:
        raise ValueError(f"FLAC: STREAMINFO promises {total} samples, the frames hold {pcm.size}")
    if md5 != b"\0" * 16 and hashlib.md5(pcm.astype("<i2").tobytes()).digest() != md5:
        raise ValueError("FLAC: MD5 mismatch")
    return pcm, rate
