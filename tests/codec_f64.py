"""float64 restatement of the BiCodec decoder (numpy; test infrastructure, CPU only).

Written from oracle/codec.c, reading the weight blob through the layout of
include/rwkvtts_codec_layout.h (restated here: numel / offset; tests/test_codec_f64.py checks them
against rwkvtts_codec_blob_bytes). Two things:

  decode(dims, blob, sem, glob)  -> (pcm, convs): the whole decoder in float64, and every conv /
      ConvTranspose output in the order oracle/codec.c computes them (a residual unit is two
      entries: its conv7 and its conv1), pre- and post-Snake.
  launch(rec, wt, x_hi, x_lo, res, rbias, lens) -> the exact float64 result of ONE k_conv launch
      from its captured inputs (BiCodecDetokenizer.capture_launch), with the error budget of the
      kernel's f32 accumulation per output element (A = sum |addend|, addend count m).

Both take `mutate`: a deliberate fault from MUTATIONS, for the tests that show what the gates
resolve (tests/test_codec_f64.py).
"""
import numpy as np

# ---- layout (include/rwkvtts_codec_layout.h) ------------------------------------------------
_CD = ("CODEBOOK OUTP_W OUTP_B FSQ_W FSQ_B SPK_W SPK_B PRE_W PRE_B EMB_W EMB_B N0_SW N0_SB N0_HW N0_HB "
       "FLN_W FLN_B LIN_W LIN_B CIN_W CIN_B SOUT_A COUT_W COUT_B").split()
_CB = "DW_W DW_B SW SB HW HB PW1_W PW1_B PW2_W PW2_B GAMMA".split()
_CU = ("SNAKE T_W T_B R0_A1 R0_W7 R0_B7 R0_A2 R0_W1 R0_B1 R1_A1 R1_W7 R1_B7 R1_A2 R1_W1 R1_B1 "
       "R2_A1 R2_W7 R2_B7 R2_A2 R2_W1 R2_B1").split()
CD = {n: i for i, n in enumerate(_CD)}
CB = {n: i for i, n in enumerate(_CB)}
CU = {n: i for i, n in enumerate(_CU)}
SPK_LATENT = 128
HOP = 320
DILS = (1, 3, 9)

# ---- the dims sets of tests/test_gpu_codec_dims.py (hop 320, codebook 8192, spk_dim = latent_dim) ----
DIMS_U2 = dict(codebook_size=8192, codebook_dim=8, latent_dim=64, n_global=32, fsq_levels=4, fsq_dims=6,
               spk_dim=64, prenet_dim=128, prenet_inter=192, prenet_layers=16, dec_channels=256, n_up=2,
               up_rates=(20, 16), up_kernels=(100, 16))
DIMS_U3 = dict(codebook_size=8192, codebook_dim=16, latent_dim=128, n_global=8, fsq_levels=5, fsq_dims=4,
               spk_dim=128, prenet_dim=512, prenet_inter=256, prenet_layers=1, dec_channels=768, n_up=3,
               up_rates=(8, 8, 5), up_kernels=(26, 8, 5))
DIMS_U1 = dict(codebook_size=8192, codebook_dim=8, latent_dim=64, n_global=32, fsq_levels=4, fsq_dims=6,
               spk_dim=64, prenet_dim=320, prenet_inter=64, prenet_layers=0, dec_channels=192, n_up=1,
               up_rates=(320,), up_kernels=(640,))
NEW_SETS = {"u2": DIMS_U2, "u3": DIMS_U3, "u1": DIMS_U1}


def n_codes(d):
    return d["fsq_levels"] ** d["fsq_dims"]


def tokens(d, T, seed):
    """(global, semantic) codes of one utterance, seeded."""
    rs = np.random.default_rng(seed)
    return rs.integers(0, n_codes(d), d["n_global"]), rs.integers(0, d["codebook_size"], T)


def numel(d, g, idx, t):
    L, P, I, S, Q = d["latent_dim"], d["prenet_dim"], d["prenet_inter"], d["spk_dim"], SPK_LATENT
    if g == 0:
        last = d["dec_channels"] >> d["n_up"]
        return {CD["CODEBOOK"]: d["codebook_size"] * d["codebook_dim"], CD["OUTP_W"]: L * d["codebook_dim"],
                CD["OUTP_B"]: L, CD["FSQ_W"]: Q * d["fsq_dims"], CD["FSQ_B"]: Q, CD["SPK_W"]: S * Q * d["n_global"],
                CD["SPK_B"]: S, CD["PRE_W"]: P * L, CD["PRE_B"]: P, CD["EMB_W"]: P * 7 * P, CD["EMB_B"]: P,
                CD["N0_SW"]: P * S, CD["N0_HW"]: P * S, CD["N0_SB"]: P, CD["N0_HB"]: P, CD["FLN_W"]: P,
                CD["FLN_B"]: P, CD["LIN_W"]: L * P, CD["LIN_B"]: L, CD["CIN_W"]: d["dec_channels"] * 7 * L,
                CD["CIN_B"]: d["dec_channels"], CD["SOUT_A"]: last, CD["COUT_W"]: 7 * last, CD["COUT_B"]: 1}[t]
    if g == 1:
        return {CB["DW_W"]: P * 7, CB["SW"]: P * S, CB["HW"]: P * S, CB["PW1_W"]: I * P, CB["PW1_B"]: I,
                CB["PW2_W"]: P * I}.get(t, P)
    Ci, Co = d["dec_channels"] >> idx, d["dec_channels"] >> (idx + 1)
    if t == CU["SNAKE"]:
        return Ci
    if t == CU["T_W"]:
        return Co * d["up_kernels"][idx] * Ci
    if t in (CU["R0_W7"], CU["R1_W7"], CU["R2_W7"]):
        return Co * 7 * Co
    if t in (CU["R0_W1"], CU["R1_W1"], CU["R2_W1"]):
        return Co * Co
    return Co


def offset(d, g, idx, t):
    """Element offset of tensor (g, idx, t); g == -1: the blob's element count."""
    off = 64
    for gg, (nidx, nt) in enumerate(((1, len(_CD)), (d["prenet_layers"], len(_CB)), (d["n_up"], len(_CU)))):
        for i in range(nidx):
            for tt in range(nt):
                if (gg, i, tt) == (g, idx, t):
                    return off
                off += (numel(d, gg, i, tt) + 63) & ~63
    return off


def tensor(d, blob, g, idx, t, shape=None):
    o = offset(d, g, idx, t)
    a = np.asarray(blob[o:o + numel(d, g, idx, t)], dtype=np.float64)
    return a.reshape(shape) if shape else a


def tensor_ref(d, blob, ref, shape=None):
    """A tensor by its reference in a launch record (group * 1000000 + index * 100 + tensor; -1: None)."""
    if ref < 0:
        return None
    return tensor(d, blob, ref // 1000000, (ref // 100) % 10000, ref % 100, shape)


# ---- arithmetic --------------------------------------------------------------------------------
def snake(x, a):
    return x + np.sin(a * x) ** 2 / (a + 1e-9)


def gelu(x):
    from math import erf
    return 0.5 * x * (1.0 + np.vectorize(erf)(x * 0.70710678118654752))


def bf16_bits(x32):
    """f32 -> bf16 bits, round to nearest even (f32_to_bf16 of csrc/common.h)."""
    u = np.ascontiguousarray(x32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)


def bf16_val(bits):
    """bf16 bits -> float64."""
    with np.errstate(invalid="ignore"):  # (rows past an utterance's end may hold any bits, NaNs among them)
        return (np.ascontiguousarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def split_hi_lo(x):
    """x -> (hi, lo) as float64 values of the bf16 planes: hi = bf16(f32(x)), lo = bf16(f32(x) - hi)."""
    x32 = np.asarray(x, dtype=np.float32)
    hi = bf16_val(bf16_bits(x32))
    lo = bf16_val(bf16_bits((x32.astype(np.float64) - hi).astype(np.float32)))
    return hi, lo


def corr(x, w, kind, K, dil, pad, s, skip=None):
    """The sum over taps and input channels of one conv (kind 0: y[t] = sum_k x[t + k dil - pad] . w[:, k];
    kind 1, ConvTranspose(K, s, p = (K - s) / 2): y[ti s + k - p] += x[ti] . w[:, k]), no bias.
    x [T][Ci], w [Co][K][Ci] -> [T (* s)][Co]. skip(k) -> output-row mask that tap k does NOT reach
    (mutations), or None."""
    T, Co = x.shape[0], w.shape[0]
    if kind == 0:
        y = np.zeros((T, Co))
        for k in range(K):
            sh = k * dil - pad
            lo, hi = max(0, -sh), min(T, T - sh)
            if hi <= lo:
                continue
            c = x[lo + sh:hi + sh] @ w[:, k, :].T
            if skip is not None and skip(k) is not None:
                c = c * (~skip(k)[lo:hi])[:, None]
            y[lo:hi] += c
        return y
    p, To = (K - s) // 2, T * s
    y = np.zeros((To, Co))
    ti = np.arange(T)
    for k in range(K):
        to = ti * s + k - p
        m = (to >= 0) & (to < To)
        if skip is not None and skip(k) is not None:
            m = m & ~skip(k)[np.clip(to, 0, To - 1)]
        if m.any():
            y[to[m]] += x[m] @ w[:, k, :].T
    return y


# ---- mutations: deliberate faults of the kind a tiling bug makes --------------------------------
# Each is applied to ONE conv (a launch, or one entry of decode()'s list) and described against the
# launch's tiling: TM output rows per time tile (32 * waves), TN columns per column tile.
MUTATIONS = ("drop_tap", "neighbour_row", "zero_row", "skip_residual")


def mutated_corr(x, w, kind, K, dil, pad, s, mutate, TM):
    """corr() with the mutation's fault in the tap sum (drop_tap, neighbour_row), else corr()."""
    T = x.shape[0]
    rows = T * (s if kind == 1 else 1)
    if mutate == "drop_tap":
        # a ConvTranspose phase loses its last tap (the largest k of phase 0); a conv its last tap
        if kind == 1:
            p = (K - s) // 2
            kr = p % s
            klast = kr + ((K - kr + s - 1) // s - 1) * s
            mask = (np.arange(rows) % s) == 0
            return corr(x, w, kind, K, dil, pad, s, skip=lambda k: mask if k == klast else None)
        if K == 1:
            return None
        return corr(x, w, kind, K, dil, pad, s, skip=lambda k: np.ones(rows, bool) if k == K - 1 else None)
    if mutate == "neighbour_row":
        # the first 32-channel chunk of the window row that tap 0 reads for a time tile's first
        # output row, and that the last tap reads for a tile's last output row, comes from the
        # neighbouring input row
        y = corr(x, w, kind, K, dil, pad, s)
        hit = False
        p = (K - s) // 2
        for t_out, first in ((((rows - 1) // TM) * TM, True), (rows - 1, False)):
            if kind == 0:  # the taps of this output row that read a row inside the utterance
                kk = [q for q in range(K) if 0 <= t_out + q * dil - pad < T]
            else:
                kk = [q for q in range(K) if (t_out + p - q) % s == 0 and 0 <= (t_out + p - q) // s < T]
            if not kk:
                continue
            k = kk[0] if first else kk[-1]
            r = t_out + k * dil - pad if kind == 0 else (t_out + p - k) // s
            rn = r + 1 if r + 1 < T else r - 1
            if not (0 <= r < T and 0 <= rn < T):
                continue
            y[t_out] += (x[rn, :32] - x[r, :32]) @ w[:, k, :32].T
            hit = True
        return y if hit else None
    return corr(x, w, kind, K, dil, pad, s)


def mutate_output(v, res_term, mutate, TM, TN):
    """The output-side faults: zero_row (the last row of the first time tile, or of the utterance if
    it has one tile only), skip_residual (the last column tile gets no residual)."""
    if mutate == "zero_row":
        v = v.copy()
        v[min(TM, v.shape[0]) - 1] = 0.0
        return v
    if mutate == "skip_residual":
        if res_term is None:
            return None
        v = v.copy()
        v[:, -TN:] -= res_term[:, -TN:]
        return v
    return v


# ---- the whole decoder -------------------------------------------------------------------------
def decode(d, blob, sem, glob, mutate=None, keep=True):
    """float64 decode -> (pcm [T * 320], convs). convs: one dict per conv in oracle/codec.c's order:
    name, kind, y (the conv's result after bias / GELU / gamma / residual), planes (y after the
    Snake its consumer applies, or None), and the conv's shape. mutate = (index into convs, name
    from MUTATIONS, TM, TN) applies that fault to that conv; a fault that does not apply to it
    (no residual, one tap) raises ValueError. Each entry also keeps the conv's activated input x, its
    residual and per-utterance bias (what a launch capture delivers); keep=False keeps no arrays
    (long utterances)."""
    sem, glob = np.asarray(sem, np.int64), np.asarray(glob, np.int64)
    T = sem.size
    L, P, I, S = d["latent_dim"], d["prenet_dim"], d["prenet_inter"], d["spk_dim"]
    Q, G, cd = SPK_LATENT, d["n_global"], d["codebook_dim"]
    t0 = lambda t, shape=None: tensor(d, blob, 0, 0, CD[t], shape)
    convs = []

    def conv(name, x, w, b, kind=0, K=1, dil=1, pad=0, s=1, act=0, gamma=None, res=None, rbias=None, alpha=None):
        """x: the activated input. alpha: the Snake of this conv's consumer (planes)."""
        idx = len(convs)
        mut = mutate[1] if mutate is not None and mutate[0] == idx else None
        TM, TN = (mutate[2], mutate[3]) if mut else (0, 0)
        acc = mutated_corr(x, w, kind, K, dil, pad, s, mut, TM) if mut else corr(x, w, kind, K, dil, pad, s)
        if acc is None:
            raise ValueError(f"mutation {mut} does not apply to conv {idx} ({name})")
        v = acc + b + (rbias if rbias is not None else 0.0)
        if act:
            v = gelu(v)
        if gamma is not None:
            v = v * gamma
        if res is not None:
            v = v + res
        if mut in ("zero_row", "skip_residual"):
            v = mutate_output(v, res, mut, TM, TN)
            if v is None:
                raise ValueError(f"mutation {mut} does not apply to conv {idx} ({name})")
        e = dict(name=name, kind=kind, ci=x.shape[1], co=w.shape[0], k=K, dil=dil, s=s)
        if keep:
            e.update(x=x, res=res, rbias=rbias, y=v, planes=snake(v, alpha) if alpha is not None else None)
        convs.append(e)
        return v

    # speaker d-vector
    half = d["fsq_levels"] // 2
    idx = glob.copy()
    code = np.zeros((G, d["fsq_dims"]))
    for k in range(d["fsq_dims"]):
        code[:, k] = ((idx % d["fsq_levels"]) - half) / half
        idx //= d["fsq_levels"]
    h = t0("FSQ_W", (Q, d["fsq_dims"])) @ code.T + t0("FSQ_B")[:, None]  # [Q][G]: flatten (c, t)
    dvec = t0("SPK_W", (S, Q * G)) @ h.reshape(-1) + t0("SPK_B")
    # semantic FVQ
    z = t0("CODEBOOK", (d["codebook_size"], cd))[sem] @ t0("OUTP_W", (L, cd)).T + t0("OUTP_B")

    def layer_norm(x, scale, shift):
        mean = x.mean(axis=1, keepdims=True)
        var = ((x - mean) ** 2).mean(axis=1, keepdims=True)
        return (x - mean) / np.sqrt(var + 1e-6) * scale + shift

    u = conv("pre", z, t0("PRE_W", (P, 1, L)), t0("PRE_B"))
    x = conv("embed", u, t0("EMB_W", (P, 7, P)), t0("EMB_B"), K=7, pad=3)
    x = layer_norm(x, t0("N0_SW", (P, S)) @ dvec + t0("N0_SB"), t0("N0_HW", (P, S)) @ dvec + t0("N0_HB"))
    for l in range(d["prenet_layers"]):
        tb = lambda t, shape=None: tensor(d, blob, 1, l, CB[t], shape)
        dw = tb("DW_W", (P, 7))
        u = np.zeros_like(x)
        for k in range(7):
            sh = k - 3
            lo, hi = max(0, -sh), min(T, T - sh)
            if hi > lo:
                u[lo:hi] += x[lo + sh:hi + sh] * dw[:, k]
        u = layer_norm(u + tb("DW_B"), tb("SW", (P, S)) @ dvec + tb("SB"), tb("HW", (P, S)) @ dvec + tb("HB"))
        hid = conv(f"pw1.{l}", u, tb("PW1_W", (I, 1, P)), tb("PW1_B"), act=1)
        x = conv(f"pw2.{l}", hid, tb("PW2_W", (P, 1, I)), tb("PW2_B"), gamma=tb("GAMMA"), res=x)
    x = layer_norm(x, t0("FLN_W"), t0("FLN_B"))
    y = conv("lin", x, t0("LIN_W", (L, 1, P)), t0("LIN_B"), rbias=dvec)
    # WaveGenerator
    C = d["dec_channels"]
    tu = lambda ub, t, shape=None: tensor(d, blob, 2, ub, CU[t], shape)
    a = conv("conv_in", y, t0("CIN_W", (C, 7, L)), t0("CIN_B"), K=7, pad=3, alpha=tu(0, "SNAKE"))
    for ub in range(d["n_up"]):
        Co, s, K = C // 2, d["up_rates"][ub], d["up_kernels"][ub]
        b = conv(f"convT.{ub}", snake(a, tu(ub, "SNAKE")), tu(ub, "T_W", (Co, K, C)), tu(ub, "T_B"), kind=1, K=K, s=s,
                 alpha=tu(ub, "R0_A1"))
        for r in range(3):
            nxt = tu(ub, f"R{r + 1}_A1") if r < 2 else (tu(ub + 1, "SNAKE") if ub + 1 < d["n_up"] else t0("SOUT_A"))
            r1 = conv(f"res7.{ub}.{r}", snake(b, tu(ub, f"R{r}_A1")), tu(ub, f"R{r}_W7", (Co, 7, Co)), tu(ub, f"R{r}_B7"),
                      K=7, dil=DILS[r], pad=3 * DILS[r], alpha=tu(ub, f"R{r}_A2"))
            b = conv(f"res1.{ub}.{r}", snake(r1, tu(ub, f"R{r}_A2")), tu(ub, f"R{r}_W1", (Co, 1, Co)), tu(ub, f"R{r}_B1"),
                     res=b, alpha=nxt)
        a, C = b, Co
    out = corr(snake(a, t0("SOUT_A")), t0("COUT_W", (1, 7, C)), 0, 7, 1, 3, 1) + t0("COUT_B")
    return np.tanh(out[:, 0]), convs


# ---- one k_conv launch -------------------------------------------------------------------------
def launch_weights(d, blob, rec):
    """The tensors launch() needs for the launch `rec` (a dict of codec.launch_plan), from the f32
    blob: the conv weights as the bf16 hi plane the kernel stages (and the lo plane on the weight-lo
    path), everything else as stored."""
    K, Ci, Co = rec["k"], rec["ci"], rec["co"]
    w32 = np.asarray(tensor_ref(d, blob, rec["w"], (Co, K, Ci)), dtype=np.float32)
    wh = bf16_val(bf16_bits(w32))
    wt = dict(w=wh, wl=None)
    if rec["wlo"]:
        wt["wl"] = bf16_val(bf16_bits((w32.astype(np.float64) - wh).astype(np.float32)))
    for name in ("bias", "gamma", "y_alpha", "mid_alpha", "bias1"):
        wt[name] = tensor_ref(d, blob, rec[name])
    wt["w1"] = None
    if rec["w1"] >= 0:
        wt["w1"] = bf16_val(bf16_bits(np.asarray(tensor_ref(d, blob, rec["w1"], (Co, 1, Co)), dtype=np.float32)))
    return wt


EPS24 = 2.0 ** -24
SIN_DELTA = 1e-6  # the hardware sine's absolute error (csrc/codec.hip, snake_fast)


def launch(rec, wt, x_hi, x_lo, res, rbias, lens, mutate=None):
    """The exact float64 result of one k_conv launch on its captured inputs.

    x_hi, x_lo: [n][rows_in][ci] float64 values of the input planes; res [n][rows_out][co] or None;
    rbias [n][co] or None; lens: frames per utterance (rows past lens * tin_mul are zeros to the
    kernel, and output rows past lens * tin_mul (* s) are not written).
    The tap sum is x_hi w_hi + x_lo w_hi (+ x_hi w_lo on the weight-lo path; x_lo w_lo is not
    computed by the kernel and not here). Returns per utterance a dict:
      y       the f32 output's exact value (bias, per-utterance bias, GELU, gamma, residual)
      planes  y through the output Snake (float64 sin), or None
      rows    valid output rows
      A, m    sum |addend| per output element and the addend count of the tap sum
      hard, model   callables factor-free: see gates()
    For a fused residual unit (kind 2) both halves run, with the mid Snake and the bf16 hi + lo
    re-split of the intermediate as the kernel does; A and m are those of the second half and
    `mid_*` carry the first half's, for gates()."""
    kind, K, dil, pad, s = rec["kind"], rec["k"], rec["dil"], rec["pad"], rec["s"]
    ck = 1 if kind == 1 else 0
    TM, TN = 32 * rec["nwv"], rec["tn"]
    outs = []
    for i, T in enumerate(lens):
        rin = T * rec["tin_mul"]
        rout = rin * (s if kind == 1 else 1)
        xh, xl = x_hi[i, :rin], x_lo[i, :rin]
        w, wl = wt["w"], wt["wl"]
        mut_sum = mutate if mutate in ("drop_tap", "neighbour_row") else None

        def tapsum(xa):
            if mut_sum:
                return mutated_corr(xa, w, ck, K, dil, pad, s, mut_sum, TM)
            return corr(xa, w, ck, K, dil, pad, s)
        acc = tapsum(xh + xl)
        if acc is None:
            raise ValueError(f"mutation {mutate} does not apply to this launch")
        A = corr(np.abs(xh) + np.abs(xl), np.abs(w), ck, K, dil, pad, s)
        ntaps = (K + s - 1) // s if kind == 1 else K
        m = ntaps * rec["ci"] * 2
        if wl is not None:
            acc = acc + corr(xh, wl, ck, K, dil, pad, s)
            A = A + corr(np.abs(xh), np.abs(wl), ck, K, dil, pad, s)
            m = ntaps * rec["ci"] * 3
        o = dict(rows=rout)
        if kind == 2:
            mid = acc + wt["bias"]
            pm = snake(mid, wt["mid_alpha"])
            ph, pl = split_hi_lo(pm)
            o.update(mid=mid, mid_planes=pm, mid_A=A, mid_m=m)
            acc = corr(ph + pl, wt["w1"], 0, 1, 1, 0, 1)
            A = corr(np.abs(ph) + np.abs(pl), np.abs(wt["w1"]), 0, 1, 1, 0, 1)
            m = rec["co"] * 2
            bias = wt["bias1"]
        else:
            bias = wt["bias"]
        v0 = acc + bias + (rbias[i] if rbias is not None else 0.0)
        v = gelu(v0) if rec["act"] else v0
        if wt["gamma"] is not None:
            v = v * wt["gamma"]
        r = res[i, :rout] if res is not None else None
        pre = v
        if r is not None:
            v = v + r
        if mutate in ("zero_row", "skip_residual"):
            v = mutate_output(v, r, mutate, TM, TN)
            if v is None:
                raise ValueError(f"mutation {mutate} does not apply to this launch")
        o.update(y=v, A=A, m=m, v0=v0, pre=pre, res=r,
                 planes=snake(v, wt["y_alpha"]) if wt["y_alpha"] is not None else (v if rec["has_planes"] else None))
        outs.append(o)
    return outs


def gates(rec, wt, o, factor):
    """(gate on y, gate on the planes' hi + lo sum) per output element for one utterance's launch()
    result `o`: |gpu - f64| <= factor(m) * 2^-23 * A through the epilogue, plus the epilogue's own terms.

    factor(m) = m is the derived hard gate (every f32 addition of the tap sum rounds, or truncates,
    by at most 2^-23 of the running sum, which |.| <= A bounds); factor(m) = c * sqrt(m) the
    random-walk model (tests/test_codec_f64.py adopts c per launch class).
    Epilogue: the tap-sum error passes GELU (slope <= 1.13) and gamma; bias, GELU, gamma and the
    residual add round a few times: 8 * 2^-24 of the magnitudes involved. Planes: the Snake's slope is
    at most 2, the hardware sine adds SIN_DELTA * 2 |sin| / (alpha + 1e-9), and hi + lo holds the
    value to 2^-16 relative.
    Fused residual unit: the first half's gate (tap sum, bias rounding, mid Snake, re-split) is an
    error of the second half's input: it enters through sum_c |w1[co][c]| * gate_mid[c]."""
    acc_err = factor(o["m"]) * 2.0 ** -23 * o["A"]
    if rec["kind"] == 2:
        mid_err = factor(o["mid_m"]) * 2.0 ** -23 * o["mid_A"] + 8 * EPS24 * np.abs(o["mid"])
        a = wt["mid_alpha"]
        pm_err = (2.0 * mid_err + SIN_DELTA * 2.0 * np.abs(np.sin(a * o["mid"])) / (a + 1e-9) +
                  (2.0 ** -16 + 8 * EPS24) * np.abs(o["mid_planes"]))
        acc_err = acc_err + pm_err @ np.abs(wt["w1"][:, 0, :]).T
    e = acc_err * (1.13 if rec["act"] else 1.0)
    if wt["gamma"] is not None:
        e = e * np.abs(wt["gamma"])
    mag = np.abs(o["v0"]) + np.abs(o["pre"]) + np.abs(o["y"]) + (np.abs(o["res"]) if o["res"] is not None else 0.0)
    gy = e + 8 * EPS24 * mag
    gp = None
    if o["planes"] is not None:
        gp = gy.copy()
        if wt["y_alpha"] is not None:
            a = wt["y_alpha"]
            gp = 2.0 * gy + SIN_DELTA * 2.0 * np.abs(np.sin(a * o["y"])) / (a + 1e-9)
        gp = gp + (2.0 ** -16 + 8 * EPS24) * np.abs(o["planes"])
    return gy, gp


# The random-walk factor c of the per-launch model gate c sqrt(m) 2^-23 A, per launch class
# (launch_class); a class not listed has the default, 8 sigma. tests/test_codec_f64.py adopts a
# factor only where a one-addend-at-a-time f32 accumulation of the same addends stays inside it
# at every element: the largest |err| / (sqrt(m) 2^-23 A) that emulation reaches on any class is 0.2, so
# no class is widened.
MODEL_FACTOR_DEFAULT = 8.0
MODEL_FACTOR = {}


def model_factor(rec):
    c = MODEL_FACTOR.get(launch_class(rec), MODEL_FACTOR_DEFAULT)
    return lambda m: c * np.sqrt(m)


def launch_class(rec):
    """What the per-launch error tables group by: the instantiation and the launch kind."""
    kind = ("conv", "convT", "fused")[rec["kind"]]
    return f"{kind}({rec['tn']},{rec['kt']},{'wlo' if rec['wlo'] else 'bf16'},{rec['nwv']})"


# ---- shared by tests/test_codec_f64.py, test_codec_plan_cpu.py and test_gpu_codec_dims.py ------------
FORM_SEPARATE_RESUNIT = 1
PCM_ATOL = 5e-4      # the end-to-end gates of tests/test_gpu_codec.py
PCM_RTOL_L2 = 1e-4


def dims_of(name):
    from rwkvtts import codec
    return {"tiny": codec.CODEC_DIMS_TINY, "full": codec.CODEC_DIMS_FULL}.get(name) or NEW_SETS[name]


_blobs, _refs = {}, {}


def blob(name, wname):
    """The weights every test of a dims set uses: wname "bf16" (MFMA operands bf16-exact) or "f32"
    (synth_codec_blob_f32: the decoder then takes the weight hi + lo path). Cached."""
    from rwkvtts import codec
    if (name, wname) not in _blobs:
        f = codec.synth_codec_blob if wname == "bf16" else codec.synth_codec_blob_f32
        _blobs[name, wname] = f(dims_of(name), seed=11)
    return _blobs[name, wname]


def reference(name, wname, T, seed):
    """(global, semantic, float64 PCM) of the utterance tokens(dims, T, seed). Cached: computed once
    per process, shared by every test that needs it, never modified."""
    key = (name, wname, T, seed)
    if key not in _refs:
        d = dims_of(name)
        g, s = tokens(d, T, seed)
        pcm, _ = decode(d, blob(name, wname), s, g, keep=False)
        pcm.setflags(write=False)
        _refs[key] = (g, s, pcm)
    return _refs[key]


def pcm_errors(got, ref):
    """(max abs, relative L2) of got against ref."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(got - ref).max()), float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-300))


def xmap_length(d, wlo, forms, want):
    """The smallest T at which every launch of a one-utterance decode that `want(rec)` names runs the
    XCD-mapped 1-D grid with surplus blocks (xmap, gx % 8 != 0), from the library's launch plan."""
    from rwkvtts import codec
    for T in range(1, 2049):
        named = [r for r in codec.launch_plan(d, wlo, forms, 1, T) if want(r)]
        assert named, "no launch of that description"
        if all(r["xmap"] and r["gx"] % 8 for r in named):
            return T
    raise AssertionError("no such length up to 2048")


# The lengths the GPU tests of the three sets run beyond T in (1, 5) and the ragged batch: the
# smallest T at which the named launches get the padded XCD-mapped grid (tests/test_codec_plan_cpu.py
# re-derives each from the launch plan).
XMAP_CASES = {
    # set: (T, forms, wlo, description, predicate)
    "u2": (410, 0, False, "conv7 @ 128 of the 20x stage",
           lambda r: r["kind"] == 0 and r["k"] == 7 and r["co"] == 128 and r["tin_mul"] == 20),
    "u3": (129, 0, False, "conv7 and conv1 @ 192",
           lambda r: r["kind"] == 0 and r["co"] == 192 and r["ci"] == 192),
    "u3s": (26, FORM_SEPARATE_RESUNIT, False, "separate-form conv7 @ 96",
            lambda r: r["kind"] == 0 and r["k"] == 7 and r["co"] == 96 and r["ci"] == 96),
    "u1s": (26, FORM_SEPARATE_RESUNIT, False, "separate-form conv7 @ 96",
            lambda r: r["kind"] == 0 and r["k"] == 7 and r["co"] == 96 and r["ci"] == 96),
}
RAGGED = (5, 2, 4)  # the ragged batch of every set (frames per utterance)


def gpu_cases(name):
    """[(T, seed)] single-utterance decodes tests/test_gpu_codec_dims.py compares with float64 for a
    set, the ragged batch's utterances included (the CPU tests hold the oracle to a quarter of the
    gates on exactly these)."""
    out = [(1, 1), (5, 5)] + [(T, 100 + i) for i, T in enumerate(RAGGED)]
    for key, (T, *_rest) in XMAP_CASES.items():
        if key.rstrip("s") == name and (T, T) not in out:
            out.append((T, T))
    return out


def plan_convs(plan):
    """For each launch of `plan`, the indices into decode()'s conv list it computes (two for a fused
    residual unit)."""
    out, j = [], 0
    for r in plan:
        out.append((j, j + 1) if r["kind"] == 2 else (j,))
        j += 2 if r["kind"] == 2 else 1
    return out


def synthetic_capture(rec, convs, idx):
    """What a launch capture would deliver for launch `rec`, from a float64 decode's convs (idx from
    plan_convs): the input planes as the bf16 hi + lo split of the activated input, the residual and
    per-utterance bias rounded to f32. One utterance."""
    first, last = convs[idx[0]], convs[idx[-1]]
    xh, xl = split_hi_lo(first["x"])
    f32 = lambda a: None if a is None else np.asarray(a, np.float32).astype(np.float64)[None]
    return xh[None], xl[None], f32(last["res"]), f32(last["rbias"])


def f32_tap_sum(rec, wt, xh, xl):
    """The first tap sum of a launch accumulated in f32 ONE ADDEND AT A TIME (numpy float32, round to
    nearest; tap by tap, channel by channel, x_hi w_hi then x_lo w_hi then x_hi w_lo): the arithmetic
    the random-walk gate models, in reference arithmetic only. Every product is exact in f32 (two
    8-bit significands). xh, xl [rows][ci] -> float64 [rows_out][co]."""
    kind, K, dil, pad, s = rec["kind"], rec["k"], rec["dil"], rec["pad"], rec["s"]
    T, Co = xh.shape[0], rec["co"]
    x32 = [np.asarray(xh, np.float32), np.asarray(xl, np.float32)]
    w32 = np.asarray(wt["w"], np.float32)
    wl32 = None if wt["wl"] is None else np.asarray(wt["wl"], np.float32)
    rows = T * (s if kind == 1 else 1)
    acc = np.zeros((rows, Co), np.float32)
    p = (K - s) // 2
    for k in range(K):
        if kind == 1:
            to = np.arange(T) * s + k - p
            m = (to >= 0) & (to < rows)
            src, dst = np.nonzero(m)[0], to[m]
        else:
            sh = k * dil - pad
            lo, hi = max(0, -sh), min(T, T - sh)
            src, dst = np.arange(lo + sh, hi + sh), np.arange(lo, hi)
        if src.size == 0:
            continue
        sub = acc[dst]
        for ci in range(rec["ci"]):
            sub += x32[0][src, ci, None] * w32[None, :, k, ci]
            sub += x32[1][src, ci, None] * w32[None, :, k, ci]
            if wl32 is not None:
                sub += x32[0][src, ci, None] * wl32[None, :, k, ci]
        acc[dst] = sub
    return acc.astype(np.float64)
