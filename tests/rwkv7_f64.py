"""Float64 restatement of oracle/rwkv7.c -- TEST INFRASTRUCTURE (a helper module like tsm_ref.py).

The same RWKV-7 x070 arithmetic as the C oracle, in numpy float64, so a test can say how much of
a GPU-vs-reference difference belongs to the kernels: the f32 oracle has rounding error of its own
(about 1e-5 on the logits at C = 1024, growing with C), this one has none worth naming.

Matrices are decoded from the blob through weights.layout (bf16 or f16, by the header's dtype).
Everything per-row is batched over a segment's rows as matrix products; only the WKV recurrence
walks row by row, vectorised over heads. State layout is the oracle's and slot_read's, per layer
[att_shift C | S[h][i][j] H*N*N | ffn_shift C].
"""
import numpy as np

from rwkvtts import _ffi
from rwkvtts import weights as W


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def _layer_norm(x, w, b, eps=1e-5):
    mean = x.mean(axis=-1, keepdims=True)
    d = x - mean
    var = (d * d).mean(axis=-1, keepdims=True)
    return d / np.sqrt(var + eps) * w + b


class Model:
    def __init__(self, blob):
        blob = np.ascontiguousarray(blob).view(np.uint8)
        hdr = blob[:256].view(np.int32)
        if hdr.view(np.uint32)[0] != 0x37545752:
            raise ValueError("bad weight blob")
        self.dtype = int(hdr[2])
        names = ["n_layer", "n_embd", "head_size", "n_ffn", "n_vocab", "d_decay", "d_aaa", "d_mv", "d_gate"]
        self.dims = d = {n: int(hdr[4 + i]) for i, n in enumerate(names)}
        self.C, self.N = d["n_embd"], d["head_size"]
        self.H = self.C // self.N
        self.per_layer = 2 * self.C + self.H * self.N * self.N
        self.g = {}
        self.layers = [dict() for _ in range(d["n_layer"])]
        ents, nb = W.layout(d)
        if nb > blob.size:
            raise ValueError("short weight blob")
        for layer, t, off, r, c, m in ents:
            if m:
                bits = blob[off:off + 2 * r * c].view(np.uint16)
                if layer < 0:  # emb and head stay packed: rows are decoded on use
                    self.g[t] = bits.reshape(r, c)
                    continue
                a = self._decode(bits).reshape(r, c)
            else:
                a = blob[off:off + 4 * r * c].view(np.float32).astype(np.float64)
            (self.g if layer < 0 else self.layers[layer])[t] = a

    def _decode(self, bits):
        if self.dtype == _ffi.DTYPE_BF16:
            return W.bf16_bits_to_f32(bits).astype(np.float64)
        return np.asarray(bits, dtype=np.uint16).view(np.float16).astype(np.float64)

    def state_floats(self):
        return self.dims["n_layer"] * self.per_layer

    def new_state(self):
        return np.zeros(self.state_floats(), dtype=np.float64)

    def forward_rows(self, state, tokens, head_rows):
        """logits[len(tokens)][head_rows] (float64); `state` (float64, oracle layout) advances in
        place by len(tokens) tokens."""
        C, N, H = self.C, self.N, self.H
        toks = np.asarray(tokens, dtype=np.int64)
        T = toks.size
        if T == 0:
            return np.zeros((0, head_rows))
        x = _layer_norm(self._decode(self.g[W.G_EMB][toks]), self.g[W.G_LN0_W], self.g[W.G_LN0_B])
        vfirst = None
        for l, p in enumerate(self.layers):
            st = state[l * self.per_layer:(l + 1) * self.per_layer]
            att_shift, S, ffn_shift = st[:C], st[C:C + H * N * N].reshape(H, N, N), st[C + H * N * N:]
            # ---- time mix ----
            xx = _layer_norm(x, p[W.L_LN1_W], p[W.L_LN1_B])
            dx = np.vstack([att_shift[None], xx[:-1]]) - xx
            att_shift[:] = xx[-1]
            xr, xw, xk, xv, xa, xg = (xx + dx * p[t] for t in (W.L_XR, W.L_XW, W.L_XK, W.L_XV, W.L_XA, W.L_XG))
            r, k, v = xr @ p[W.L_WR].T, xk @ p[W.L_WK].T, xv @ p[W.L_WV].T
            w = np.exp(-np.exp(-0.5) * _sigmoid(p[W.L_W0] + np.tanh(xw @ p[W.L_W1T].T) @ p[W.L_W2T].T))
            a = _sigmoid(p[W.L_A0] + (xa @ p[W.L_A1T].T) @ p[W.L_A2T].T)
            g = _sigmoid(xg @ p[W.L_G1T].T) @ p[W.L_G2T].T
            kk = (k * p[W.L_KK]).reshape(T, H, N)
            kk = kk / np.maximum(np.sqrt((kk * kk).sum(-1, keepdims=True)), 1e-12)
            k = k * (1.0 + (a - 1.0) * p[W.L_KA])
            if l == 0:
                vfirst = v
            else:
                v = v + (vfirst - v) * _sigmoid(p[W.L_V0] + (xv @ p[W.L_V1T].T) @ p[W.L_V2T].T)
            # ---- WKV-7: S = S diag(w) - (S kk)(kk*a)^T + v k^T; y = S r ----
            rh, kh, vh, wh = (z.reshape(T, H, N) for z in (r, k, v, w))
            bh = kk * a.reshape(T, H, N)
            y = np.empty((T, H, N))
            Sc = S.copy()
            for t in range(T):
                sa = np.einsum("hij,hj->hi", Sc, kk[t])
                Sc = Sc * wh[t][:, None, :] - sa[:, :, None] * bh[t][:, None, :] + vh[t][:, :, None] * kh[t][:, None, :]
                y[t] = np.einsum("hij,hj->hi", Sc, rh[t])
            S[:] = Sc
            # ---- GroupNorm(H, eps 64e-5) + bonus, gate, output ----
            mean = y.mean(-1, keepdims=True)
            dy = y - mean
            gn = dy / np.sqrt((dy * dy).mean(-1, keepdims=True) + 64e-5)
            gn = gn.reshape(T, C) * p[W.L_LNX_W] + p[W.L_LNX_B]
            bonus = (rh * kh * p[W.L_RK].reshape(H, N)).sum(-1, keepdims=True)
            att = (gn + (bonus * vh).reshape(T, C)) * g
            x = x + att @ p[W.L_WO].T
            # ---- channel mix ----
            xx = _layer_norm(x, p[W.L_LN2_W], p[W.L_LN2_B])
            kx = xx + (np.vstack([ffn_shift[None], xx[:-1]]) - xx) * p[W.L_FFN_XK]
            ffn_shift[:] = xx[-1]
            kf = np.maximum(kx @ p[W.L_FFN_K].T, 0.0)
            x = x + (kf * kf) @ p[W.L_FFN_V].T
        if head_rows <= 0:
            return np.zeros((T, 0))
        xo = _layer_norm(x, self.g[W.G_LNOUT_W], self.g[W.G_LNOUT_B])
        return xo @ self._decode(self.g[W.G_HEAD][:head_rows]).T
