"""Float64 NumPy forward of ESM C over the packed blob of proteingym_amd.esmc.pack: an independent reading of the blob layout (the
SwiGLU block order of ffn.1.weight included), the q / k LayerNorm over the whole width, the rotate-half rotary, the scaled residual
and the untied 64-column head (esm/layers/{attention,blocks,transformer_stack,regression_head}.py).  Shared by test_esmc_host.py
and test_gpu_esmc.py."""
from math import erf, sqrt

import numpy as np

_erf = np.vectorize(erf)


def _layernorm(x, w, b=None, eps=1e-5):
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    y = (x - mu) / np.sqrt(var + eps) * w
    return y if b is None else y + b


def numpy_forward(cfg, blob, ids):
    """log_softmax(sequence_logits) [T, 64] in float64 for one row of ids (no padding)."""
    D, F, V, H, L = cfg["embed_dim"], cfg["ffn_dim"], cfg["vocab"], cfg["heads"], cfg["layers"]
    dh = D // H
    o = 0

    def take(*shape):
        nonlocal o
        n = int(np.prod(shape))
        a = blob[o:o + n].astype(np.float64).reshape(shape)
        o += n
        return a
    ids = np.asarray(ids)
    T = len(ids)
    x = take(V, D)[ids]
    inv = (1.0 / (10000 ** (np.arange(0, dh, 2, dtype=np.float32) / np.float32(dh)))).astype(np.float32)
    ang = (np.arange(T, dtype=np.float32)[:, None] * inv[None, :]).astype(np.float64)
    cos, sin = np.concatenate([np.cos(ang)] * 2, -1)[:, None, :], np.concatenate([np.sin(ang)] * 2, -1)[:, None, :]

    def rot(t):
        return t * cos + np.concatenate([-t[..., dh // 2:], t[..., :dh // 2]], -1) * sin
    s = sqrt(L / 36)
    for _ in range(L):
        ln1_w, ln1_b, wqkv = take(D), take(D), take(3 * D, D)
        q_ln, k_ln, wo = take(D), take(D), take(D, D)
        ln2_w, ln2_b = take(D), take(D)
        w1 = take(F // 32, 64, D)                     # blocks of 32 gate rows then 32 up rows
        gate_w, up_w = w1[:, :32].reshape(F, D), w1[:, 32:].reshape(F, D)
        w2 = take(D, F)
        q, k, v = np.split(_layernorm(x, ln1_w, ln1_b) @ wqkv.T, 3, axis=-1)
        q, k = rot(_layernorm(q, q_ln).reshape(T, H, dh)), rot(_layernorm(k, k_ln).reshape(T, H, dh))
        sc = np.einsum("thd,shd->hts", q, k) / sqrt(dh)
        p = np.exp(sc - sc.max(-1, keepdims=True))
        p /= p.sum(-1, keepdims=True)
        x = x + (np.einsum("hts,shd->thd", p, v.reshape(T, H, dh)).reshape(T, D) @ wo.T) / s
        h = _layernorm(x, ln2_w, ln2_b)
        g = h @ gate_w.T
        x = x + ((g / (1.0 + np.exp(-g))) * (h @ up_w.T) @ w2.T) / s
    x = _layernorm(x, take(D))
    w0, b0, lw, lb, w3, b3 = take(D, D), take(D), take(D), take(D), take(V, D), take(V)
    assert o == blob.size
    u = x @ w0.T + b0
    logits = _layernorm(0.5 * u * (1.0 + _erf(u / sqrt(2.0))), lw, lb) @ w3.T + b3
    logits -= logits.max(-1, keepdims=True)
    return logits - np.log(np.exp(logits).sum(-1, keepdims=True))
