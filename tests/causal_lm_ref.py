"""Float64 NumPy forward of the causal decoder (RITA / GPT-2) over the packed blob of proteingym_amd.causal_lm.pack: an independent
reading of the blob layout, the GPT-2 Conv1D transposes and RITA's rotate-half rotary (rita_modeling.py:36-62).  Shared by
test_causal_lm_host.py and test_gpu_causal_lm.py."""
import numpy as np


def _layernorm(x, w, b, eps):
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * w + b


def numpy_forward(cfg, blob, ids, dtype=np.float64):
    """log_softmax(logits) [T, V] for one row of ids, computed in `dtype`: float64 is the reference; float32 is the same forward in plain
    fp32, whose distance from the float64 one (noise32) sizes the tolerance of long contexts."""
    D, F, V, H, L, P = cfg["embed_dim"], cfg["ffn_dim"], cfg["vocab"], cfg["heads"], cfg["layers"], cfg["max_positions"]
    dh, eps, rita = D // H, cfg["ln_eps"], cfg["family"] == "rita"
    w = blob.astype(dtype)
    o = 0

    def take(*shape):
        nonlocal o
        n = int(np.prod(shape))
        a = w[o:o + n].reshape(shape)
        o += n
        return a
    ids = np.asarray(ids)
    T = len(ids)
    wte = take(V, D)
    x = wte[ids]
    if not rita:
        x = x + take(P, D)[:T]
    inv = (1.0 / (10000 ** (np.arange(0, dh, 2, dtype=np.float32) / np.float32(dh)))).astype(np.float32)
    ang = (np.arange(T, dtype=np.float32)[:, None] * inv[None, :]).astype(dtype)    # fp32 angle, as the reference
    cos, sin = np.concatenate([np.cos(ang)] * 2, -1)[:, None, :], np.concatenate([np.sin(ang)] * 2, -1)[:, None, :]

    def rot(t):
        return t * cos + np.concatenate([-t[..., dh // 2:], t[..., :dh // 2]], -1) * sin
    mask = np.tril(np.ones((T, T), bool))
    for _ in range(L):
        ln1_w, ln1_b = take(D), take(D)
        (wq, bq), (wk, bk), (wv, bv) = ((take(D, D), take(D)) for _ in range(3))
        wo, bo = take(D, D), take(D)
        ln2_w, ln2_b = take(D), take(D)
        w1, b1, w2, b2 = take(F, D), take(F), take(D, F), take(D)
        h = _layernorm(x, ln1_w, ln1_b, eps)
        q, k, v = ((h @ W.T + b).reshape(T, H, dh) for W, b in ((wq, bq), (wk, bk), (wv, bv)))
        if rita:
            q, k = rot(q), rot(k)
        s = np.einsum("thd,shd->hts", q, k) / float(np.sqrt(dh))
        s = np.where(mask[None], s, dtype(-np.inf))
        p = np.exp(s - s.max(-1, keepdims=True))
        p /= p.sum(-1, keepdims=True)
        x = x + np.einsum("hts,shd->thd", p, v).reshape(T, D) @ wo.T + bo
        u = _layernorm(x, ln2_w, ln2_b, eps) @ w1.T + b1
        g = 0.5 * u * (1.0 + np.tanh(float(np.sqrt(2.0 / np.pi)) * (u + 0.044715 * u ** 3)))
        x = x + g @ w2.T + b2
    lnf_w, lnf_b = take(D), take(D)
    head = take(V, D) if rita else wte
    assert o == w.size
    logits = _layernorm(x, lnf_w, lnf_b, eps) @ head.T
    logits -= logits.max(-1, keepdims=True)
    return logits - np.log(np.exp(logits).sum(-1, keepdims=True))
