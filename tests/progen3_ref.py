"""Plain NumPy restatement of the ProGen3 forward (proteingym/baselines/progen3/progen3/modeling.py, model/attention.py, model/moe.py)
from an eager-layout state dict, and of its expert block alone as pgmi_op_moe computes it; the inputs and case lists of
tests/test_gpu_progen3.py.  Every function computes in `dtype`: float64 is the reference.  Pinned against the live reference's own
layers (1e-12, tests/test_progen3_host.py, when the reference tree is present) and always against the recorded goldens."""
import numpy as np

GAP = 1e-3                      # the router-gap condition of the fixtures and the op cases: p[k-th] - p[(k+1)-th] >= GAP in every row


def softmax(s):
    p = np.exp(s - s.max(-1, keepdims=True))
    return p / p.sum(-1, keepdims=True)


def log_softmax(s):
    z = s - s.max(-1, keepdims=True)
    return z - np.log(np.exp(z).sum(-1, keepdims=True))


def rmsnorm(x, w, eps):
    return x * (1.0 / np.sqrt((x * x).mean(-1, keepdims=True) + eps)) * w


def silu(x):
    return x / (1.0 + np.exp(-x))


def rotary_tables(T, dh, theta):
    """attention.py RotaryPositionalEmbedding: inv_freq and the angles in fp32, cos / sin of cat(angles, angles) [T, dh]."""
    inv = (np.float32(theta) ** -(np.arange(0, dh, 2, dtype=np.float32) / np.float32(dh))).astype(np.float32)
    ang = np.outer(np.arange(T, dtype=np.float32), inv).astype(np.float32)
    ang = np.concatenate([ang, ang], axis=1)
    return np.cos(ang), np.sin(ang)


def rotate_half(x):
    h = x.shape[-1] // 2
    return np.concatenate([-x[..., h:], x[..., :h]], axis=-1)


def route(h, gate, top_k):
    """(probabilities [M,E], chosen experts [M,k] best first with ties to the lower index, weights [M,k] divided by their sum)."""
    p = softmax(h @ gate.T)
    ids = np.argsort(-p, axis=-1, kind="stable")[:, :top_k]
    w = np.take_along_axis(p, ids, axis=-1)
    return p, ids, w / w.sum(-1, keepdims=True)


def router_gap(p, top_k):
    """The smallest p[k-th largest] - p[(k+1)-th largest] over the rows (inf when every expert is chosen)."""
    if top_k >= p.shape[-1]:
        return np.inf
    s = -np.sort(-p, axis=-1)
    return float((s[:, top_k - 1] - s[:, top_k]).min())


def expert(h, w1, w3, w2, gated):
    a = silu(h @ w1.T)
    return (a * (h @ w3.T) if gated else a) @ w2.T


def moe_block(h, gate, w1, w3, w2, top_k, gated, dtype=np.float64):
    """model/moe.py SparseMoeBlock on rows h [M,D]: gate [E,D] (unused for one expert), w1 / w3 [E,F,D], w2 [E,D,F].
    Returns (out [M,D], probabilities, ids, weights)."""
    h = np.asarray(h).astype(dtype)
    w1, w2 = np.asarray(w1).astype(dtype), np.asarray(w2).astype(dtype)
    w3 = np.asarray(w3).astype(dtype) if gated else [None] * len(w1)
    E = w1.shape[0]
    if E == 1:
        return expert(h, w1[0], w3[0], w2[0], gated), None, None, None
    p, ids, w = route(h, np.asarray(gate).astype(dtype), top_k)
    out = np.zeros_like(h)
    for e in range(E):
        rows, kk = np.nonzero(ids == e)
        if rows.size:
            out[rows] += expert(h[rows], w1[e], w3[e], w2[e], gated) * w[rows, kk, None]
    return out, p, ids, w


def attention(h, wq, wk, wv, wo, H, KV, cos, sin):
    """model/attention.py Attention.forward on one sequence h [T,D]: projections, rotate-half rotary with the tables cos / sin [T, dh],
    repeat_kv, causal softmax attention scaled by dh^-1/2, o_proj."""
    T, D = h.shape
    dh = D // H
    q = (h @ wq.T).reshape(T, H, dh)
    kk = (h @ wk.T).reshape(T, KV, dh)
    v = (h @ wv.T).reshape(T, KV, dh)
    q = q * cos[:, None] + rotate_half(q) * sin[:, None]
    kk = kk * cos[:, None] + rotate_half(kk) * sin[:, None]
    kk, v = np.repeat(kk, H // KV, axis=1), np.repeat(v, H // KV, axis=1)          # repeat_kv: query head h reads head h // (H / KV)
    s = np.einsum("thd,shd->hts", q, kk) * h.dtype.type(dh) ** -0.5
    s = np.where(np.triu(np.ones((T, T), dtype=bool), 1)[None], -np.inf, s)
    return np.einsum("hts,shd->thd", softmax(s), v).reshape(T, D) @ wo.T


def forward(sd, cfg, ids, dtype=np.float64, tables=None):
    """One unpadded sequence ids [T] through the model of the eager-layout state dict `sd` (numpy arrays) and the dims `cfg`
    (proteingym_amd.progen3.config_from_json's dict).  Returns (log_softmax(logits) [T,V], per layer: (router probabilities [T,E],
    chosen experts [T,k]) -- empty for one expert).  tables: (cos, sin) [T, dh] to use instead of rotary_tables' own."""
    g = lambda k: np.asarray(sd[k]).astype(dtype)
    T, D, H, KV, E, k = len(ids), cfg["embed_dim"], cfg["heads"], cfg["kv_heads"], cfg["n_experts"], cfg["top_k"]
    dh = D // H
    cos, sin = (np.asarray(t).astype(dtype) for t in (tables or rotary_tables(T, dh, cfg["rope_theta"])))
    x = g("model.embed_tokens.weight")[np.asarray(ids)] + g("model.embed_seq_id.weight")[0]
    routers = []
    for i in range(cfg["layers"]):
        p = f"model.layers.{i}."
        a = p + ("norm_attn_norm." if cfg.get("fused_attention_norm") else "")
        h = rmsnorm(x, g(a + "input_layernorm.weight"), cfg["ln_eps"])
        x = x + attention(h, *(g(a + f"self_attn.{n}_proj.weight") for n in "qkvo"), H, KV, cos, sin)
        h = rmsnorm(x, g(a + "post_attention_layernorm.weight"), cfg["ln_eps"])
        m = p + "block_sparse_moe."
        w1 = np.stack([g(m + f"experts.{e}.w1.weight") for e in range(E)])
        w3 = np.stack([g(m + f"experts.{e}.w3.weight") for e in range(E)]) if cfg["gated"] else None
        w2 = np.stack([g(m + f"experts.{e}.w2.weight") for e in range(E)])
        out, pr, chosen, _ = moe_block(h, g(m + "gate.weight") if E > 1 else None, w1, w3, w2, k, cfg["gated"], dtype)
        if E > 1:
            routers.append((pr, chosen))
        x = x + out
    x = rmsnorm(x, g("model.norm.weight"), cfg["ln_eps"])
    return log_softmax(x @ g("lm_head.weight").T), routers


def pass_mean(lp, ids):
    """scorer.py _log_likelihoods for one unpadded row: the mean over the T - 1 targets of log p(ids[t+1] | ids[<=t])."""
    ids = np.asarray(ids)
    return lp[np.arange(len(ids) - 1), ids[1:]].mean()


# ---- op cases (tests/test_gpu_progen3.py) ---------------------------------------------------------------------------------------------
D_OP, F_OP = 128, 192
OP_CASES = [(M, E, k, gated, None) for M in (1, 33, 200) for (E, k) in ((4, 2), (8, 2), (2, 2), (1, 1)) for gated in (1, 0)]
OP_CASES += [(200, 4, 2, 1, "empty_expert"), (200, 8, 2, 1, "same_pair")]


def moe_inputs(M, E, k, gated, special=None, D=D_OP, F=F_OP):
    """fp32 (h, gate, w1, w3, w2) of an expert block whose float64 router probabilities keep the k-th and the (k+1)-th expert at least
    GAP apart in every row: seeds are tried until they do.  special "empty_expert": column 0 of every row is 1 and expert 1's gate
    weighs it by -50, so no row picks expert 1; "same_pair": experts 2 and 5 weigh it by 8 and 7, so every row picks (2, 5)."""
    for attempt in range(1000):
        rng = np.random.default_rng(1000003 * M + 1009 * E + 17 * k + gated + 7919 * attempt)
        h = rng.standard_normal((M, D)).astype(np.float32)
        gate = (rng.standard_normal((E, D)) * 1.5 / np.sqrt(D)).astype(np.float32)
        if special:
            h[:, 0] = 1.0
            gate[:, 0] = 0.0
            if special == "empty_expert":
                gate[1, 0] = -50.0
            else:
                gate[2, 0], gate[5, 0] = 8.0, 7.0
        w1 = (rng.standard_normal((E, F, D)) / np.sqrt(D)).astype(np.float32)
        w3 = (rng.standard_normal((E, F, D)) / np.sqrt(D)).astype(np.float32)
        w2 = (rng.standard_normal((E, D, F)) / np.sqrt(F)).astype(np.float32)
        if E == 1 or router_gap(softmax(h.astype(np.float64) @ gate.astype(np.float64).T), k) >= GAP:
            return h, gate, w1, w3, w2
    raise RuntimeError("no seed satisfies the router-gap condition")
