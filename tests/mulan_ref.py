"""Float64 NumPy forward of MULAN (StructEsmForMaskedLM) over the packed blob of proteingym_amd.mulan.pack, written from the reference's
formulae (mulan/model_utils.py:59-97,141-188, dataset.py:306-314, compute_fitness.py:27-126) and sharing no code with the package:
the collate rule of the angle rows, the structure adapter (Linear(7 -> D), one ESM layer without rotary, LayerNorm), the embedding
sum before token dropout, ESM2's rotary stack and tied head, and both score rules.  Shared by test_mulan_host.py and test_gpu_mulan.py."""
from math import erf, sqrt

import numpy as np

_erf = np.vectorize(erf)
PAD, MASKED, PLDDT_MAX_BAD = 4.0, -4.0, 70.0


def _layernorm(x, w, b, eps=1e-5):
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * w + b


def _gelu(u):
    return 0.5 * u * (1.0 + _erf(u / sqrt(2.0)))


def collate(angles, plddt, masked=()):
    """struct_inputs [T][7] of one forward: rows of pLDDT <= 70 and the two end rows (padded pLDDT 4.0) are 4.0, then -4.0 at `masked`."""
    a = np.array(angles, dtype=np.float64)
    p = np.array(plddt, dtype=np.float64)
    p[0] = p[-1] = PAD
    a[p <= PLDDT_MAX_BAD] = PAD
    a[list(masked)] = MASKED
    return a


class _Blob:
    def __init__(self, blob):
        self.blob, self.o = blob, 0

    def take(self, *shape):
        n = int(np.prod(shape))
        a = self.blob[self.o:self.o + n].astype(np.float64).reshape(shape)
        self.o += n
        return a

    def layer(self, D, F):
        t = self.take
        return dict(ln1=(t(D), t(D)), q=(t(D, D), t(D)), k=(t(D, D), t(D)), v=(t(D, D), t(D)), o=(t(D, D), t(D)), ln2=(t(D), t(D)),
                    fc1=(t(F, D), t(F)), fc2=(t(D, F), t(D)))


def _layer(x, L, H, rot):
    T, D = x.shape
    dh = D // H
    h = _layernorm(x, *L["ln1"])
    q = ((h @ L["q"][0].T + L["q"][1]) * dh ** -0.5).reshape(T, H, dh)
    k = (h @ L["k"][0].T + L["k"][1]).reshape(T, H, dh)
    v = (h @ L["v"][0].T + L["v"][1]).reshape(T, H, dh)
    if rot is not None:
        q, k = rot(q), rot(k)
    sc = np.einsum("thd,shd->hts", q, k)
    p = np.exp(sc - sc.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    x = x + np.einsum("hts,shd->thd", p, v).reshape(T, D) @ L["o"][0].T + L["o"][1]
    return x + _gelu(_layernorm(x, *L["ln2"]) @ L["fc1"][0].T + L["fc1"][1]) @ L["fc2"][0].T + L["fc2"][1]


def numpy_logits(cfg, blob, ids, struct_inputs, adapter_rotary=False):
    """logits [T, V] in float64 for one row of ids and its collated angle rows [T][7] (no padding).  adapter_rotary: the WRONG model
    that rotates q and k inside the adapter as well (tests show the device does not compute it)."""
    D, F, V, H, n_layers = cfg["embed_dim"], cfg["ffn_dim"], cfg["vocab"], cfg["heads"], cfg["layers"]
    mask_id = cfg["mask_token_id"]
    dh = D // H
    b = _Blob(blob)
    ids = np.asarray(ids)
    T = len(ids)
    E = b.take(V, D)
    lnb = (b.take(D), b.take(D)) if cfg["emb_layer_norm_before"] else None
    main = [b.layer(D, F) for _ in range(n_layers)]
    lna = (b.take(D), b.take(D))
    w0, b0, lw, lb, bias = b.take(D, D), b.take(D), b.take(D), b.take(D), b.take(V)
    mlp_w, mlp_b = b.take(D, 7), b.take(D)
    ad = b.layer(D, 4 * D)
    ad_ln = (b.take(D), b.take(D))
    assert b.o == blob.size
    inv = (1.0 / (10000 ** (np.arange(0, dh, 2, dtype=np.float32) / np.float32(dh)))).astype(np.float32)
    ang = (np.arange(T, dtype=np.float32)[:, None] * inv[None, :]).astype(np.float64)
    cos, sin = np.concatenate([np.cos(ang)] * 2, -1)[:, None, :], np.concatenate([np.sin(ang)] * 2, -1)[:, None, :]

    def rot(t):
        return t * cos + np.concatenate([-t[..., dh // 2:], t[..., :dh // 2]], -1) * sin
    struct = _layernorm(_layer(np.asarray(struct_inputs, dtype=np.float64) @ mlp_w.T + mlp_b, ad, H, rot if adapter_rotary else None), *ad_ln)
    x = E[ids] + struct
    if cfg["token_dropout"]:
        x = np.where((ids == mask_id)[:, None], 0.0, x)
        x = x * (1 - 0.15 * 0.8) / (1 - (ids == mask_id).sum() / T)
    if lnb is not None:
        x = _layernorm(x, *lnb)
    for L in main:
        x = _layer(x, L, H, rot)
    x = _layernorm(x, *lna)
    return _layernorm(_gelu(x @ w0.T + b0), lw, lb) @ E.T + bias


def log_softmax(logits):
    logits = logits - logits.max(-1, keepdims=True)
    return logits - np.log(np.exp(logits).sum(-1, keepdims=True))


def masked_forward(cfg, blob, wt_ids, angles, plddt, positions, adapter_rotary=False):
    """log-softmax [T, V] of the forward that masks `positions`: <mask> tokens, -4 angle rows (mask_mutated_positions)."""
    ids = np.array(wt_ids)
    ids[list(positions)] = cfg["mask_token_id"]
    return log_softmax(numpy_logits(cfg, blob, ids, collate(angles, plddt, positions), adapter_rotary))


def group_logprobs(lp, first=5, groups=21, width=21):
    """[.., 446] log-probabilities -> [.., 21]: log of the summed probability of each amino-acid letter's 21 tokens."""
    g = lp[..., first:first + groups * width].reshape(*lp.shape[:-1], groups, width)
    m = g.max(-1, keepdims=True)
    return (m + np.log(np.exp(g - m).sum(-1, keepdims=True)))[..., 0]


def set_table(cfg, blob, wt_ids, angles, plddt, set_off, set_pos):
    """The table pgmi_mulan_set_logprobs returns, in float64: per (set, position) the log-softmax row (plain) or the group row."""
    rows = []
    for s in range(len(set_off) - 1):
        ps = [int(p) for p in set_pos[set_off[s]:set_off[s + 1]]]
        lp = masked_forward(cfg, blob, wt_ids, angles, plddt, ps)
        rows.append(group_logprobs(lp[ps]) if cfg["vocab"] == 446 else lp[ps])
    return np.concatenate(rows)


def scores(cfg, blob, wt_ids, angles, plddt, mutants, range_start, vocabulary):
    """predict_mut (compute_fitness.py:27-77) for mutants given in the assay's numbering: one masked forward per mutant, the sum over
    its sub-mutations of log(p[mt] / p[wt]) -- at the token of the letter (plain; `vocabulary` = the token list) or over the 21 tokens
    that start at letter + 'p' (Foldseek)."""
    out = []
    cache = {}
    for m in mutants:
        subs = [(s[0], int(s[1:-1]) - range_start + 1, s[-1]) for s in m.split(":")]
        key = tuple(sorted({p for _, p, _ in subs}))
        if key not in cache:
            cache[key] = np.exp(masked_forward(cfg, blob, wt_ids, angles, plddt, [p for _, p, _ in subs]))
        probs, score = cache[key], 0.0
        for wt, p, mt in subs:
            if cfg["vocab"] == 446:
                a, c = vocabulary.index(wt + "p"), vocabulary.index(mt + "p")
                score += np.log(probs[p, c:c + 21].sum() / probs[p, a:a + 21].sum())
            else:
                score += np.log(probs[p, vocabulary.index(mt)] / probs[p, vocabulary.index(wt)])
        out.append(score)
    return np.array(out)
