"""A torch restatement of S2F's inference (proteingym/baselines/S3F: s3f/gvp_layer.py GVP, GVPLayerNorm, GVPConv, GVPConvLayer;
s3f/gvp.py GVPGNN.forward and rbf; s3f/model.py MyESM / FusionNetwork; s3f/task.py inference; script/evaluate.py get_prob), written
from those files and independent of proteingym_amd/s2f.py.  Every function takes the dtype of its tensors: float64 is the reference
of the GPU tests, float32 measures how far fp32 torch is from it.  The state dict uses the task's own key names."""
import math

import numpy as np
import torch

ORDER = "GASPVTCILNDQKEMHFRYW"                      # torchdrug residue ids
ESM_TOKENS = ("<cls>", "<pad>", "<eos>", "<unk>", "L", "A", "G", "V", "S", "E", "R", "T", "I", "D", "P", "K", "Q", "N", "F", "Y", "M", "H",
              "W", "C", "X", "B", "U", "Z", "O", ".", "-", "<null_1>", "<mask>")
SM = "model.structure_model."
QM = "model.sequence_model.model."


def tensors(sd, dtype, device="cpu"):
    return {k: torch.as_tensor(np.array(v)).to(device=device, dtype=dtype) for k, v in sd.items() if np.asarray(v).dtype.kind == "f"}


def radius_edges(pos, r=10.0, cap=32):
    """Edges (j -> i): for centre i, walk j upwards, keep those with |p_i - p_j|^2 < r^2 (i itself counts) until cap + 1 are kept, then
    forget i.  Returns int64 [2, E] = (j row, i row)."""
    p = [[float(c) for c in row] for row in np.asarray(pos, dtype=np.float64)]
    js, is_ = [], []
    for i, a in enumerate(p):
        taken = 0
        for j, b in enumerate(p):
            if taken == cap + 1:
                break
            if (a[0] - b[0]) ** 2 + (a[1] - b[1]) ** 2 + (a[2] - b[2]) ** 2 < r * r:
                taken += 1
                if j != i:
                    js.append(j)
                    is_.append(i)
    return torch.tensor([js, is_], dtype=torch.int64).reshape(2, -1)


def norm_no_nan(x, dim, keepdim=False, sqrt=True):
    out = torch.clamp((x * x).sum(dim, keepdim), min=1e-8)
    return out.sqrt() if sqrt else out


def gvp(W, p, s, v, relu, vo):
    """GVP with vector gate and activations (relu or None, None).  v None: no vector input (zeros out when vo > 0)."""
    if v is None:
        s = s @ W[p + "ws.weight"].T + W[p + "ws.bias"]
        v_out = s.new_zeros(s.shape[0], vo, 3) if vo else None
    else:
        vt = v.transpose(-1, -2)                                    # [n, 3, vi]
        vh = vt @ W[p + "wh.weight"].T                              # [n, 3, h]
        vn = norm_no_nan(vh, -2)                                    # [n, h]
        s = torch.cat([s, vn], -1) @ W[p + "ws.weight"].T + W[p + "ws.bias"]
        v_out = None
        if vo:
            v_out = (vh @ W[p + "wv.weight"].T).transpose(-1, -2)   # [n, vo, 3]
            gate = s @ W[p + "wsv.weight"].T + W[p + "wsv.bias"]    # on s before the scalar activation
            v_out = v_out * torch.sigmoid(gate).unsqueeze(-1)
    if relu:
        s = torch.relu(s)
    return s, v_out


def tuple_ln(W, p, s, v):
    s = torch.nn.functional.layer_norm(s, (s.shape[-1],), W[p + "scalar_norm.weight"], W[p + "scalar_norm.bias"], 1e-5)
    if v is None:
        return s, None
    vn = norm_no_nan(v, -1, keepdim=True, sqrt=False)
    vn = torch.sqrt(vn.mean(-2, keepdim=True))
    return s, v / vn


def rbf(d, dim=16):
    mu = torch.linspace(0.0, 20.0, dim).to(d)                  # the reference builds the centres in the default dtype, float32
    return torch.exp(-((d[:, None] - mu[None, :]) / (20.0 / dim)) ** 2)


def edge_features(W, pos, edges):
    j, i = edges
    vec = pos[i] - pos[j]
    s, v = tuple_ln(W, SM + "W_e.0.", rbf(vec.norm(dim=-1)), vec[:, None, :])
    return gvp(W, SM + "W_e.1.", s, v, False, 1)


def conv_layer(W, p, s, v, edges, es, ev, trace=None):
    j, i = edges
    n = s.shape[0]
    ms, mv = torch.cat([s[j], es, s[i]], -1), torch.cat([v[j], ev, v[i]], -2)
    ms, mv = gvp(W, p + "conv.message_func.0.", ms, mv, True, 16)
    ms, mv = gvp(W, p + "conv.message_func.1.", ms, mv, True, 16)
    ms, mv = gvp(W, p + "conv.message_func.2.", ms, mv, False, 16)
    cnt = s.new_zeros(n).index_add_(0, i, s.new_ones(len(i))).clamp(min=1)
    ds = torch.zeros_like(s).index_add_(0, i, ms) / cnt[:, None]
    dv = torch.zeros_like(v).index_add_(0, i, mv) / cnt[:, None, None]
    if trace is not None:
        trace["msg_s"], trace["msg_v"] = ds, dv
    s, v = tuple_ln(W, p + "norm.0.", s + ds, v + dv)
    fs, fv = gvp(W, p + "ff_func.0.", s, v, True, 32)
    fs, fv = gvp(W, p + "ff_func.1.", fs, fv, False, 16)
    return tuple_ln(W, p + "norm.1.", s + fs, v + fv)


def structure_graph(W, pos, like, r=10.0, cap=32):
    """What depends on the structure only: (edges, e_s, e_v), on the device and in the dtype of `like`."""
    edges = radius_edges(pos, r, cap).to(like.device)
    es, ev = edge_features(W, torch.as_tensor(np.array(pos)).to(like), edges)
    return edges, es, ev


def gvp_gnn(W, pos, x, layers=5, r=10.0, cap=32, graph=None):
    """GVPGNN.forward on one graph: x [L, D] -> dict(edges, e_s, e_v, node_s, node_v (after the last layer), out [L, 256]).
    graph: a structure_graph() result to reuse instead of building it from pos."""
    edges, es, ev = structure_graph(W, pos, x, r, cap) if graph is None else graph
    h = x @ W[SM + "residue_embdding.weight"].T
    s, _ = tuple_ln(W, SM + "W_v.0.", h, None)
    s, v = gvp(W, SM + "W_v.1.", s, None, False, 16)
    for l in range(layers):
        s, v = conv_layer(W, f"{SM}layers.{l}.", s, v, edges, es, ev)
    os_, ov = tuple_ln(W, SM + "W_out.0.", s, v)
    out, _ = gvp(W, SM + "W_out.1.", os_, ov, True, 0)
    return dict(edges=edges, e_s=es, e_v=ev, node_s=s, node_v=v, out=out)


def head_logprobs(W, out, seq_logits, plddt, threshold=70.0):
    """task.inference + get_prob's log_softmax: [L, 20]."""
    pred = out @ W["linear.weight"].T + W["linear.bias"]
    if threshold:
        low = torch.as_tensor(np.asarray(plddt, dtype=np.float64) < threshold).to(out.device)
        pred = torch.where(low[:, None], seq_logits, pred)
    return torch.log_softmax(pred, -1)


def gvp_forward(sd, pos, plddt, x, seq_logits, dtype=torch.float64, layers=5, threshold=70.0):
    """Batch [B, L, D] / [B, L, 20] -> (lp [B, L, 20], node_s [B, L, 256], node_v [B, L, 16, 3]) as numpy."""
    W = tensors(sd, dtype)
    lps, ss, vs = [], [], []
    for xb, qb in zip(torch.as_tensor(np.asarray(x)).to(dtype), torch.as_tensor(np.asarray(seq_logits)).to(dtype)):
        g = gvp_gnn(W, pos, xb, layers)
        lps.append(head_logprobs(W, g["out"], qb, plddt, threshold))
        ss.append(g["node_s"])
        vs.append(g["node_v"])
    return torch.stack(lps).numpy(), torch.stack(ss).numpy(), torch.stack(vs).numpy()


# -- ESM2 (fair-esm esm2.py / modules.py / multihead_attention.py / rotary_embedding.py) -----------------------------------------
def esm2(W, tokens, heads, layers):
    """tokens int64 [T] (no padding) -> (representations[layers] [T, D], logits [T, 33]).  Token dropout as in training-free inference:
    <mask> rows zeroed, the rest scaled by (1 - 0.12) / (1 - masked fraction)."""
    emb = W[QM + "embed_tokens.weight"]
    tok = torch.as_tensor(np.asarray(tokens), dtype=torch.int64).to(emb.device)
    T = len(tok)
    dtype = emb.dtype
    D = emb.shape[1]
    dh = D // heads
    is_mask = tok == ESM_TOKENS.index("<mask>")
    x = emb[tok].masked_fill(is_mask[:, None], 0.0)
    x = x * (1 - 0.15 * 0.8) / (1 - is_mask.sum().to(dtype) / T)
    inv = 1.0 / (10000 ** (torch.arange(0, dh, 2).float() / dh))          # rotary_embedding.py: the tables are built in float32
    ang = torch.arange(T).float()[:, None] * inv[None, :]
    ang = torch.cat([ang, ang], -1)
    cos, sin = ang.cos().to(emb), ang.sin().to(emb)

    def rot(t):
        a, b = t.chunk(2, -1)
        return t * cos + torch.cat([-b, a], -1) * sin

    def ln(t, p):
        return torch.nn.functional.layer_norm(t, (D,), W[QM + p + ".weight"], W[QM + p + ".bias"], 1e-5)

    def lin(t, p):
        return t @ W[QM + p + ".weight"].T + W[QM + p + ".bias"]

    def gelu(t):
        return t * 0.5 * (1.0 + torch.erf(t / math.sqrt(2.0)))

    for l in range(layers):
        p = f"layers.{l}."
        h = ln(x, p + "self_attn_layer_norm")
        q = (lin(h, p + "self_attn.q_proj") * dh ** -0.5).view(T, heads, dh).transpose(0, 1)
        k = lin(h, p + "self_attn.k_proj").view(T, heads, dh).transpose(0, 1)
        v = lin(h, p + "self_attn.v_proj").view(T, heads, dh).transpose(0, 1)
        a = torch.softmax(rot(q) @ rot(k).transpose(-1, -2), -1)
        x = x + lin((a @ v).transpose(0, 1).reshape(T, D), p + "self_attn.out_proj")
        x = x + lin(gelu(lin(ln(x, p + "final_layer_norm"), p + "fc1")), p + "fc2")
    rep = ln(x, "emb_layer_norm_after")
    h = ln(gelu(lin(rep, "lm_head.dense")), "lm_head.layer_norm")
    return rep, h @ emb.T + W[QM + "lm_head.bias"]


def set_tables(sd, seq, pos, plddt, sets, heads, esm_layers, dtype=torch.float64, layers=5, threshold=70.0, device="cpu", W=None,
               graph=None):
    """For each set of 0-based residue indices: the [L, 20] log-probability table of FusionNetwork on the sequence with the set's
    residues at <mask>.  Also returns the ESM-only tables (log_softmax of the 20 mapped logit columns)."""
    W = tensors(sd, dtype, device) if W is None else W
    base = [0] + [ESM_TOKENS.index(a) for a in seq] + [2]
    cols = [ESM_TOKENS.index(a) for a in ORDER]
    full, esm_only = [], []
    for st in sets:
        tok = list(base)
        for i in st:
            tok[1 + i] = ESM_TOKENS.index("<mask>")
        rep, logits = esm2(W, tok, heads, esm_layers)
        q = logits[1:-1][:, cols]
        g = gvp_gnn(W, pos, rep[1:-1], layers, graph=graph)
        full.append(head_logprobs(W, g["out"], q, plddt, threshold))
        esm_only.append(torch.log_softmax(q, -1))
    return torch.stack(full).cpu().numpy(), torch.stack(esm_only).cpu().numpy()


def scores(rows, tables, set_of):
    """get_prob: rows [(sites, sub-mutations, target)], set_of[n] = index of the row's table."""
    out = []
    for (sites, muts, _), s in zip(rows, set_of):
        lp = tables[s]
        out.append(sum(float(lp[i, ORDER.index(m[-1])]) - float(lp[i, ORDER.index(m[0])]) for i, m in zip(sites, muts)))
    return np.array(out)
