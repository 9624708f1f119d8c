"""TEST INFRASTRUCTURE ONLY -- ProteinMPNN restated from the model's definition in torch on the CPU, in float64 (the yardstick of
tests/test_gpu_mpnn.py) or float32 (what "fp32 torch" deviates from float64 by, which sizes the GPU bounds).  Pinned to the unmodified
reference forward by tests/test_mpnn_host.py.  The decoding order comes in as ``rank`` (or ``randn``), never from a generator.

Neighbour ties: ascending distance, then ascending index (a stable sort) -- the rule of include/pgmi.h.

``factorised_log_probs`` is the numpy model of what the HIP path computes: the first decoder Linear split by input block and hoisted
(DESIGN.md 4.6h), W3 applied after the sum over the edges.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

PAIRS = [(1, 1), (0, 0), (2, 2), (3, 3), (4, 4), (1, 0), (1, 2), (1, 3), (1, 4), (0, 2), (0, 3), (0, 4), (4, 2), (4, 3), (3, 2), (0, 1),
         (2, 1), (3, 1), (4, 1), (2, 0), (3, 0), (4, 0), (2, 4), (3, 4), (2, 3)]       # (atom of i, atom of j): N CA C O CB


def _t(sd, dtype, device="cpu"):
    return {k: torch.as_tensor(np.asarray(v), dtype=dtype, device=device) for k, v in sd.items()}


def _as(a, dtype, w):
    """a (array or tensor) as a tensor of ``dtype`` on the device of the weights ``w``"""
    dev = w["W_e.weight"].device
    return a.to(dtype=dtype, device=dev) if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a), dtype=dtype, device=dev)


def _lin(w, name, x):
    return F.linear(x, w[f"{name}.weight"], w.get(f"{name}.bias"))


def _norm(w, name, x):
    return F.layer_norm(x, (x.shape[-1],), w[f"{name}.weight"], w[f"{name}.bias"], 1e-5)


def _gelu(x):
    return x * 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))


def _gather(nodes, E_idx):
    """nodes [L, C] (or [B, L, C]) at E_idx [L, K] -> [.., L, K, C]"""
    return nodes[..., E_idx, :]


def features(w, X, mask, residue_idx, chain, num_edges):
    """E [L, K, 128] after norm_edges, E_idx [L, K]"""
    dtype = w["W_e.weight"].dtype
    X, mask = _as(X, dtype, w), _as(mask, dtype, w)
    ridx, chain = _as(residue_idx, torch.long, w), _as(chain, torch.long, w)
    L = X.shape[0]
    b = X[:, 1] - X[:, 0]
    c = X[:, 2] - X[:, 1]
    a = torch.cross(b, c, dim=-1)
    Cb = -0.58273431 * a + 0.56802827 * b - 0.54067466 * c + X[:, 1]
    atoms = [X[:, 0], X[:, 1], X[:, 2], X[:, 3], Cb]
    m2 = mask[:, None] * mask[None, :]
    dX = atoms[1][None, :, :] - atoms[1][:, None, :]
    D = m2 * torch.sqrt((dX ** 2).sum(-1) + 1e-6)
    D_adj = D + (1.0 - m2) * D.max(-1, keepdim=True)[0]
    K = min(num_edges, L)
    D_sorted, order = torch.sort(D_adj, dim=-1, stable=True)
    E_idx, D_nb = order[:, :K], D_sorted[:, :K]
    mu = torch.linspace(2.0, 22.0, 16, dtype=dtype, device=X.device)

    def rbf(Dm):
        return torch.exp(-(((Dm[..., None] - mu) / 1.25) ** 2))

    blocks = [rbf(D_nb)]
    for pa, pb in PAIRS[1:]:
        Dab = torch.sqrt(((atoms[pa][:, None, :] - atoms[pb][None, :, :]) ** 2).sum(-1) + 1e-6)
        blocks.append(rbf(torch.gather(Dab, 1, E_idx)))
    offset = torch.gather(ridx[:, None] - ridx[None, :], 1, E_idx)
    same = torch.gather((chain[:, None] == chain[None, :]).long(), 1, E_idx)
    d = torch.clip(offset + 32, 0, 64) * same + (1 - same) * 65
    pos = _lin(w, "features.embeddings.linear", F.one_hot(d, 66).to(dtype))
    E = torch.cat([pos] + blocks, -1)
    E = F.linear(E, w["features.edge_embedding.weight"])
    return _norm(w, "features.norm_edges", E), E_idx


def _mlp(w, p, names, x):
    return _lin(w, f"{p}.{names[2]}", _gelu(_lin(w, f"{p}.{names[1]}", _gelu(_lin(w, f"{p}.{names[0]}", x)))))


def _ffn(w, p, x):
    return _lin(w, f"{p}.dense.W_out", _gelu(_lin(w, f"{p}.dense.W_in", x)))


def encoder(w, E, E_idx, mask, n_layers=3):
    dtype = E.dtype
    mask = _as(mask, dtype, w)
    L, K, H = E.shape
    h_V = torch.zeros(L, H, dtype=dtype, device=E.device)
    h_E = _lin(w, "W_e", E)
    attend = mask[:, None] * mask[E_idx]
    for i in range(n_layers):
        p = f"encoder_layers.{i}"
        x = torch.cat([h_V[:, None, :].expand(-1, K, -1), h_E, _gather(h_V, E_idx)], -1)
        dh = (attend[..., None] * _mlp(w, p, ("W1", "W2", "W3"), x)).sum(-2) / 30.0
        h_V = _norm(w, f"{p}.norm1", h_V + dh)
        h_V = mask[:, None] * _norm(w, f"{p}.norm2", h_V + _ffn(w, p, h_V))
        x = torch.cat([h_V[:, None, :].expand(-1, K, -1), h_E, _gather(h_V, E_idx)], -1)
        h_E = _norm(w, f"{p}.norm3", h_E + _mlp(w, p, ("W11", "W12", "W13"), x))
    return h_V, h_E


def decoder(w, h_V, h_E, E_idx, mask, S, rank, n_layers=3):
    """log-probabilities [B, L, 21]; S, rank integer [B, L]"""
    dtype = h_V.dtype
    mask, S, rank = _as(mask, dtype, w), _as(S, torch.long, w), _as(rank, torch.long, w)
    B, L = S.shape
    K = E_idx.shape[1]
    h_S = w["W_s.weight"][S]                                             # [B, L, H]
    bw = (mask[None, :, None] * (rank[:, :, None] > rank[:, E_idx]).to(dtype))[..., None]     # [B, L, K, 1]
    fw = mask[None, :, None, None] * (1.0 - bw)
    hE = h_E[None].expand(B, -1, -1, -1)
    enc_part = fw * torch.cat([hE, torch.zeros_like(hE), _gather(h_V, E_idx)[None].expand(B, -1, -1, -1)], -1)
    hv = h_V[None].expand(B, -1, -1)
    for i in range(n_layers):
        p = f"decoder_layers.{i}"
        esv = bw * torch.cat([hE, h_S[:, E_idx, :], hv[:, E_idx, :]], -1) + enc_part
        x = torch.cat([hv[:, :, None, :].expand(-1, -1, K, -1), esv], -1)
        dh = _mlp(w, p, ("W1", "W2", "W3"), x).sum(-2) / 30.0
        hv = _norm(w, f"{p}.norm1", hv + dh)
        hv = mask[None, :, None] * _norm(w, f"{p}.norm2", hv + _ffn(w, p, hv))
    return F.log_softmax(_lin(w, "W_out", hv), -1)


def forward(sd, num_edges, X, mask, residue_idx, chain, S, rank, dtype=torch.float64):
    """dict of numpy arrays: E_idx, E, h_V, h_E, log_probs [B, L, 21], scores [B]"""
    w = _t(sd, dtype)
    with torch.no_grad():
        E, E_idx = features(w, X, mask, residue_idx, chain, num_edges)
        h_V, h_E = encoder(w, E, E_idx, mask)
        lp = decoder(w, h_V, h_E, E_idx, mask, S, rank)
    out = dict(E_idx=E_idx.numpy(), E=E.numpy(), h_V=h_V.numpy(), h_E=h_E.numpy(), log_probs=lp.numpy())
    out["scores"] = scores(out["log_probs"], S, mask)
    return out


def scores(log_probs, S, mask):
    """pmpnn_ll [B] = -(sum_i mask_i (-log p_i[S_i])) / sum_i mask_i, float64"""
    lp = np.asarray(log_probs, dtype=np.float64)
    S = np.asarray(S, dtype=np.int64)
    mask = np.asarray(mask, dtype=np.float64)
    nll = -np.take_along_axis(lp, S[..., None], -1)[..., 0]
    return -(nll * mask).sum(-1) / mask.sum()


def rank_from_randn(randn, mask, chain_M=None, chain_M_pos=None):
    """the reference's line, in torch fp32: rank = inverse of argsort((chain_M chain_M_pos mask + 1e-4) |randn|)"""
    cm = torch.as_tensor(np.asarray(mask), dtype=torch.float32)
    if chain_M is not None:
        cm = torch.as_tensor(np.asarray(chain_M), dtype=torch.float32) * cm
    if chain_M_pos is not None:
        cm = torch.as_tensor(np.asarray(chain_M_pos), dtype=torch.float32) * cm
    r = torch.as_tensor(np.atleast_2d(np.asarray(randn)), dtype=torch.float32)
    order = torch.argsort((cm + 0.0001) * torch.abs(r))
    return torch.argsort(order).numpy().astype(np.int32)


def factorised_log_probs(sd, h_V, h_E, E_idx, mask, S, rank, n_layers=3):
    """numpy float64 model of the HIP decoder: pre = A_i + mask_i (E'_ik + (bw ? T[S_j] + P_j : Penc_j)), GELU, W2, GELU, sum over k,
    then W3 on the sum + K b3."""
    w = {k: np.asarray(v, dtype=np.float64) for k, v in sd.items()}
    h_V, h_E, mask = (np.asarray(a, dtype=np.float64) for a in (h_V, h_E, mask))
    S, rank, E_idx = np.asarray(S), np.asarray(rank), np.asarray(E_idx)
    B, L = S.shape
    K, H = E_idx.shape[1], h_V.shape[1]
    def gelu(x):
        return x * 0.5 * (1.0 + torch.erf(torch.from_numpy(np.ascontiguousarray(x / math.sqrt(2.0)))).numpy())

    def ln(x, name):
        mu = x.mean(-1, keepdims=True)
        var = ((x - mu) ** 2).mean(-1, keepdims=True)
        return (x - mu) / np.sqrt(var + 1e-5) * w[f"{name}.weight"] + w[f"{name}.bias"]

    bw = (mask[None, :, None] != 0) & (rank[:, :, None] > rank[:, E_idx])           # [B, L, K]
    hv = np.broadcast_to(h_V, (B, L, H))
    for i in range(n_layers):
        p = f"decoder_layers.{i}"
        W1 = w[f"{p}.W1.weight"]
        W1a, W1b, W1c, W1d = W1[:, :H], W1[:, H:2 * H], W1[:, 2 * H:3 * H], W1[:, 3 * H:]
        Ep = h_E @ W1b.T                                    # [L, K, H]
        T = w["W_s.weight"] @ W1c.T                         # [21, H]
        Penc = h_V @ W1d.T                                  # [L, H]
        A = hv @ W1a.T + w[f"{p}.W1.bias"]                  # [B, L, H]
        P = hv @ W1d.T
        seq = T[S][:, E_idx, :] + P[:, E_idx, :]            # [B, L, K, H]
        pre = A[:, :, None, :] + mask[None, :, None, None] * (Ep[None] + np.where(bw[..., None], seq, Penc[E_idx][None]))
        n = gelu(gelu(pre) @ w[f"{p}.W2.weight"].T + w[f"{p}.W2.bias"]).sum(-2)
        dh = (n @ w[f"{p}.W3.weight"].T + K * w[f"{p}.W3.bias"]) / 30.0
        hv = ln(hv + dh, f"{p}.norm1")
        ff = gelu(hv @ w[f"{p}.dense.W_in.weight"].T + w[f"{p}.dense.W_in.bias"]) @ w[f"{p}.dense.W_out.weight"].T + w[f"{p}.dense.W_out.bias"]
        hv = mask[None, :, None] * ln(hv + ff, f"{p}.norm2")
    logits = hv @ w["W_out.weight"].T + w["W_out.bias"]
    logits = logits - logits.max(-1, keepdims=True)
    return logits - np.log(np.exp(logits).sum(-1, keepdims=True))
