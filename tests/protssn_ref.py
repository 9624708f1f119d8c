"""ProtSSN's EGNN and scoring restated on plain torch ops (float64 by default), for the tests and the benchmark's baseline.

It follows proteingym/baselines/protssn as the reference runs it: per edge the unsplit 2654-wide first Linear on
cat[x_i, x_j, edge_attr, rel_dist], ``index_add_`` over edge_index[1], the node MLP on cat[x, m_i] with the residual.  It shares no code
with proteingym_amd.protssn's packing or device path: it reads the checkpoint's state dict as it is.
"""
import numpy as np
import torch
import torch.nn.functional as F

PREFIX = "GNN_model."
AA = "ARNDCQEGHILKMFPSTWYV"


def tensors(sd, dtype=torch.float64, device="cpu"):
    return {k: torch.as_tensor(np.array(v)).to(device=device, dtype=dtype) for k, v in sd.items()}


def layer_messages(W, n, x, pos, centre, nb, edge_attr):
    """m_ij [E, h] and their sums m_i [L, h] of layer n: x_i = x[edge_index[1]] (the neighbour), x_j = x[edge_index[0]] (the centre)."""
    p = f"{PREFIX}mpnn_layes.{n}."
    rel = pos[centre] - pos[nb]
    d2 = (rel ** 2).sum(-1, keepdim=True)
    inp = torch.cat([x[nb], x[centre], edge_attr, d2], dim=-1)
    m = F.silu(F.linear(F.silu(F.linear(inp, W[p + "edge_mlp.0.weight"], W[p + "edge_mlp.0.bias"])), W[p + "edge_mlp.3.weight"],
                        W[p + "edge_mlp.3.bias"]))
    m_i = torch.zeros(x.shape[0], m.shape[1], dtype=x.dtype, device=x.device).index_add_(0, nb, m)
    return m, m_i


def forward(sd, esm_rep, pos, centre, nb, edge_attr, layers=6, dtype=torch.float64, device="cpu", W=None):
    """(log(softmax(lin(x)) + 1e-9) [L, 20], x after the last layer [L, D]) as tensors of `dtype`."""
    W = W if W is not None else tensors(sd, dtype, device)
    as_t = lambda a: a if torch.is_tensor(a) else torch.as_tensor(np.array(a))
    to = lambda a: as_t(a).to(device=device, dtype=dtype)
    idx = lambda a: as_t(a).to(device=device, dtype=torch.long)
    x, pos, edge_attr, centre, nb = to(esm_rep), to(pos), to(edge_attr), idx(centre), idx(nb)
    for n in range(layers):
        p = f"{PREFIX}mpnn_layes.{n}."
        _, m_i = layer_messages(W, n, x, pos, centre, nb, edge_attr)
        hid = F.silu(F.linear(torch.cat([x, m_i], dim=-1), W[p + "node_mlp.0.weight"], W[p + "node_mlp.0.bias"]))
        x = x + F.linear(hid, W[p + "node_mlp.3.weight"], W[p + "node_mlp.3.bias"])
    out = F.linear(x, W[PREFIX + "lin.weight"], W[PREFIX + "lin.bias"])
    return torch.log(torch.softmax(out[:, :20], dim=1) + 1e-9), x


def message_sums(sd, esm_rep, pos, centre, nb, edge_attr, dtype=torch.float64):
    """m_i [L, h] of layer 0 as a numpy array."""
    W = tensors(sd, dtype)
    to = lambda a: torch.as_tensor(np.array(a)).to(dtype)
    idx = lambda a: torch.as_tensor(np.array(a)).long()
    return layer_messages(W, 0, to(esm_rep), to(pos), idx(centre), idx(nb), to(edge_attr))[1].numpy()


def label_row(rows, sequence, lp, offset=1):
    """compute_fitness.py label_row, restated apart from proteingym_amd.protssn's."""
    total = 0.0
    for row in rows.split(":" if ":" in rows else ";"):
        if row.lower() == "wt":
            continue
        wt, idx, mt = row[0], int(row[1:-1]) - offset, row[-1]
        assert sequence[idx] == wt, f"The {row}, {sequence[idx]}"
        total += float(lp[idx, AA.index(mt)] - lp[idx, AA.index(wt)])
    return total


def slow_graph(ca, k, cutoff=30.0):
    """get_calpha_graph's edge list, one pair at a time: (centre, neighbour, distance) lists."""
    ca = np.asarray(ca, dtype=np.float64)
    L = len(ca)
    dist = np.zeros((L, L))
    for i in range(L):
        for j in range(L):
            dist[i, j] = np.sqrt(((ca[i] - ca[j]) ** 2).sum())
    src, dst, dl = [], [], []
    for i in range(L):
        cand = [j for j in range(L) if dist[i, j] < cutoff and j != i]
        if len(cand) > k:
            cand = [int(j) for j in np.argsort(dist[i])[1:k + 1]]
        if len(cand) == 0:
            cand = [int(np.argsort(dist[i])[1])]
        for j in cand:
            src.append(i)
            dst.append(j)
            dl.append(dist[i, j])
    return src, dst, dl


def slow_edge_attr(src, dst, dl, n, ca, c):
    """The 93 attributes of every edge, one edge at a time, in float64 (the reference rounds to float32 at the end)."""
    n, ca, c = (np.asarray(a, dtype=np.float64) for a in (n, ca, c))
    frames = []
    for i in range(len(ca)):
        u = (n[i] - ca[i]) / np.linalg.norm(n[i] - ca[i])
        t = (c[i] - ca[i]) / np.linalg.norm(c[i] - ca[i])
        nn = np.cross(u, t) / np.linalg.norm(np.cross(u, t))
        frames.append((nn, u, np.cross(nn, u)))
    out = np.zeros((len(src), 93))
    for e, (s, d, dist) in enumerate(zip(src, dst, dl)):
        out[e, min(abs(s - d), 64)] = 1.0
        for x in range(15):
            out[e, 65 + x] = np.exp(-((dist / 4) ** 2) / 1.5 ** x)
        out[e, 80] = 1.0 if dist <= 8 else 0.0
        basis = np.stack(frames[d])
        parts = [basis @ (ca[s] - ca[d])] + [basis @ frames[s][j] for j in range(3)]
        out[e, 81:] = np.concatenate(parts)
    return out


def toy_backbone(ca, seed=0):
    """N and C atoms around given C-alpha positions: bond lengths 1.46 and 1.52, directions seeded and never parallel."""
    rng = np.random.default_rng(seed)
    ca = np.asarray(ca, dtype=np.float64)
    a = rng.standard_normal(ca.shape)
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    b = rng.standard_normal(ca.shape)
    b -= 0.5 * (b * a).sum(1, keepdims=True) * a            # keeps at least half of the component across a
    b /= np.linalg.norm(b, axis=1, keepdims=True)
    return ca + 1.46 * a, ca, ca + 1.52 * b


def serpentine(L, seed=1):
    """The benchmark scripts' compact toy fold: a 5 x 5 serpentine lattice at 4.6 A, perturbed by 0.3 A."""
    rng = np.random.default_rng(seed)
    pts = []
    for t in range(L):
        z, r = divmod(t, 25)
        y, x = divmod(r, 5)
        if y % 2:
            x = 4 - x
        if z % 2:
            y, x = 4 - y, 4 - x
        pts.append((4.6 * x, 4.6 * y, 4.6 * z))
    return np.array(pts) + 0.3 * rng.standard_normal((L, 3))


def fair_to_hf(arrays, cfg):
    """A float64 HF EsmModel that holds the fair-esm arrays of proteingym_amd.synthetic.blob_to_arrays (tests only: the inverse of the
    key map of proteingym_amd.protssn.hf_to_fair, written out on its own)."""
    from transformers import EsmConfig, EsmModel
    hc = EsmConfig(vocab_size=33, hidden_size=cfg["embed_dim"], num_hidden_layers=cfg["layers"], num_attention_heads=cfg["heads"],
                   intermediate_size=cfg["ffn_dim"], position_embedding_type="rotary", token_dropout=bool(cfg["token_dropout"]),
                   pad_token_id=1, mask_token_id=32, layer_norm_eps=1e-5, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    model = EsmModel(hc, add_pooling_layer=False).double().eval()
    names = {"self_attn_layer_norm": "attention.LayerNorm", "self_attn.q_proj": "attention.self.query", "self_attn.k_proj": "attention.self.key",
             "self_attn.v_proj": "attention.self.value", "self_attn.out_proj": "attention.output.dense", "final_layer_norm": "LayerNorm",
             "fc1": "intermediate.dense", "fc2": "output.dense"}
    sd = model.state_dict()
    put = lambda k, a: sd[k].copy_(torch.as_tensor(np.asarray(a)).double())
    put("embeddings.word_embeddings.weight", arrays["embed_tokens.weight"])
    for i in range(cfg["layers"]):
        for a, b in names.items():
            for leaf in ("weight", "bias"):
                put(f"encoder.layer.{i}.{b}.{leaf}", arrays[f"layers.{i}.{a}.{leaf}"])
    for leaf in ("weight", "bias"):
        put(f"encoder.emb_layer_norm_after.{leaf}", arrays[f"emb_layer_norm_after.{leaf}"])
    model.load_state_dict(sd)
    return model


def hf_residue_rows(model, tokens):
    """last_hidden_state[0, 1 : T - 1] of one sequence as a numpy array."""
    with torch.no_grad():
        t = torch.as_tensor(np.asarray(tokens)).long()[None]
        return model(input_ids=t, attention_mask=torch.ones_like(t)).last_hidden_state[0, 1:-1].numpy()


# the toy assay of tests/golden/ProtSSN_toy (make_golden_protssn.py records it; tests/test_gpu_protssn.py rebuilds its models)
TOY_NAME = "TOY_PSSN"
TOY_ESM = dict(layers=2, embed_dim=128, heads=2, ffn_dim=512, max_positions=0, token_dropout=1, emb_layer_norm_before=0)
TOY_MODELS = (("k10_h64", 10, 64, 11), ("k20_h96", 20, 96, 12))        # name, k, h, seed


def toy_esm():
    """(cfg, blob) of the toy's seeded two-layer ESM2."""
    from proteingym_amd import _lib, synthetic
    cfg = dict(TOY_ESM, arch=_lib.ARCH_ESM2)
    return cfg, synthetic.random_weights(cfg, seed=3)


def toy_state_dict(h, seed, node_in=128, layers=6):
    from proteingym_amd import protssn
    return protssn.random_state_dict(seed, node_in, h, gain=0.5, layers=layers, bias_std=0.02)
