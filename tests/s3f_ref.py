"""A torch restatement of S3F's inference on top of tests/s2f_ref.py (proteingym/baselines/S3F: s3f/gvp.py SurfGVP.forward,
surface_feature_init and residue2surface; s3f/surface.py knn_atoms; s3f/dataset.py load_surface and MutantDataset.truncate;
compute_fitness.py:122-137; script/evaluate.py predict / load_dataset / get_prob), written from those files and independent of
proteingym_amd/s3f.py.  Nothing is folded here: surf_in_linear runs on every (point, neighbour) row and surf_in_mlp on the 1322-wide
concatenation, as the reference does.  Every function takes the dtype of its tensors."""
import numpy as np
import torch

import s2f_ref
from s2f_ref import SM

K_RES, K_SURF = 3, 16


def nearest(q, c, k, skip_self=False):
    """For every row of q the k nearest rows of c by squared distance, nearest first, ties to the lower index; float64 on the
    coordinates as given.  Returns (int64 [n, k], squared distances [n, k], the (k + 1)-th squared distance [n], inf if there is none)."""
    q, c = np.asarray(q, dtype=np.float64), np.asarray(c, dtype=np.float64)
    d2 = ((q[:, None, :] - c[None, :, :]) ** 2).sum(-1)
    if skip_self:
        d2[np.arange(len(q)), np.arange(len(q))] = np.inf
    order = np.argsort(d2, axis=1, kind="stable")
    idx = order[:, :k]
    rows = np.arange(len(q))[:, None]
    nxt = d2[rows[:, 0], order[:, k]] if d2.shape[1] > k else np.full(len(q), np.inf)
    return idx, d2[rows, idx], nxt


def knn_margin(q, c, k, skip_self=False, ordered=False):
    """The smallest relative gap (b - a) / b between the k-th and the (k + 1)-th squared distance over the points; with `ordered`
    also between consecutive members of the list (a list whose order matters)."""
    _, d, nxt = nearest(q, c, k, skip_self)
    seq = np.concatenate([d, nxt[:, None]], 1)
    seq = seq[:, (0 if ordered else k - 1):]
    a, b = seq[:, :-1], seq[:, 1:]
    with np.errstate(invalid="ignore"):
        gap = np.where(np.isinf(b), np.inf, (b - a) / np.where(np.isinf(b), 1.0, b))
    return float(gap.min())


def surface_lists(pos, spos):
    """(src int64 [Ns, 16]: every point's 16 nearest other points in ascending index; res int64 [Ns, 3] and res_dist [Ns, 3]: its three
    nearest C-alpha atoms, nearest first, and the distances)."""
    src = np.sort(nearest(spos, spos, K_SURF, skip_self=True)[0], axis=1)
    res, d2, _ = nearest(spos, pos, K_RES)
    return src, res, np.sqrt(d2)


def surface_edges(src):
    """(source row, centre row) of the edge list, by (centre, source)."""
    n = len(src)
    return torch.as_tensor(np.stack([src.reshape(-1), np.repeat(np.arange(n), K_SURF)]), dtype=torch.int64)


def surface_edge_features(W, spos, edges):
    j, i = edges
    vec = spos[j] - spos[i]                                       # pos[source] - pos[centre]: the opposite of the residue graph's
    s, v = s2f_ref.tuple_ln(W, SM + "surf_W_e.0.", s2f_ref.rbf((spos[i] - spos[j]).norm(dim=-1)), vec[:, None, :])
    return s2f_ref.gvp(W, SM + "surf_W_e.1.", s, v, False, 1)


def surface_input(W, x, res, res_dist, feat):
    """surface_feature_init's node half: x [L, D] -> [Ns, D]."""
    n = len(res)
    h = torch.cat([x[torch.as_tensor(res.reshape(-1))], torch.as_tensor(res_dist.reshape(-1, 1)).to(x)], -1).view(n, K_RES, -1)
    h = (h @ W[SM + "surf_in_linear.weight"].T).mean(1)
    h = torch.cat([h, feat], -1) @ W[SM + "surf_in_mlp.0.weight"].T + W[SM + "surf_in_mlp.0.bias"]
    h = torch.relu(torch.nn.functional.layer_norm(h, (h.shape[-1],), W[SM + "surf_in_mlp.2.weight"], W[SM + "surf_in_mlp.2.bias"], 1e-5))
    return h @ W[SM + "surf_in_mlp.4.weight"].T + W[SM + "surf_in_mlp.4.bias"]


def surface_structure(W, pos, spos, like):
    """What depends on the structure only: dict(src, res, res_dist, edges, e_s, e_v)."""
    src, res, res_dist = surface_lists(pos, spos)
    edges = surface_edges(src).to(like.device)
    es, ev = surface_edge_features(W, torch.as_tensor(np.array(spos)).to(like), edges)
    return dict(src=src, res=res, res_dist=res_dist, edges=edges, e_s=es, e_v=ev)


def surface_gnn(W, x, feat, st, layers=5, trace=None):
    """One copy: x [L, D] -> (surf_W_out's rows [Ns, 256], node state (s, v) after the last layer)."""
    h = surface_input(W, x, st["res"], st["res_dist"], feat)
    if trace is not None:
        trace["init"] = h
    s, _ = s2f_ref.tuple_ln(W, SM + "surf_W_v.0.", h, None)
    s, v = s2f_ref.gvp(W, SM + "surf_W_v.1.", s, None, False, 16)
    for l in range(layers):
        s, v = s2f_ref.conv_layer(W, f"{SM}surf_layers.{l}.", s, v, st["edges"], st["e_s"], st["e_v"])
        if trace is not None and l == 0:
            trace["layer0_s"], trace["layer0_v"] = s, v
    os_, ov = s2f_ref.tuple_ln(W, SM + "surf_W_out.0.", s, v)
    out, _ = s2f_ref.gvp(W, SM + "surf_W_out.1.", os_, ov, True, 0)
    return out, s, v


def surf_gvp(W, pos, spos, feat, xs, layers=5, graph=None, st=None, trace=None):
    """SurfGVP.forward on one loader batch: xs = the [L, D] inputs of its copies, all on one structure and surface.  Returns
    dict(node_feature [B, L, 256], bb [B, L, 256], surf_out [B, Ns, 256], surf_s, surf_v, pooled [256]).  res2surf is None in
    the reference's forward, so the readout is the mean of surf_W_out's rows over every surface point of the batch."""
    like = xs[0]
    st = surface_structure(W, pos, spos, like) if st is None else st
    graph = s2f_ref.structure_graph(W, pos, like) if graph is None else graph
    feat = torch.as_tensor(np.array(feat)).to(like)
    bb = [s2f_ref.gvp_gnn(W, pos, x, layers, graph=graph)["out"] for x in xs]
    surf = [surface_gnn(W, x, feat, st, layers, trace if b == 0 else None) for b, x in enumerate(xs)]
    pooled = torch.cat([o for o, _, _ in surf], 0)[None].mean(dim=1)[0]
    return dict(node_feature=torch.stack([b + pooled for b in bb]), bb=torch.stack(bb), surf_out=torch.stack([o for o, _, _ in surf]),
                surf_s=torch.stack([s for _, s, _ in surf]), surf_v=torch.stack([v for _, _, v in surf]), pooled=pooled)


def groups(n, batch_size):
    """The unshuffled loader's batches over n items."""
    return [list(range(a, min(a + batch_size, n))) for a in range(0, n, batch_size)]


def gvp_forward(sd, pos, plddt, spos, feat, x, seq_logits, batch_size=1, dtype=torch.float64, layers=5, threshold=70.0):
    """Copies [B, L, D] / [B, L, 20] in loader batches of batch_size -> numpy (lp [B, L, 20], surf_s [B, Ns, 256], surf_v [B, Ns, 16, 3],
    pool_sum [B, 256] = the column sum of each copy's surf_W_out rows)."""
    W = s2f_ref.tensors(sd, dtype)
    xs = torch.as_tensor(np.asarray(x)).to(dtype)
    qs = torch.as_tensor(np.asarray(seq_logits)).to(dtype)
    st = surface_structure(W, pos, spos, xs)
    graph = s2f_ref.structure_graph(W, pos, xs)
    lp, ss, sv, ps = [], [], [], []
    for g in groups(len(xs), batch_size):
        out = surf_gvp(W, pos, spos, feat, [xs[b] for b in g], layers, graph, st)
        for n, b in enumerate(g):
            lp.append(s2f_ref.head_logprobs(W, out["node_feature"][n], qs[b], plddt, threshold))
        ss.append(out["surf_s"]), sv.append(out["surf_v"]), ps.append(out["surf_out"].sum(1))
    return torch.stack(lp).numpy(), torch.cat(ss).numpy(), torch.cat(sv).numpy(), torch.cat(ps).numpy()


# -- surface files and truncation ----------------------------------------------------------------------------------------------------
def read_surfaces(dicts):
    """compute_fitness.py:122-137 on the unpickled dicts of an assay's pdb files: points and [hks | curvatures] concatenated, the
    res2surf arrays concatenated unchanged."""
    pts = np.concatenate([np.asarray(d["surf_points"], dtype=np.float32) for d in dicts])
    feat = np.concatenate([np.concatenate([np.asarray(d["surf_hks"], dtype=np.float32), np.asarray(d["surf_curvatures"], dtype=np.float32)], -1)
                           for d in dicts])
    return pts, feat, np.concatenate([np.asarray(d["res2surf"]) for d in dicts])


def truncate(pts, feat, res2surf, s_start, start, end):
    """MutantDataset.truncate's surface half: residues [start, end) of a structure that begins at s_start keep the points their res2surf
    rows name; returns (points, features, the re-indexed res2surf rows)."""
    rows = np.asarray(res2surf)[start - s_start:end - s_start]
    kept, inverse = np.unique(rows, return_inverse=True)
    return pts[kept], feat[kept], inverse.reshape(rows.shape)


# -- end to end ----------------------------------------------------------------------------------------------------------------------
def sequence_tables(sd, seq, pos, plddt, spos, feat, sets, batch_size, heads, esm_layers, dtype=torch.float64, layers=5, threshold=70.0):
    """For the masked sequences `sets` (0-based residue indices each) of one window, in loader order and batches of batch_size: the
    [L, 20] log-probability tables of FusionNetwork(MyESM, SurfGVP) under ResidueTypePrediction.inference."""
    W = s2f_ref.tensors(sd, dtype)
    base = [0] + [s2f_ref.ESM_TOKENS.index(a) for a in seq] + [2]
    cols = [s2f_ref.ESM_TOKENS.index(a) for a in s2f_ref.ORDER]
    reps, qs = [], []
    for st_ in sets:
        tok = list(base)
        for i in st_:
            tok[1 + i] = s2f_ref.ESM_TOKENS.index("<mask>")
        rep, logits = s2f_ref.esm2(W, tok, heads, esm_layers)
        reps.append(rep[1:-1])
        qs.append(logits[1:-1][:, cols])
    st = surface_structure(W, pos, spos, reps[0])
    graph = s2f_ref.structure_graph(W, pos, reps[0])
    full = [None] * len(sets)
    for g in groups(len(sets), batch_size):
        out = surf_gvp(W, pos, spos, feat, [reps[b] for b in g], layers, graph, st)
        for n, b in enumerate(g):
            full[b] = s2f_ref.head_logprobs(W, out["node_feature"][n], qs[b], plddt, threshold)
    return torch.stack(full).numpy()
