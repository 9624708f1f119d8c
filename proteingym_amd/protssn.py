"""ProtSSN scoring on libpgmi (include/pgmi.h, ProtSSN section).

Replaces proteingym/baselines/protssn's model side: one unmasked ESM2-650M forward of the structure's own sequence, its residue rows
through a six-layer EGNN over the k-nearest C-alpha graph (k = 10, 20 or 30), a 20-way head and log(softmax + 1e-9).  The graph, its 93
edge attributes and the CATH normalisation are built here in numpy; the EGNN and ESM2 run in HIP (csrc/api_protssn.hip, egnn.hip on
the ESM2 encoder).  Up to nine checkpoints share one ESM2 forward per assay.  Nothing is downloaded.

torch_geometric, Bio and scipy's use by the reference are not run here; each reading of their behaviour is one named function or
table: ``read_pdb`` (Bio.PDB's parser and the reference's residue filter), ``calpha_graph`` (get_calpha_graph's three branches over
scipy's cdist), ``edge_attributes`` (get_edge_features, distance_featurizer and the orientation block), ``normalize``
(NormalizeProtein), ``EDGE_FLOW`` (torch_geometric's source_to_target flow) and ``label_row`` (compute_fitness.py label_row).
"""
from __future__ import annotations

import ctypes as C
import json
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from . import esm as pesm

# compute_fitness.py amino_acids_type: the 20 columns of the head
AA_ORDER = "ARNDCQEGHILKMFPSTWYV"
THREE_TO_ONE = {"ALA": "A", "ARG": "R", "ASN": "N", "ASP": "D", "CYS": "C", "GLN": "Q", "GLU": "E", "GLY": "G", "HIS": "H", "ILE": "I",
                "LEU": "L", "LYS": "K", "MET": "M", "PHE": "F", "PRO": "P", "SER": "S", "THR": "T", "TRP": "W", "TYR": "Y", "VAL": "V"}
# edge_index = [centres; neighbours]; MessagePassing's default flow is source_to_target: x_j = x[edge_index[0]] (the centre),
# x_i = x[edge_index[1]] (the neighbour), and messages are summed at edge_index[1]
EDGE_FLOW = "centre->neighbour"
CUTOFF, SEQ_DIST_CUT, EDGE_ATTR_DIM, LAYERS, NODE_IN = 30.0, 64, 93, 6, 1280
KS, HS = (10, 20, 30), (512, 768, 1280)
OFFSETS = {"A0A140D2T1_ZIKV_Sourisseau_2019": 291}          # compute_fitness.py predict
PREFIX = "GNN_model."
# src/config/egnn.yaml, the fields the released checkpoints were trained with and this path computes
YAML_FIXED = dict(embedding=False, residual=False, mlp_num=2, dropout=0, edge_attr_dim=EDGE_ATTR_DIM, output_dim=20)


class ProtssnConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("abi_version", "node_in", "hidden", "layers", "edge_attr_dim", "precision", "edge_chunk")]


def _up32(v: int) -> int:
    return (v + 31) // 32 * 32


def dims(node_in: int, hidden: int, edge_attr_dim: int = EDGE_ATTR_DIM) -> dict:
    """The widths of one layer and their padded forms (include/pgmi.h)."""
    Hh = 2 * (2 * node_in + edge_attr_dim + 1)
    return dict(D=node_in, h=hidden, A=edge_attr_dim, Hh=Hh, Hp=_up32(Hh), hp=_up32(hidden), Ap=_up32(edge_attr_dim + 1))


# -- PDB ---------------------------------------------------------------------------------------------------------------------
def read_pdb(path_or_lines) -> Tuple[np.ndarray, np.ndarray, np.ndarray, str]:
    """get_receptor_inference restated on fixed columns: the first model, every chain in file order, ATOM and HETATM records, HOH
    skipped, the first alternate location of an atom; a residue is kept only with N, CA and C.  Returns (N, CA, C float64 [L, 3] --
    the float32 values Bio.PDB stores -- and the one-letter sequence of the kept residues).  A kept residue whose name is not one of
    the 20 standard ones is a ValueError that names it (the reference drops such a protein into wrong_proteins)."""
    if isinstance(path_or_lines, (str, os.PathLike)):
        with open(path_or_lines) as f:
            lines = f.read().splitlines()
    else:
        lines = list(path_or_lines)
    residues, key = [], None
    for line in lines:
        rec = line[:6]
        if rec.startswith("ENDMDL"):
            break
        if rec not in ("ATOM  ", "HETATM"):
            continue
        resname = line[17:20].strip()
        if resname == "HOH":
            continue
        k = (line[21], line[22:27], resname)
        if k != key:
            residues.append((k, {}))
            key = k
        atoms = residues[-1][1]
        name = line[12:16].strip()
        if name in ("N", "CA", "C") and name not in atoms:
            atoms[name] = (float(line[30:38]), float(line[38:46]), float(line[46:54]))
    kept = [(k, a) for k, a in residues if len(a) == 3]
    if not kept:
        raise ValueError("no residue with N, CA and C in the PDB file")
    seq = []
    for (chain, resid, resname), _ in kept:
        if resname not in THREE_TO_ONE:
            raise ValueError(f"residue {resname} {chain}{resid.strip()} is not one of the 20 standard amino acids")
        seq.append(THREE_TO_ONE[resname])
    pick = lambda n: np.array([a[n] for _, a in kept], dtype=np.float32).astype(np.float64)
    return pick("N"), pick("CA"), pick("C"), "".join(seq)


# -- graph -------------------------------------------------------------------------------------------------------------------
def calpha_graph(ca: np.ndarray, k: int, cutoff: float = CUTOFF) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """get_calpha_graph's edge list: per centre c the residues closer than `cutoff` (float64 distances, c itself removed) in ascending
    index; more than k of them: argsort(distances[c])[1 : k + 1] instead; none: the nearest other residue.  Returns (centre,
    neighbour int32 [E], distance float64 [E]) in the reference's order."""
    ca = np.asarray(ca, dtype=np.float64)
    if len(ca) <= 1:
        raise ValueError("rec contains only 1 residue!")
    dist = np.sqrt(((ca[:, None, :] - ca[None, :, :]) ** 2).sum(-1))
    centre, nb = [], []
    for c in range(len(ca)):
        dst = [int(j) for j in np.where(dist[c] < cutoff)[0] if j != c]
        if len(dst) > k:
            dst = [int(j) for j in np.argsort(dist[c])[1:k + 1]]
        if not dst:
            dst = [int(j) for j in np.argsort(dist[c])[1:2]]
        centre += [c] * len(dst)
        nb += dst
    centre, nb = np.array(centre, dtype=np.int32), np.array(nb, dtype=np.int32)
    return centre, nb, dist[centre, nb]


def local_frames(n: np.ndarray, ca: np.ndarray, c: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(n_i, u_i, v_i) float64 [L, 3] of every residue (get_calpha_graph's loop)."""
    u = (n - ca) / np.linalg.norm(n - ca, axis=1, keepdims=True)
    t = (c - ca) / np.linalg.norm(c - ca, axis=1, keepdims=True)
    nrm = np.cross(u, t)
    nrm = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
    return nrm, u, np.cross(nrm, u)


def edge_attributes(centre, nb, dist, n, ca, c) -> np.ndarray:
    """float32 [E, 93]: the one-hot of min(|c - n|, 64), 15 exp(-((d / 4)^2) / 1.5^x), the contact flag d <= 8, and the 12 orientation
    values in the NEIGHBOUR's basis (n_i, u_i, v_i): the float32 C-alpha difference centre - neighbour, then the centre's n_i, u_i, v_i."""
    centre, nb = np.asarray(centre), np.asarray(nb)
    E = len(centre)
    out = np.zeros((E, EDGE_ATTR_DIM), dtype=np.float32)
    out[np.arange(E), np.minimum(np.abs(centre.astype(np.int64) - nb), SEQ_DIST_CUT)] = 1.0
    d = np.asarray(dist, dtype=np.float64)
    for x in range(15):
        out[:, SEQ_DIST_CUT + 1 + x] = np.exp(-((d / 4) ** 2) / float(1.5 ** x)).astype(np.float32)
    out[:, SEQ_DIST_CUT + 16] = d <= 8
    ni, ui, vi = local_frames(np.asarray(n, np.float64), np.asarray(ca, np.float64), np.asarray(c, np.float64))
    basis = np.stack([ni[nb], ui[nb], vi[nb]], axis=1)                              # [E, 3, 3], rows n_i, u_i, v_i of the neighbour
    ca32 = np.asarray(ca, dtype=np.float32)                                         # the reference subtracts the float32 tensor
    diff = (ca32[centre] - ca32[nb]).astype(np.float64)
    o = SEQ_DIST_CUT + 17
    for j, vec in enumerate((diff, ni[centre], ui[centre], vi[centre])):
        out[:, o + 3 * j:o + 3 * j + 3] = np.einsum("eij,ej->ei", basis, vec).astype(np.float32)
    return out


def load_norm(k: int, repo_path: Optional[str] = None, norm_dir: Optional[str] = None) -> Dict[str, np.ndarray]:
    """pos_std [3], edge_attr_mean [93], edge_attr_std [93] of cath_k{k}_mean_attr.pt, from norm_dir or
    <repo_path>/proteingym/baselines/protssn/norm; a norm_dir may hold one protssn_norm.npz (keys k{k}_<name>) instead."""
    d = norm_dir or os.path.join(repo_path or ".", "proteingym", "baselines", "protssn", "norm")
    names = ("pos_std", "edge_attr_mean", "edge_attr_std")
    npz = os.path.join(d, "protssn_norm.npz")
    if os.path.isfile(npz):
        with np.load(npz) as z:
            return {n: np.asarray(z[f"k{k}_{n}"], dtype=np.float32) for n in names}
    path = os.path.join(d, f"cath_k{k}_mean_attr.pt")
    if not os.path.isfile(path):
        raise FileNotFoundError(f"{path}: no normalisation file (--repo_path or --norm_dir; this path never downloads)")
    import torch
    dic = torch.load(path, map_location="cpu", weights_only=True)
    return {n: dic[n].float().numpy() for n in names}


def normalize(ca: np.ndarray, edge_attr: np.ndarray, norm: Dict[str, np.ndarray]) -> Tuple[np.ndarray, np.ndarray]:
    """NormalizeProtein in float32: pos - mean(pos), / (mean(pos_std) + 1e-10); edge_attr[:, 64:] standardised (column 64, the last
    one-hot column, included: skip_edge_attr is 64)."""
    eps = np.float32(1e-10)
    pos = np.asarray(ca, dtype=np.float32)
    pos = pos - pos.mean(axis=0, dtype=np.float32)
    pos = pos / (norm["pos_std"].astype(np.float32).mean(dtype=np.float32) + eps)
    ea = np.array(edge_attr, dtype=np.float32)
    s = SEQ_DIST_CUT
    ea[:, s:] = (ea[:, s:] - norm["edge_attr_mean"][s:].astype(np.float32)) / (norm["edge_attr_std"][s:].astype(np.float32) + eps)
    return pos, ea


def build_graph(n, ca, c, k: int, norm: Dict[str, np.ndarray]):
    """(pos float32 [L, 3], centre, neighbour int32 [E], edge_attr float32 [E, 93]), normalised: what pgmi_protssn_set_graph takes."""
    centre, nb, dist = calpha_graph(ca, k)
    pos, ea = normalize(ca, edge_attributes(centre, nb, dist, n, ca, c), norm)
    return pos, centre, nb, ea


# -- weights -----------------------------------------------------------------------------------------------------------------
def key_shapes(node_in: int = NODE_IN, hidden: int = 512, layers: int = LAYERS, edge_attr_dim: int = EDGE_ATTR_DIM):
    """(state-dict key, shape) of GNN_model(EGNN): dropout 0 is an nn.Identity, so the Linears keep indices 0 and 3."""
    d = dims(node_in, hidden, edge_attr_dim)
    D, h, Hh = d["D"], d["h"], d["Hh"]
    out = []
    for n in range(layers):
        p = f"{PREFIX}mpnn_layes.{n}."
        out += [(p + "edge_mlp.0.weight", (Hh, Hh // 2)), (p + "edge_mlp.0.bias", (Hh,)),
                (p + "edge_mlp.3.weight", (h, Hh)), (p + "edge_mlp.3.bias", (h,)),
                (p + "node_mlp.0.weight", (2 * D, D + h)), (p + "node_mlp.0.bias", (2 * D,)),
                (p + "node_mlp.3.weight", (D, 2 * D)), (p + "node_mlp.3.bias", (D,))]
    return out + [(PREFIX + "lin.weight", (20, D)), (PREFIX + "lin.bias", (20,))]


def param_count(node_in: int = NODE_IN, hidden: int = 512, layers: int = LAYERS) -> int:
    """The checkpoint's parameter count (the protssn README's 148 M / 160 M / 184 M), pads not counted."""
    return sum(int(np.prod(s)) for _, s in key_shapes(node_in, hidden, layers))


def _to_np(t) -> np.ndarray:
    return t.detach().to("cpu").float().numpy() if hasattr(t, "detach") else np.asarray(t, dtype=np.float32)


def _pad(a: np.ndarray, shape) -> np.ndarray:
    out = np.zeros(shape, dtype=np.float32)
    out[tuple(slice(0, s) for s in a.shape)] = a
    return out


def pack(sd, node_in: int = NODE_IN, hidden: int = 512, layers: int = LAYERS) -> np.ndarray:
    """The blob of include/pgmi.h from the checkpoint's state dict: W1's column blocks Wi | Wj | We, every width padded with zeros.
    Anything missing, unexpected or of another shape is an error."""
    want = key_shapes(node_in, hidden, layers)
    names = {k for k, _ in want}
    missing = sorted(k for k in names if k not in sd)
    unexpected = sorted(k for k in sd if k not in names)
    if missing or unexpected:
        raise ValueError(f"not a ProtSSN k*_h{hidden} state dict: missing {missing[:5]}, unexpected {unexpected[:5]}")
    for k, shape in want:
        if tuple(np.shape(sd[k])) != shape:
            raise ValueError(f"{k}: shape {tuple(np.shape(sd[k]))}, this path needs {shape}")
    d = dims(node_in, hidden)
    D, h, A, Hp, hp, Ap = d["D"], d["h"], d["A"], d["Hp"], d["hp"], d["Ap"]
    parts = []
    for n in range(layers):
        p = f"{PREFIX}mpnn_layes.{n}."
        w1 = _to_np(sd[p + "edge_mlp.0.weight"])
        parts += [_pad(w1[:, :D], (Hp, D)), _pad(w1[:, D:2 * D], (Hp, D)), _pad(w1[:, 2 * D:], (Hp, Ap)),
                  _pad(_to_np(sd[p + "edge_mlp.0.bias"]), (Hp,)),
                  _pad(_to_np(sd[p + "edge_mlp.3.weight"]), (hp, Hp)), _pad(_to_np(sd[p + "edge_mlp.3.bias"]), (hp,))]
        w3 = _to_np(sd[p + "node_mlp.0.weight"])
        parts += [np.concatenate([w3[:, :D], _pad(w3[:, D:], (2 * D, hp))], axis=1), _to_np(sd[p + "node_mlp.0.bias"]),
                  _to_np(sd[p + "node_mlp.3.weight"]), _to_np(sd[p + "node_mlp.3.bias"])]
    parts += [_to_np(sd[PREFIX + "lin.weight"]), _to_np(sd[PREFIX + "lin.bias"])]
    return np.concatenate([np.ascontiguousarray(a, dtype=np.float32).ravel() for a in parts])


def unpack(blob: np.ndarray, node_in: int = NODE_IN, hidden: int = 512, layers: int = LAYERS) -> List[Dict[str, np.ndarray]]:
    """The blob's tensors by name, pads included: per layer Wi, Wj, We, b1, W2, b2, W3, b3, W4, b4; last {lin_w, lin_b}."""
    d = dims(node_in, hidden)
    D, Hp, hp, Ap = d["D"], d["Hp"], d["hp"], d["Ap"]
    shapes = [("Wi", (Hp, D)), ("Wj", (Hp, D)), ("We", (Hp, Ap)), ("b1", (Hp,)), ("W2", (hp, Hp)), ("b2", (hp,)),
              ("W3", (2 * D, D + hp)), ("b3", (2 * D,)), ("W4", (D, 2 * D)), ("b4", (D,))]
    out, o = [], 0
    for group in [shapes] * layers + [[("lin_w", (20, D)), ("lin_b", (20,))]]:
        cur = {}
        for name, s in group:
            m = int(np.prod(s))
            cur[name] = blob[o:o + m].reshape(s)
            o += m
        out.append(cur)
    if o != blob.size:
        raise ValueError(f"blob has {blob.size} elements, the layout needs {o}")
    return out


def random_state_dict(seed: int, node_in: int = NODE_IN, hidden: int = 512, gain: float = 1.0, layers: int = LAYERS,
                      bias_std: float = 0.0) -> Dict[str, np.ndarray]:
    """A seeded checkpoint: every Linear of the layers Xavier-normal (std = sqrt(2 / (fan_in + fan_out))) times `gain`, as EGNN_Sparse's
    init_ draws them; lin as nn.Linear's default.  init_ zeroes the biases; bias_std > 0 draws them N(0, bias_std^2) instead, so that a
    test reads every bias."""
    rng = np.random.default_rng(seed)
    sd = {}
    for k, shape in key_shapes(node_in, hidden, layers):
        if ".lin." in k:
            b = 1.0 / np.sqrt(node_in)
            a = rng.uniform(-b, b, shape)
        elif k.endswith("weight"):
            a = rng.standard_normal(shape) * (gain * np.sqrt(2.0 / (shape[0] + shape[1])))
        else:
            a = rng.standard_normal(shape) * bias_std
        sd[k] = a.astype(np.float32)
    return sd


def load_checkpoint(model_dir: str, k: int, h: int):
    """torch.load(<model_dir>/protssn_k{k}_h{h}.pt), as compute_fitness.py prepare reads it."""
    import torch
    path = os.path.join(model_dir, f"protssn_k{k}_h{h}.pt")
    if not os.path.isfile(path):
        raise FileNotFoundError(f"{path}: no such checkpoint (this path never downloads)")
    return dict(torch.load(path, map_location="cpu", weights_only=True))


# -- ESM2 --------------------------------------------------------------------------------------------------------------------
_HF_LAYER = (("attention.LayerNorm", "self_attn_layer_norm"), ("attention.self.query", "self_attn.q_proj"),
             ("attention.self.key", "self_attn.k_proj"), ("attention.self.value", "self_attn.v_proj"),
             ("attention.output.dense", "self_attn.out_proj"), ("LayerNorm", "final_layer_norm"), ("intermediate.dense", "fc1"),
             ("output.dense", "fc2"))


def _hf_ignored(key: str) -> bool:
    """What EsmModel carries and last_hidden_state never reads: the pooler, the contact head, rotary buffers, and the learned
    position table some releases keep for rotary models."""
    return (key.startswith("pooler.") or key.startswith("contact_head.") or key.endswith("inv_freq") or key.endswith("position_ids")
            or key == "embeddings.position_embeddings.weight")


def hf_to_fair(sd, hf_config: dict) -> Tuple[dict, Dict[str, np.ndarray]]:
    """(ESM2 cfg, state dict under the names esm.pack_state_dict packs) from an HF EsmModel state dict and its config.  EsmModel has no LM
    head: lm_head.* are zeros, which pgmi_esm_residue_rows never reads.  What this path does not compute is refused."""
    get = hf_config.get
    if get("position_embedding_type") != "rotary":
        raise ValueError(f"position_embedding_type {get('position_embedding_type')!r}: this path runs rotary ESM2 models")
    if get("emb_layer_norm_before"):
        raise ValueError("emb_layer_norm_before is set: ESM2 models have none")
    if abs(float(get("layer_norm_eps", 1e-5)) - 1e-5) > 1e-12:
        raise ValueError(f"layer_norm_eps {get('layer_norm_eps')}: this path runs 1e-5")
    if int(get("vocab_size", 33)) != 33:
        raise ValueError(f"vocab_size {get('vocab_size')}: this path runs the 33-token ESM alphabet")
    D, layers = int(get("hidden_size")), int(get("num_hidden_layers"))
    cfg = dict(arch=_lib.ARCH_ESM2, layers=layers, embed_dim=D, heads=int(get("num_attention_heads")),
               ffn_dim=int(get("intermediate_size")), max_positions=0, token_dropout=int(bool(get("token_dropout"))),
               emb_layer_norm_before=0)
    out, used = {}, set()

    def take(src, dst):
        if src not in sd:
            raise ValueError(f"not an HF EsmModel state dict: {src} is missing")
        out[dst] = _to_np(sd[src])
        used.add(src)
    take("embeddings.word_embeddings.weight", "embed_tokens.weight")
    for i in range(layers):
        for a, b in _HF_LAYER:
            for leaf in ("weight", "bias"):
                take(f"encoder.layer.{i}.{a}.{leaf}", f"layers.{i}.{b}.{leaf}")
    for leaf in ("weight", "bias"):
        take(f"encoder.emb_layer_norm_after.{leaf}", f"emb_layer_norm_after.{leaf}")
    unexpected = sorted(k for k in sd if k not in used and not _hf_ignored(k))
    if unexpected:
        raise ValueError(f"unexpected keys in the HF EsmModel state dict: {unexpected[:5]}")
    out["lm_head.dense.weight"] = np.zeros((D, D), np.float32)
    for k in ("lm_head.dense.bias", "lm_head.layer_norm.weight", "lm_head.layer_norm.bias"):
        out[k] = np.zeros(D, np.float32)
    out["lm_head.bias"] = np.zeros(33, np.float32)
    return cfg, out


def load_plm(path: str, device: int = 0, precision: str = "f16x3", max_rows: int = 0) -> pesm.EsmModel:
    """--plm: a fair-esm ESM2 .pt, or a local HF EsmModel directory (config.json + model.safetensors / pytorch_model.bin)."""
    if os.path.isdir(path):
        with open(os.path.join(path, "config.json")) as f:
            hf_config = json.load(f)
        st = os.path.join(path, "model.safetensors")
        if os.path.isfile(st):
            from safetensors.numpy import load_file
            sd = load_file(st)
        else:
            import torch
            sd = torch.load(os.path.join(path, "pytorch_model.bin"), map_location="cpu", weights_only=True)
        sd = {k[len("esm."):] if k.startswith("esm.") else k: v for k, v in sd.items() if not k.startswith("lm_head.")}
        cfg, fair = hf_to_fair(sd, hf_config)
    elif str(path).endswith(".pt") and os.path.isfile(path):
        cfg, fair = pesm._upgrade_state_dict(path)
        if cfg["arch"] != _lib.ARCH_ESM2:
            raise ValueError(f"{path}: ProtSSN runs on an ESM2 model")
    else:
        raise FileNotFoundError(f"{path}: --plm takes a local fair-esm ESM2 .pt or a local HF EsmModel directory (nothing is downloaded)")
    return pesm.EsmModel(cfg, pesm.pack_state_dict(cfg, fair), device=device, precision=precision, max_rows=max_rows)


def tokenize(seq: str) -> np.ndarray:
    ids = np.empty(len(seq) + 2, dtype=np.int32)
    ids[0], ids[-1] = pesm.VOCABULARY.index("<cls>"), pesm.VOCABULARY.index("<eos>")
    for i, a in enumerate(seq):
        ids[i + 1] = pesm.VOCABULARY.index(a)
    return ids


def residue_rows(esm: pesm.EsmModel, seq: str) -> np.ndarray:
    """esm_rep: float32 [L, D], EsmModel(...).last_hidden_state[0, 1 : L + 1] of the whole sequence."""
    tok = tokenize(seq)
    rows = np.empty((len(seq), esm.cfg["embed_dim"]), np.float32)
    _lib.check(_lib.load().pgmi_esm_residue_rows(esm._h, _lib.ptr(tok, _lib._i32p), tok.size, _lib.ptr(rows, _lib._f32p)))
    return rows


# -- scoring -----------------------------------------------------------------------------------------------------------------
def label_row(rows: str, sequence: str, token_probs: np.ndarray, offset_idx: int = 1) -> float:
    """compute_fitness.py label_row: the separator is ':' when present, else ';'; 'wt' (any case) scores 0; a wild-type letter that
    differs from the sequence is an error that names the row."""
    sep = ":" if ":" in rows else ";"
    total = 0
    for row in rows.split(sep):
        if row.lower() == "wt":
            total = total + 0
            continue
        try:
            wt, idx, mt = row[0], int(row[1:-1]) - offset_idx, row[-1]
        except ValueError:
            raise ValueError(f"row: {row}, sequence: {sequence}") from None
        if not 0 <= idx < len(sequence) or sequence[idx] != wt:
            have = sequence[idx] if 0 <= idx < len(sequence) else "nothing"
            raise ValueError(f"The {row}, {have}: the structure's residue at that position is not {wt}")
        total = total + (token_probs[idx, AA_ORDER.index(mt)] - token_probs[idx, AA_ORDER.index(wt)]).item()
    return total


def ensemble_mean(columns: Dict[str, Sequence[float]]) -> np.ndarray:
    """The per-row mean of the columns whose name starts with ProtSSN, ProtSSN_ensemble itself excluded (the reference averages a
    previous run's ensemble column into the new one)."""
    cols = [np.asarray(v, dtype=np.float64) for k, v in columns.items() if k.startswith("ProtSSN") and k != "ProtSSN_ensemble"]
    if not cols:
        raise ValueError("no ProtSSN column to average")
    return np.mean(cols, axis=0)


def parse_model_name(name: str) -> Tuple[int, int]:
    try:
        k, h = name.split("_")
        k, h = int(k[1:]), int(h[1:])
    except ValueError:
        raise ValueError(f"--gnn_model_name {name!r}: expected k<k>_h<h>") from None
    if k not in KS:
        raise ValueError(f"Invalid k: {k}")
    if h not in HS:
        raise ValueError(f"Invalid h: {h}")
    return k, h


def check_yaml(cfg: dict) -> int:
    """The egnn block of src/config/egnn.yaml: what the released checkpoints use, anything else refused.  Returns n_layers."""
    for key, want in YAML_FIXED.items():
        if key in cfg and cfg[key] != want:
            raise ValueError(f"gnn_config {key} = {cfg[key]!r}: this path runs {want!r}, as the released checkpoints do")
    return int(cfg.get("n_layers", LAYERS))


# -- model -------------------------------------------------------------------------------------------------------------------
class ProtSSN(_lib.SideHandle):
    """One device-resident checkpoint (EGNN + head)."""

    PREFIX, NAME = "protssn", "ProtSSN "

    def __init__(self, blob: np.ndarray, node_in: int = NODE_IN, hidden: int = 512, layers: int = LAYERS, device: int = 0,
                 precision: str = "f16x3", edge_chunk: int = 0):
        if precision not in ("f16x3", "fp32"):
            raise ValueError(f"precision {precision!r}: ProtSSN runs in f16x3 or fp32")
        self.D, self.h = node_in, hidden
        self.config = ProtssnConfig(abi_version=_lib.ABI_VERSION, node_in=node_in, hidden=hidden, layers=layers, edge_attr_dim=EDGE_ATTR_DIM,
                                    precision=_lib.PRECISIONS[precision], edge_chunk=edge_chunk)
        self._create(self.config, blob, device)
        self.L = 0

    def set_graph(self, pos, centre, nb, edge_attr):
        p, c, n, ea = _lib.as_f32(pos), _lib.as_i32(centre), _lib.as_i32(nb), _lib.as_f32(edge_attr)
        if p.ndim != 2 or p.shape[1] != 3 or c.shape != n.shape or ea.shape != (c.size, EDGE_ATTR_DIM):
            raise ValueError(f"pos {p.shape}, centre {c.shape}, neighbour {n.shape}, edge_attr {ea.shape}: expected [L, 3], [E], [E], [E, 93]")
        _lib.check(_lib.load().pgmi_protssn_set_graph(self._h, _lib.ptr(p, _lib._f32p), p.shape[0], c.size, _lib.ptr(c, _lib._i32p),
                                                      _lib.ptr(n, _lib._i32p), _lib.ptr(ea, _lib._f32p)))
        self.L = p.shape[0]

    def forward(self, esm_rep, want_hidden: bool = False):
        """esm_rep [L, D] -> log-probabilities [L, 20] (and the node rows after the last layer)."""
        x = _lib.as_f32(esm_rep)
        if x.shape != (self.L, self.D):
            raise ValueError(f"esm_rep {x.shape}: expected [{self.L}, {self.D}]")
        lp = np.empty((self.L, 20), np.float32)
        hid = np.empty((self.L, self.D), np.float32) if want_hidden else None
        _lib.check(_lib.load().pgmi_protssn_forward(self._h, _lib.ptr(x, _lib._f32p), _lib.ptr(lp, _lib._f32p), _lib.ptr(hid, _lib._f32p)))
        return (lp, hid) if want_hidden else lp


def from_state_dict(sd, node_in: int = NODE_IN, hidden: int = 512, layers: int = LAYERS, **kw) -> ProtSSN:
    return ProtSSN(pack(sd, node_in, hidden, layers), node_in, hidden, layers, **kw)


def op_egnn_message(sd, node_in: int, hidden: int, pos, centre, nb, edge_attr, x, precision: str = "f16x3", edge_chunk: int = 0,
                    device: int = 0) -> np.ndarray:
    """One layer's aggregated messages m_i float32 [L, hidden] through pgmi_op_egnn_message; sd: a one-layer state dict."""
    blob = _lib.as_f32(pack(sd, node_in, hidden, 1))
    cfg = ProtssnConfig(abi_version=_lib.ABI_VERSION, node_in=node_in, hidden=hidden, layers=1, edge_attr_dim=EDGE_ATTR_DIM,
                        precision=_lib.PRECISIONS[precision], edge_chunk=edge_chunk)
    p, c, n, ea, xx = _lib.as_f32(pos), _lib.as_i32(centre), _lib.as_i32(nb), _lib.as_f32(edge_attr), _lib.as_f32(x)
    out = np.empty((p.shape[0], hidden), np.float32)
    f, i = _lib._f32p, _lib._i32p
    _lib.check(_lib.load().pgmi_op_egnn_message(device, C.byref(cfg), _lib.ptr(blob, f), blob.size, _lib.ptr(p, f), p.shape[0], c.size,
                                                _lib.ptr(c, i), _lib.ptr(n, i), _lib.ptr(ea, f), _lib.ptr(xx, f), _lib.ptr(out, f)))
    return out


def score_structure(models: Dict[str, Tuple[int, ProtSSN]], esm_rep: np.ndarray, n, ca, c, norms: Dict[int, Dict[str, np.ndarray]]):
    """{name: log-probabilities [L, 20]} of the checkpoints {name: (k, model)} on one structure; the graph of each k is built once."""
    graphs, out = {}, {}
    for name, (k, model) in models.items():
        if k not in graphs:
            graphs[k] = build_graph(n, ca, c, k, norms[k])
        model.set_graph(*graphs[k])
        out[name] = model.forward(esm_rep)
    return out
