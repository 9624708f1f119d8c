"""ESM-IF1 (esm_if1_gvp4_t16_142M_UR50) scoring on libpgmi (include/pgmi.h, arch PGMI_ARCH_ESMIF1).

Replaces proteingym/baselines/esm/compute_fitness_esm_if1.py.  The reference runs the whole GVP-Transformer -- GVP-GNN, 8 encoder layers,
8 decoder layers -- on every batch of mutants although every mutant of an assay is conditioned on the same backbone.  Here the backbone
is encoded ONCE per assay by the torch restatement below (Encoder: featuriser, k-NN graph, GVP-GNN, transformer layers; one forward of
L + 2 rows, float32 or float64, on any torch device), its output handed to pgmi_esmif1_set_memory, which caches every decoder layer's
key / value projections of it, and only the decoder (csrc/api_esmif1.hip on csrc/attention_prefix.hip) runs per mutant, packed without
pad rows.

The restatement needs neither torch_geometric nor biotite: message passing is an index_add over the kept edges, and the backbone is read
by read_backbone below.  File references are to proteingym/baselines/esm/esm/inverse_folding/ unless a path says otherwise.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib

# esm/data.py Alphabet.from_architecture("invariant_gvp"): 4 prepended specials, the 27 standard tokens, one <null_1> to reach a multiple of
# 8, then <mask>, <cath>, <af2>.  <cath> is prepended, nothing is appended.
STANDARD = "LAGVSERTIDPKQNFYMHWCXBUZO.-"
ALL_TOKS = ["<null_0>", "<pad>", "<eos>", "<unk>"] + list(STANDARD) + ["<null_1>", "<mask>", "<cath>", "<af2>"]
TOK = {t: i for i, t in enumerate(ALL_TOKS)}
PAD, UNK, MASK, CATH = TOK["<pad>"], TOK["<unk>"], TOK["<mask>"], TOK["<cath>"]
N_VOCAB = len(ALL_TOKS)                                  # 35

# pretrained.py:132-149: module names of the released checkpoint -> the open-source module names, applied in this order
RENAMES = (("W_v", "embed_graph.embed_node"), ("W_e", "embed_graph.embed_edge"), ("embed_scores.0", "embed_confidence"),
           ("embed_score.", "embed_graph.embed_confidence."), ("seq_logits_projection.", ""), ("embed_ingraham_features", "embed_dihedrals"),
           ("embed_gvp_in_local_frame.0", "embed_gvp_output"), ("embed_features_in_local_frame.0", "embed_gvp_input_features"))
# buffers of the reference's modules that hold no weight
IGNORED_SUFFIXES = ("embed_positions._float_tensor",)


def tokenize(seq: str) -> np.ndarray:
    """<cath> + one id per letter (a letter outside the alphabet: <unk>); int32 [len(seq) + 1]."""
    return np.array([CATH] + [TOK.get(c, UNK) for c in seq], dtype=np.int32)


# -- checkpoint ------------------------------------------------------------------------------------------------------------
def rename_key(name: str) -> str:
    for old, new in RENAMES:
        name = name.replace(old, new)
    return name


def rename_state_dict(sd) -> dict:
    return {rename_key(k): v for k, v in sd.items() if "version" not in k}


def config_from_args(args) -> dict:
    """Every width from the checkpoint's args (a Namespace or a dict); nothing is hard-coded."""
    a = dict(vars(args)) if not isinstance(args, dict) else dict(args)
    if "invariant_gvp" not in str(a.get("arch", "")):
        raise ValueError(f"not an ESM-IF1 checkpoint: arch {a.get('arch')!r}")
    cfg = dict(enc_dim=int(a["encoder_embed_dim"]), enc_layers=int(a["encoder_layers"]), enc_heads=int(a["encoder_attention_heads"]),
               enc_ffn=int(a["encoder_ffn_embed_dim"]),
               embed_dim=int(a["decoder_embed_dim"]), layers=int(a["decoder_layers"]), heads=int(a["decoder_attention_heads"]),
               ffn_dim=int(a["decoder_ffn_embed_dim"]),
               node_s=int(a["gvp_node_hidden_dim_scalar"]), node_v=int(a["gvp_node_hidden_dim_vector"]),
               edge_s=int(a["gvp_edge_hidden_dim_scalar"]), edge_v=int(a["gvp_edge_hidden_dim_vector"]),
               gvp_layers=int(a["gvp_num_encoder_layers"]), top_k=int(a["gvp_top_k_neighbors"]), vocab=N_VOCAB)
    return cfg


def _gvp_shapes(prefix: str, si: int, vi: int, so: int, vo: int, gate: bool) -> Dict[str, tuple]:
    """gvp_modules.py GVP(in_dims, out_dims): wh [h, vi], ws [so, h + si] + bias, wv [vo, h], (vector_gate) wg [vo, so] + bias."""
    h = max(vi, vo)
    out = {prefix + "wh.weight": (h, vi), prefix + "ws.weight": (so, h + si), prefix + "ws.bias": (so,), prefix + "wv.weight": (vo, h)}
    if gate:
        out[prefix + "wg.weight"] = (vo, so)
        out[prefix + "wg.bias"] = (vo,)
    return out


def _linear(prefix: str, n_out: int, n_in: int, bias: bool = True) -> Dict[str, tuple]:
    out = {prefix + ".weight": (n_out, n_in)}
    if bias:
        out[prefix + ".bias"] = (n_out,)
    return out


def _norm(prefix: str, n: int) -> Dict[str, tuple]:
    return {prefix + ".weight": (n,), prefix + ".bias": (n,)}


def _attention(prefix: str, D: int, kdim: int) -> Dict[str, tuple]:
    out = {}
    for name, n_in in (("k_proj", kdim), ("v_proj", kdim), ("q_proj", D), ("out_proj", D)):
        out.update(_linear(prefix + name, D, n_in))
    return out


def decoder_keys(cfg: dict) -> List[str]:
    """The decoder's weights in the order of the C ABI's blob (include/pgmi.h, ESM-IF1)."""
    keys = ["decoder.embed_tokens.weight"]
    for i in range(cfg["layers"]):
        p = f"decoder.layers.{i}."
        keys += [p + "self_attn_layer_norm.weight", p + "self_attn_layer_norm.bias"]
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            keys += [p + f"self_attn.{n}.weight", p + f"self_attn.{n}.bias"]
        keys += [p + "encoder_attn_layer_norm.weight", p + "encoder_attn_layer_norm.bias"]
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            keys += [p + f"encoder_attn.{n}.weight", p + f"encoder_attn.{n}.bias"]
        keys += [p + "final_layer_norm.weight", p + "final_layer_norm.bias", p + "fc1.weight", p + "fc1.bias", p + "fc2.weight", p + "fc2.bias"]
    return keys + ["decoder.layer_norm.weight", "decoder.layer_norm.bias", "decoder.output_projection.weight"]


def expected_shapes(cfg: dict) -> Dict[str, tuple]:
    """Every weight of GVPTransformerModel(args) with its shape, under the open-source names."""
    E, D, V = cfg["enc_dim"], cfg["embed_dim"], cfg["vocab"]
    ns, nv, es, ev = cfg["node_s"], cfg["node_v"], cfg["edge_s"], cfg["edge_v"]
    s: Dict[str, tuple] = {"encoder.embed_tokens.weight": (V, E)}
    s.update(_linear("encoder.embed_gvp_input_features", E, 15))
    s.update(_linear("encoder.embed_confidence", E, 16))
    s.update(_linear("encoder.embed_dihedrals.node_embedding", E, 6))
    s.update({"encoder.embed_dihedrals.norm_nodes.gain": (E,), "encoder.embed_dihedrals.norm_nodes.bias": (E,)})
    g = "encoder.gvp_encoder."
    s.update(_gvp_shapes(g + "embed_graph.embed_node.0.", 7, 3, ns, nv, False))
    s.update(_norm(g + "embed_graph.embed_node.1.scalar_norm", ns))
    s.update(_gvp_shapes(g + "embed_graph.embed_edge.0.", 34, 1, es, ev, False))
    s.update(_norm(g + "embed_graph.embed_edge.1.scalar_norm", es))
    s.update(_linear(g + "embed_graph.embed_confidence", ns, 16))
    for i in range(cfg["gvp_layers"]):
        p = g + f"encoder_layers.{i}."
        s.update(_gvp_shapes(p + "conv.message_func.0.", 2 * ns + es, 2 * nv + ev, ns, nv, True))
        s.update(_gvp_shapes(p + "conv.message_func.1.", ns, nv, ns, nv, True))
        s.update(_gvp_shapes(p + "conv.message_func.2.", ns, nv, ns, nv, False))
        s.update(_norm(p + "norm.0.scalar_norm", ns))
        s.update(_norm(p + "norm.1.scalar_norm", ns))
        s.update(_gvp_shapes(p + "ff_func.0.", ns, nv, 4 * ns, 2 * nv, True))
        s.update(_gvp_shapes(p + "ff_func.1.", 4 * ns, 2 * nv, ns, nv, False))
    s.update(_linear("encoder.embed_gvp_output", E, ns + 3 * nv))
    for i in range(cfg["enc_layers"]):
        p = f"encoder.layers.{i}."
        s.update(_attention(p + "self_attn.", E, E))
        s.update(_norm(p + "self_attn_layer_norm", E))
        s.update(_linear(p + "fc1", cfg["enc_ffn"], E))
        s.update(_linear(p + "fc2", E, cfg["enc_ffn"]))
        s.update(_norm(p + "final_layer_norm", E))
    s.update(_norm("encoder.layer_norm", E))
    s["decoder.embed_tokens.weight"] = (V, D)
    for i in range(cfg["layers"]):
        p = f"decoder.layers.{i}."
        s.update(_attention(p + "self_attn.", D, D))
        s.update(_norm(p + "self_attn_layer_norm", D))
        s.update(_attention(p + "encoder_attn.", D, E))
        s.update(_norm(p + "encoder_attn_layer_norm", D))
        s.update(_linear(p + "fc1", cfg["ffn_dim"], D))
        s.update(_linear(p + "fc2", D, cfg["ffn_dim"]))
        s.update(_norm(p + "final_layer_norm", D))
    s.update(_norm("decoder.layer_norm", D))
    s["decoder.output_projection.weight"] = (V, D)
    return s


def check_state_dict(cfg: dict, sd, where: str = "state dict") -> dict:
    """The renamed state dict without its weightless buffers; a missing key, an extra key or a wrong shape raises (load_state_dict's
    strict check, restated)."""
    sd = {k: v for k, v in sd.items() if not k.endswith(IGNORED_SUFFIXES)}
    want = expected_shapes(cfg)
    missing = sorted(set(want) - set(sd))
    extra = sorted(set(sd) - set(want))
    if missing:
        raise RuntimeError(f"Missing key(s) in ESM-IF1 {where}: {missing[:8]}{'...' if len(missing) > 8 else ''}")
    if extra:
        raise RuntimeError(f"Unexpected key(s) in ESM-IF1 {where}: {extra[:8]}{'...' if len(extra) > 8 else ''}")
    for k, shp in want.items():
        if tuple(sd[k].shape) != tuple(shp):
            raise RuntimeError(f"ESM-IF1 {where}: {k} has shape {tuple(sd[k].shape)}, the args give {tuple(shp)}")
    return sd


def _np(a) -> np.ndarray:
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.asarray(a)


def weight_count(cfg: dict) -> int:
    shp = expected_shapes(cfg)
    return int(sum(int(np.prod(shp[k])) for k in decoder_keys(cfg)))


def pack_decoder(cfg: dict, sd) -> np.ndarray:
    """The C ABI's blob: the decoder's weights, fp32, in decoder_keys' order."""
    blob = np.empty(weight_count(cfg), dtype=np.float32)
    o = 0
    for k in decoder_keys(cfg):
        a = _np(sd[k]).astype(np.float32, copy=False)
        blob[o:o + a.size] = a.ravel()
        o += a.size
    assert o == blob.size
    return blob


def load_checkpoint(path: str) -> Tuple[dict, dict]:
    """A checkpoint {"args": Namespace(arch="...invariant_gvp..."), "model": state_dict} -> (cfg, checked state dict, renamed)."""
    import torch
    try:
        ckpt = torch.load(path, map_location="cpu", weights_only=True)
    except Exception:                # the args are an argparse.Namespace
        ckpt = torch.load(path, map_location="cpu", weights_only=False)
    cfg = config_from_args(ckpt["args"])
    return cfg, check_state_dict(cfg, rename_state_dict(ckpt["model"]), where=os.path.basename(path))


# -- backbone --------------------------------------------------------------------------------------------------------------
BACKBONE = ("N", "CA", "C")


def read_backbone(path_or_lines, chain: Optional[str] = "A") -> Tuple[np.ndarray, str]:
    """util.py load_coords restated for PDB files: model 1, the ATOM records of `chain` (None: every chain) named N, CA or C
    (biotite's filter_backbone: amino-acid residues, no hetero atoms), one row per residue in file order, NaN for an atom the residue
    lacks.  Returns (coords float32 [L, 3, 3], the residues' one-letter sequence).  The PDB parsing is esm3.read_pdb's."""
    from .esm3 import THREE_TO_ONE
    if isinstance(path_or_lines, (str, os.PathLike)):
        if str(path_or_lines).endswith("cif"):
            raise ValueError("mmCIF structures are not supported: convert to PDB")
        with open(path_or_lines) as f:
            lines = f.read().splitlines()
    else:
        lines = list(path_or_lines)
    residues, key, chains = [], None, set()
    for line in lines:
        rec = line[:6]
        if rec.startswith("ENDMDL"):
            break
        if rec != "ATOM  ":
            continue
        ch, name = line[21], line[12:16].strip()
        chains.add(ch)
        if (chain is not None and ch != chain) or name not in BACKBONE:
            continue
        k = (ch, int(line[22:26]), line[26], line[17:20].strip())
        if k != key:
            residues.append((k[3], {}))
            key = k
        atoms = residues[-1][1]
        if name in atoms:                              # a further alternate location of an atom already read: the first one stands
            continue
        atoms[name] = (float(line[30:38]), float(line[38:46]), float(line[46:54]))
    if not chains:
        raise ValueError("No chains found in the input file.")
    if chain is not None and chain not in chains:
        raise ValueError(f"Chain {chain} not found in input file")
    coords = np.full((len(residues), 3, 3), np.nan, dtype=np.float32)
    for i, (_, atoms) in enumerate(residues):
        for j, name in enumerate(BACKBONE):
            if name in atoms:
                coords[i, j] = atoms[name]
    return coords, "".join(THREE_TO_ONE.get(r, "X") for r, _ in residues)


# -- encoder ---------------------------------------------------------------------------------------------------------------
def _nan_to_num(t):
    import torch
    return torch.where(torch.isfinite(t), t, torch.zeros((), dtype=t.dtype, device=t.device))


def _norm_eps(t, dim=-1, keepdim=False, eps=1e-8):
    import torch
    return torch.sqrt((t * t).sum(dim, keepdim=keepdim) + eps)


def _unit(t):
    """util.py normalize: t / sqrt(|t|^2 + 1e-8), non-finite -> 0."""
    return _nan_to_num(t / _norm_eps(t, keepdim=True))


def _rbf(values, v_min, v_max, n_bins=16):
    import torch
    centers = torch.linspace(v_min, v_max, n_bins, device=values.device, dtype=values.dtype)
    z = (values.unsqueeze(-1) - centers) / ((v_max - v_min) / n_bins)
    return torch.exp(-z ** 2)


def _dihedral_angles(X, unit):
    """The three backbone dihedrals per residue from the 3 L atoms in chain order, phi[0] / psi[-1] / omega[-1] zero; [L, 3]."""
    import torch
    X = X.reshape(-1, 3)
    U = unit(X[1:] - X[:-1])
    u2, u1, u0 = U[:-2], U[1:-1], U[2:]
    n2, n1 = unit(torch.cross(u2, u1, dim=-1)), unit(torch.cross(u1, u0, dim=-1))
    cosD = torch.clamp((n2 * n1).sum(-1), -1 + 1e-7, 1 - 1e-7)
    D = torch.sign((u2 * n1).sum(-1)) * torch.acos(cosD)
    return torch.nn.functional.pad(D, [1, 2]).reshape(-1, 3)


def _sinusoid(positions, dim, padding_idx):
    """esm/modules.py SinusoidalPositionalEmbedding: float32 table (sin | cos halves) indexed by positions; the padding row is zero."""
    import torch
    n = int(positions.max()) + 1
    half = dim // 2
    f = torch.exp(torch.arange(half, dtype=torch.float) * -(math.log(10000) / (half - 1)))
    a = torch.arange(n, dtype=torch.float).unsqueeze(1) * f.unsqueeze(0)
    tab = torch.cat([torch.sin(a), torch.cos(a)], dim=1)
    if dim % 2:
        tab = torch.cat([tab, torch.zeros(n, 1)], dim=1)
    if padding_idx < n:
        tab[padding_idx] = 0
    return tab[positions.cpu()]


class Encoder:
    """GVPTransformerEncoder.forward for ONE backbone, restated on plain tensors (gvp_transformer_encoder.py, gvp_encoder.py, features.py,
    gvp_modules.py, gvp_utils.py, transformer_layer.py, util.py CoordBatchConverter).  encode(coords [L, 3, 3]) returns the encoder output
    [S, D_enc] with S = L + 2 (the converter pads one all-inf residue at each end) less the rows whose N is NaN (the reference's padding
    mask: they are masked keys there, and dropping a masked key from the memory is the same softmax)."""

    def __init__(self, cfg: dict, sd, device="cpu", dtype=None):
        import torch
        self.cfg = cfg
        self.device = torch.device(device)
        self.dtype = dtype or torch.float32
        self.w = {k: torch.as_tensor(_np(v)).to(self.device, self.dtype) for k, v in sd.items() if k.startswith("encoder.")}

    # gvp_modules.py ---------------------------------------------------------------------------------------------------
    def _lin(self, name, x):
        import torch
        return torch.nn.functional.linear(x, self.w[name + ".weight"], self.w.get(name + ".bias"))

    def _gvp(self, p, s, v, act: bool, gate: bool):
        """GVP.forward with vectors in: vh = wh over the channels, s' = ws([s | |vh|]); v' = wv(vh), gated by sigmoid(wg(s')) when the
        layer has activations and a gate, by sigmoid(|v'|) when it has activations only, not at all without activations."""
        import torch
        vh = torch.nn.functional.linear(v.transpose(-1, -2), self.w[p + "wh.weight"])            # [n, 3, h]
        vn = _norm_eps(vh, dim=-2)
        s = self._lin(p + "ws", torch.cat([s, vn], -1))
        if act:
            s = torch.relu(s)
        v = torch.nn.functional.linear(vh, self.w[p + "wv.weight"]).transpose(-1, -2)             # [n, vo, 3]
        if act:
            g = self._lin(p + "wg", s).unsqueeze(-1) if gate else _norm_eps(v, dim=-1, keepdim=True)
            v = v * torch.sigmoid(g)
        return s, v

    def _tuple_norm(self, p, s, v, eps=1e-4):
        """LayerNorm on (s, V): nn.LayerNorm on s; the vectors divided by the root mean squared norm over the channels whose squared norm
        (+ eps) exceeds 2 eps, the others zeroed."""
        import torch
        s = torch.nn.functional.layer_norm(s, s.shape[-1:], self.w[p + "scalar_norm.weight"], self.w[p + "scalar_norm.bias"])
        vn = (v * v).sum(-1, keepdim=True) + eps
        nz = vn > 2 * eps
        vn = (vn * nz).sum(-2, keepdim=True) / (eps + nz.sum(-2, keepdim=True).to(v.dtype))
        return s, nz * (v / torch.sqrt(vn + eps))

    # features.py ------------------------------------------------------------------------------------------------------
    @staticmethod
    def _node_features(coords):
        """GVPInputFeaturizer.get_node_features without the coord-mask column: (cos | sin of the dihedrals [S, 6], forward / backward CA
        directions and the virtual side-chain direction [S, 3, 3])."""
        import torch
        D = _dihedral_angles(coords, _unit)
        scalars = torch.cat([torch.cos(D), torch.sin(D)], -1)
        ca = coords[:, 1]
        zero = torch.zeros(1, 3, dtype=coords.dtype, device=coords.device)
        fwd = torch.cat([_unit(ca[1:] - ca[:-1]), zero])
        bwd = torch.cat([zero, _unit(ca[:-1] - ca[1:])])
        c, n = _unit(coords[:, 2] - ca), _unit(coords[:, 0] - ca)
        side = -_unit(c + n) * math.sqrt(1 / 3) - _unit(torch.cross(c, n, dim=-1)) * math.sqrt(2 / 3)
        return scalars, torch.stack([fwd, bwd, side], dim=-2)

    def graph(self, coords, coord_mask, padding_mask):
        """get_edge_features + flatten_graph: the k nearest neighbours (self included) of every residue by CA distance, residues without
        coordinates ranked behind by sequence distance; every edge with an end that lacks coordinates or is padding is dropped.
        Returns (node [E], neighbour [E], distance [E]) of the kept edges: edge_index[0] is the node, edge_index[1] its neighbour."""
        import torch
        ca = coords[:, 1]
        S = ca.shape[0]
        m2 = coord_mask[:, None] & coord_mask[None, :]
        r2 = (~padding_mask)[:, None] & (~padding_mask)[None, :]
        D = m2 * _norm_eps(ca[None, :, :] - ca[:, None, :], dim=-1)
        pos = torch.arange(S, device=ca.device)
        dseq = (pos[:, None] - pos[None, :]).abs()
        adj = _nan_to_num(D) + (~m2) * (1e8 + dseq * 1e6) + (~r2) * 1e10
        k = min(self.cfg["top_k"], S) if self.cfg["top_k"] != -1 else S
        dist, nb = torch.topk(adj, k, dim=-1, largest=False)
        keep = (dist < 5e7).reshape(-1)
        node = pos[:, None].expand(S, k).reshape(-1)
        return node[keep], nb.reshape(-1)[keep], dist.reshape(-1)[keep]

    def _edge_features(self, coords, node, nb, dist):
        """34 scalars (16 distance RBFs over [0, 20], cos | sin of (node - neighbour) at 8 frequencies, two missing-coordinate flags that
        are zero on every kept edge) and one unit vector node - neighbour per kept edge."""
        import torch
        f = torch.exp(torch.arange(0, 16, 2, dtype=torch.float32, device=coords.device) * -(np.log(10000.0) / 16))
        ang = (node - nb).unsqueeze(-1) * f
        s = torch.cat([_rbf(dist, 0., 20.), torch.cos(ang), torch.sin(ang)], -1).to(coords.dtype)
        ca = coords[:, 1]
        v = _unit(ca[node] - ca[nb]).unsqueeze(-2)
        s = torch.cat([_nan_to_num(s), torch.zeros(s.shape[0], 2, dtype=s.dtype, device=s.device)], -1)
        return s, _nan_to_num(v)

    def message(self, p, s, v, es, ev, node, nb):
        """GVPConv with aggr="mean" under MessagePassing's default flow: the message of edge (node, neighbour) is built from
        (x[node], edge, x[neighbour]) and averaged AT THE NEIGHBOUR; a residue no neighbour list contains receives zeros."""
        import torch
        ms, mv = torch.cat([s[node], es, s[nb]], -1), torch.cat([v[node], ev, v[nb]], -2)
        ms, mv = self._gvp(p + "message_func.0.", ms, mv, True, True)
        ms, mv = self._gvp(p + "message_func.1.", ms, mv, True, True)
        ms, mv = self._gvp(p + "message_func.2.", ms, mv, False, False)
        n = s.shape[0]
        count = torch.zeros(n, dtype=s.dtype, device=s.device).index_add_(0, nb, torch.ones_like(nb, dtype=s.dtype)).clamp(min=1)
        out_s = torch.zeros(n, ms.shape[-1], dtype=s.dtype, device=s.device).index_add_(0, nb, ms) / count[:, None]
        out_v = torch.zeros(n, mv.shape[-2], 3, dtype=s.dtype, device=s.device).index_add_(0, nb, mv) / count[:, None, None]
        return out_s, out_v

    def gvp_encoder(self, coords, coord_mask, padding_mask, confidence):
        import torch
        g = "encoder.gvp_encoder."
        scalars, vectors = self._node_features(coords)
        s, v = self._gvp(g + "embed_graph.embed_node.0.", torch.cat([scalars, coord_mask.to(coords.dtype).unsqueeze(-1)], -1), vectors, False, False)
        s, v = self._tuple_norm(g + "embed_graph.embed_node.1.", s, v)
        s = s + self._lin(g + "embed_graph.embed_confidence", _rbf(confidence, 0., 1.))
        node, nb, dist = self.graph(coords, coord_mask, padding_mask)
        es, ev = self._edge_features(coords, node, nb, dist)
        es, ev = self._gvp(g + "embed_graph.embed_edge.0.", es, ev, False, False)
        es, ev = self._tuple_norm(g + "embed_graph.embed_edge.1.", es, ev)
        for i in range(self.cfg["gvp_layers"]):
            p = g + f"encoder_layers.{i}."
            ds, dv = self.message(p + "conv.", s, v, es, ev, node, nb)
            s, v = self._tuple_norm(p + "norm.0.", s + ds, v + dv)
            ds, dv = self._gvp(p + "ff_func.0.", s, v, True, True)
            ds, dv = self._gvp(p + "ff_func.1.", ds, dv, False, False)
            s, v = self._tuple_norm(p + "norm.1.", s + ds, v + dv)
        return s, v

    # gvp_transformer_encoder.py ----------------------------------------------------------------------------------------
    def embed(self, coords_in, confidence, padding_mask):
        import torch
        E = self.cfg["enc_dim"]
        coord_mask = torch.isfinite(coords_in).all(-1).all(-1)
        coords = _nan_to_num(coords_in)
        mask_tokens = torch.where(padding_mask, PAD, MASK)
        x = self.w["encoder.embed_tokens.weight"][mask_tokens] * math.sqrt(E)
        # DihedralFeatures: F.normalize (x / max(|x|, 1e-12)), Linear, then its own Normalize: unbiased variance, (sigma + eps) below
        h = self._lin("encoder.embed_dihedrals.node_embedding",
                      (lambda D: torch.cat([torch.cos(D), torch.sin(D)], -1))(_dihedral_angles(coords, lambda t: torch.nn.functional.normalize(t, dim=-1))))
        mu, sigma = h.mean(-1, keepdim=True), torch.sqrt(h.var(-1, keepdim=True) + 1e-6)
        x = x + self.w["encoder.embed_dihedrals.norm_nodes.gain"] * (h - mu) / (sigma + 1e-6) + self.w["encoder.embed_dihedrals.norm_nodes.bias"]
        s, v = self.gvp_encoder(coords, coord_mask, padding_mask, confidence)
        # the local frame of every residue (util.py get_rotation_frames): rows e1 = C - CA, e2 = N - CA orthogonalised, e3 = e1 x e2;
        # rotate(v, R^T) = v R^T
        e1 = _unit(coords[:, 2] - coords[:, 1])
        v2 = coords[:, 0] - coords[:, 1]
        e2 = _unit(v2 - e1 * (e1 * v2).sum(-1, keepdim=True))
        R = torch.stack([e1, e2, torch.cross(e1, e2, dim=-1)], dim=-2)
        Rt = R.transpose(-2, -1)
        x = x + self._lin("encoder.embed_gvp_output", torch.cat([s, (v @ Rt).flatten(-2, -1)], -1))
        x = x + self._lin("encoder.embed_confidence", _rbf(confidence, 0., 1.))
        scalars, vectors = self._node_features(coords)
        x = x + self._lin("encoder.embed_gvp_input_features", torch.cat([scalars, (vectors @ Rt).flatten(-2, -1)], -1))
        positions = torch.where(padding_mask, PAD, torch.arange(x.shape[0], device=x.device) + PAD + 1)
        x = x + _sinusoid(positions, E, PAD).to(x.device, x.dtype)
        return x * (~padding_mask).to(x.dtype).unsqueeze(-1)

    def _attention(self, p, x, key_padding_mask):
        import torch
        H = self.cfg["enc_heads"]
        S, E = x.shape
        dh = E // H
        q = (self._lin(p + "q_proj", x) * dh ** -0.5).reshape(S, H, dh).transpose(0, 1)
        k = self._lin(p + "k_proj", x).reshape(S, H, dh).transpose(0, 1)
        v = self._lin(p + "v_proj", x).reshape(S, H, dh).transpose(0, 1)
        a = q @ k.transpose(-1, -2)
        a = a.masked_fill(key_padding_mask[None, None, :], float("-inf"))
        a = torch.softmax(a, dim=-1)
        return self._lin(p + "out_proj", (a @ v).transpose(0, 1).reshape(S, E))

    def encode(self, coords) -> np.ndarray:
        """coords [L, 3, 3] (N, CA, C; NaN where an atom is missing) -> encoder output, float64 numpy [S', D_enc]."""
        import torch
        with torch.no_grad():
            c = torch.as_tensor(np.asarray(coords, dtype=np.float32))
            c = torch.nn.functional.pad(c, (0, 0, 0, 0, 1, 1), value=float("inf")).to(self.device)
            # CoordBatchConverter: confidence 1 on residues whose atoms are all finite, 0 elsewhere, -1 on padding rows (N = NaN)
            padding_mask = torch.isnan(c[:, 0, 0])
            coord_mask = torch.isfinite(c.sum(-2).sum(-1))
            confidence = torch.ones(c.shape[0], device=self.device, dtype=self.dtype) * coord_mask + (-1.) * padding_mask
            x = self.embed(c.to(self.dtype), confidence, padding_mask)
            F = torch.nn.functional
            for i in range(self.cfg["enc_layers"]):
                p = f"encoder.layers.{i}."
                h = F.layer_norm(x, x.shape[-1:], self.w[p + "self_attn_layer_norm.weight"], self.w[p + "self_attn_layer_norm.bias"])
                x = x + self._attention(p + "self_attn.", h, padding_mask)
                h = F.layer_norm(x, x.shape[-1:], self.w[p + "final_layer_norm.weight"], self.w[p + "final_layer_norm.bias"])
                x = x + self._lin(p + "fc2", torch.relu(self._lin(p + "fc1", h)))
            x = F.layer_norm(x, x.shape[-1:], self.w["encoder.layer_norm.weight"], self.w["encoder.layer_norm.bias"])
            return x[~padding_mask].double().cpu().numpy()


# -- model -----------------------------------------------------------------------------------------------------------------
class EsmIf1Decoder(_lib.ModelHandle):
    """Device-resident ESM-IF1 decoder (f16x3).  max_memory: the largest encoder memory in rows (residues + 2)."""
    CREATE = "pgmi_esmif1_model_create"

    def __init__(self, cfg: dict, weights: np.ndarray, device: int = 0, max_rows: int = 0, max_memory: int = 1026):
        super().__init__(cfg, weights, device, max_rows, arch_arg=int(cfg["enc_dim"]), arch=_lib.ARCH_ESMIF1, vocab=cfg["vocab"],
                         max_positions=int(max_memory))
        self.memory_rows = 0

    @staticmethod
    def _weight_count(lib, c, arch_arg):
        return lib.pgmi_esmif1_weight_count(C.byref(c), arch_arg)

    def set_memory(self, enc_out: np.ndarray):
        e = _lib.as_f32(enc_out)
        if e.ndim != 2 or e.shape[1] != self.cfg["enc_dim"]:
            raise ValueError(f"encoder output must be [S, {self.cfg['enc_dim']}], got {e.shape}")
        self.memory_rows = 0
        _lib.check(_lib.load().pgmi_esmif1_set_memory(self._h, _lib.ptr(e, _lib._f32p), e.shape[0]))
        self.memory_rows = e.shape[0]

    @staticmethod
    def _pad(seqs: Sequence[np.ndarray]):
        lens = _lib.as_i32([len(v) for v in seqs])
        t = np.full((len(seqs), int(lens.max())), PAD, dtype=np.int32)
        for i, v in enumerate(seqs):
            t[i, :len(v)] = v
        return t, lens

    def token_logprobs(self, seqs: Sequence[np.ndarray]) -> np.ndarray:
        """seqs: token arrays (tokenize); out [B, T, V], row (b, t) = log p(. | memory, seqs[b][:t + 1]); NaN beyond a sequence."""
        t, lens = self._pad(seqs)
        out = np.empty(t.shape + (self.cfg["vocab"],), dtype=np.float32)
        _lib.check(_lib.load().pgmi_esmif1_token_logprobs(self._h, _lib.ptr(t, _lib._i32p), _lib.ptr(lens, _lib._i32p), t.shape[0], t.shape[1],
                                                          _lib.ptr(out, _lib._f32p)))
        return out

    def sequence_loglik(self, seqs: Sequence[np.ndarray]) -> np.ndarray:
        """float64 [B]: the mean log-probability of every sequence's residues = the reference's -mean(cross_entropy)."""
        t, lens = self._pad(seqs)
        out = np.empty(t.shape[0], dtype=np.float64)
        _lib.check(_lib.load().pgmi_esmif1_sequence_loglik(self._h, _lib.ptr(t, _lib._i32p), _lib.ptr(lens, _lib._i32p), t.shape[0], t.shape[1],
                                                           _lib.ptr(out, _lib._f64p)))
        return out


class EsmIf1Model:
    """Encoder (torch, once per structure) + decoder (libpgmi).  encoder_device: a torch device for the one encoder forward (default: the
    GPU the decoder runs on); the decoder always runs in HIP on `device`.  The encoder is created first: in a process that uses both,
    torch's HIP runtime has to be initialised before libpgmi's, or torch finds no device."""

    def __init__(self, cfg: dict, sd, device: int = 0, max_rows: int = 0, max_memory: int = 1026, encoder_device=None, encoder_dtype=None):
        self.cfg = cfg
        self.encoder = Encoder(cfg, sd, device=encoder_device if encoder_device is not None else f"cuda:{device}", dtype=encoder_dtype)
        self.decoder = EsmIf1Decoder(cfg, pack_decoder(cfg, sd), device=device, max_rows=max_rows, max_memory=max_memory)

    def set_structure(self, coords: np.ndarray) -> np.ndarray:
        enc = self.encoder.encode(coords)
        self.decoder.set_memory(enc)
        return enc

    def score(self, seqs: Sequence[str], max_batch: int = 4096) -> np.ndarray:
        """esmif1_ll of every sequence given the structure last set, float64: sequences sorted by length and handed over in batches; the
        library chunks a batch to its row budget.  Neither changes a sequence's bits."""
        toks = [tokenize(s) for s in seqs]
        order = np.argsort([len(t) for t in toks], kind="stable")
        out = np.empty(len(toks), dtype=np.float64)
        for b0 in range(0, len(order), max_batch):
            idx = order[b0:b0 + max_batch]
            out[idx] = self.decoder.sequence_loglik([toks[i] for i in idx])
        return out

    def close(self):
        self.decoder.close()


def from_checkpoint(path: str, device: int = 0, max_rows: int = 0, max_memory: int = 1026, encoder_device=None) -> EsmIf1Model:
    cfg, sd = load_checkpoint(path)
    return EsmIf1Model(cfg, sd, device=device, max_rows=max_rows, max_memory=max_memory, encoder_device=encoder_device)
