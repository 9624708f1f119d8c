"""ProSST structure tokens on libpgmi (include/pgmi.h, ProSST section).

Replaces the model side of proteingym/baselines/prosst/prosst/structure/quantizer.py (venusrem/structure is the same code): one local
subgraph per residue (at most 40 residues within 10 A), each through the six-layer GVP-GNN of ``AutoGraphEncoder`` at node (256, 32) /
edge (64, 2), mean-pooled, L2-normalised and assigned to the nearest of K k-means centres.  The checkpoint (``AE.pt``) is packed into a
blob and run in HIP (csrc/api_prosst.hip); every requested codebook is assigned from one encoder pass.  What this writes is what
``compute_fitness.py`` of ProSST and VenusREM reads as ``structure_sequence/<K>/<name>.fasta``.  The ProSST transformer is not
computed here: its model code is not in the reference tree (it is loaded from the hub with ``trust_remote_code``).  Nothing is
downloaded.

Read from the reference, not run (Bio, torch_geometric, torch_scatter, biotite, pathos are stand-ins here): ``read_backbone`` (Bio's
PDBParser and seq1), the graph rules (scipy's float64 distance matrix, numpy's argsort), ``scatter_mean`` and ``KMeans.predict``.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib

NODE_IN, NODE_H, EDGE_IN, EDGE_H, LAYERS = (20, 3), (256, 32), (32, 1), (64, 2), 6
RADIUS, MAX_NODES, THRESHOLD, DEPTH = 10.0, 40, 30, 50
VOCAB_SIZES = (20, 64, 128, 512, 1024, 2048, 4096)        # PdbQuantizer's assertion
MAX_L = 8192
BACKBONE = ("N", "CA", "C", "O")
THREE_TO_ONE = {"ALA": "A", "ARG": "R", "ASN": "N", "ASP": "D", "CYS": "C", "GLN": "Q", "GLU": "E", "GLY": "G", "HIS": "H", "ILE": "I",
                "LEU": "L", "LYS": "K", "MET": "M", "PHE": "F", "PRO": "P", "SER": "S", "THR": "T", "TRP": "W", "TYR": "Y", "VAL": "V"}


class ProsstConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("abi_version", "node_s", "node_v", "edge_s", "edge_v", "layers", "max_nodes", "threshold")] + \
               [("radius", C.c_float)]


def make_config(layers: int = LAYERS, radius: float = RADIUS, max_nodes: int = MAX_NODES, threshold: int = THRESHOLD,
                node_h: Tuple[int, int] = NODE_H, edge_h: Tuple[int, int] = EDGE_H) -> ProsstConfig:
    return ProsstConfig(abi_version=_lib.ABI_VERSION, node_s=node_h[0], node_v=node_h[1], edge_s=edge_h[0], edge_v=edge_h[1], layers=layers,
                        max_nodes=max_nodes, threshold=threshold, radius=radius)


# -- checkpoint --------------------------------------------------------------------------------------------------------------
def _gvp_shapes(prefix: str, si: int, vi: int, so: int, vo: int) -> List[Tuple[str, Tuple[int, ...]]]:
    """A GVP's tensors in blob order.  h = max(vi, vo) (layer.py GVP.__init__); vector_gate is False: no wsv."""
    h = max(vi, vo)
    out = [(prefix + "wh.weight", (h, vi)), (prefix + "ws.weight", (so, si + h)), (prefix + "ws.bias", (so,))]
    if vo:
        out.append((prefix + "wv.weight", (vo, h)))
    return out


def key_shapes(layers: int = LAYERS) -> List[Tuple[str, Tuple[int, ...]]]:
    """(key of AutoGraphEncoder's state dict, shape) in blob order (include/pgmi.h)."""
    ns, nv = NODE_H
    es, ev = EDGE_H
    out = [("W_v.0.scalar_norm.weight", (NODE_IN[0],)), ("W_v.0.scalar_norm.bias", (NODE_IN[0],))]
    out += _gvp_shapes("W_v.1.", *NODE_IN, ns, nv)
    out += [("W_e.0.scalar_norm.weight", (EDGE_IN[0],)), ("W_e.0.scalar_norm.bias", (EDGE_IN[0],))]
    out += _gvp_shapes("W_e.1.", *EDGE_IN, es, ev)
    for l in range(layers):
        q = f"layers.{l}."
        out += _gvp_shapes(q + "conv.message_func.0.", 2 * ns + es, 2 * nv + ev, ns, nv)
        out += _gvp_shapes(q + "conv.message_func.1.", ns, nv, ns, nv)
        out += _gvp_shapes(q + "conv.message_func.2.", ns, nv, ns, nv)
        for n in (0, 1):
            out += [(f"{q}norm.{n}.scalar_norm.weight", (ns,)), (f"{q}norm.{n}.scalar_norm.bias", (ns,))]
        out += _gvp_shapes(q + "ff_func.0.", ns, nv, 4 * ns, 2 * nv)
        out += _gvp_shapes(q + "ff_func.1.", 4 * ns, 2 * nv, ns, nv)
    out += [("W_out.0.scalar_norm.weight", (ns,)), ("W_out.0.scalar_norm.bias", (ns,))]
    return out + _gvp_shapes("W_out.1.", ns, nv, ns, 0)


def _ignored(key: str) -> bool:
    """The training head (``dense.*``) and the empty ``dummy_param`` of every GVP and vector dropout."""
    return key.startswith("dense.") or key.endswith("dummy_param")


def _to_np(t) -> np.ndarray:
    return t.detach().to("cpu").float().numpy() if hasattr(t, "detach") else np.asarray(t, dtype=np.float32)


def pack(sd, layers: int = LAYERS) -> np.ndarray:
    """The blob of an AutoGraphEncoder state dict.  Anything missing, unexpected or of another shape is an error."""
    want = key_shapes(layers)
    names = {k for k, _ in want}
    missing = sorted(k for k in names if k not in sd)
    unexpected = sorted(k for k in sd if k not in names and not _ignored(k))
    if missing or unexpected:
        raise ValueError(f"not a ProSST AutoGraphEncoder state dict: missing {missing[:5]}, unexpected {unexpected[:5]}")
    for k, shape in want:
        if tuple(np.shape(sd[k])) != shape:
            raise ValueError(f"{k}: shape {tuple(np.shape(sd[k]))}, this path needs {shape}")
    return np.concatenate([_to_np(sd[k]).ravel() for k, _ in want]).astype(np.float32)


def random_state_dict(seed: int, layers: int = LAYERS) -> Dict[str, np.ndarray]:
    """A seeded state dict (tests, benchmarks): Linear weights N(0, 1 / fan_in), LayerNorm gains near 1, plus the keys a real checkpoint
    carries and this path ignores."""
    rng = np.random.default_rng(seed)
    sd: Dict[str, np.ndarray] = {}
    for k, shape in key_shapes(layers):
        if "scalar_norm.weight" in k:
            a = 1.0 + 0.1 * rng.standard_normal(shape)
        elif k.endswith("bias"):
            a = 0.1 * rng.standard_normal(shape)
        else:
            a = rng.standard_normal(shape) / np.sqrt(shape[-1])
        sd[k] = a.astype(np.float32)
    sd["W_v.1.dummy_param"] = np.zeros(0, np.float32)
    sd["layers.0.dropout.0.vdropout.dummy_param"] = np.zeros(0, np.float32)
    sd["dense.0.weight"] = np.zeros((2 * NODE_H[0], NODE_H[0]), np.float32)
    sd["dense.0.bias"] = np.zeros(2 * NODE_H[0], np.float32)
    return sd


def load_checkpoint(path: str):
    """torch.load(path) of a local AE.pt, as PdbQuantizer.__init__ reads it."""
    import torch
    if not os.path.isfile(path):
        raise FileNotFoundError(f"{path}: no such checkpoint (this path never downloads)")
    return dict(torch.load(path, map_location="cpu", weights_only=True))


# -- codebooks ---------------------------------------------------------------------------------------------------------------
def read_codebook(path: str) -> np.ndarray:
    """Centres float32 [K, 256] of ``<K>.joblib`` (a fitted sklearn KMeans: its ``cluster_centers_``; needs joblib and sklearn) or of
    a ``.npy`` array."""
    if not os.path.isfile(path):
        raise FileNotFoundError(f"{path}: no such codebook (this path never downloads)")
    if path.endswith(".npy"):
        c = np.load(path, allow_pickle=False)
    elif path.endswith(".joblib"):
        try:
            import joblib
            import sklearn  # noqa: F401  the pickled object is a sklearn KMeans
        except ImportError as e:
            raise ImportError(f"{path}: reading a .joblib codebook needs joblib and scikit-learn ({e}); "
                              "save cluster_centers_ as .npy instead") from e
        c = joblib.load(path).cluster_centers_
    else:
        raise ValueError(f"{path}: a codebook is a .joblib KMeans or a .npy array")
    c = np.asarray(c)
    if c.ndim != 2 or c.shape[1] != NODE_H[0] or c.shape[0] < 1:
        raise ValueError(f"{path}: centres of shape {c.shape}, expected [K, {NODE_H[0]}]")
    if not np.isfinite(c).all():
        raise ValueError(f"{path}: a centre is not finite")
    return np.ascontiguousarray(c, dtype=np.float32)


def find_codebook(cluster_dir: str, K: int) -> str:
    for ext in (".joblib", ".npy"):
        p = os.path.join(cluster_dir, f"{K}{ext}")
        if os.path.isfile(p):
            return p
    raise FileNotFoundError(f"{cluster_dir}: neither {K}.joblib nor {K}.npy (this path never downloads)")


# -- PDB ---------------------------------------------------------------------------------------------------------------------
def read_backbone(path_or_lines) -> Tuple[str, np.ndarray]:
    """generate_graph's reading of a PDB file: the residues with a blank hetero flag (ATOM records), their N, CA, C, O as float32
    [L, 4, 3] and seq1 of their names (an unknown name is 'X').  Fixed columns, as s2f.read_ca and esmif1.read_backbone read them.
    Where this differs from Bio's PDBParser: Bio iterates every model and chain; this reads the first model (every chain, in file
    order), the project's precedent.  The first alternate location of an atom stands (Bio keeps the one with the highest occupancy).
    A residue without one of the four atoms makes the reference fail with a KeyError; here the file is refused and the residue named."""
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
        if rec != "ATOM  ":
            continue
        k = (line[21], line[22:27], line[17:20].strip())
        if k != key:
            residues.append((k, {}))
            key = k
        atoms, name = residues[-1][1], line[12:16].strip()
        if name in BACKBONE and name not in atoms:
            atoms[name] = (float(line[30:38]), float(line[38:46]), float(line[46:54]))
    if not residues:
        raise ValueError("no residues (ATOM records) in the PDB file")
    X = np.empty((len(residues), 4, 3), dtype=np.float32)
    for i, ((ch, num, res), atoms) in enumerate(residues):
        for j, name in enumerate(BACKBONE):
            if name not in atoms:
                raise ValueError(f"residue {res} {ch.strip()}{num.strip()} has no {name} atom (the reference fails on it with KeyError '{name}')")
            X[i, j] = atoms[name]
    if len(residues) == 3:
        raise ValueError("3 residues: the reference's torch.cross without dim runs over the residue axis there, not over x, y, z")
    return "".join(THREE_TO_ONE.get(k[2], "X") for k, _ in residues), X


# -- model -------------------------------------------------------------------------------------------------------------------
class Quantizer(_lib.SideHandle):
    """Device-resident structure encoder: set_structure once per protein, embed once, assign per codebook."""

    PREFIX, NAME = "prosst", "ProSST "

    def __init__(self, blob: np.ndarray, layers: int = LAYERS, device: int = 0, radius: float = RADIUS, max_nodes: int = MAX_NODES,
                 threshold: int = THRESHOLD, node_h: Tuple[int, int] = NODE_H, edge_h: Tuple[int, int] = EDGE_H):
        self.config = make_config(layers, radius, max_nodes, threshold, node_h, edge_h)
        self._create(self.config, blob, device)
        self.L = 0

    def set_structure(self, X):
        x = _lib.as_f32(X)
        if x.ndim != 3 or x.shape[1:] != (4, 3):
            raise ValueError(f"X {x.shape}: expected [L, 4, 3] (N, CA, C, O)")
        self.L = 0
        _lib.check(_lib.load().pgmi_prosst_set_structure(self._h, _lib.ptr(x, _lib._f32p), x.shape[0]))
        self.L = x.shape[0]

    def subgraphs(self) -> dict:
        """The test view: edges [2, E], e_s [E, 64], e_v [E, 2, 3], node_off [L + 1], nodes [N], edge_off [L + 1], edge_gid [ES]."""
        lib = _lib.load()
        n = np.zeros(3, np.int64)
        _lib.check(lib.pgmi_prosst_subgraphs(self._h, _lib.ptr(n, _lib._i64p), None, None, None, None, None, None, None))
        E, N, ES = (int(v) for v in n)
        out = dict(edges=np.empty((2, E), np.int32), e_s=np.empty((E, EDGE_H[0]), np.float32), e_v=np.empty((E, EDGE_H[1], 3), np.float32),
                   node_off=np.empty(self.L + 1, np.int32), nodes=np.empty(N, np.int32), edge_off=np.empty(self.L + 1, np.int32),
                   edge_gid=np.empty(ES, np.int32))
        _lib.check(lib.pgmi_prosst_subgraphs(self._h, None, _lib.ptr(out["edges"], _lib._i32p), _lib.ptr(out["e_s"], _lib._f32p),
                                             _lib.ptr(out["e_v"], _lib._f32p), _lib.ptr(out["node_off"], _lib._i32p),
                                             _lib.ptr(out["nodes"], _lib._i32p), _lib.ptr(out["edge_off"], _lib._i32p),
                                             _lib.ptr(out["edge_gid"], _lib._i32p)))
        return out

    def embed(self, want_pooled: bool = False, sub: Optional[int] = None, n_nodes: int = 0):
        """The normalised embeddings [L, 256]; with want_pooled also the means before the normalisation; with sub (and its node count)
        also (node_s [n, 256], node_v [n, 32, 3]) of that subgraph after the last layer."""
        out = np.empty((self.L, NODE_H[0]), np.float32)
        pooled = np.empty((self.L, NODE_H[0]), np.float32) if want_pooled else None
        ns = np.empty((n_nodes, NODE_H[0]), np.float32) if sub is not None else None
        nv = np.empty((n_nodes, NODE_H[1], 3), np.float32) if sub is not None else None
        _lib.check(_lib.load().pgmi_prosst_embed(self._h, _lib.ptr(out, _lib._f32p), _lib.ptr(pooled, _lib._f32p), -1 if sub is None else int(sub),
                                                 _lib.ptr(ns, _lib._f32p), _lib.ptr(nv, _lib._f32p)))
        res = (out,) + ((pooled,) if want_pooled else ()) + ((ns, nv) if sub is not None else ())
        return res if len(res) > 1 else out

    def assign(self, centres) -> np.ndarray:
        """Tokens int32 [L] of the last embed() against centres [K, 256]."""
        c = _lib.as_f32(centres)
        if c.ndim != 2 or c.shape[1] != NODE_H[0]:
            raise ValueError(f"centres {c.shape}: expected [K, {NODE_H[0]}]")
        tok = np.empty(self.L, np.int32)
        _lib.check(_lib.load().pgmi_prosst_assign(self._h, _lib.ptr(c, _lib._f32p), c.shape[0], _lib.ptr(tok, _lib._i32p)))
        return tok


def host_subgraphs(X, config: Optional[ProsstConfig] = None) -> dict:
    """The library's host graph pass alone (no device): edges [2, E], node_off [L + 1], nodes [N], edge_off [L + 1], edge_gid [ES] as
    Quantizer.subgraphs gives them, and what the kernels read: in_off [N + 1], in_gid [ES], in_src [ES] = per node copy its incoming
    subgraph edges in ascending source order as (global edge, copy of the source)."""
    lib = _lib.load()
    x = _lib.as_f32(X)
    if x.ndim != 3 or x.shape[1:] != (4, 3):
        raise ValueError(f"X {x.shape}: expected [L, 4, 3] (N, CA, C, O)")
    cfg = config or make_config()
    L, n = x.shape[0], np.zeros(3, np.int64)
    _lib.check(lib.pgmi_op_prosst_subgraphs(C.byref(cfg), _lib.ptr(x, _lib._f32p), L, _lib.ptr(n, _lib._i64p), *[None] * 8))
    E, N, ES = (int(v) for v in n)
    out = dict(edges=np.empty((2, E), np.int32), node_off=np.empty(L + 1, np.int32), nodes=np.empty(N, np.int32),
               edge_off=np.empty(L + 1, np.int32), edge_gid=np.empty(ES, np.int32), in_off=np.empty(N + 1, np.int32),
               in_gid=np.empty(ES, np.int32), in_src=np.empty(ES, np.int32))
    _lib.check(lib.pgmi_op_prosst_subgraphs(C.byref(cfg), _lib.ptr(x, _lib._f32p), L, None, *[_lib.ptr(a, _lib._i32p) for a in out.values()]))
    return out


def op_assign(emb, centres, device: int = 0) -> np.ndarray:
    """The assignment alone on pre-computed embeddings [n, 256]: re-quantising without the encoder."""
    x, c = _lib.as_f32(emb), _lib.as_f32(centres)
    if x.ndim != 2 or c.ndim != 2 or x.shape[1] != NODE_H[0] or c.shape[1] != NODE_H[0]:
        raise ValueError(f"emb {x.shape} / centres {c.shape}: expected [n, {NODE_H[0]}] and [K, {NODE_H[0]}]")
    tok = np.empty(x.shape[0], np.int32)
    _lib.check(_lib.load().pgmi_op_prosst_assign(device, _lib.ptr(x, _lib._f32p), x.shape[0], _lib.ptr(c, _lib._f32p), c.shape[0],
                                                 _lib.ptr(tok, _lib._i32p)))
    return tok


class PdbQuantizer:
    """The reference's PdbQuantizer contract on the HIP path: ``q(pdb_file)`` is the list of structure tokens of the file's residues,
    ``q(pdb_file, return_residue_seq=True)`` is (aa_seq, tokens).  ``structure_vocab_size`` may be a list: ``tokens_for`` then returns
    every codebook's tokens from one encoder pass.  model_path and cluster_dir must be given: the released AE.pt and <K>.joblib are not
    shipped with this package."""

    def __init__(self, structure_vocab_size=2048, max_distance: float = RADIUS, subgraph_depth=None, subgraph_interval: int = 1,
                 anchor_nodes=None, model_path: Optional[str] = None, cluster_dir: Optional[str] = None, cluster_model=None, device: int = 0,
                 state_dict=None, codebooks: Optional[Dict[int, np.ndarray]] = None):
        sizes = [structure_vocab_size] if isinstance(structure_vocab_size, int) else list(structure_vocab_size)
        if subgraph_interval != 1 or subgraph_depth not in (None, DEPTH) or anchor_nodes is not None:
            raise ValueError("this path runs subgraph_interval 1, subgraph_depth 50 and every residue as an anchor")
        if float(max_distance) != RADIUS:
            # the reference's membership mask is hard-wired to < 10 while its edge cutoffs take max_distance: one radius cannot restate both
            raise ValueError(f"max_distance {max_distance}: this path runs 10 (the reference's subgraph membership is fixed at 10 A)")
        if state_dict is None:
            if model_path is None:
                raise ValueError("model_path: the path of AE.pt (the released checkpoint is not shipped; nothing is downloaded)")
            state_dict = load_checkpoint(model_path)
        self.codebooks: Dict[int, np.ndarray] = {}
        for K in sizes:
            if codebooks is not None and K in codebooks:
                c = np.ascontiguousarray(codebooks[K], dtype=np.float32)
            else:
                if cluster_dir is None:
                    raise ValueError("cluster_dir: the folder of <K>.joblib / <K>.npy (not shipped; nothing is downloaded)")
                name = cluster_model[sizes.index(K)] if cluster_model else None
                c = read_codebook(os.path.join(cluster_dir, name) if name else find_codebook(cluster_dir, K))
            if c.shape[0] != K:
                raise ValueError(f"codebook {K}: {c.shape[0]} centres")
            self.codebooks[K] = c
        self.structure_vocab_size = sizes[0]
        self.model = Quantizer(pack(state_dict), device=device)

    def tokens_for(self, pdb_file) -> Tuple[str, Dict[int, List[int]]]:
        """(aa_seq, {K: tokens}) of one file: one encoder pass, one assignment per codebook."""
        seq, X = read_backbone(pdb_file)
        if len(seq) > MAX_L:
            raise ValueError(f"{len(seq)} residues: this path takes at most {MAX_L}")
        self.model.set_structure(X)
        self.model.embed()
        return seq, {K: self.model.assign(c).tolist() for K, c in self.codebooks.items()}

    def __call__(self, pdb_file, return_residue_seq: bool = False):
        seq, toks = self.tokens_for(pdb_file)
        labels = toks[self.structure_vocab_size]
        return (seq, labels) if return_residue_seq else labels

    def close(self):
        self.model.close()


def fasta_text(name: str, tokens: Sequence[int]) -> str:
    """One structure_sequence file as compute_fitness.py reads it: the header, then the comma-joined tokens on one line."""
    return f">{name}\n" + ",".join(str(int(t)) for t in tokens)
