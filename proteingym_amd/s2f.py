"""S2F scoring on libpgmi (include/pgmi.h, S2F section).

Replaces proteingym/baselines/S3F's model side for the S2F configuration (config/evaluate/s2f.yaml): ESM-2 on the masked wild type,
its last-layer residue rows through a 5-layer GVP-GNN over the 10 A C-alpha radius graph, a 20-way head, and ESM's own logits on
residues with pLDDT < 70.  The checkpoint is the task state dict (``model.sequence_model.model.*``, ``model.structure_model.*``,
``linear.*``); both halves are packed into blobs and run in HIP (csrc/api_s2f.hip on the ESM2 encoder).  The reference forwards one
masked copy per distinct site tuple; the masked input depends only on the window and the SET of sites, so every distinct (window, set)
is forwarded once.  S3F's surface branch is not computed.  Nothing is downloaded.

The behaviours of torchdrug, torch_geometric and torch_cluster this file restates are each in one named function or table:
``RESIDUE_ORDER`` (torchdrug's residue ids), ``radius_graph`` (torch_cluster's cap and order), ``EDGE_FLOW`` (torch_geometric's
source_to_target flow with torchdrug's (node_in, node_out) edge list).  They are read from the libraries' documented behaviour.
"""
from __future__ import annotations

import ctypes as C
import os
import re
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from . import esm as pesm

# torchdrug.data.Protein.residue_symbol2id: the id of each one-letter code; the 20 columns of the head are in this order
RESIDUE_ORDER = "GASPVTCILNDQKEMHFRYW"
# the token id of each of those letters in the ESM alphabet (MyESM.mapping)
AA_COLS = np.array([pesm.VOCABULARY.index(a) for a in RESIDUE_ORDER], dtype=np.int32)
# an edge of torchdrug's edge list is (node_in, node_out); GVPConv's propagate reads it as (source j, target i) and aggregates at i
EDGE_FLOW = "j->i"
RADIUS, MAX_NEIGHBORS, PLDDT_THRESHOLD = 10.0, 32, 70.0
NODE_H, EDGE_IN, EDGE_H, LAYERS = (256, 16), (16, 1), (64, 1), 5
MODEL_WINDOW = 1022
# script/evaluate.py load_dataset: assays with a hard-coded sequence window (0-based start, end)
FIXED_WINDOWS = {"POLG_HCVJF_Qi_2014": (1981, 2225), "A0A140D2T1_ZIKV_Sourisseau_2019": (290, 794),
                 "B2L11_HUMAN_Dutta_2010_binding-Mcl-1": (119, 197)}
BRCA2_ID, BRCA2_WINDOW = "BRCA2_HUMAN_Erwood_2022_HEK293T", (1820, 2832)


class S2fConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("abi_version", "node_in", "node_s", "node_v", "edge_s", "edge_v", "rbf", "layers",
                                         "max_neighbors")] + [("radius", C.c_float), ("plddt_threshold", C.c_float)]


def make_config(node_in: int = 1280, layers: int = LAYERS, max_neighbors: int = MAX_NEIGHBORS, radius: float = RADIUS,
                plddt_threshold: float = PLDDT_THRESHOLD) -> S2fConfig:
    return S2fConfig(abi_version=_lib.ABI_VERSION, node_in=node_in, node_s=NODE_H[0], node_v=NODE_H[1], edge_s=EDGE_H[0], edge_v=EDGE_H[1],
                     rbf=EDGE_IN[0], layers=layers, max_neighbors=max_neighbors, radius=radius, plddt_threshold=plddt_threshold)


# -- checkpoint --------------------------------------------------------------------------------------------------------------
def _gvp_shapes(prefix: str, si: int, vi: int, so: int, vo: int) -> List[Tuple[str, Tuple[int, ...]]]:
    """A GVP's tensors in blob order.  h = max(vi, vo) (gvp_layer.py GVP.__init__); no vector input: ws only."""
    if not vi:
        return [(prefix + "ws.weight", (so, si)), (prefix + "ws.bias", (so,))]
    h = max(vi, vo)
    out = [(prefix + "wh.weight", (h, vi)), (prefix + "ws.weight", (so, si + h)), (prefix + "ws.bias", (so,))]
    if vo:
        out += [(prefix + "wv.weight", (vo, h)), (prefix + "wsv.weight", (vo, so)), (prefix + "wsv.bias", (vo,))]
    return out


def gvp_key_shapes(node_in: int = 1280, layers: int = LAYERS) -> List[Tuple[str, Tuple[int, ...]]]:
    """(key under model.structure_model. / the task, shape) in blob order (include/pgmi.h)."""
    ns, nv = NODE_H
    es, ev = EDGE_H
    p = "model.structure_model."
    out = [(p + "residue_embdding.weight", (node_in, node_in)),
           (p + "W_v.0.scalar_norm.weight", (node_in,)), (p + "W_v.0.scalar_norm.bias", (node_in,))]
    out += _gvp_shapes(p + "W_v.1.", node_in, 0, ns, nv)
    out += [(p + "W_e.0.scalar_norm.weight", (EDGE_IN[0],)), (p + "W_e.0.scalar_norm.bias", (EDGE_IN[0],))]
    out += _gvp_shapes(p + "W_e.1.", EDGE_IN[0], EDGE_IN[1], es, ev)
    for l in range(layers):
        q = f"{p}layers.{l}."
        out += _gvp_shapes(q + "conv.message_func.0.", 2 * ns + es, 2 * nv + ev, ns, nv)
        out += _gvp_shapes(q + "conv.message_func.1.", ns, nv, ns, nv)
        out += _gvp_shapes(q + "conv.message_func.2.", ns, nv, ns, nv)
        for n in (0, 1):
            out += [(f"{q}norm.{n}.scalar_norm.weight", (ns,)), (f"{q}norm.{n}.scalar_norm.bias", (ns,))]
        out += _gvp_shapes(q + "ff_func.0.", ns, nv, 4 * ns, 2 * nv)
        out += _gvp_shapes(q + "ff_func.1.", 4 * ns, 2 * nv, ns, nv)
    out += [(p + "W_out.0.scalar_norm.weight", (ns,)), (p + "W_out.0.scalar_norm.bias", (ns,))]
    out += _gvp_shapes(p + "W_out.1.", ns, nv, ns, 0)
    return out + [("linear.weight", (20, ns)), ("linear.bias", (20,))]


SEQ_PREFIX = "model.sequence_model.model."


def _ignored(key: str) -> bool:
    """Buffers and heads the inference path never reads: MyESM.mapping, _VDropout.dummy_param, AttributeMasking's mlp; fair-esm's
    contact head and rotary inv_freq buffers."""
    return (key.endswith(".mapping") or key.endswith("dummy_param") or key.startswith("mlp.") or ".contact_head." in key
            or key.endswith("rot_emb.inv_freq"))


def _to_np(t) -> np.ndarray:
    return t.detach().to("cpu").float().numpy() if hasattr(t, "detach") else np.asarray(t, dtype=np.float32)


def pack(sd, esm_cfg: dict, layers: int = LAYERS) -> Tuple[np.ndarray, np.ndarray]:
    """(ESM2 blob, GVP blob) from the task state dict.  Anything missing or unexpected is an error."""
    node_in = esm_cfg["embed_dim"]
    gvp = gvp_key_shapes(node_in, layers)
    esm_keys = [SEQ_PREFIX + k for k in pesm.expected_keys(esm_cfg)]
    want = {k for k, _ in gvp} | set(esm_keys)
    tied = SEQ_PREFIX + "lm_head.weight"
    missing = sorted(k for k in want if k not in sd)
    unexpected = sorted(k for k in sd if k not in want and k != tied and not _ignored(k))
    if missing or unexpected:
        raise ValueError(f"not an S2F task state dict: missing {missing[:5]}, unexpected {unexpected[:5]}")
    for k, shape in gvp:
        if tuple(np.shape(sd[k])) != shape:
            raise ValueError(f"{k}: shape {tuple(np.shape(sd[k]))}, this path needs {shape}")
    gvp_blob = np.concatenate([_to_np(sd[k]).ravel() for k, _ in gvp]).astype(np.float32)
    esm_blob = np.concatenate([_to_np(sd[k]).ravel() for k in esm_keys]).astype(np.float32)
    return esm_blob, gvp_blob


def random_state_dict(seed: int, esm_cfg: dict, layers: int = LAYERS, esm_blob: Optional[np.ndarray] = None) -> Dict[str, np.ndarray]:
    """A seeded task state dict (tests, benchmarks): Linear weights N(0, 1 / fan_in), LayerNorm gains near 1, plus the buffers a real
    checkpoint carries.  esm_blob: the ESM2 half (synthetic.random_weights); left out when None."""
    rng = np.random.default_rng(seed)
    sd: Dict[str, np.ndarray] = {}
    for k, shape in gvp_key_shapes(esm_cfg["embed_dim"], layers):
        if "scalar_norm.weight" in k:
            a = 1.0 + 0.1 * rng.standard_normal(shape)
        elif k.endswith("bias"):
            a = 0.1 * rng.standard_normal(shape)
        else:
            a = rng.standard_normal(shape) / np.sqrt(shape[-1])
        sd[k] = a.astype(np.float32)
    sd["model.sequence_model.mapping"] = np.asarray(AA_COLS, dtype=np.int64)
    sd["mlp.layers.0.weight"] = np.zeros((1, 1), dtype=np.float32)
    if esm_blob is not None:
        from . import synthetic
        for k, a in synthetic.blob_to_arrays(esm_cfg, esm_blob).items():
            sd[SEQ_PREFIX + k] = a
    return sd


# -- graph -------------------------------------------------------------------------------------------------------------------
def radius_graph(pos: np.ndarray, r: float = RADIUS, max_num_neighbors: int = MAX_NEIGHBORS) -> Tuple[np.ndarray, np.ndarray]:
    """torch_cluster.radius_graph(pos, r, max_num_neighbors, loop=False) as its CUDA kernel keeps neighbours: per centre i the candidates
    j in ascending index with squared distance < r^2, self included; the first max_num_neighbors + 1 are kept, then the self edge is
    dropped.  Returns (src j, dst i), sorted by (i, j); distances in float64 from the coordinates as given."""
    p = np.asarray(pos, dtype=np.float64)
    d2 = ((p[:, None, :] - p[None, :, :]) ** 2).sum(-1)
    src, dst = [], []
    for i in range(len(p)):
        cand = np.flatnonzero(d2[i] < r * r)[:max_num_neighbors + 1]
        cand = cand[cand != i]
        src.append(cand)
        dst.append(np.full(len(cand), i))
    if not src:
        return np.zeros(0, np.int32), np.zeros(0, np.int32)
    return np.concatenate(src).astype(np.int32), np.concatenate(dst).astype(np.int32)


# -- PDB ---------------------------------------------------------------------------------------------------------------------
def read_ca(path_or_lines) -> Tuple[np.ndarray, np.ndarray]:
    """C-alpha coordinates float32 [n, 3] and B-factors float32 [n] of the first model, every chain in file order (bio_load_pdb +
    subgraph(CA)); fixed columns as esm3.read_pdb reads them; the first alternate location of an atom wins."""
    if isinstance(path_or_lines, (str, os.PathLike)):
        with open(path_or_lines) as f:
            lines = f.read().splitlines()
    else:
        lines = list(path_or_lines)
    xyz, bf, seen = [], [], set()
    for line in lines:
        rec = line[:6]
        if rec.startswith("ENDMDL"):
            break
        if rec not in ("ATOM  ", "HETATM") or line[12:16].strip() != "CA" or len(line[17:20].strip()) != 3:
            continue
        key = (line[21], line[22:27])
        if key in seen:
            continue
        seen.add(key)
        xyz.append((float(line[30:38]), float(line[38:46]), float(line[46:54])))
        bf.append(float(line[60:66]))
    if not xyz:
        raise ValueError("no C-alpha atoms in the PDB file")
    return np.array(xyz, dtype=np.float32), np.array(bf, dtype=np.float32)


def load_structure(structdir: str, pdb_files: str, pdb_range: str, dms_id: str = ""):
    """compute_fitness.py:103-120: the C-alpha atoms of the '|'-separated files concatenated; (pos, plddt, start, end) with the
    0-based sequence range [start, end) the structure covers."""
    parts = [read_ca(os.path.join(structdir, f)) for f in pdb_files.split("|")]
    pos, bf = np.concatenate([p for p, _ in parts]), np.concatenate([b for _, b in parts])
    rng = str(pdb_range).split("-")
    start, end = int(rng[0]) - 1, int(rng[-1])
    if dms_id == "POLG_HCVJF_Qi_2014":
        start, end = FIXED_WINDOWS[dms_id]
    return pos, bf, start, end


# -- mutants, windows, position sets ---------------------------------------------------------------------------------------------
def get_optimal_window(mutation_position_relative: int, seq_len_wo_special: int, model_window: int) -> Tuple[int, int]:
    """script/evaluate.py:70-79."""
    half = model_window // 2
    if seq_len_wo_special <= model_window:
        return 0, seq_len_wo_special
    if mutation_position_relative < half:
        return 0, model_window
    if mutation_position_relative >= seq_len_wo_special - half:
        return seq_len_wo_special - model_window, seq_len_wo_special
    return max(0, mutation_position_relative - half), min(seq_len_wo_special, mutation_position_relative + half)


def window_for(dms_id: str, sites: Sequence[int], seq_len: int) -> Tuple[int, int]:
    """load_dataset's window of one site tuple (0-based [start, end))."""
    if dms_id in FIXED_WINDOWS:
        start, end = FIXED_WINDOWS[dms_id]
    elif seq_len > MODEL_WINDOW:
        start, end = get_optimal_window(sites[0], seq_len, MODEL_WINDOW)
    else:
        start, end = 0, seq_len
    if dms_id == BRCA2_ID and end > BRCA2_WINDOW[1]:
        start, end = BRCA2_WINDOW
    return start, end


def sort_mutants(mutants: Sequence[str], scores: Sequence[float]):
    """load_dataset: [(sites tuple 0-based, sub-mutation list, DMS_score)] sorted as Python sorts those tuples."""
    rows = [(tuple(int(y[1:-1]) - 1 for y in m.split(":")), m.split(":"), float(t)) for m, t in zip(mutants, scores)]
    return sorted(rows)


def position_sets(rows, dms_id: str, seq_len: int):
    """Distinct (window, set of sites) in order of first appearance.  Returns windows [(start, end)], per window the CSR
    (set_off, set_pos: window-relative residue indices, ascending) of its sets, and per mutant (window index, set index)."""
    windows: List[Tuple[int, int]] = []
    w_index: Dict[Tuple[int, int], int] = {}
    sets: List[Dict[Tuple[int, ...], int]] = []
    csr: List[Tuple[List[int], List[int]]] = []
    where = []
    for sites, _, _ in rows:
        win = window_for(dms_id, sites, seq_len)
        w = w_index.get(win)
        if w is None:
            w = w_index[win] = len(windows)
            windows.append(win)
            sets.append({})
            csr.append(([0], []))
        key = tuple(sorted(set(s - win[0] for s in sites)))
        if key[0] < 0 or key[-1] >= win[1] - win[0]:
            raise ValueError(f"sites {sites} lie outside their window {win}")
        s = sets[w].get(key)
        if s is None:
            s = sets[w][key] = len(csr[w][0]) - 1
            csr[w][1].extend(key)
            csr[w][0].append(len(csr[w][1]))
        where.append((w, s))
    return windows, [(np.array(o, np.int32), np.array(p, np.int32)) for o, p in csr], where


def cut_structure(pos, plddt, s_start: int, s_end: int, start: int, end: int):
    """MutantDataset.__getitem__: the structure cut to the sequence window, or the reference's ValueError; then assign_structure's
    assertion that the residue counts agree."""
    if s_start <= start and s_end >= end:
        pos, plddt = pos[start - s_start:end - s_start], plddt[start - s_start:end - s_start]
    elif s_start != start or s_end != end:
        raise ValueError("the structure range (%d, %d) doesn't match the sequence range (%d, %d)" % (s_start, s_end, start, end))
    assert len(pos) == end - start, f"structure has {len(pos)} residues, the sequence window {end - start}"
    return pos, plddt


def score_rows(rows, where, tables, windows) -> np.ndarray:
    """get_prob: per mutant the sum over its sub-mutations of lp[site, mt] - lp[site, wt], in sub-mutation order, float32 sums like
    the reference's; tables[w] is [n_sets, L_w, 20]."""
    out = np.empty(len(rows), dtype=np.float32)
    for n, ((sites, muts, _), (w, s)) in enumerate(zip(rows, where)):
        lp = tables[w][s]
        idx = np.array(sites) - windows[w][0]
        mt = [RESIDUE_ORDER.find(m[-1]) for m in muts]       # -1 (an unknown letter) reads the last column, as the reference's index does
        wt = [RESIDUE_ORDER.find(m[0]) for m in muts]
        out[n] = (lp[idx, mt].astype(np.float32) - lp[idx, wt].astype(np.float32)).sum(dtype=np.float32)
    return out


def tokenize(seq: str) -> np.ndarray:
    ids = np.empty(len(seq) + 2, dtype=np.int32)
    ids[0], ids[-1] = pesm.VOCABULARY.index("<cls>"), pesm.VOCABULARY.index("<eos>")
    for i, a in enumerate(seq):
        if a not in RESIDUE_ORDER:
            raise ValueError(f"residue {i + 1}: {a!r} is not one of the 20 amino acids")
        ids[i + 1] = pesm.VOCABULARY.index(a)
    return ids


# -- yaml --------------------------------------------------------------------------------------------------------------------
def load_yaml(path: str, context: Dict[str, str]) -> dict:
    """util.load_config without jinja: plain substitution of the {{ name }} placeholders (a missing name becomes empty), then YAML."""
    import yaml
    with open(path) as f:
        raw = f.read()
    raw = re.sub(r"\{\{\s*(\w+)\s*\}\}", lambda m: str(context.get(m.group(1)) or ""), raw)
    return yaml.safe_load(raw)


def check_yaml(cfg: dict, node_in: int = 1280, esm_name: Optional[str] = "ESM-2-650M") -> dict:
    """The fields this path reads; anything it does not compute is refused.  node_in / esm_name: the released model's; a test hook of
    the CLI names the dimensions of a smaller seeded ESM2 (esm_name None: not compared)."""
    if cfg.get("surface_path"):
        raise ValueError("surface_path is set: S3F's surface branch (precomputed surface point clouds, a second graph) is not computed "
                         "on this path; S2F and S2F-MSA are")
    task = cfg["task"]
    model = task["model"]
    sm, qm = model["structure_model"], model["sequence_model"]
    if sm.get("class") == "SurfGVP":
        raise ValueError("structure_model SurfGVP: S3F's surface branch is not computed on this path; S2F (GVPGNN) is")
    if task.get("class") != "ResidueTypePrediction" or model.get("class") != "FusionNetwork" or sm.get("class") != "GVPGNN" or \
            qm.get("class") != "MyESM":
        raise ValueError("this path runs ResidueTypePrediction(FusionNetwork(MyESM, GVPGNN)) only")
    if esm_name is not None and qm.get("model") != esm_name:
        raise ValueError(f"sequence_model.model {qm.get('model')!r}: this path runs {esm_name}")
    want = dict(node_in_dim=[node_in, 0], node_h_dim=list(NODE_H), edge_in_dim=list(EDGE_IN), edge_h_dim=list(EDGE_H))
    for k, v in want.items():
        if list(sm.get(k, [])) != v:
            raise ValueError(f"structure_model.{k} = {sm.get(k)}: this path runs {v}")
    if not sm.get("vector_gate", True):
        raise ValueError("structure_model.vector_gate false: this path runs the vector gate")
    if "activations" in sm:
        raise ValueError("structure_model.activations: this path runs the default (relu, None)")
    layers = int(sm.get("num_layers", 3))
    edge_layers = (cfg["task"].get("graph_construction_model") or {}).get("edge_layers") or []
    if len(edge_layers) != 1 or edge_layers[0].get("class") != "SpatialEdge" or float(edge_layers[0].get("min_distance", 5)) != 0:
        raise ValueError("graph_construction_model: this path runs one SpatialEdge layer with min_distance 0 on AlphaCarbonNode")
    thr = task.get("plddt_threshold")
    return dict(layers=layers, radius=float(edge_layers[0]["radius"]), max_neighbors=int(edge_layers[0].get("max_num_neighbors", 32)),
                plddt_threshold=float(thr) if thr else None)


# -- model -------------------------------------------------------------------------------------------------------------------
class S2F(_lib.SideHandle):
    """Device-resident S2F: an ESM2 model (nullable: GNN only) plus the GVP blob."""

    PREFIX, NAME = "s2f", "GVP "

    def __init__(self, gvp_blob: np.ndarray, esm: Optional[pesm.EsmModel] = None, node_in: Optional[int] = None, layers: int = LAYERS,
                 device: int = 0, max_neighbors: int = MAX_NEIGHBORS, radius: float = RADIUS,
                 plddt_threshold: Optional[float] = PLDDT_THRESHOLD):
        self.esm = esm
        self.D = int(esm.cfg["embed_dim"] if esm is not None else node_in)
        # task.py: `if self.plddt_threshold:` -- no threshold, no fallback: every pLDDT is above -inf
        thr = float(plddt_threshold) if plddt_threshold else -3.0e38
        self.config = make_config(self.D, layers, max_neighbors, radius, thr)
        self._create(self.config, gvp_blob, device, esm._h if esm is not None else None)
        self.L = 0

    def set_structure(self, pos, plddt):
        p, q = _lib.as_f32(pos), _lib.as_f32(plddt)
        if p.ndim != 2 or p.shape[1] != 3 or q.shape != (p.shape[0],):
            raise ValueError(f"pos {p.shape} / plddt {q.shape}: expected [L, 3] and [L]")
        _lib.check(_lib.load().pgmi_s2f_set_structure(self._h, _lib.ptr(p, _lib._f32p), _lib.ptr(q, _lib._f32p), p.shape[0]))
        self.L = p.shape[0]

    def graph(self):
        """(src, dst, e_s [E, 64], e_v [E, 3]) of the structure."""
        n = C.c_int32()
        lib = _lib.load()
        _lib.check(lib.pgmi_s2f_graph(self._h, C.byref(n), None, None, None, None))
        E = n.value
        src, dst = np.empty(E, np.int32), np.empty(E, np.int32)
        es, ev = np.empty((E, EDGE_H[0]), np.float32), np.empty((E, 3), np.float32)
        _lib.check(lib.pgmi_s2f_graph(self._h, C.byref(n), _lib.ptr(src, _lib._i32p), _lib.ptr(dst, _lib._i32p), _lib.ptr(es, _lib._f32p),
                                      _lib.ptr(ev, _lib._f32p)))
        return src, dst, es, ev

    def gvp_forward(self, node_feat, seq_logits, want_nodes: bool = False):
        """node_feat [B, L, D], seq_logits [B, L, 20] -> lp [B, L, 20] (and the node state after the last layer)."""
        x, q = _lib.as_f32(node_feat), _lib.as_f32(seq_logits)
        if x.ndim != 3 or x.shape[1:] != (self.L, self.D) or q.shape != (x.shape[0], self.L, 20):
            raise ValueError(f"node_feat {x.shape} / seq_logits {q.shape}: expected [B, {self.L}, {self.D}] and [B, {self.L}, 20]")
        B = x.shape[0]
        lp = np.empty((B, self.L, 20), np.float32)
        ns = np.empty((B, self.L, NODE_H[0]), np.float32) if want_nodes else None
        nv = np.empty((B, self.L, NODE_H[1], 3), np.float32) if want_nodes else None
        _lib.check(_lib.load().pgmi_s2f_gvp_forward(self._h, _lib.ptr(x, _lib._f32p), _lib.ptr(q, _lib._f32p), B, _lib.ptr(lp, _lib._f32p),
                                                    _lib.ptr(ns, _lib._f32p), _lib.ptr(nv, _lib._f32p)))
        return (lp, ns, nv) if want_nodes else lp

    def set_logprobs(self, wt_tokens, set_off, set_pos, want_full: bool = False):
        """One forward per position set: [n_entries, 20] rows of (set, position); with want_full also [n_sets, L, 20]."""
        wt, so, sp = _lib.as_i32(wt_tokens), _lib.as_i32(set_off), _lib.as_i32(set_pos)
        out = np.empty((int(so[-1]), 20), np.float32)
        full = np.empty((so.size - 1, self.L, 20), np.float32) if want_full else None
        _lib.check(_lib.load().pgmi_s2f_set_logprobs(self._h, _lib.ptr(wt, _lib._i32p), wt.size, _lib.ptr(AA_COLS, _lib._i32p),
                                                     _lib.ptr(so, _lib._i32p), _lib.ptr(sp, _lib._i32p), so.size - 1,
                                                     _lib.ptr(out, _lib._f32p), _lib.ptr(full, _lib._f32p)))
        return (out, full) if want_full else out

    def score_assay(self, dms_id: str, target_seq: str, rows, pos, plddt, s_start: int, s_end: int) -> np.ndarray:
        """The sorted mutants (sort_mutants) of one assay against its structure: float32 [n]."""
        windows, csr, where = position_sets(rows, dms_id, len(target_seq))
        tables = []
        for (start, end), (set_off, set_pos) in zip(windows, csr):
            p, q = cut_structure(pos, plddt, s_start, s_end, start, end)
            self.set_structure(p, q)
            tables.append(self.set_logprobs(tokenize(target_seq[start:end]), set_off, set_pos, want_full=True)[1])
        return score_rows(rows, where, tables, windows)


def from_state_dict(sd, esm_cfg: dict, layers: int = LAYERS, device: int = 0, precision: str = "f16x3", max_rows: int = 0, **kw) -> S2F:
    esm_blob, gvp_blob = pack(sd, esm_cfg, layers)
    esm = pesm.EsmModel(esm_cfg, esm_blob, device=device, precision=precision, max_rows=max_rows)
    return S2F(gvp_blob, esm, layers=layers, device=device, **kw)


def load_checkpoint(path: str):
    """torch.load(path)['model'] of a local file, as compute_fitness.py:83 reads it."""
    import torch
    if not os.path.isfile(path):
        raise FileNotFoundError(f"{path}: no such checkpoint (this path never downloads)")
    return {k: v for k, v in torch.load(path, map_location="cpu", weights_only=True)["model"].items()}
