"""S3F scoring on libpgmi (include/pgmi.h, S3F section).

Replaces proteingym/baselines/S3F's model side for the S3F configuration (config/evaluate/s3f.yaml): S2F (proteingym_amd/s2f.py) plus
SurfGVP's surface half, a second GVP-GNN over the 16-nearest-neighbour graph of a precomputed surface point cloud whose points take
the ESM2 rows of their three nearest C-alpha atoms.  ``SurfGVP.residue2surface`` returns nothing, so what reaches a residue is the mean
of ``surf_W_out``'s rows over all surface points of the loader's batch; with the yaml's ``batch_size: 2`` on an unshuffled loader two
consecutive masked sequences share that row.  This module reproduces the pairing from the yaml (``pool_groups``).

The surface files are the caller's: one pickle per pdb file, ``<pdb stem>.pkl``, a dict of numpy arrays (``surf_points``,
``surf_normals``, ``surf_hks``, ``surf_curvatures``, ``res2surf``) as the reference's script/process_surface.py writes them.  Reading
one unpickles it: only point this at files you made.  Everything before the surface MLP's LayerNorm is linear in the ESM2 rows and is
folded once per checkpoint in float64 (``fold``).  Nothing is downloaded.
"""
from __future__ import annotations

import ctypes as C
import os
import pickle
from typing import Dict, List, Optional, Tuple

import numpy as np

from . import _lib, s2f
from . import esm as pesm

SURF_IN, SURF_EDGE_IN, SURF_RES_NEIGHBORS, SURF_NEIGHBORS = (42, 0), (16, 1), 3, 16
MIN_POINTS = SURF_NEIGHBORS + 1            # below it knn_graph returns short neighbour lists
SM = "model.structure_model."


class S3fConfig(C.Structure):
    _fields_ = [("s2f", s2f.S2fConfig), ("surf_feat", C.c_int32), ("surf_res_neighbors", C.c_int32), ("surf_neighbors", C.c_int32)]


# -- checkpoint --------------------------------------------------------------------------------------------------------------
def surf_key_shapes(node_in: int = 1280, layers: int = s2f.LAYERS):
    """(the surface MLP's keys as the checkpoint has them, the surface GNN's keys in blob order), each a list of (key, shape)."""
    D, H = node_in, 2 * node_in
    mlp = [(SM + "surf_in_linear.weight", (D, D + 1)), (SM + "surf_in_mlp.0.weight", (H, D + SURF_IN[0])), (SM + "surf_in_mlp.0.bias", (H,)),
           (SM + "surf_in_mlp.2.weight", (H,)), (SM + "surf_in_mlp.2.bias", (H,)), (SM + "surf_in_mlp.4.weight", (D, H)),
           (SM + "surf_in_mlp.4.bias", (D,))]
    gnn = []
    for k, shape in s2f.gvp_key_shapes(node_in, layers):
        name = k[len(SM):] if k.startswith(SM) else None
        if name and name.split(".")[0] in ("W_v", "W_e", "layers", "W_out"):
            gnn.append((SM + "surf_" + name, shape))
    return mlp, gnn


def fold(sd, node_in: int) -> Dict[str, np.ndarray]:
    """The part of the surface MLP before its LayerNorm, as float64 arrays: with surf_in_linear.weight = [W_x | w_d] and
    surf_in_mlp.0.weight = [W_1h | W_1f], the pre-LayerNorm row of point p is mean_k Z[res_k(p)] + Wsf [feat_p | mean_k d_k(p)] + b_1
    with Z = X Wz^T, Wz = W_1h W_x and Wsf = [W_1f | W_1h w_d]."""
    D = node_in
    w_in = np.asarray(s2f._to_np(sd[SM + "surf_in_linear.weight"]), dtype=np.float64)
    w_1 = np.asarray(s2f._to_np(sd[SM + "surf_in_mlp.0.weight"]), dtype=np.float64)
    w_1h, w_1f = w_1[:, :D], w_1[:, D:]
    return dict(Wz=w_1h @ w_in[:, :D], Wsf=np.concatenate([w_1f, (w_1h @ w_in[:, D])[:, None]], 1),
                b1=np.asarray(s2f._to_np(sd[SM + "surf_in_mlp.0.bias"]), dtype=np.float64))


def pack(sd, esm_cfg: dict, layers: int = s2f.LAYERS) -> Tuple[np.ndarray, np.ndarray]:
    """(ESM2 blob, S3F blob) from the task state dict.  Anything missing or unexpected is an error."""
    node_in = esm_cfg["embed_dim"]
    gvp = s2f.gvp_key_shapes(node_in, layers)
    mlp, gnn = surf_key_shapes(node_in, layers)
    esm_keys = [s2f.SEQ_PREFIX + k for k in pesm.expected_keys(esm_cfg)]
    want = {k for k, _ in gvp + mlp + gnn} | set(esm_keys)
    tied = s2f.SEQ_PREFIX + "lm_head.weight"
    missing = sorted(k for k in want if k not in sd)
    unexpected = sorted(k for k in sd if k not in want and k != tied and not s2f._ignored(k))
    if missing or unexpected:
        raise ValueError(f"not an S3F task state dict: missing {missing[:5]}, unexpected {unexpected[:5]}")
    for k, shape in gvp + mlp + gnn:
        if tuple(np.shape(sd[k])) != shape:
            raise ValueError(f"{k}: shape {tuple(np.shape(sd[k]))}, this path needs {shape}")
    f = fold(sd, node_in)
    parts = [s2f._to_np(sd[k]).ravel() for k, _ in gvp]
    parts += [f["Wz"].ravel(), f["Wsf"].ravel(), f["b1"].ravel()]
    parts += [s2f._to_np(sd[SM + "surf_in_mlp." + k]).ravel() for k in ("2.weight", "2.bias", "4.weight", "4.bias")]
    parts += [s2f._to_np(sd[k]).ravel() for k, _ in gnn]
    esm_blob = np.concatenate([s2f._to_np(sd[k]).ravel() for k in esm_keys]).astype(np.float32)
    return esm_blob, np.concatenate(parts).astype(np.float32)


def random_state_dict(seed: int, esm_cfg: dict, layers: int = s2f.LAYERS, esm_blob: Optional[np.ndarray] = None) -> Dict[str, np.ndarray]:
    """s2f.random_state_dict plus seeded surface tensors drawn by the same rule."""
    sd = s2f.random_state_dict(seed, esm_cfg, layers, esm_blob)
    rng = np.random.default_rng(seed + 7919)
    mlp, gnn = surf_key_shapes(esm_cfg["embed_dim"], layers)
    for k, shape in mlp + gnn:
        if "scalar_norm.weight" in k or k.endswith("surf_in_mlp.2.weight"):
            a = 1.0 + 0.1 * rng.standard_normal(shape)
        elif k.endswith("bias"):
            a = 0.1 * rng.standard_normal(shape)
        else:
            a = rng.standard_normal(shape) / np.sqrt(shape[-1])
        sd[k] = a.astype(np.float32)
    return sd


# -- surface files -------------------------------------------------------------------------------------------------------------
def load_surface(surfdir: str, pdb_files: str):
    """compute_fitness.py:122-137: the pickles of the '|'-separated pdb files.  (points f32 [Ns, 3], features f32 [Ns, 42] = [hks |
    curvatures], res2surf int64 [L, 3, 21]).  Several files: the points and features concatenated as graph_concat packs them, the
    res2surf arrays concatenated AS THEY ARE -- the reference adds no offset, so a later file's rows name points of the first."""
    pts, feat, r2s = [], [], []
    for f in pdb_files.split("|"):
        path = os.path.join(surfdir, f.split(".")[0] + ".pkl")
        if not os.path.isfile(path):
            raise FileNotFoundError(f"{path}: no surface file for {f} (script/process_surface.py writes them; this path does not)")
        with open(path, "rb") as fin:
            d = pickle.load(fin)
        p = np.asarray(d["surf_points"], dtype=np.float32)
        x = np.concatenate([np.asarray(d["surf_hks"], dtype=np.float32), np.asarray(d["surf_curvatures"], dtype=np.float32)], -1)
        if p.ndim != 2 or p.shape[1] != 3 or x.shape != (len(p), SURF_IN[0]):
            raise ValueError(f"{path}: surf_points {p.shape}, features {x.shape}; expected [Ns, 3] and [Ns, {SURF_IN[0]}]")
        pts.append(p)
        feat.append(x)
        r2s.append(np.asarray(d["res2surf"], dtype=np.int64))
    return np.concatenate(pts), np.concatenate(feat), np.concatenate(r2s)


def cut_surface(points, feat, res2surf, s_start: int, s_end: int, start: int, end: int):
    """MutantDataset.truncate: whenever the structure covers the window -- equal ranges included -- the surface keeps the points that
    the kept residues' res2surf rows name, in their order.  Otherwise the reference raises (s2f.cut_structure has the message)."""
    if not (s_start <= start and s_end >= end):
        raise ValueError("the structure range (%d, %d) doesn't match the sequence range (%d, %d)" % (s_start, s_end, start, end))
    if len(res2surf) != s_end - s_start:
        raise ValueError(f"res2surf has {len(res2surf)} rows, the structure {s_end - s_start} residues")
    idx = np.asarray(res2surf[start - s_start:end - s_start]).ravel()
    if idx.size and (idx.min() < 0 or idx.max() >= len(points)):
        raise ValueError("res2surf names a surface point that does not exist")
    mask = np.zeros(len(points), dtype=bool)
    mask[idx] = True
    if mask.sum() < MIN_POINTS:
        raise ValueError(f"the window ({start}, {end}) keeps {int(mask.sum())} surface points; the {SURF_NEIGHBORS}-neighbour graph needs "
                         f"at least {MIN_POINTS}")
    return np.ascontiguousarray(points[mask]), np.ascontiguousarray(feat[mask])


# -- masked sequences and pool groups ----------------------------------------------------------------------------------------------
def masked_sequences(rows, dms_id: str, seq_len: int):
    """load_dataset's list of masked sequences: one per run of equal site tuples in the sorted mutants.  Returns [(window, window-
    relative sorted site set)] and per mutant the index of its sequence (get_prob's counter)."""
    seqs, seq_of = [], []
    last = None
    for sites, _, _ in rows:
        if last is None or sites != last:
            win = s2f.window_for(dms_id, sites, seq_len)
            key = tuple(sorted(set(s - win[0] for s in sites)))
            if key[0] < 0 or key[-1] >= win[1] - win[0]:
                raise ValueError(f"sites {sites} lie outside their window {win}")
            seqs.append((win, key))
        seq_of.append(len(seqs) - 1)
        last = sites
    return seqs, seq_of


def pool_groups(n: int, batch_size: int) -> np.ndarray:
    """The unshuffled DataLoader's batches over n masked sequences as CSR offsets: consecutive runs of batch_size, the last may be
    short."""
    if batch_size < 1:
        raise ValueError(f"batch_size {batch_size}")
    return np.array(list(range(0, n, batch_size)) + [n], dtype=np.int32)


# -- yaml --------------------------------------------------------------------------------------------------------------------
def check_yaml(cfg: dict, node_in: int = 1280, esm_name: Optional[str] = "ESM-2-650M") -> dict:
    """s2f.check_yaml for the S3F configuration: SurfGVP with the released surface dimensions and a surface_path."""
    sm = cfg["task"]["model"]["structure_model"]
    if sm.get("class") != "SurfGVP":
        raise ValueError(f"structure_model {sm.get('class')}: this path runs SurfGVP (S3F); S2F's GVPGNN is score_s2f_proteingym's")
    if not cfg.get("surface_path"):
        raise ValueError("surface_path is empty: S3F needs the folder of surface files (--surfdir)")
    want = dict(surf_in_dim=list(SURF_IN), surf_edge_in_dim=list(SURF_EDGE_IN), num_surf_res_neighbor=SURF_RES_NEIGHBORS,
                num_surf_graph_neighbor=SURF_NEIGHBORS)
    defaults = dict(num_surf_res_neighbor=3, num_surf_graph_neighbor=16)
    for k, v in want.items():
        got = sm.get(k, defaults.get(k))
        if (list(got) if isinstance(got, (list, tuple)) else got) != v:
            raise ValueError(f"structure_model.{k} = {sm.get(k)}: this path runs {v}")
    residue = {k: v for k, v in sm.items() if k not in want}
    residue["class"] = "GVPGNN"
    inner = dict(cfg, surface_path=None, task=dict(cfg["task"], model=dict(cfg["task"]["model"], structure_model=residue)))
    out = s2f.check_yaml(inner, node_in, esm_name)
    out["batch_size"] = int(cfg.get("batch_size", 1))
    if out["batch_size"] < 1:
        raise ValueError(f"batch_size {cfg.get('batch_size')}")
    return out


# -- model -------------------------------------------------------------------------------------------------------------------
class S3F(_lib.SideHandle):
    """Device-resident S3F: an ESM2 model (nullable: the two GNNs only) plus the S3F blob."""

    PREFIX, NAME = "s3f", "S3F "

    def __init__(self, blob: np.ndarray, esm: Optional[pesm.EsmModel] = None, node_in: Optional[int] = None, layers: int = s2f.LAYERS,
                 device: int = 0, max_neighbors: int = s2f.MAX_NEIGHBORS, radius: float = s2f.RADIUS,
                 plddt_threshold: Optional[float] = s2f.PLDDT_THRESHOLD):
        self.esm = esm
        self.D = int(esm.cfg["embed_dim"] if esm is not None else node_in)
        thr = float(plddt_threshold) if plddt_threshold else -3.0e38
        self.config = S3fConfig(s2f=s2f.make_config(self.D, layers, max_neighbors, radius, thr), surf_feat=SURF_IN[0],
                                surf_res_neighbors=SURF_RES_NEIGHBORS, surf_neighbors=SURF_NEIGHBORS)
        self._create(self.config, blob, device, esm._h if esm is not None else None)
        self.L = self.Ns = 0

    def set_structure(self, pos, plddt, surf_pos, surf_feat):
        p, q, sp, sf = _lib.as_f32(pos), _lib.as_f32(plddt), _lib.as_f32(surf_pos), _lib.as_f32(surf_feat)
        if p.ndim != 2 or p.shape[1] != 3 or q.shape != (p.shape[0],):
            raise ValueError(f"pos {p.shape} / plddt {q.shape}: expected [L, 3] and [L]")
        if sp.ndim != 2 or sp.shape[1] != 3 or sf.shape != (sp.shape[0], SURF_IN[0]):
            raise ValueError(f"surf_pos {sp.shape} / surf_feat {sf.shape}: expected [Ns, 3] and [Ns, {SURF_IN[0]}]")
        self.L = self.Ns = 0
        _lib.check(_lib.load().pgmi_s3f_set_structure(self._h, _lib.ptr(p, _lib._f32p), _lib.ptr(q, _lib._f32p), p.shape[0],
                                                      _lib.ptr(sp, _lib._f32p), _lib.ptr(sf, _lib._f32p), sp.shape[0]))
        self.L, self.Ns = p.shape[0], sp.shape[0]

    def graph(self):
        """dict: the residue edges (src, dst, e_s, e_v) as S2F.graph, and the surface's surf_src [Ns, 16], surf_res [Ns, 3],
        surf_res_dist [Ns, 3], surf_e_s [16 Ns, 64], surf_e_v [16 Ns, 3]."""
        n = C.c_int32()
        lib = _lib.load()
        none = [None] * 9
        _lib.check(lib.pgmi_s3f_graph(self._h, C.byref(n), *none))
        E, Ns, K = n.value, self.Ns, SURF_NEIGHBORS
        out = dict(src=np.empty(E, np.int32), dst=np.empty(E, np.int32), e_s=np.empty((E, s2f.EDGE_H[0]), np.float32),
                   e_v=np.empty((E, 3), np.float32), surf_src=np.empty((Ns, K), np.int32), surf_res=np.empty((Ns, SURF_RES_NEIGHBORS), np.int32),
                   surf_res_dist=np.empty((Ns, SURF_RES_NEIGHBORS), np.float32), surf_e_s=np.empty((Ns * K, s2f.EDGE_H[0]), np.float32),
                   surf_e_v=np.empty((Ns * K, 3), np.float32))
        _lib.check(lib.pgmi_s3f_graph(self._h, C.byref(n), *[_lib.ptr(a, _lib._i32p if a.dtype == np.int32 else _lib._f32p) for a in out.values()]))
        return out

    def gvp_forward(self, node_feat, seq_logits, pool_off=None, want_surface: bool = False):
        """node_feat [B, L, D], seq_logits [B, L, 20] -> lp [B, L, 20]; pool_off: CSR of the pool groups over the copies (default: each
        copy alone).  want_surface: also (surf_s [B, Ns, 256], surf_v [B, Ns, 16, 3], pool_sum [B, 256])."""
        x, q = _lib.as_f32(node_feat), _lib.as_f32(seq_logits)
        if x.ndim != 3 or x.shape[1:] != (self.L, self.D) or q.shape != (x.shape[0], self.L, 20):
            raise ValueError(f"node_feat {x.shape} / seq_logits {q.shape}: expected [B, {self.L}, {self.D}] and [B, {self.L}, 20]")
        B = x.shape[0]
        po = _lib.as_i32(pool_groups(B, 1) if pool_off is None else pool_off)
        lp = np.empty((B, self.L, 20), np.float32)
        ss = np.empty((B, self.Ns, s2f.NODE_H[0]), np.float32) if want_surface else None
        sv = np.empty((B, self.Ns, s2f.NODE_H[1], 3), np.float32) if want_surface else None
        ps = np.empty((B, s2f.NODE_H[0]), np.float32) if want_surface else None
        _lib.check(_lib.load().pgmi_s3f_gvp_forward(self._h, _lib.ptr(x, _lib._f32p), _lib.ptr(q, _lib._f32p), B, _lib.ptr(po, _lib._i32p),
                                                    po.size - 1, _lib.ptr(lp, _lib._f32p), _lib.ptr(ss, _lib._f32p), _lib.ptr(sv, _lib._f32p),
                                                    _lib.ptr(ps, _lib._f32p)))
        return (lp, ss, sv, ps) if want_surface else lp

    def set_logprobs(self, wt_tokens, set_off, set_pos, pool_off=None, want_full: bool = False):
        """S2F.set_logprobs with the pool groups over the sets (default: each set alone)."""
        wt, so, sp = _lib.as_i32(wt_tokens), _lib.as_i32(set_off), _lib.as_i32(set_pos)
        po = _lib.as_i32(pool_groups(so.size - 1, 1) if pool_off is None else pool_off)
        out = np.empty((int(so[-1]), 20), np.float32)
        full = np.empty((so.size - 1, self.L, 20), np.float32) if want_full else None
        _lib.check(_lib.load().pgmi_s3f_set_logprobs(self._h, _lib.ptr(wt, _lib._i32p), wt.size, _lib.ptr(s2f.AA_COLS, _lib._i32p),
                                                     _lib.ptr(so, _lib._i32p), _lib.ptr(sp, _lib._i32p), so.size - 1, _lib.ptr(po, _lib._i32p),
                                                     po.size - 1, _lib.ptr(out, _lib._f32p), _lib.ptr(full, _lib._f32p)))
        return (out, full) if want_full else out

    def profile_view(self, part: int):
        """The profiling view of the residue half (0) or the surface half (1), with EsmModel's profile methods."""
        return super().profile_view(part)

    def score_assay(self, dms_id: str, target_seq: str, rows, pos, plddt, s_start: int, s_end: int, surface, batch_size: int = 1) -> np.ndarray:
        """The sorted mutants (s2f.sort_mutants) of one assay against its structure and surface (load_surface): float32 [n].  One
        forward per masked sequence of the reference's list; a pooled row is shared by the sequences of one loader batch, so with
        batch_size > 1 equal site sets with different batch partners are forwarded again."""
        seqs, seq_of = masked_sequences(rows, dms_id, len(target_seq))
        groups = pool_groups(len(seqs), batch_size)
        tables: List[Optional[np.ndarray]] = [None] * len(seqs)
        i0 = 0
        while i0 < len(seqs):                                            # a run of sequences with one window
            win = seqs[i0][0]
            i1 = i0
            while i1 < len(seqs) and seqs[i1][0] == win:
                i1 += 1
            if batch_size > 1 and (i0 % batch_size or (i1 % batch_size and i1 != len(seqs))):
                raise ValueError(f"{dms_id}: a loader batch (batch_size {batch_size}) holds masked sequences of two windows around sequence "
                                 f"{i0 if i0 % batch_size else i1}; its pooled surface row spans two surfaces, which this path does not "
                                 "compute (batch_size 1 does not pool across sequences)")
            start, end = win
            p, q = s2f.cut_structure(pos, plddt, s_start, s_end, start, end)
            sp, sf = cut_surface(*surface, s_start, s_end, start, end)
            self.set_structure(p, q, sp, sf)
            set_off = np.cumsum([0] + [len(k) for _, k in seqs[i0:i1]]).astype(np.int32)
            set_pos = np.array([x for _, k in seqs[i0:i1] for x in k], dtype=np.int32)
            po = groups[(groups >= i0) & (groups <= i1)] - i0
            full = self.set_logprobs(s2f.tokenize(target_seq[start:end]), set_off, set_pos, po, want_full=True)[1]
            for i in range(i0, i1):
                tables[i] = full[i - i0:i - i0 + 1]
            i0 = i1
        return s2f.score_rows(rows, [(i, 0) for i in seq_of], tables, [w for w, _ in seqs])


def from_state_dict(sd, esm_cfg: dict, layers: int = s2f.LAYERS, device: int = 0, precision: str = "f16x3", max_rows: int = 0, **kw) -> S3F:
    esm_blob, blob = pack(sd, esm_cfg, layers)
    esm = pesm.EsmModel(esm_cfg, esm_blob, device=device, precision=precision, max_rows=max_rows)
    return S3F(blob, esm, layers=layers, device=device, **kw)


load_checkpoint = s2f.load_checkpoint
