"""ESM3 (esm3_open) scoring on libpgmi (include/pgmi.h, arch PGMI_ARCH_ESM3), with or without structure.

Replaces the ESM3 half of proteingym/baselines/evoscale/compute_fitness.py: ``score_mutations_with_pdb`` (:145-289, structure from a
PDB chain) and ``score_mutations`` (:20-143, sequence only) over ``_score_mutations_common`` (:292-474).  The trunk runs in HIP
(csrc/api_esm3.hip: ESM C's blocks, the folded multi-track embedding, block 0's geometric attention on csrc/geom_attention.hip);
the structure tokenizer (esm/models/vqvae.py StructureTokenEncoder) runs its geometric attention on the same kernel at S = 16 and
the rest in fp32 torch, once per distinct window.  What the reference does per position -- encode the window, tokenize its
structure, one masked forward -- is done per distinct window here, the masked rows of a window batched into one call.

The PDB reader is a restatement of esm/utils/structure/protein_chain.py:593-680 (ProteinChain.from_pdb) without biotite: model 1,
the first chain or ``chain_id``, ATOM records of amino-acid residues only, the first alternate location, MSE's selenium in the SD
column, a residue name without a one-letter form as X.
"""
from __future__ import annotations

import ctypes as C
import os
import re
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib, esmc
from .esmc import (AA_TO_TOKEN, CLS, EOS, HEAD_DIM, MASK, VOCAB, WINDOW_SIZE, Parsed, check_letters, combine, deinterleave_w1,  # noqa: F401
                   interleave_w1, masked_rows, parse_mutations, swiglu_hidden, tokenize, window)

# esm/utils/constants/esm3.py
STRUCTURE_VOCAB = 4096 + 5
STRUCTURE_MASK, STRUCTURE_EOS, STRUCTURE_BOS = 4096, 4097, 4098
KNN = 16                                                   # vqvae.py:194
RELPOS_BINS = 32                                           # vqvae.py:191-193
RELEASED = {"esm3_open": dict(embed_dim=1536, heads=24, layers=48, v_heads=256)}                       # pretrained.py:101-117
RELEASED_ENCODER = dict(d_model=1024, v_heads=128, layers=2, d_out=128, n_codes=4096)                  # pretrained.py:30-34
SNAPSHOT_MODEL = "data/weights/esm3_sm_open_v1.pth"
SNAPSHOT_ENCODER = "data/weights/esm3_structure_encoder_v0.pth"
# residue_constants.atom_types (the AlphaFold atom37 order)
ATOM37 = ["N", "CA", "C", "CB", "O", "CG", "CG1", "CG2", "OG", "OG1", "SG", "CD", "CD1", "CD2", "ND1", "ND2", "OD1", "OD2", "SD", "CE",
          "CE1", "CE2", "CE3", "NE", "NE1", "NE2", "OE1", "OE2", "CH2", "NH1", "NH2", "OH", "CZ", "CZ2", "CZ3", "NZ", "OXT"]
ATOM_ORDER = {a: i for i, a in enumerate(ATOM37)}
THREE_TO_ONE = {"ALA": "A", "ARG": "R", "ASN": "N", "ASP": "D", "CYS": "C", "GLN": "Q", "GLU": "E", "GLY": "G", "HIS": "H", "ILE": "I",
                "LEU": "L", "LYS": "K", "MET": "M", "PHE": "F", "PRO": "P", "SER": "S", "THR": "T", "TRP": "W", "TYR": "Y", "VAL": "V",
                "MSE": "M", "SEC": "U", "PYL": "O"}


# -- checkpoint ------------------------------------------------------------------------------------------------------------
def geom_keys(i: int) -> List[str]:
    p = f"transformer.blocks.{i}.geom_attn."
    return [p + "distance_scale_per_head", p + "rotation_scale_per_head", p + "s_norm.weight", p + "proj.weight", p + "out_proj.weight"]


def expected_keys(n_layers: int) -> List[str]:
    """The keys of ESM3.state_dict() that go into the blob, in blob order (include/pgmi.h); the five other output heads, the function
    and residue-annotation tables are not packed."""
    keys = ["encoder.sequence_embed.weight", "encoder.plddt_projection.weight", "encoder.plddt_projection.bias",
            "encoder.structure_per_res_plddt_projection.weight", "encoder.structure_per_res_plddt_projection.bias",
            "encoder.structure_tokens_embed.weight", "encoder.ss8_embed.weight", "encoder.sasa_embed.weight"]
    for i in range(n_layers):
        p = f"transformer.blocks.{i}."
        keys += [p + "attn.layernorm_qkv.0.weight", p + "attn.layernorm_qkv.0.bias", p + "attn.layernorm_qkv.1.weight",
                 p + "attn.q_ln.weight", p + "attn.k_ln.weight", p + "attn.out_proj.weight"]
        if i == 0:
            keys += geom_keys(0)
        keys += [p + "ffn.0.weight", p + "ffn.0.bias", p + "ffn.1.weight", p + "ffn.3.weight"]
    return keys + ["transformer.norm.weight"] + ["output_heads.sequence_head." + k for k in
                                                 ("0.weight", "0.bias", "2.weight", "2.bias", "3.weight", "3.bias")]


def shapes(cfg: dict) -> Dict[str, tuple]:
    """Shape of every packed key."""
    D, F, V, Hv = cfg["embed_dim"], cfg["ffn_dim"], cfg["vocab"], cfg["v_heads"]
    fixed = {"encoder.sequence_embed.weight": (V, D), "encoder.plddt_projection.weight": (D, 16),
             "encoder.structure_per_res_plddt_projection.weight": (D, 16), "encoder.structure_tokens_embed.weight": (STRUCTURE_VOCAB, D),
             "encoder.ss8_embed.weight": (11, D), "encoder.sasa_embed.weight": (19, D),
             "output_heads.sequence_head.0.weight": (D, D), "output_heads.sequence_head.3.weight": (V, D),
             "output_heads.sequence_head.3.bias": (V,)}
    tails = {"attn.layernorm_qkv.1.weight": (3 * D, D), "attn.out_proj.weight": (D, D), "ffn.1.weight": (2 * F, D), "ffn.3.weight": (D, F),
             "geom_attn.distance_scale_per_head": (Hv,), "geom_attn.rotation_scale_per_head": (Hv,), "geom_attn.proj.weight": (15 * Hv, D),
             "geom_attn.out_proj.weight": (D, 3 * Hv)}
    out = {}
    for k in expected_keys(cfg["layers"]):
        tail = k.split(".", 3)[-1] if k.startswith("transformer.blocks.") else None
        out[k] = fixed.get(k) or tails.get(tail, (D,))
    return out


OUTPUT_HEADS = ("sequence_head", "structure_head", "ss8_head", "sasa_head", "function_head", "residue_head")      # esm3.py:158-166


def state_dict_keys(n_layers: int) -> List[str]:
    """Every key of ESM3.state_dict() (tests/golden/esm3_state_dict_keys.json holds the reference's own list): the packed keys, the
    function and residue-annotation tables and the five output heads this path does not read."""
    keys = expected_keys(n_layers)
    keys += [f"encoder.function_embed.{k}.weight" for k in range(8)] + ["encoder.residue_embed.weight"]
    for h in OUTPUT_HEADS[1:]:
        keys += [f"output_heads.{h}." + k for k in ("0.weight", "0.bias", "2.weight", "2.bias", "3.weight", "3.bias")]
    return keys


def encoder_state_dict_keys(n_layers: int) -> List[str]:
    """Every key of StructureTokenEncoder.state_dict() (vqvae.py:182-194; blocks without plain attention, every Linear and LayerNorm
    with a bias)."""
    keys = []
    for i in range(n_layers):
        p = f"transformer.blocks.{i}."
        keys += [p + "geom_attn.distance_scale_per_head", p + "geom_attn.rotation_scale_per_head"]
        keys += [p + m + b for m in ("geom_attn.s_norm", "geom_attn.proj", "geom_attn.out_proj", "ffn.0", "ffn.1", "ffn.3") for b in (".weight", ".bias")]
    return keys + ["pre_vq_proj.weight", "pre_vq_proj.bias", "codebook.embeddings", "codebook.N", "codebook.z_avg",
                   "relative_positional_embedding.embedding.weight"]


def config_from_state_dict(sd, model_type: Optional[str] = None) -> dict:
    """d from the sequence table, layers from the block count, the SwiGLU width from ffn.1.weight, heads = d / 64, v_heads from the
    geometric attention's scale vector."""
    D = int(np.shape(sd["encoder.sequence_embed.weight"])[1])
    L = 0
    while f"transformer.blocks.{L}.attn.out_proj.weight" in sd:
        L += 1
    if L == 0 or D % HEAD_DIM or "transformer.blocks.0.geom_attn.proj.weight" not in sd:
        raise ValueError(f"not an ESM3 state dict: d_model {D}, {L} blocks (head_dim 64 needs d % 64 == 0; block 0 has geom_attn)")
    F = int(np.shape(sd["transformer.blocks.0.ffn.1.weight"])[0]) // 2
    Hv = int(np.shape(sd["transformer.blocks.0.geom_attn.distance_scale_per_head"])[0])
    cfg = dict(layers=L, embed_dim=D, heads=D // HEAD_DIM, ffn_dim=F, vocab=VOCAB, v_heads=Hv)
    if model_type is not None:
        if model_type not in RELEASED:
            raise ValueError(f"model_type {model_type!r}: this path scores {sorted(RELEASED)}")
        shape = dict(embed_dim=D, heads=D // HEAD_DIM, layers=L, v_heads=Hv)
        if shape != RELEASED[model_type]:
            print(f"Warning: checkpoint {shape} is not the released {model_type} configuration {RELEASED[model_type]}")
    return cfg


def check_state_dict(sd, where: str = "state dict") -> dict:
    """Keys against the reference's own list, shapes of the packed keys, and the zero padding rows the embedding fold relies on."""
    cfg = config_from_state_dict(sd)
    want = state_dict_keys(cfg["layers"])
    missing, unexpected = sorted(set(want) - set(sd)), sorted(set(sd) - set(want))
    if missing or unexpected:
        raise ValueError(f"{where}: not an ESM3 state dict (missing {missing[:5]}, unexpected {unexpected[:5]})")
    for k, s in shapes(cfg).items():
        if tuple(np.shape(sd[k])) != s:
            raise ValueError(f"{where}: {k} has shape {tuple(np.shape(sd[k]))}, expected {s}")
    for k in range(8):
        if np.any(np.asarray(sd[f"encoder.function_embed.{k}.weight"])[0] != 0):
            raise ValueError(f"{where}: encoder.function_embed.{k}.weight[0] (the padding row) is not zero: the embedding fold takes it as zero")
    return cfg


def _torch_load(path: str) -> Dict[str, np.ndarray]:
    import torch
    raw = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(raw, dict):
        raise ValueError(f"{path}: expected a state dict, got {type(raw).__name__}")
    return {k: (v.detach().to(torch.float32).numpy() if v.is_floating_point() else v.numpy()) for k, v in raw.items()}


def load_state_dicts(path: str) -> Tuple[Dict[str, np.ndarray], Optional[Dict[str, np.ndarray]]]:
    """(ESM3 state dict, structure encoder state dict or None) from a snapshot directory holding data/weights/esm3_sm_open_v1.pth and
    esm3_structure_encoder_v0.pth (also looked for next to each other), or from the model's .pth alone (the encoder then from the same
    directory if it is there).  Floats upcast to fp32.  Never downloads."""
    if os.path.isdir(path):
        cands = [(os.path.join(path, SNAPSHOT_MODEL), os.path.join(path, SNAPSHOT_ENCODER)),
                 (os.path.join(path, os.path.basename(SNAPSHOT_MODEL)), os.path.join(path, os.path.basename(SNAPSHOT_ENCODER)))]
        found = [c for c in cands if os.path.isfile(c[0])]
        if not found:
            raise FileNotFoundError(f"{path}: no ESM3 weights at {SNAPSHOT_MODEL}")
        model_path, enc_path = found[0]
    else:
        if not os.path.isfile(path):
            raise FileNotFoundError(path)
        model_path, enc_path = path, os.path.join(os.path.dirname(path), os.path.basename(SNAPSHOT_ENCODER))
    sd = _torch_load(model_path)
    check_state_dict(sd, model_path)
    enc = None
    if os.path.isfile(enc_path):
        enc = _torch_load(enc_path)
        check_encoder_state_dict(enc, enc_path)
    return sd, enc


def weight_count(cfg: dict) -> int:
    return int(sum(int(np.prod(s)) for s in shapes(cfg).values()))


def pack(cfg: dict, sd) -> np.ndarray:
    """The blob of include/pgmi.h (PGMI_ARCH_ESM3): the packed keys in expected_keys order, ffn.1.weight interleaved."""
    shp = shapes(cfg)
    blob = np.empty(weight_count(cfg), dtype=np.float32)
    o = 0
    for k in expected_keys(cfg["layers"]):
        a = np.asarray(sd[k], dtype=np.float32)
        if a.shape != shp[k]:
            raise ValueError(f"{k} has shape {a.shape}, expected {shp[k]}")
        if k.endswith("ffn.1.weight"):
            a = interleave_w1(a)
        blob[o:o + a.size] = a.ravel()
        o += a.size
    assert o == blob.size
    return blob


def unpack(cfg: dict, blob: np.ndarray) -> Dict[str, np.ndarray]:
    """Inverse of pack."""
    sd, o = {}, 0
    for k, s in shapes(cfg).items():
        n = int(np.prod(s))
        a = blob[o:o + n].reshape(s)
        sd[k] = deinterleave_w1(a) if k.endswith("ffn.1.weight") else a
        o += n
    assert o == blob.size
    return sd


# -- structure encoder checkpoint ------------------------------------------------------------------------------------------
def encoder_config_from_state_dict(sd) -> dict:
    L = 0
    while f"transformer.blocks.{L}.geom_attn.proj.weight" in sd:
        L += 1
    if L == 0:
        raise ValueError("not a StructureTokenEncoder state dict: no geometric blocks")
    D = int(np.shape(sd["pre_vq_proj.weight"])[1])
    return dict(d_model=D, v_heads=int(np.shape(sd["transformer.blocks.0.geom_attn.distance_scale_per_head"])[0]), layers=L,
                d_out=int(np.shape(sd["pre_vq_proj.weight"])[0]), n_codes=int(np.shape(sd["codebook.embeddings"])[0]),
                ffn_dim=int(np.shape(sd["transformer.blocks.0.ffn.1.weight"])[0]) // 2)


def check_encoder_state_dict(sd, where: str = "state dict") -> dict:
    cfg = encoder_config_from_state_dict(sd)
    want = encoder_state_dict_keys(cfg["layers"])
    missing, unexpected = sorted(set(want) - set(sd)), sorted(set(sd) - set(want))
    if missing or unexpected:
        raise ValueError(f"{where}: not a StructureTokenEncoder state dict (missing {missing[:5]}, unexpected {unexpected[:5]})")
    return cfg


# -- geometry (fp32, the reference's operation order) -------------------------------------------------------------------------
def _gram_schmidt(neg_x_axis, origin, xy_plane):
    """affine3d.py:288-323 (Affine3D.from_graham_schmidt, eps 1e-10): rot [n,3,3] with columns (x, e1, e2), trans."""
    f = np.float32
    x_axis = origin - neg_x_axis
    e1 = xy_plane - origin
    x_axis = x_axis / np.sqrt((x_axis ** 2).sum(-1, keepdims=True, dtype=f) + f(1e-10))
    dot = (x_axis * e1).sum(-1, keepdims=True, dtype=f)
    e1 = e1 - x_axis * dot
    e1 = e1 / np.sqrt((e1 ** 2).sum(-1, keepdims=True, dtype=f) + f(1e-10))
    e2 = np.cross(x_axis, e1).astype(f)
    return np.stack([x_axis, e1, e2], axis=-1).astype(f), origin.astype(f)


def build_frames(coords: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """affine3d.py:326-374 (build_affine3d_from_coordinates) for one chain: coords [T, >=3, 3] (N, CA, C first) -> rot [T,9] row-major,
    trans [T,3], mask [T].  A token has a frame when its N, CA and C are finite and below 1e6; the others carry the frame of the mean
    N / CA / C of the framed tokens, or the identity (translation 0) when there is none."""
    f = np.float32
    c = np.array(coords[:, :3, :], dtype=f)
    with np.errstate(invalid="ignore"):
        mask = (np.isfinite(c) & (c < 1e6)).all(-1).all(-1)
    c[~mask] = 0
    avg = (c.sum(0, dtype=f) / f(np.float32(mask.sum()) + f(1e-8))).astype(f)            # [3,3]: mean N, CA, C
    hole_rot, hole_trans = _gram_schmidt(avg[2][None], avg[1][None], avg[0][None])
    if not mask.any():
        hole_rot = np.eye(3, dtype=f)[None]
    rot, trans = _gram_schmidt(c[:, 2], c[:, 1], c[:, 0])
    rot = np.where(mask[:, None, None], rot, hole_rot)
    trans = np.where(mask[:, None], trans, hole_trans)
    return np.ascontiguousarray(rot.reshape(-1, 9), dtype=f), np.ascontiguousarray(trans, dtype=f), mask


def normalize_coordinates(atom37: np.ndarray) -> np.ndarray:
    """normalize_coordinates.py:34-79: coordinates in the frame of the chain's mean N / CA / C (Gram-Schmidt, origin at the mean CA);
    unchanged when that frame's translation is 0; infinite entries stay infinite."""
    f = np.float32
    x = np.array(atom37, dtype=f)
    bb = x[:, :3, :]
    mask = np.isfinite(bb).all(-1).all(-1)
    avg = (np.where(mask[:, None, None], bb, f(0)).sum(0, dtype=f) / f(np.float32(mask.sum()) + f(1e-8))).astype(f)
    rot, trans = _gram_schmidt(avg[2][None], avg[1][None], avg[0][None])
    R, t = rot[0], trans[0]
    if not np.sqrt((t ** 2).sum(dtype=f)) > 0:
        return x
    inv_t = -(R.T @ t).astype(f)                       # Affine3D.invert: rot^T, -rot^T trans
    is_inf = np.isinf(x)
    with np.errstate(invalid="ignore"):
        y = (np.einsum("ij,laj->lai", R.T, x).astype(f) + inv_t).astype(f)
    y[is_inf] = np.inf
    return y


def per_res_plddt(coords: np.ndarray) -> np.ndarray:
    """esm3.py:522-526: 1 where any atom of the token has all-finite coordinates."""
    return np.isfinite(coords).all(-1).any(-1).astype(np.int32)


# -- PDB ---------------------------------------------------------------------------------------------------------------------
class Chain:
    """What score_mutations_with_pdb reads of a ProteinChain."""

    def __init__(self, sequence, atom37_positions, residue_index, insertion_code):
        self.sequence, self.atom37_positions = sequence, atom37_positions
        self.residue_index, self.insertion_code = residue_index, insertion_code


def read_pdb(path_or_lines, chain_id: Optional[str] = None) -> Chain:
    """protein_chain.py:593-680 restated (module docstring).  path_or_lines: a path, or the file's lines."""
    if isinstance(path_or_lines, (str, os.PathLike)):
        with open(path_or_lines) as f:
            lines = f.read().splitlines()
    else:
        lines = list(path_or_lines)
    atoms = []                                         # (hetero, chain, res_id, ins_code, res_name, atom_name, xyz)
    for line in lines:
        rec = line[:6]
        if rec.startswith("ENDMDL"):
            break                                      # model 1
        if rec not in ("ATOM  ", "HETATM"):
            continue
        atoms.append((rec == "HETATM", line[21], int(line[22:26]), line[26].strip(), line[17:20].strip(), line[12:16].strip(), line[16],
                      (float(line[30:38]), float(line[38:46]), float(line[46:54]))))
    if not atoms:
        raise ValueError("no atoms in the PDB file")
    if chain_id is None or chain_id == "detect":
        chain_id = atoms[0][1]
    residues, key, seen = [], None, set()
    for hetero, ch, res_id, ins, res_name, atom_name, altloc, xyz in atoms:
        # amino-acid, non-hetero atoms of the chain: a three-letter residue name that is not water (nucleotides have shorter names)
        if hetero or ch != chain_id or len(res_name) != 3 or res_name == "HOH":
            continue
        k = (res_id, ins, res_name)
        if k != key:
            residues.append((res_id, ins, res_name, []))
            key, seen = k, set()
        if atom_name in seen:                          # another alternate location of an atom already read
            continue
        seen.add(atom_name)
        residues[-1][3].append((atom_name, xyz))
    n = len(residues)
    pos = np.full((n, 37, 3), np.nan, dtype=np.float32)
    residue_index = np.full(n, -1, dtype=np.int64)
    insertion_code = np.full(n, "", dtype="<U4")
    seq = []
    for i, (res_id, ins, res_name, res_atoms) in enumerate(residues):
        seq.append(THREE_TO_ONE.get(res_name, "X"))
        residue_index[i], insertion_code[i] = res_id, ins
        for atom_name, xyz in res_atoms:
            if atom_name == "SE" and res_name == "MSE":
                atom_name = "SD"                       # the selenium in the sulphur column
            if atom_name in ATOM_ORDER:
                pos[i, ATOM_ORDER[atom_name]] = xyz
    return Chain("".join(seq), pos, residue_index, insertion_code)


def residue_map(chain: Chain, pdb_range: Optional[str] = None) -> Dict[int, int]:
    """compute_fitness.py:196-227: {position in the target sequence: index in the chain}.  pdb_range "start-end" shifts the PDB's
    numbering by start - 1 (a range that does not parse: no shift, with the reference's warning).  A residue with an insertion code
    fails as the reference's int("12A") does."""
    pdb_offset = 0
    if pdb_range is not None and not (isinstance(pdb_range, float) and np.isnan(pdb_range)) and pdb_range:
        try:
            start, _end = map(int, str(pdb_range).split("-"))
            pdb_offset = start - 1
        except Exception:
            print(f"Warning: Could not parse pdb_range '{pdb_range}', using no offset")
    out = {}
    for i, residue_id in enumerate(chain.residue_index):
        ins = chain.insertion_code[i] if chain.insertion_code is not None else ""
        rid = f"{residue_id}{ins}" if ins and ins.strip() else residue_id
        out[int(rid) + pdb_offset] = i
    return out


def parse_mutations_pdb(mutations: Sequence[str], id_to_idx: Dict[int, int]) -> List[Parsed]:
    """compute_fitness.py:229-286: as esmc.parse_mutations, but a part is valid when its position is in the PDB; there is no
    wild-type check on this path.  A multi-mutant is dropped on its first bad part."""
    out = []
    for mutation in mutations:
        parts = mutation.split(":") if ":" in mutation else [mutation]
        wt_s, mt_s, pos, seq_pos, ok = "", "", [], [], True
        for part in parts:
            m = re.match(r"([A-Z])(\d+)([A-Z])", part)
            if not m:
                print(f"Warning: Could not parse mutation {part}, skipping")
                ok = False
                break
            wt, p, mt = m.group(1), int(m.group(2)), m.group(3)
            if p not in id_to_idx:
                print(f"Warning: Position {p} not found in PDB, skipping")
                ok = False
                break
            wt_s, mt_s = wt_s + wt, mt_s + mt
            pos.append(p)
            seq_pos.append(id_to_idx[p])
        if ok:
            out.append((wt_s, pos, mt_s, seq_pos, mutation))
    return out


# -- structure tokenizer -----------------------------------------------------------------------------------------------------
def geom_attention(proj, rot, trans, mask, w_rot, w_dist, per_row_frames: bool, device: int = 0) -> np.ndarray:
    """pgmi_op_geom_attention: proj [B,S,15H], frames [B or 1... ,S,.], softplus-ed per-head weights [H] -> [B,S,3H]."""
    proj = _lib.as_f32(proj)
    B, S, W = proj.shape
    H = W // 15
    out = np.empty((B, S, 3 * H), dtype=np.float32)
    rot, trans, mask = _lib.as_f32(rot), _lib.as_f32(trans), _lib.as_i32(mask)
    n = B if per_row_frames else 1
    assert rot.size == n * S * 9 and trans.size == n * S * 3 and mask.size == n * S and W == 15 * H
    w_rot, w_dist = _lib.as_f32(w_rot), _lib.as_f32(w_dist)
    _lib.check(_lib.load().pgmi_op_geom_attention(device, _lib.ptr(proj, _lib._f32p), _lib.ptr(rot, _lib._f32p), _lib.ptr(trans, _lib._f32p),
                                                  _lib.ptr(mask, _lib._i32p), int(per_row_frames), _lib.ptr(w_rot, _lib._f32p),
                                                  _lib.ptr(w_dist, _lib._f32p), B, S, H, _lib.ptr(out, _lib._f32p)))
    return out


class StructureEncoder:
    """vqvae.py StructureTokenEncoder.encode for one chain: k-NN (16) on CA, neighbourhood frames, relative-position embedding
    (clamped to +-32), the geometric-only blocks (bias, expansion 4), pre_vq_proj, nearest code.  The geometric attention runs on
    libpgmi's kernel (one batch row per residue, S = the neighbourhood), everything else in fp32 torch on ``torch_device``.

    The reference's encoder blocks do not zero frameless queries (mask_and_zero_frameless is off there) and the kernel does.  That
    changes no token: a neighbourhood's frameless rows are masked as keys in every block, so row 0 of a framed residue never reads
    them, and the embedding of a frameless residue is replaced by zero before pre_vq_proj (vqvae.py:320)."""

    def __init__(self, sd: Dict[str, np.ndarray], device: int = 0, torch_device: Optional[str] = None, attention=None):
        import torch
        self.cfg = encoder_config_from_state_dict(sd)
        self.device = device
        self.torch_device = torch.device(torch_device or "cpu")
        self.w = {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(self.torch_device) for k, v in sd.items()
                  if np.asarray(v).dtype.kind == "f"}
        self.attention = attention or (lambda *a: geom_attention(*a, per_row_frames=True, device=self.device))

    @staticmethod
    def knn_edges(ca: np.ndarray, mask: np.ndarray) -> np.ndarray:
        """misc.py:85-124 (knn_graph) for one unpadded chain: [L, min(16, L)] neighbour indices, the residue itself first."""
        import torch
        L = len(ca)
        c = torch.from_numpy(np.nan_to_num(np.asarray(ca, dtype=np.float32)))
        m = torch.from_numpy(np.asarray(mask, dtype=bool))
        valid = m[None, :] & m[:, None]
        dists = (c.unsqueeze(-2) - c.unsqueeze(-3)).norm(dim=-1)
        ar = torch.arange(L)
        seq = (ar.unsqueeze(-1) - ar.unsqueeze(-2)).abs().to(dists.dtype).mul(1e2).add(1e6)
        _, edges = torch.where(valid, dists, seq).sort(dim=-1, descending=False)
        return edges[:, :min(KNN, L)].numpy()

    def embed(self, atom37: np.ndarray):
        """(normalized coordinates [L,37,3], pre-quantisation embedding z [L, d_out] as a torch tensor, frame mask [L])."""
        import torch
        import torch.nn.functional as TF
        w, dev = self.w, self.torch_device
        coords = normalize_coordinates(atom37)
        rot, trans, mask = build_frames(coords)
        L = len(coords)
        bb = np.array(coords[:, :3, :], dtype=np.float32)
        bb[~mask] = 0                                                   # vqvae.py:278-279
        edges = self.knn_edges(bb[:, 1], mask)
        E = edges.shape[1]
        k_rot, k_trans, k_mask = rot[edges], trans[edges], mask[edges].astype(np.int32)      # [L,E,.]
        res = np.arange(1, L + 1, dtype=np.int64)[edges]                # from_atom37: residue_index 1 .. L
        diff = np.clip(res - res[:, :1], -RELPOS_BINS, RELPOS_BINS) + RELPOS_BINS + 1
        z = w["relative_positional_embedding.embedding.weight"][torch.from_numpy(diff).to(dev)]          # [L,E,D]
        D = z.shape[-1]
        for i in range(self.cfg["layers"]):
            p = f"transformer.blocks.{i}."
            ns = TF.layer_norm(z, (D,), w[p + "geom_attn.s_norm.weight"], w[p + "geom_attn.s_norm.bias"])
            pr = TF.linear(ns, w[p + "geom_attn.proj.weight"], w[p + "geom_attn.proj.bias"])
            ctx = self.attention(pr.cpu().numpy(), k_rot, k_trans, k_mask, TF.softplus(w[p + "geom_attn.rotation_scale_per_head"]).cpu().numpy(),
                                 TF.softplus(w[p + "geom_attn.distance_scale_per_head"]).cpu().numpy())
            z = z + TF.linear(torch.from_numpy(ctx).to(dev), w[p + "geom_attn.out_proj.weight"], w[p + "geom_attn.out_proj.bias"])
            h = TF.linear(TF.layer_norm(z, (D,), w[p + "ffn.0.weight"], w[p + "ffn.0.bias"]), w[p + "ffn.1.weight"], w[p + "ffn.1.bias"])
            x1, x2 = h.chunk(2, dim=-1)
            z = z + TF.linear(TF.silu(x1) * x2, w[p + "ffn.3.weight"], w[p + "ffn.3.bias"])
        z0 = z[:, 0, :].masked_fill(~torch.from_numpy(mask).to(dev)[:, None], 0)
        return coords, TF.linear(z0, w["pre_vq_proj.weight"], w["pre_vq_proj.bias"]), mask

    def distances(self, y):
        """codebook.py:63-67."""
        e = self.w["codebook.embeddings"]
        return (y ** 2).sum(dim=1, keepdim=True) - 2 * y @ e.t() + (e.t() ** 2).sum(dim=0, keepdim=True)

    def encode(self, atom37: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        """(normalized coordinates [L,37,3] fp32, structure tokens [L] int32) for the residues of one window."""
        coords, y, _ = self.embed(atom37)
        return coords, self.distances(y).argmin(dim=1).cpu().numpy().astype(np.int32)


def pad_window(coords: np.ndarray, tokens: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """encoding.py:97-109: infinite coordinates and the BOS / EOS structure tokens around the residues."""
    c = np.full((len(coords) + 2,) + coords.shape[1:], np.inf, dtype=np.float32)
    c[1:-1] = coords
    t = np.concatenate([[STRUCTURE_BOS], np.asarray(tokens, dtype=np.int32), [STRUCTURE_EOS]]).astype(np.int32)
    return c, t


# -- model -----------------------------------------------------------------------------------------------------------------
class ESM3(_lib.ModelHandle):
    """Device-resident ESM3 trunk (f16x3) with, optionally, its structure encoder."""
    CREATE = "pgmi_esm3_model_create"

    def __init__(self, cfg: dict, weights: np.ndarray, device: int = 0, max_rows: int = 0, encoder: Optional[StructureEncoder] = None):
        super().__init__(cfg, weights, device, max_rows, arch_arg=int(cfg["v_heads"]), arch=_lib.ARCH_ESM3, vocab=VOCAB, ln_eps=1e-5)
        self.encoder = encoder
        self.windows_encoded = 0

    @staticmethod
    def _weight_count(lib, c, arch_arg):
        return lib.pgmi_esm3_weight_count(C.byref(c), arch_arg)

    def set_window(self, T: int, structure_tokens=None, coords=None):
        """Binds the structure of a window of T tokens (<cls> + residues + <eos>): structure tokens [T] and coordinates [T, >=3, 3]
        (N, CA, C first; non-finite where missing, the <cls> / <eos> rows included).  Both None: sequence-only scoring -- every
        residue's structure token is the mask token, no token has a frame (the geometric branch is skipped), per_res_plddt is 0."""
        if structure_tokens is None:
            structure_tokens = np.concatenate([[STRUCTURE_BOS], np.full(T - 2, STRUCTURE_MASK), [STRUCTURE_EOS]])
        st = _lib.as_i32(structure_tokens)
        if coords is None:
            coords = np.full((T, 3, 3), np.nan, dtype=np.float32)
        coords = np.asarray(coords, dtype=np.float32)
        if st.shape != (T,) or coords.shape[0] != T:
            raise ValueError(f"window of {T} tokens: structure tokens {st.shape}, coordinates {coords.shape}")
        rot, trans, mask = build_frames(coords)
        pl, fm = per_res_plddt(coords), _lib.as_i32(mask)
        _lib.check(_lib.load().pgmi_esm3_set_structure(self._h, _lib.ptr(st, _lib._i32p), _lib.ptr(pl, _lib._i32p), _lib.ptr(rot, _lib._f32p),
                                                       _lib.ptr(trans, _lib._f32p), _lib.ptr(fm, _lib._i32p), T))

    token_logprobs = esmc.ESMC.token_logprobs
    masked_logprobs = esmc.ESMC.masked_logprobs

    def _score(self, sequence: str, parsed: Sequence[Parsed], atom37, window_size: int) -> Dict[str, float]:
        """compute_fitness.py:292-474 with the positions grouped by window: one tokenizer pass and one batched call per window."""
        if not parsed:
            print("No valid mutations to score")
            return {}
        check_letters(parsed)
        positions = sorted({p for _, _, _, sp, _ in parsed for p in sp})
        by_window: Dict[Tuple[int, int], List[int]] = {}
        for p in positions:
            by_window.setdefault(window(p, len(sequence), window_size), []).append(p)
        lp_by_pos = {}
        for (s, e), ps in by_window.items():
            T = e - s + 2
            if atom37 is None:
                self.set_window(T)
            else:
                if self.encoder is None:
                    raise ValueError("scoring with structure needs the structure encoder's weights (esm3_structure_encoder_v0.pth)")
                coords, tokens = self.encoder.encode(atom37[s:e])
                self.windows_encoded += 1
                padded_coords, padded_tokens = pad_window(coords, tokens)
                self.set_window(T, padded_tokens, padded_coords)
            tokens, mask = masked_rows(sequence, ps, window_size)
            lp_by_pos.update(zip(ps, self.masked_logprobs(tokens, mask)))
        return combine(parsed, lp_by_pos)

    def score_mutations(self, sequence: str, mutations: Sequence[str], window_size: int = WINDOW_SIZE) -> Dict[str, float]:
        """compute_fitness.py score_mutations with an ESM3 model: sequence only, the wild type checked against ``sequence``."""
        if len(sequence) == 0:
            raise ValueError("Empty sequence provided")
        return self._score(sequence, parse_mutations(sequence, mutations), None, window_size)

    def score_mutations_with_pdb(self, pdb_path, mutations: Sequence[str], chain_id: Optional[str] = None, use_structure: bool = True,
                                 window_size: int = WINDOW_SIZE, pdb_range: Optional[str] = None) -> Dict[str, float]:
        """compute_fitness.py score_mutations_with_pdb: the sequence is the PDB chain's, positions map through its residue numbers."""
        chain = read_pdb(pdb_path, chain_id)
        if len(chain.sequence) == 0:
            raise ValueError("Could not extract valid sequence from PDB file")
        print(f"Extracted sequence of length {len(chain.sequence)} from PDB")
        parsed = parse_mutations_pdb(mutations, residue_map(chain, pdb_range))
        return self._score(chain.sequence, parsed, chain.atom37_positions if use_structure else None, window_size)


def from_state_dict(sd, encoder_sd=None, device: int = 0, max_rows: int = 0, model_type: Optional[str] = None,
                    torch_device: Optional[str] = None) -> ESM3:
    cfg = config_from_state_dict(sd, model_type)
    enc = StructureEncoder(encoder_sd, device=device, torch_device=torch_device) if encoder_sd is not None else None
    return ESM3(cfg, pack(cfg, sd), device=device, max_rows=max_rows, encoder=enc)


def from_pretrained(path: str, model_type: Optional[str] = "esm3_open", device: int = 0, max_rows: int = 0,
                    torch_device: Optional[str] = None) -> ESM3:
    sd, enc = load_state_dicts(path)
    return from_state_dict(sd, enc, device=device, max_rows=max_rows, model_type=model_type, torch_device=torch_device)
