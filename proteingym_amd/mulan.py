"""MULAN scoring on libpgmi (include/pgmi.h, arch PGMI_ARCH_MULAN).

Replaces the model and data side of proteingym/baselines/mulan (compute_fitness.py, mulan/{model.py,model_utils.py,dataset.py,
tokenizer.py,pdb_utils.py}): a checkpoint directory (config.json, model.safetensors or pytorch_model.bin) is packed into ESM2's blob
followed by the structure adapter's weights, the forward runs in HIP (csrc/api_mulan.hip on the ESM2 encoder), and ``score_chunk``
reproduces ``calc_fitness`` / ``predict_mut`` (compute_fitness.py:27-94) for one structure chunk.  The reference runs one forward per
mutant; its masked input -- tokens and angle rows -- depends only on the SET of mutated positions, so every distinct set is forwarded
once (saprot.position_sets).  The per-residue angle rows come from the reference's cached dataset folder or from the structure file
through the dihedral routine below.  Nothing is downloaded.
"""
from __future__ import annotations

import gzip
import io
import json
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from . import esm as pesm
from . import saprot

N_ANGLES = 7                                               # phi, psi, chi1 .. chi5 (model.py:16 struct_data_dim)
PAD_VALUE = 4.0                                            # tokenizer.py:39
MASK_VALUE = -4.0                                          # compute_fitness.py:124
NAN_DEGREES = 182.0                                        # tokenizer.py:38 (nan_fill_value)
PLDDT_THRESHOLD = 70.0                                     # dataset.py:311: rows with pLDDT <= 70 are padded
MAX_PEPTIDE_BOND = 1.8                                     # pdb_utils.py:20
LN_EPS = 1e-5
ROW_WIDTH = 11                                             # the stored row: bfactor, x, y, z, phi, psi, chi1 .. chi5
ADAPTER = "esm.embeddings.struct_embeddings."
# tokenizer.py:33-35: the number of chi angles stored per residue letter; the rest of the row is padding
ROT_LEN = {"N": 2, "W": 2, "G": 0, "I": 2, "D": 2, "V": 1, "K": 4, "F": 2, "R": 5, "H": 2, "M": 3, "T": 1, "S": 1, "Q": 3, "L": 2,
           "A": 0, "C": 1, "P": 2, "E": 3, "Y": 2, "X": 5}
THREE_TO_ONE = {"ALA": "A", "ARG": "R", "ASN": "N", "ASP": "D", "CYS": "C", "GLN": "Q", "GLU": "E", "GLY": "G", "HIS": "H", "ILE": "I",
                "LEU": "L", "LYS": "K", "MET": "M", "PHE": "F", "PRO": "P", "SER": "S", "THR": "T", "TRP": "W", "TYR": "Y", "VAL": "V"}
# the standard side-chain dihedrals: chi_n of a residue is the dihedral of atoms n-1 .. n+2 of its list
CHI_ATOMS = {
    "ARG": ("N", "CA", "CB", "CG", "CD", "NE", "CZ", "NH1"), "ASN": ("N", "CA", "CB", "CG", "OD1"), "ASP": ("N", "CA", "CB", "CG", "OD1"),
    "CYS": ("N", "CA", "CB", "SG"), "GLN": ("N", "CA", "CB", "CG", "CD", "OE1"), "GLU": ("N", "CA", "CB", "CG", "CD", "OE1"),
    "HIS": ("N", "CA", "CB", "CG", "ND1"), "ILE": ("N", "CA", "CB", "CG1", "CD1"), "LEU": ("N", "CA", "CB", "CG", "CD1"),
    "LYS": ("N", "CA", "CB", "CG", "CD", "CE", "NZ"), "MET": ("N", "CA", "CB", "CG", "SD", "CE"), "PHE": ("N", "CA", "CB", "CG", "CD1"),
    "PRO": ("N", "CA", "CB", "CG", "CD"), "SER": ("N", "CA", "CB", "OG"), "THR": ("N", "CA", "CB", "OG1"),
    "TRP": ("N", "CA", "CB", "CG", "CD1"), "TYR": ("N", "CA", "CB", "CG", "CD1"), "VAL": ("N", "CA", "CB", "CG1"),
    "MSE": ("N", "CA", "CB", "CG", "SE", "CE"),
}


# -- angle rows ----------------------------------------------------------------------------------------------------------------
def dihedral(p0, p1, p2, p3) -> float:
    """The dihedral angle of four points in degrees, in (-180, 180], IUPAC sign (cis = 0)."""
    b0, b1, b2 = np.asarray(p0, float) - p1, np.asarray(p2, float) - p1, np.asarray(p3, float) - p2
    b1 = b1 / np.linalg.norm(b1)
    v, w = b0 - np.dot(b0, b1) * b1, b2 - np.dot(b2, b1) * b1
    return float(np.degrees(np.arctan2(np.dot(np.cross(b1, v), w), np.dot(v, w))))


def read_chain(pdb_path: str, chain: str = "A") -> List[Tuple[str, Dict[str, np.ndarray], float]]:
    """The residues of `chain` in the first model of a PDB file, in file order: (residue name, atom name -> coordinates, B-factor of
    CA).  ATOM records and HETATM records of MSE; the first alternate location; a residue without CA is an error, as in
    AnglesFromStructure (pdb_utils.py:59)."""
    out, index = [], {}
    with open(pdb_path) as f:
        for line in f:
            rec = line[:6]
            if rec.startswith("ENDMDL"):
                break
            if not (rec == "ATOM  " or (rec == "HETATM" and line[17:20] == "MSE")) or line[21] != chain:
                continue
            if line[16] not in " A1":
                continue
            key = (line[22:27], line[17:20])
            if key not in index:
                index[key] = len(out)
                out.append([line[17:20].strip(), {}, None])
            r = out[index[key]]
            name = line[12:16].strip()
            if name not in r[1]:
                r[1][name] = np.array([float(line[30:38]), float(line[38:46]), float(line[46:54])])
                if name == "CA":
                    r[2] = float(line[60:66])
    for name, atoms, b in out:
        if b is None:
            raise KeyError(f"{pdb_path}: a {name} residue of chain {chain} has no CA atom")
    return [(n, a, b) for n, a, b in out]


def structure_rows(pdb_path: str, chain: str = "A") -> Tuple[str, np.ndarray]:
    """(dataset sequence, rows [L][11]) of one structure file, as tokenizer.py:42-90 stores them: per residue bfactor, x, y, z of CA,
    then phi, psi, chi1 .. chi_k in radians (from degrees rounded to 2 decimals; undefined: 182 degrees) with k = ROT_LEN of the
    letter, padded with 4.0.  Residues other than the 20 standard ones and MSE (letter X) are dropped after the angles are taken
    (preproc_df).  A peptide bond longer than 1.8 A is a chain break: no psi before it and no phi after it."""
    res = read_chain(pdb_path, chain)
    seq, rows = [], []
    for i, (name, atoms, bfac) in enumerate(res):
        letter = THREE_TO_ONE.get(name, "X" if name == "MSE" else None)
        if letter is None:
            continue

        def bonded(a, b):
            return "C" in a and "N" in b and np.linalg.norm(a["C"] - b["N"]) <= MAX_PEPTIDE_BOND
        ang = [np.nan] * N_ANGLES
        bb = all(k in atoms for k in ("N", "CA", "C"))
        if bb and i > 0 and bonded(res[i - 1][1], atoms):
            ang[0] = dihedral(res[i - 1][1]["C"], atoms["N"], atoms["CA"], atoms["C"])
        if bb and i + 1 < len(res) and bonded(atoms, res[i + 1][1]):
            ang[1] = dihedral(atoms["N"], atoms["CA"], atoms["C"], res[i + 1][1]["N"])
        chain_atoms = CHI_ATOMS.get(name, ()) if name != "MSE" else ()      # MSE: no side-chain dihedral is defined (all five undefined)
        for n in range(len(chain_atoms) - 3):
            quad = chain_atoms[n:n + 4]
            if all(k in atoms for k in quad):
                ang[2 + n] = dihedral(*(atoms[k] for k in quad))
        k = ROT_LEN[letter]
        deg = np.around(np.array(ang[:2 + k], dtype=np.float64), 2)
        deg[np.isnan(deg)] = NAN_DEGREES
        row = np.full(ROW_WIDTH, PAD_VALUE, dtype=np.float64)
        row[0] = bfac
        row[1:4] = atoms["CA"]
        row[4:6 + k] = np.deg2rad(deg)
        seq.append(letter)
        rows.append(row)
    return "".join(seq), np.array(rows, dtype=np.float64).reshape(-1, ROW_WIDTH)


def _load_npy(path: str) -> np.ndarray:
    with open(path, "rb") as f:
        head = f.read(2)
    if head == b"\x1f\x8b":
        with gzip.open(path, "rb") as f:
            return np.load(io.BytesIO(f.read()), allow_pickle=False)
    return np.load(path, allow_pickle=False)


def load_dataset_folder(path: str, use_foldseek: bool, split: str = "test") -> Optional[Dict[str, Tuple[str, np.ndarray]]]:
    """tokenizer.py:137-149 / dataset.py:56-60: name -> (sequence, rows [L][11]) of the reference's cached dataset folder, or None when
    the folder holds no <split>_names.json.  <split>_angles.npy.gz is a gzip stream of a .npy (a plain .npy is accepted) holding the
    rows of all proteins concatenated; with use_foldseek the sequences are the combined strings (amino-acid letter + 3Di letter per
    residue) of <split>_foldseek_masked_sequences.json."""
    names_file = os.path.join(path, f"{split}_names.json") if path else ""
    if not path or not os.path.exists(names_file):
        return None
    with open(names_file) as f:
        names = json.load(f)
    with open(os.path.join(path, f"{split}_foldseek_masked_sequences.json" if use_foldseek else f"{split}_sequences.json")) as f:
        seqs = json.load(f)
    rows = np.asarray(_load_npy(os.path.join(path, f"{split}_angles.npy.gz")), dtype=np.float64)
    lengths = [len(s) // 2 if use_foldseek else len(s) for s in seqs]
    if len(names) != len(seqs) or rows.ndim != 2 or rows.shape[1] != ROW_WIDTH or sum(lengths) != rows.shape[0]:
        raise ValueError(f"{path}: {len(names)} names, {len(seqs)} sequences of {sum(lengths)} residues, angle rows {rows.shape} "
                         f"(expected [{sum(lengths)}, {ROW_WIDTH}])")
    off = np.concatenate([[0], np.cumsum(lengths)])
    return {n: (s, rows[off[i]:off[i + 1]]) for i, (n, s) in enumerate(zip(names, seqs))}


def save_dataset_folder(path: str, entries: Sequence[Tuple[str, str, np.ndarray]], combined: Optional[Sequence[str]] = None,
                        split: str = "test"):
    """Writes (name, sequence, rows) entries in the layout load_dataset_folder reads (tests; the reference's own writer is `deli`)."""
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, f"{split}_names.json"), "w") as f:
        json.dump([e[0] for e in entries], f)
    with open(os.path.join(path, f"{split}_sequences.json"), "w") as f:
        json.dump([e[1] for e in entries], f)
    buf = io.BytesIO()
    np.save(buf, np.concatenate([np.asarray(e[2], dtype=np.float64).reshape(-1, ROW_WIDTH) for e in entries]))
    with gzip.GzipFile(os.path.join(path, f"{split}_angles.npy.gz"), "wb", mtime=0) as f:
        f.write(buf.getvalue())
    if combined is not None:
        with open(os.path.join(path, f"{split}_foldseek_masked_sequences.json"), "w") as f:
            json.dump(list(combined), f)


def chunk_features(rows: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """dataset.py:137-149: (angles f32 [L + 2][7], pLDDT f32 [L + 2]) of one protein's stored rows [L][11] -- the <cls> and <eos> rows
    are 4.0 throughout, their pLDDT included.  These are the RAW rows: the pLDDT <= 70 padding and the -4 of masked positions are
    applied per forward (collate_rows; on the device, mulan_rows_kernel)."""
    rows = np.asarray(rows)
    if rows.ndim != 2 or rows.shape[1] != ROW_WIDTH:
        raise ValueError(f"angle rows have shape {rows.shape}, expected [L, {ROW_WIDTH}]")
    full = np.full((rows.shape[0] + 2, ROW_WIDTH), PAD_VALUE, dtype=np.float32)
    full[1:-1] = rows
    return np.ascontiguousarray(full[:, 4:]), np.ascontiguousarray(full[:, 0])


def collate_rows(angles: np.ndarray, plddt: np.ndarray, masked: Sequence[int] = ()) -> np.ndarray:
    """The model's struct_inputs [T][7] of one forward (dataset.py:306-314, then compute_fitness.py:117-126): rows with pLDDT <= 70 --
    the two end rows among them -- are 4.0, then the masked positions are -4.0."""
    out = np.array(angles, dtype=np.float32, copy=True)
    out[np.asarray(plddt) <= PLDDT_THRESHOLD] = PAD_VALUE
    out[0] = out[-1] = PAD_VALUE
    out[list(masked)] = MASK_VALUE
    return out


def tokenize(sequence: str, use_foldseek: bool) -> np.ndarray:
    """<cls> + the dataset sequence + <eos>: ESM2's alphabet, or SaProt's over a combined string (amino-acid + 3Di letter pairs)."""
    if use_foldseek:
        if len(sequence) % 2:
            raise ValueError(f"combined Foldseek sequence has odd length {len(sequence)}")
        return saprot.tokenize(sequence[0::2], sequence[1::2])
    ids = np.empty(len(sequence) + 2, dtype=np.int32)
    ids[0], ids[-1] = pesm.VOCABULARY.index("<cls>"), pesm.VOCABULARY.index("<eos>")
    for i, a in enumerate(sequence):
        if a not in ROT_LEN:
            raise ValueError(f"residue {i + 1}: {a!r} is not a letter of the dataset sequence (the 20 amino acids and X)")
        ids[i + 1] = pesm.VOCABULARY.index(a)
    return ids


# -- checkpoint --------------------------------------------------------------------------------------------------------------
def _layer_pairs(e: str, h: str):
    pairs = [("self_attn_layer_norm", "attention.LayerNorm"), ("self_attn.q_proj", "attention.self.query"),
             ("self_attn.k_proj", "attention.self.key"), ("self_attn.v_proj", "attention.self.value"),
             ("self_attn.out_proj", "attention.output.dense"), ("final_layer_norm", "LayerNorm"),
             ("fc1", "intermediate.dense"), ("fc2", "output.dense")]
    return [(e + a + "." + x, h + b + "." + x) for a, b in pairs for x in ("weight", "bias")]


def hf_keys(cfg: dict) -> List[Tuple[str, str]]:
    """(blob key, checkpoint key) in blob order: SaProt's list (ESM2's blob), then the adapter."""
    out = saprot.hf_keys(cfg)
    out += [(f"struct.MLP.{x}", ADAPTER + f"MLP.{x}") for x in ("weight", "bias")]
    out += _layer_pairs("struct.layers.0.", ADAPTER + "encoder.layer.0.")
    return out + [(f"struct.emb_layer_norm_after.{x}", ADAPTER + f"encoder.emb_layer_norm_after.{x}") for x in ("weight", "bias")]


def _ignored(key: str) -> bool:
    return (key.startswith(("esm.contact_head.", "contact_head.", "angle_regression_head.")) or key.endswith("rotary_embeddings.inv_freq")
            or key.endswith("position_ids") or key.endswith("position_embeddings.weight") or key == "lm_head.decoder.weight")


def base_vocabulary(layers: int, use_foldseek: bool) -> List[str]:
    """model_utils.py:492-504 (auto_detect_base_tokenizer): ESM2's alphabet, or SaProt's with --use_foldseek.  The reference knows two
    depths (6: ESM2 8M; 12: ESM2 35M or SaProt 35M) and asserts on any other; this path takes any depth, by the same flag.  Six layers
    with --use_foldseek is refused: the reference would read the combined strings with ESM2's tokenizer."""
    if use_foldseek and layers == 6:
        raise ValueError("a 6-layer MULAN with --use_foldseek: the reference pairs it with ESM2's tokenizer (no Foldseek tokens)")
    return saprot.vocabulary() if use_foldseek else list(pesm.VOCABULARY)


def config_from_hf(c: dict, use_foldseek: bool, sd=None) -> dict:
    """The model dimensions from config.json; refuses what the kernels do not compute."""
    if c.get("position_embedding_type", "absolute") != "rotary":
        raise ValueError(f"position_embedding_type {c.get('position_embedding_type')!r}: this path runs rotary positions only "
                         "(the reference would add a learned position table to the embedding)")
    if float(c.get("layer_norm_eps", 1e-12)) != LN_EPS:
        raise ValueError(f"layer_norm_eps {c.get('layer_norm_eps')}: the kernels' LayerNorm epsilon is {LN_EPS}")
    vocab = base_vocabulary(int(c["num_hidden_layers"]), use_foldseek)
    mask, pad = vocab.index("<mask>"), vocab.index("<pad>")
    if int(c["vocab_size"]) != len(vocab):
        raise ValueError(f"vocab_size {c['vocab_size']}: the base vocabulary {'with' if use_foldseek else 'without'} --use_foldseek has "
                         f"{len(vocab)} tokens")
    if int(c.get("pad_token_id", pad)) != pad or int(c.get("mask_token_id", mask)) != mask:
        raise ValueError(f"pad_token_id {c.get('pad_token_id')} / mask_token_id {c.get('mask_token_id')}: expected {pad} / {mask}")
    if c.get("hidden_act", "gelu") != "gelu":
        raise ValueError(f"hidden_act {c.get('hidden_act')!r}: this path runs erf-GELU only")
    if c.get("tie_word_embeddings", True) is False:
        raise ValueError("tie_word_embeddings false: the LM head of this path is the embedding table")
    lnb = bool(c.get("emb_layer_norm_before", False))
    if sd is not None:
        if lnb and "esm.embeddings.layer_norm.weight" not in sd:
            raise ValueError("emb_layer_norm_before is true but the checkpoint has no esm.embeddings.layer_norm weights")
        extra = sorted(k for k in sd if k.startswith(ADAPTER + "encoder.layer.") and not k.startswith(ADAPTER + "encoder.layer.0."))
        width = sd[ADAPTER + "MLP.weight"].shape[1] if ADAPTER + "MLP.weight" in sd else N_ANGLES
        if extra or width != N_ANGLES:
            raise ValueError(f"the checkpoint's structure adapter has {'more than one layer' if extra else f'{width} inputs'}: the "
                             "reference's from_pretrained passes no arguments and would build one layer of seven inputs")
    return dict(arch=_lib.ARCH_MULAN, layers=int(c["num_hidden_layers"]), embed_dim=int(c["hidden_size"]),
                heads=int(c["num_attention_heads"]), ffn_dim=int(c["intermediate_size"]), vocab=len(vocab), max_positions=0,
                token_dropout=int(bool(c.get("token_dropout", False))), emb_layer_norm_before=int(lnb), mask_token_id=mask,
                groups=saprot.GROUPS if use_foldseek else 0)


def weight_count(cfg: dict) -> int:
    D = cfg["embed_dim"]
    layer = 2 * D + 4 * (D * D + D) + 2 * D + 4 * D * D + 4 * D + 4 * D * D + D
    return saprot.weight_count(cfg) + D * N_ANGLES + D + layer + 2 * D


def pack(cfg: dict, sd) -> np.ndarray:
    """The checkpoint's state dict in blob order.  lm_head.bias may be stored as lm_head.decoder.bias; the tied decoder weight, the
    contact and angle heads, the rotary inv_freq buffers, position_ids and unused position tables are ignored; anything else missing
    or unexpected is an error."""
    sd = dict(sd)
    if "lm_head.bias" not in sd and "lm_head.decoder.bias" in sd:
        sd["lm_head.bias"] = sd.pop("lm_head.decoder.bias")
    sd.pop("lm_head.decoder.bias", None)
    keys = hf_keys(cfg)
    want = {h for _, h in keys}
    missing = sorted(h for h in want if h not in sd)
    unexpected = sorted(k for k in sd if k not in want and not _ignored(k))
    if missing or unexpected:
        raise ValueError(f"not a MULAN (StructEsmForMaskedLM) state dict: missing {missing[:5]}, unexpected {unexpected[:5]}")
    blob = np.empty(weight_count(cfg), dtype=np.float32)
    o = 0
    for _, h in keys:
        t = sd[h]
        a = t.detach().to("cpu").float().numpy() if hasattr(t, "detach") else np.asarray(t, dtype=np.float32)
        if o + a.size > blob.size:
            raise ValueError(f"state dict holds more weights than the configuration's {blob.size} (at {h}, shape {a.shape})")
        blob[o:o + a.size] = a.ravel()
        o += a.size
    if o != blob.size:
        raise ValueError(f"state dict holds {o} weights, the configuration needs {blob.size}")
    return blob


def load_checkpoint(path: str, use_foldseek: bool = False):
    """(cfg, state dict) of a local checkpoint directory; a vocab.txt beside it is checked against the base vocabulary."""
    if not os.path.isdir(path):
        raise ValueError(f"{path!r} is not a local directory (config.json, model.safetensors or pytorch_model.bin): this path never downloads")
    if not os.path.isfile(os.path.join(path, "config.json")):
        raise FileNotFoundError(f"{path}: no config.json")
    with open(os.path.join(path, "config.json")) as f:
        c = json.load(f)
    vocab_file = os.path.join(path, "vocab.txt")
    if os.path.isfile(vocab_file):
        want = base_vocabulary(int(c["num_hidden_layers"]), use_foldseek)
        if saprot.read_vocab(vocab_file) != want:
            raise ValueError(f"{vocab_file} is not the base vocabulary ({len(want)} tokens) this model is read with")
    st, pt = os.path.join(path, "model.safetensors"), os.path.join(path, "pytorch_model.bin")
    if os.path.isfile(st):
        from safetensors.numpy import load_file
        sd = {k: np.asarray(v, dtype=np.float32) for k, v in load_file(st).items() if np.issubdtype(v.dtype, np.floating)}
    elif os.path.isfile(pt):
        import torch
        sd = {k: v.float().numpy() for k, v in torch.load(pt, map_location="cpu", weights_only=True).items() if v.is_floating_point()}
    else:
        raise FileNotFoundError(f"{path}: no model.safetensors or pytorch_model.bin")
    return config_from_hf(c, use_foldseek, sd), sd


# -- an assay chunk ------------------------------------------------------------------------------------------------------------
def parse_chunk(mutants: Sequence[str], target_seq: str, range_start: int, chunk_len: int, use_foldseek: bool):
    """The mutants of one structure chunk: parsed against the whole target sequence (get_mutated_sequence's assertions), positions
    rebased to the chunk's tokens (pos - range_start + 1, compute_fitness.py:87; <cls> is token 0).  The letters pick columns only
    (:61-75): token ids of ESM2's alphabet, or SaProt's amino-acid groups with use_foldseek.  A sub-mutation outside the chunk is a
    ValueError naming the mutant: the reference's negative or overlong index would read another token."""
    sub_pos, sub_wt, sub_mt, mut_off = pesm.parse_mutants(mutants, target_seq, 1)
    wt_g, mt_g = saprot._ESM_TO_GROUP[sub_wt], saprot._ESM_TO_GROUP[sub_mt]
    if (mt_g < 0).any() or (wt_g < 0).any():
        k = int(np.flatnonzero((mt_g < 0) | (wt_g < 0))[0])
        raise AssertionError("Mutant to_AA is invalid: " + str(mutants[int(np.searchsorted(mut_off, k, side="right")) - 1]))
    pos = sub_pos.astype(np.int64) - range_start + 1
    bad = np.flatnonzero((pos < 1) | (pos > chunk_len))
    if bad.size:
        i = int(np.searchsorted(mut_off, bad[0], side="right")) - 1
        raise ValueError(f"mutant {mutants[i]}: position {int(sub_pos[bad[0]])} lies outside its structure chunk "
                         f"{range_start}-{range_start + chunk_len - 1}")
    if use_foldseek:
        return pos.astype(np.int32), wt_g.astype(np.int32), mt_g.astype(np.int32), mut_off
    return pos.astype(np.int32), sub_wt.astype(np.int32), sub_mt.astype(np.int32), mut_off


# -- model -------------------------------------------------------------------------------------------------------------------
class Mulan(_lib.ModelHandle):
    """Device-resident MULAN (ESM2's or SaProt's encoder behind the structure adapter)."""
    CREATE = "pgmi_mulan_model_create"

    def __init__(self, cfg: dict, weights: np.ndarray, device: int = 0, precision: str = "f16x3", max_rows: int = 0):
        self.precision = precision
        self.groups = int(cfg.get("groups", 0))
        self.width = self.groups or int(cfg["vocab"])
        self.T = 0
        super().__init__(cfg, weights, device, max_rows, arch_arg=(int(cfg["mask_token_id"]), self.groups),
                         precision=_lib.PRECISIONS[precision], arch=_lib.ARCH_MULAN, vocab=cfg["vocab"], max_positions=0,
                         token_dropout=cfg["token_dropout"], emb_layer_norm_before=cfg["emb_layer_norm_before"])

    @staticmethod
    def _weight_count(lib, c, arch_arg):
        import ctypes as C
        return lib.pgmi_mulan_weight_count(C.byref(c))

    def set_structure(self, angles, plddt):
        """Binds one chunk: raw angle rows [T][7] and pLDDT [T] (chunk_features) of <cls> + residues + <eos>."""
        a, p = _lib.as_f32(angles), _lib.as_f32(plddt)
        if a.ndim != 2 or a.shape[1] != N_ANGLES or p.shape != (a.shape[0],):
            raise ValueError(f"angles {a.shape} / pLDDT {p.shape}: expected [T, {N_ANGLES}] and [T]")
        _lib.check(_lib.load().pgmi_mulan_set_structure(self._h, _lib.ptr(a, _lib._f32p), _lib.ptr(p, _lib._f32p), a.shape[0]))
        self.T = a.shape[0]

    def token_logprobs(self, tokens, row_off=None, row_pos=None) -> np.ndarray:
        """log_softmax(logits) over all V columns for explicit rows [B,T]; row b's masked positions row_pos[row_off[b]:row_off[b+1]]
        choose its -4 angle rows (none by default): [B,T,V]."""
        t = _lib.as_i32(np.atleast_2d(np.asarray(tokens)))
        B, T = t.shape
        ro = _lib.as_i32(np.zeros(B + 1) if row_off is None else row_off)
        rp = _lib.as_i32(np.zeros(1) if row_pos is None or len(row_pos) == 0 else row_pos)
        if ro.size != B + 1:
            raise ValueError(f"row_off has {ro.size} entries for {B} rows")
        out = np.empty((B, T, int(self.cfg["vocab"])), dtype=np.float32)
        _lib.check(_lib.load().pgmi_mulan_token_logprobs(self._h, _lib.ptr(t, _lib._i32p), B, T, _lib.ptr(ro, _lib._i32p),
                                                         _lib.ptr(rp, _lib._i32p), _lib.ptr(out, _lib._f32p)))
        return out

    def set_logprobs(self, wt_tokens, set_off, set_pos) -> np.ndarray:
        """One forward per position set (CSR), the set's tokens <mask> and its angle rows -4; [n_entries, V] log-probabilities at every
        (set, position), or [n_entries, 21] amino-acid group log-probabilities for a Foldseek model."""
        wt, so, sp = _lib.as_i32(wt_tokens), _lib.as_i32(set_off), _lib.as_i32(set_pos)
        out = np.empty((int(so[-1]), self.width), dtype=np.float32)
        _lib.check(_lib.load().pgmi_mulan_set_logprobs(self._h, _lib.ptr(wt, _lib._i32p), wt.size, _lib.ptr(so, _lib._i32p),
                                                       _lib.ptr(sp, _lib._i32p), so.size - 1, _lib.ptr(out, _lib._f32p)))
        return out

    def score_chunk(self, wt_tokens, angles, plddt, pos, wt_col, mt_col, mut_off) -> np.ndarray:
        """calc_fitness for the parsed mutants of one chunk (parse_chunk) on its structure (chunk_features): float64 [n_mut]."""
        if len(mut_off) <= 1:
            return np.zeros(0, dtype=np.float64)
        if len(wt_tokens) != len(plddt):
            raise ValueError(f"the chunk has {len(wt_tokens)} tokens but {len(plddt)} angle rows")
        self.set_structure(angles, plddt)
        set_off, set_pos, entry = saprot.position_sets(pos, mut_off)
        table = self.set_logprobs(wt_tokens, set_off, set_pos)
        return pesm.score_parsed(table, entry, wt_col, mt_col, mut_off)

    profile_enable = pesm.EsmModel.profile_enable
    profile_reset = pesm.EsmModel.profile_reset
    profile = pesm.EsmModel.profile


def from_state_dict(cfg: dict, sd, device: int = 0, precision: str = "f16x3", max_rows: int = 0) -> Mulan:
    return Mulan(cfg, pack(cfg, sd), device=device, precision=precision, max_rows=max_rows)


def from_pretrained(path: str, use_foldseek: bool = False, device: int = 0, precision: str = "f16x3", max_rows: int = 0) -> Mulan:
    cfg, sd = load_checkpoint(path, use_foldseek)
    return from_state_dict(cfg, sd, device=device, precision=precision, max_rows=max_rows)
