"""ProteinMPNN on libpgmi (include/pgmi.h, ProteinMPNN section): the PDB parser and featurise inputs with the reference's semantics
(proteingym/baselines/protein_mpnn/protein_mpnn_utils.py parse_PDB / tied_featurize), checkpoint -> blob, the decoding-order rank and
the device-resident model.  Host code here is numpy only; torch is imported where a checkpoint is read.

The structure is encoded once (``MpnnModel.set_structure``); every mutant then costs the three decoder layers only."""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib

ALPHABET = "ACDEFGHIKLMNPQRSTVWYX"
LETTER = {a: i for i, a in enumerate(ALPHABET)}
HIDDEN, FFN, VOCAB = 128, 512, 21
_AA3 = ["ALA", "ARG", "ASN", "ASP", "CYS", "GLN", "GLU", "GLY", "HIS", "ILE", "LEU", "LYS", "MET", "PHE", "PRO", "SER", "THR", "TRP",
        "TYR", "VAL"]
_AA1 = "ARNDCQEGHILKMFPSTWYV"
_3TO1 = dict(zip(_AA3, _AA1))
# the chain names the reference looks for, in the order it concatenates them
CHAIN_ALPHABET = [chr(c) for c in range(ord("A"), ord("Z") + 1)] + [chr(c) for c in range(ord("a"), ord("z") + 1)] + \
    [str(i) for i in range(300)]
BACKBONE = ("N", "CA", "C", "O")


class MpnnConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("abi_version", "hidden", "num_edges", "enc_layers", "dec_layers", "precision")]


# ---- PDB -------------------------------------------------------------------------------------------------------------------------
def parse_pdb(path: str) -> List[Tuple[str, str, np.ndarray]]:
    """[(chain, sequence, xyz float64 [n, 4, 3])] in CHAIN_ALPHABET order.  Per chain the residue numbers from the smallest to the
    largest one seen: a number without ATOM records is one masked 'X' (NaN coordinates); insertion codes are residues of their own,
    sorted by code; HETATM MSE counts as MET; the first record of an atom wins; a residue name outside the 20 is 'X'."""
    chains: Dict[str, Dict[int, Dict[str, Tuple[str, Dict[str, np.ndarray]]]]] = {}
    with open(path, "rb") as f:
        for raw in f:
            line = raw.decode("utf-8", "ignore").rstrip()
            if line[:6] == "HETATM" and line[17:20] == "MSE":
                line = line.replace("HETATM", "ATOM  ").replace("MSE", "MET")
            if line[:4] != "ATOM":
                continue
            ch, atom, resi, resn = line[21:22], line[12:16].strip(), line[17:20], line[22:27].strip()
            xyz = np.array([float(line[i:i + 8]) for i in (30, 38, 46)])
            if resn[-1].isalpha():
                resa, num = resn[-1], int(resn[:-1]) - 1
            else:
                resa, num = "", int(resn) - 1
            name_atoms = chains.setdefault(ch, {}).setdefault(num, {}).setdefault(resa, (resi, {}))
            name_atoms[1].setdefault(atom, xyz)
    out = []
    for ch in CHAIN_ALPHABET:
        if ch not in chains:
            continue
        res = chains[ch]
        seq, xyz = [], []
        for num in range(min(res), max(res) + 1):
            if num not in res:
                seq.append("X")
                xyz.append(np.full((4, 3), np.nan))
                continue
            for code in sorted(res[num]):
                name, atoms = res[num][code]
                seq.append(_3TO1.get(name, "X"))
                xyz.append(np.stack([atoms.get(a, np.full(3, np.nan)) for a in BACKBONE]))
        out.append((ch, "".join(seq), np.array(xyz).reshape(-1, 4, 3)))
    return out


def featurize(chains, designed_chains: Optional[Sequence[str]] = None, fixed_positions: Optional[Dict[str, Sequence[int]]] = None):
    """The model's inputs for one structure, as tied_featurize packs them: designed chains (sorted) first, then the other chains
    (sorted).  Returns a dict: X float32 [L, 4, 3] (NaN -> 0), mask float32 [L] (0 where any backbone atom is missing), residue_idx
    int32 [L] (+100 per chain), chain_encoding int32 [L] (1, 2, ..), S int32 [L], chain_M / chain_M_pos float32 [L] (designed chain;
    position not fixed -- they act on the decoding order only), seq str."""
    by = {c: (s, x) for c, s, x in chains}
    names = [c for c, _, _ in chains]
    designed = sorted(names if designed_chains is None else [c for c in designed_chains])
    for c in designed:
        if c not in by:
            raise ValueError(f"chain {c!r} is not in the structure (chains: {names})")
    fixed = sorted(c for c in names if c not in designed)
    X, S, ridx, enc, cm, cmp_ = [], [], [], [], [], []
    l0 = 0
    for n, c in enumerate(designed + fixed, start=1):
        s, x = by[c]
        X.append(x)
        S.extend(LETTER[a] for a in s)
        ridx.append(100 * (n - 1) + np.arange(l0, l0 + len(s)))
        l0 += len(s)
        enc.append(np.full(len(s), n))
        is_designed = c in designed
        cm.append(np.full(len(s), 1.0 if is_designed else 0.0))
        pos = np.ones(len(s))
        if is_designed and fixed_positions and fixed_positions.get(c):
            pos[np.array(fixed_positions[c]) - 1] = 0.0
        cmp_.append(pos)
    X = np.concatenate(X, 0)
    mask = np.isfinite(X.sum((1, 2))).astype(np.float32)
    X = np.where(np.isnan(X), 0.0, X).astype(np.float32)
    S = np.asarray(S, dtype=np.int32)
    return dict(X=X, mask=mask, residue_idx=np.concatenate(ridx).astype(np.int32), chain_encoding=np.concatenate(enc).astype(np.int32),
                S=S, chain_M=np.concatenate(cm).astype(np.float32), chain_M_pos=np.concatenate(cmp_).astype(np.float32),
                seq="".join(ALPHABET[i] for i in S))


# ---- weights ---------------------------------------------------------------------------------------------------------------------
def key_shapes(enc_layers: int = 3, dec_layers: int = 3) -> List[Tuple[str, Tuple[int, ...]]]:
    """(name, shape) of ProteinMPNN(ca_only=False).state_dict(), in its order: the blob's order."""
    H = HIDDEN

    def lin(name, n, k):
        return [(f"{name}.weight", (n, k)), (f"{name}.bias", (n,))]

    def norm(name):
        return [(f"{name}.weight", (H,)), (f"{name}.bias", (H,))]

    out = lin("features.embeddings.linear", 16, 66) + [("features.edge_embedding.weight", (H, 416))] + norm("features.norm_edges")
    out += lin("W_e", H, H) + [("W_s.weight", (VOCAB, H))]
    for i in range(enc_layers):
        p = f"encoder_layers.{i}"
        out += norm(f"{p}.norm1") + norm(f"{p}.norm2") + norm(f"{p}.norm3")
        out += lin(f"{p}.W1", H, 3 * H) + lin(f"{p}.W2", H, H) + lin(f"{p}.W3", H, H)
        out += lin(f"{p}.W11", H, 3 * H) + lin(f"{p}.W12", H, H) + lin(f"{p}.W13", H, H)
        out += lin(f"{p}.dense.W_in", FFN, H) + lin(f"{p}.dense.W_out", H, FFN)
    for i in range(dec_layers):
        p = f"decoder_layers.{i}"
        out += norm(f"{p}.norm1") + norm(f"{p}.norm2")
        out += lin(f"{p}.W1", H, 4 * H) + lin(f"{p}.W2", H, H) + lin(f"{p}.W3", H, H)
        out += lin(f"{p}.dense.W_in", FFN, H) + lin(f"{p}.dense.W_out", H, FFN)
    return out + lin("W_out", VOCAB, H)


def random_state_dict(seed: int, enc_layers: int = 3, dec_layers: int = 3) -> Dict[str, np.ndarray]:
    """Random weights for tests and benches (numpy default_rng): matrices N(0, 1 / fan_in) scaled so activations stay O(1), biases
    N(0, 0.1^2), LayerNorm gains 1 + N(0, 0.1^2) and biases N(0, 0.1^2) so that neither is invisible."""
    rng = np.random.default_rng(seed)
    sd = {}
    for name, shape in key_shapes(enc_layers, dec_layers):
        if ".norm" in name:
            v = rng.normal(0.0, 0.1, size=shape) + (1.0 if name.endswith("weight") else 0.0)
        elif name == "W_s.weight":
            v = rng.normal(0.0, 1.0, size=shape)
        elif len(shape) == 2:
            v = rng.normal(0.0, 1.0 / np.sqrt(shape[1]), size=shape)
        else:
            v = rng.normal(0.0, 0.1, size=shape)
        sd[name] = v.astype(np.float32)
    return sd


def blob_from_state_dict(sd, enc_layers: int = 3, dec_layers: int = 3) -> np.ndarray:
    parts = []
    for name, shape in key_shapes(enc_layers, dec_layers):
        if name not in sd:
            raise _lib.PgmiError(f"checkpoint has no tensor {name!r}")
        v = np.asarray(sd[name].detach().cpu().numpy() if hasattr(sd[name], "detach") else sd[name], dtype=np.float32)
        if tuple(v.shape) != tuple(shape):
            raise _lib.PgmiError(f"{name}: shape {tuple(v.shape)}, expected {tuple(shape)} (CA-only checkpoints are not supported)")
        parts.append(v.ravel())
    extra = set(sd) - {n for n, _ in key_shapes(enc_layers, dec_layers)}
    if extra:
        raise _lib.PgmiError(f"checkpoint has tensors this model does not know: {sorted(extra)[:4]}")
    return np.concatenate(parts)


def load_checkpoint(path: str) -> Tuple[np.ndarray, int]:
    """(blob, num_edges) of a ProteinMPNN checkpoint file ({'model_state_dict', 'num_edges', 'noise_level'})."""
    import torch
    ck = torch.load(path, map_location="cpu")
    sd = ck["model_state_dict"]
    n_enc = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("encoder_layers."))
    n_dec = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("decoder_layers."))
    return blob_from_state_dict(sd, n_enc, n_dec), int(ck["num_edges"])


def save_checkpoint(path: str, sd: Dict[str, np.ndarray], num_edges: int, noise_level: float = 0.0) -> None:
    import torch
    torch.save({"model_state_dict": {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, "num_edges": int(num_edges),
                "noise_level": noise_level}, path)


# ---- decoding order ----------------------------------------------------------------------------------------------------------------
def rank_from_randn(randn: np.ndarray, mask: np.ndarray, chain_M: Optional[np.ndarray] = None, chain_M_pos: Optional[np.ndarray] = None):
    """rank[b, i] = position of residue i in argsort((chain_M chain_M_pos mask + 1e-4) |randn[b]|), in fp32 as the reference
    multiplies it; int32 [B, L]."""
    randn = np.atleast_2d(np.asarray(randn, dtype=np.float32))
    cm = np.asarray(mask, dtype=np.float32)
    if chain_M is not None:
        cm = np.asarray(chain_M, dtype=np.float32) * cm
    if chain_M_pos is not None:
        cm = np.asarray(chain_M_pos, dtype=np.float32) * cm
    key = (cm + np.float32(0.0001))[None, :] * np.abs(randn)
    order = np.argsort(key, axis=-1, kind="stable")
    rank = np.empty_like(order)
    np.put_along_axis(rank, order, np.broadcast_to(np.arange(order.shape[1]), order.shape), axis=-1)
    return rank.astype(np.int32)


def encode_sequences(seqs: Sequence[str], L: int) -> np.ndarray:
    S = np.empty((len(seqs), L), dtype=np.uint8)
    for b, s in enumerate(seqs):
        if len(s) != L:
            raise ValueError(f"sequence {b} has {len(s)} letters, the structure has {L}")
        try:
            S[b] = [LETTER[a] for a in s]
        except KeyError as e:
            raise ValueError(f"sequence {b}: letter {e.args[0]!r} is not in {ALPHABET}") from None
    return S


# ---- the model -------------------------------------------------------------------------------------------------------------------
class MpnnModel(_lib.SideHandle):
    """A device-resident ProteinMPNN."""

    PREFIX = "mpnn"

    def __init__(self, blob: np.ndarray, num_edges: int = 48, device: int = 0, enc_layers: int = 3, dec_layers: int = 3):
        c = MpnnConfig(abi_version=_lib.ABI_VERSION, hidden=HIDDEN, num_edges=num_edges, enc_layers=enc_layers, dec_layers=dec_layers,
                       precision=_lib.PREC_FP32)
        self._create(c, blob, device)
        self.num_edges = num_edges
        self.L = self.K = 0
        self.mask = self.chain_M = self.chain_M_pos = None

    def set_structure(self, X, mask, residue_idx, chain_encoding, chain_M=None, chain_M_pos=None):
        """Graph, edge features, encoder and the mutant-independent decoder tables of one backbone; chain_M / chain_M_pos are kept
        for the decoding order of ``scores``."""
        X = _lib.as_f32(X)
        L = X.shape[0]
        if X.shape != (L, 4, 3):
            raise _lib.PgmiError("X must be [L, 4, 3]")
        mask, ridx, ch = _lib.as_f32(mask), _lib.as_i32(residue_idx), _lib.as_i32(chain_encoding)
        if not (mask.shape == ridx.shape == ch.shape == (L,)):
            raise _lib.PgmiError("mask, residue_idx and chain_encoding must be [L]")
        _lib.check(_lib.load().pgmi_mpnn_set_structure(self._h, _lib.ptr(X, _lib._f32p), _lib.ptr(mask, _lib._f32p),
                                                       _lib.ptr(ridx, _lib._i32p), _lib.ptr(ch, _lib._i32p), L))
        self.L, self.K = L, min(self.num_edges, L)
        self.mask, self.chain_M, self.chain_M_pos = mask, chain_M, chain_M_pos

    def graph(self):
        E_idx = np.empty((self.L, self.K), dtype=np.int32)
        E = np.empty((self.L, self.K, HIDDEN), dtype=np.float32)
        _lib.check(_lib.load().pgmi_mpnn_graph(self._h, _lib.ptr(E_idx, _lib._i32p), _lib.ptr(E, _lib._f32p)))
        return E_idx, E

    def encoder(self):
        h_V = np.empty((self.L, HIDDEN), dtype=np.float32)
        h_E = np.empty((self.L, self.K, HIDDEN), dtype=np.float32)
        _lib.check(_lib.load().pgmi_mpnn_encoder(self._h, _lib.ptr(h_V, _lib._f32p), _lib.ptr(h_E, _lib._f32p)))
        return h_V, h_E

    def _inputs(self, S, rank):
        S = np.ascontiguousarray(S, dtype=np.uint8)
        rank = _lib.as_i32(rank)
        if S.ndim != 2 or S.shape[1] != self.L or rank.shape != S.shape:
            raise _lib.PgmiError(f"S and rank must be [B, {self.L}]")
        return S, rank

    def log_probs(self, S, rank) -> np.ndarray:
        S, rank = self._inputs(S, rank)
        out = np.empty(S.shape + (VOCAB,), dtype=np.float32)
        _lib.check(_lib.load().pgmi_mpnn_log_probs(self._h, _lib.ptr(S, _lib._u8p), _lib.ptr(rank, _lib._i32p), S.shape[0],
                                                   _lib.ptr(out, _lib._f32p)))
        return out

    def scores_from_rank(self, S, rank) -> np.ndarray:
        S, rank = self._inputs(S, rank)
        out = np.empty(S.shape[0], dtype=np.float64)
        _lib.check(_lib.load().pgmi_mpnn_scores(self._h, _lib.ptr(S, _lib._u8p), _lib.ptr(rank, _lib._i32p), S.shape[0],
                                                _lib.ptr(out, _lib._f64p)))
        return out

    def scores(self, seqs, randn=None, seed: int = 0) -> np.ndarray:
        """pmpnn_ll of every sequence (str, or rows of letter indices): one forward each under the order drawn from randn [B, L]
        (None: standard normals of numpy's default_rng(seed))."""
        S = encode_sequences(seqs, self.L) if len(seqs) and isinstance(seqs[0], str) else np.asarray(seqs, dtype=np.uint8)
        if randn is None:
            randn = np.random.default_rng(seed).standard_normal((S.shape[0], self.L)).astype(np.float32)
        return self.scores_from_rank(S, rank_from_randn(randn, self.mask, self.chain_M, self.chain_M_pos))
