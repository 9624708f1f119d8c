"""VespaG scoring on libpgmi (include/pgmi.h, VespaG section).

Replaces proteingym/baselines/vespag/vespag: one unmasked ESM2-3B forward per protein of a FASTA (data/embeddings.py), the residue rows
through FNN([256], 2560, 20) (models/fnn.py, models/utils.py construct_fnn), mask_non_mutations and compute_mutation_score
(utils/mutations.py).  The encoder and the head run in HIP (csrc/api_vespag.hip, vespag.hip on the ESM2 encoder): a library of sequences
goes to the device in one call, sorted by length and chunked there, and its residue rows never leave the device on their way into the
head.  Tokenisation, the mutation parser, the landscape's order and the score are host work, here.  Nothing is downloaded.

Each reading of the reference is one named function: ``clean_sequence`` (data/embeddings.py:83-86), ``SAV`` / ``Mutation``
(utils/mutations.py:17-66), ``landscape`` (runner/predict.py:155-163), ``wt_columns`` (mask_non_mutations),
``mutation_score`` (compute_mutation_score), ``read_mutation_file``, ``read_fasta`` (SeqIO's record ids), ``apply_id_map``
(runner/predict.py:126-130).

One deviation: a wild-type residue outside the 20 letters makes the reference's mask_non_mutations raise (str.index); here that row is
left unmasked (wt column -1) and a full landscape lists all 20 targets for it.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import re
from dataclasses import dataclass
from typing import Dict, Iterable, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import _lib
from . import esm as pesm

AMINO_ACIDS = "ACDEFGHIKLMNPQRSTVWY"          # utils/utils.py:15: the head's 20 columns
INPUT_DIM, HIDDEN, OUT, NEGATIVE_SLOPE = 2560, 256, 20, 0.01      # DEFAULT_MODEL_PARAMETERS, get_embedding_dim("esm2"), nn.LeakyReLU()
KEYS = ("net.0.weight", "net.0.bias", "net.3.weight", "net.3.bias")   # Linear, Dropout, LeakyReLU, Linear: indices 0 and 3
MAX_RESIDUES_PER_CALL = 65536                 # packed rows of one device call: 640 MiB at D = 2560


class VespagConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("abi_version", "input_dim", "hidden", "out", "precision")] + [("negative_slope", C.c_float)]


# -- checkpoint --------------------------------------------------------------------------------------------------------------
def _to_np(t) -> np.ndarray:
    return t.detach().to("cpu").float().numpy() if hasattr(t, "detach") else np.asarray(t, dtype=np.float32)


def check_state_dict(sd) -> Tuple[int, int]:
    """(input_dim, hidden) of an FNN([hidden], input_dim, 20) state dict; anything else is refused with the cause named."""
    keys = list(sd)
    other = [k for k in keys if k.split(".")[0] in ("conv", "fnn", "combined")]
    if other:
        raise ValueError(f"a CNN or combined VespaG checkpoint (key {other[0]!r}): predict loads the FNN only, and so does this path")
    odd = [k for k in keys if not re.fullmatch(r"net\.\d+\.(weight|bias)", k)]
    if odd:
        raise ValueError(f"not a VespaG FNN state dict: unexpected key {odd[0]!r}")
    linears = sorted({int(k.split(".")[1]) for k in keys})
    if len(linears) != 2:
        raise ValueError(f"a VespaG FNN with {max(len(linears) - 1, 0)} hidden layers (Linear layers at net.{linears}): this path runs "
                         "hidden_dims = [256], one hidden layer")
    if linears != [0, 3]:
        raise ValueError(f"Linear layers at net.{linears}: FNN([256], dropout_rate=0.2) has them at net.0 and net.3")
    missing = [k for k in KEYS if k not in sd]
    if missing:
        raise ValueError(f"not a VespaG FNN state dict: {missing[0]} is missing")
    w1, b1, w2, b2 = (tuple(np.shape(sd[k])) for k in KEYS)
    if len(w1) != 2 or len(w2) != 2:
        raise ValueError(f"net.0.weight {w1}, net.3.weight {w2}: two matrices expected")
    hidden, input_dim = w1
    if input_dim == 1024:
        raise ValueError("input_dim 1024: a checkpoint for ProtT5 embeddings; this path has no T5 encoder and runs the ESM2 checkpoints")
    if b1 != (hidden,) or w2 != (OUT, hidden) or b2 != (OUT,):
        raise ValueError(f"net.0.bias {b1}, net.3.weight {w2}, net.3.bias {b2}: expected ({hidden},), ({OUT}, {hidden}), ({OUT},)")
    return int(input_dim), int(hidden)


def pack(sd) -> np.ndarray:
    """The blob of include/pgmi.h: net.0.weight, net.0.bias, net.3.weight, net.3.bias."""
    check_state_dict(sd)
    return np.concatenate([np.ascontiguousarray(_to_np(sd[k]), dtype=np.float32).ravel() for k in KEYS])


def load_checkpoint(path: str) -> Dict[str, np.ndarray]:
    """torch.load(state_dict_v2.pt) under esm.load_checkpoint_file's rule (weights_only), checked, as float32 arrays."""
    if not os.path.isfile(path):
        raise FileNotFoundError(f"{path}: no such checkpoint (this path never downloads)")
    sd = pesm.load_checkpoint_file(path)
    if not isinstance(sd, dict):
        raise ValueError(f"{path}: a {type(sd).__name__}, not a state dict")
    check_state_dict(sd)
    return {k: _to_np(sd[k]) for k in KEYS}


def random_state_dict(seed: int, input_dim: int = INPUT_DIM, hidden: int = HIDDEN, gain: float = 1.0, bias_std: float = 0.0) -> Dict[str, np.ndarray]:
    """A seeded checkpoint: kaiming_normal_(a = 0.01) weights (std = sqrt(2 / (1 + a^2) / fan_in), models/fnn.py:45) times `gain`; FNN
    zeroes the biases, bias_std > 0 draws them N(0, bias_std^2) instead so that a test reads every bias."""
    rng = np.random.default_rng(seed)
    sd = {}
    for name, shape in zip(KEYS, ((hidden, input_dim), (hidden,), (OUT, hidden), (OUT,))):
        if name.endswith("weight"):
            a = rng.standard_normal(shape) * (gain * math.sqrt(2.0 / (1.0 + NEGATIVE_SLOPE ** 2) / shape[1]))
        else:
            a = rng.standard_normal(shape) * bias_std
        sd[name] = a.astype(np.float32)
    return sd


# -- sequences ---------------------------------------------------------------------------------------------------------------
def clean_sequence(seq: str) -> str:
    """data/embeddings.py:84: re.sub(r"[UZOB]", "X", seq)."""
    return re.sub(r"[UZOB]", "X", seq)


def tokenize(seq: str) -> np.ndarray:
    """<cls> + the ESM alphabet's ids of clean_sequence(seq) + <eos>, uint8.  A letter outside the alphabet is refused by name (the HF
    tokenizer would map it to <unk>)."""
    s = clean_sequence(seq)
    if not s:
        raise ValueError("an empty sequence has no residue rows")
    ids = np.empty(len(s) + 2, dtype=np.uint8)
    ids[0], ids[-1] = pesm.VOCABULARY.index("<cls>"), pesm.VOCABULARY.index("<eos>")
    for i, a in enumerate(s):
        if len(a) != 1 or not a.isupper() or a not in pesm.VOCABULARY:
            raise ValueError(f"residue {a!r} at position {i + 1} is not a letter of the ESM alphabet")
        ids[i + 1] = pesm.VOCABULARY.index(a)
    return ids


def pack_library(seqs: Sequence[str]) -> Tuple[np.ndarray, np.ndarray]:
    """(tokens uint8, seq_off int64 [n + 1]) as pgmi_pppl_create takes a library."""
    toks = [tokenize(s) for s in seqs]
    off = np.zeros(len(toks) + 1, dtype=np.int64)
    np.cumsum([t.size for t in toks], out=off[1:])
    return np.concatenate(toks), off


def wt_columns(seq: str) -> np.ndarray:
    """mask_non_mutations' column per residue; -1 (the row stays unmasked) for a residue outside the 20 letters."""
    return np.array([AMINO_ACIDS.find(a) for a in seq], dtype=np.int32)


def read_fasta(path: str) -> Dict[str, str]:
    """{rec.id: str(rec.seq)} as SeqIO.parse(path, "fasta") gives them: the id is the header up to the first whitespace."""
    out, cur = {}, None
    with open(path) as f:
        for line in f:
            line = line.rstrip("\r\n")
            if line.startswith(">"):
                fields = line[1:].split(None, 1)
                cur = fields[0] if fields else ""
                out[cur] = []
            elif line.strip():
                if cur is None:
                    raise ValueError(f"{path}: sequence data before the first '>' header")
                out[cur].append(line.strip())
    return {k: "".join(v) for k, v in out.items()}


# -- mutations ---------------------------------------------------------------------------------------------------------------
@dataclass
class SAV:
    position: int                 # zero-indexed
    from_aa: str
    to_aa: str
    one_indexed: bool = False

    @classmethod
    def from_sav_string(cls, s: str, one_indexed: bool = False, offset: int = 0) -> "SAV":
        try:
            position = int(s[1:-1]) - offset
        except ValueError:
            raise ValueError(f"mutant {s!r}: expected <from><position><to>, e.g. A25G") from None
        return SAV(position - 1 if one_indexed else position, s[0], s[-1], one_indexed)

    def __str__(self) -> str:
        return f"{self.from_aa}{self.position + 1 if self.one_indexed else self.position}{self.to_aa}"

    def __hash__(self):
        return hash(str(self))

    def __iter__(self):
        yield self


@dataclass
class Mutation:
    savs: List[SAV]

    @classmethod
    def from_mutation_string(cls, s: str, one_indexed: bool = False, offset: int = 0) -> "Mutation":
        return Mutation([SAV.from_sav_string(x, one_indexed, offset) for x in s.split(":")])

    def __str__(self) -> str:
        return ":".join(str(s) for s in self.savs)

    def __hash__(self):
        return hash(str(self))

    def __iter__(self):
        yield from self.savs


def landscape(seq: str, one_indexed: bool = True) -> List[SAV]:
    """runner/predict.py:155-163: position-major, AMINO_ACIDS order, the wild type skipped."""
    return [SAV(i, wt, aa, one_indexed) for i, wt in enumerate(seq) for aa in AMINO_ACIDS if aa != wt]


def read_mutation_file(path: str, one_indexed: bool = True) -> Dict[str, List[Mutation]]:
    """utils/mutations.py read_mutation_file: a CSV with a header line; column 0 the protein id, column 1 the mutant."""
    import pandas as pd
    out: Dict[str, List[Mutation]] = {}
    for row in pd.read_csv(path, dtype=str, keep_default_na=False).itertuples(index=False):
        out.setdefault(row[0], []).append(Mutation.from_mutation_string(row[1], one_indexed))
    return out


def mutation_score(y: np.ndarray, mutation: Union[SAV, Mutation], normalize: bool = True) -> float:
    """compute_mutation_score: the float32 entries y[position][to_aa] summed as Python floats (float64), then 1 / (1 + exp(-s)).  A
    position outside the sequence or a target outside the 20 letters is refused with the mutant named; from_aa is never read."""
    score = 0
    for sav in mutation:
        col = AMINO_ACIDS.find(sav.to_aa) if len(sav.to_aa) == 1 else -1
        if col < 0:
            raise ValueError(f"mutant {mutation}: target {sav.to_aa!r} is not one of {AMINO_ACIDS}")
        if not 0 <= sav.position < len(y):
            raise ValueError(f"mutant {mutation}: position {sav} is outside the sequence of {len(y)} residues")
        score = score + float(y[sav.position][col])
    return 1 / (1 + math.exp(-score)) if normalize else float(score)


def score_mutations(y: np.ndarray, mutations: Iterable[Union[SAV, Mutation]], normalize: bool = True) -> Dict[str, float]:
    """{str(mutation): score} in first-seen order (the reference's dict keyed by the mutation's string)."""
    return {str(m): mutation_score(y, m, normalize) for m in mutations}


# -- embeddings --------------------------------------------------------------------------------------------------------------
def load_embeddings(path: str) -> Dict[str, np.ndarray]:
    """{id: float32 [L, D]} from an .npz, or from the reference's .h5 where h5py is installed."""
    if str(path).endswith(".npz"):
        with np.load(path) as z:
            return {k: np.asarray(z[k], dtype=np.float32) for k in z.files}
    if str(path).endswith((".h5", ".hdf5")):
        try:
            import h5py
        except ImportError:
            raise RuntimeError(f"{path}: reading HDF5 embeddings needs h5py, which is not installed; convert the file to .npz "
                               "(np.savez(out, **{id: rows})) or install h5py") from None
        with h5py.File(path, "r") as f:
            return {k: np.array(v[()], dtype=np.float32) for k, v in f.items()}
    raise ValueError(f"{path}: embeddings are read from .npz or .h5")


def apply_id_map(embeddings: Dict[str, np.ndarray], path: str) -> Dict[str, np.ndarray]:
    """runner/predict.py:126-130: a header-less CSV of (embedding id, FASTA id); each entry moves to its FASTA id."""
    import csv
    with open(path, newline="") as f:
        id_map = {row[0]: row[1] for row in csv.reader(f) if row}
    for from_id, to_id in id_map.items():
        if from_id not in embeddings:
            raise KeyError(f"--id-map: no embedding with id {from_id!r}")
        embeddings[to_id] = embeddings[from_id]
        del embeddings[from_id]
    return embeddings


def check_embedding(pid: str, seq: str, rows: np.ndarray, input_dim: int) -> np.ndarray:
    if rows.ndim != 2 or rows.shape != (len(seq), input_dim):
        raise ValueError(f"{pid}: embedding of shape {tuple(rows.shape)}, the sequence has {len(seq)} residues and the head reads {input_dim} columns")
    return rows


# -- model -------------------------------------------------------------------------------------------------------------------
def plan_chunks(lengths: Sequence[int], row_cap: int):
    """The device's plan for sequences of `lengths` residues (pgmi_op_packed_rows_plan; host only): (order, chunks, packed_off) --
    the sequences as they run, the chunks as lists of sequence indices, the packed row of every sequence's first residue."""
    lib = _lib.load()
    n = len(lengths)
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.asarray(lengths, dtype=np.int64) + 2, out=off[1:])
    order, ends, nch, packed = np.full(n, -1, np.int32), np.full(n, -1, np.int32), np.zeros(1, np.int32), np.zeros(n + 1, np.int64)
    _lib.check(lib.pgmi_op_packed_rows_plan(_lib.ptr(off, _lib._i64p), n, int(row_cap), _lib.ptr(order, _lib._i32p), _lib.ptr(ends, _lib._i32p),
                                            _lib.ptr(nch, _lib._i32p), _lib.ptr(packed, _lib._i64p)))
    bounds = [0] + ends[:nch[0]].tolist()
    return order.tolist(), [order[a:b].tolist() for a, b in zip(bounds, bounds[1:])], packed.tolist()


def packed_rows(esm: pesm.EsmModel, seqs: Sequence[str], row_cap: int = 0, want_stats: bool = False):
    """[float32 [L_i, D]] of every sequence through pgmi_esm_packed_rows (one call; the device sorts and chunks)."""
    tok, off = pack_library(seqs)
    D = esm.cfg["embed_dim"]
    rows = np.empty((int(off[-1]) - 2 * len(seqs), D), np.float32)
    stats = np.zeros(3, np.int64)
    _lib.check(_lib.load().pgmi_esm_packed_rows(esm._h, _lib.ptr(tok, _lib._u8p), _lib.ptr(off, _lib._i64p), len(seqs), int(row_cap),
                                                _lib.ptr(rows, _lib._f32p), _lib.ptr(stats, _lib._i64p)))
    starts = off[:-1] - 2 * np.arange(len(seqs))
    out = [rows[s:s + len(q)] for s, q in zip(starts, seqs)]
    return (out, dict(chunks=int(stats[0]), tokens=int(stats[1]), padded_tokens=int(stats[2]))) if want_stats else out


def call_groups(lengths: Sequence[int], max_residues: int = MAX_RESIDUES_PER_CALL) -> List[List[int]]:
    """The sequences of a FASTA as they go to the device: longest first, in calls of at most max_residues residues (one sequence at
    least), so a FASTA of any size runs in a bounded packed buffer.  Lists of indices into `lengths`."""
    groups, total = [[]], 0
    for i in sorted(range(len(lengths)), key=lambda i: -lengths[i]):
        if groups[-1] and total + lengths[i] > max_residues:
            groups.append([])
            total = 0
        groups[-1].append(i)
        total += lengths[i]
    return [g for g in groups if g]


class VespaG(_lib.SideHandle):
    """One device-resident head, with or without the ESM2 model it borrows (close the head first)."""

    PREFIX, NAME = "vespag", "VespaG "

    def __init__(self, blob: np.ndarray, input_dim: int = INPUT_DIM, hidden: int = HIDDEN, esm: Optional[pesm.EsmModel] = None,
                 device: int = 0, precision: str = "f16x3", negative_slope: float = NEGATIVE_SLOPE):
        if precision not in ("f16x3", "fp32"):
            raise ValueError(f"precision {precision!r}: VespaG runs in f16x3 or fp32")
        self.D, self.H, self.esm = input_dim, hidden, esm
        self.config = VespagConfig(abi_version=_lib.ABI_VERSION, input_dim=input_dim, hidden=hidden, out=OUT,
                                   precision=_lib.PRECISIONS[precision], negative_slope=negative_slope)
        self._create(self.config, blob, device, esm._h if esm is not None else None)

    def _call_landscapes(self, seqs: Sequence[str], want_rows: bool):
        tok, off = pack_library(seqs)
        R = int(off[-1]) - 2 * len(seqs)
        wt = np.concatenate([wt_columns(s) for s in seqs])
        y = np.empty((R, OUT), np.float32)
        rows = np.empty((R, self.D), np.float32) if want_rows else None
        _lib.check(_lib.load().pgmi_vespag_landscapes(self._h, _lib.ptr(tok, _lib._u8p), _lib.ptr(off, _lib._i64p), len(seqs),
                                                      _lib.ptr(wt, _lib._i32p), _lib.ptr(y, _lib._f32p), _lib.ptr(rows, _lib._f32p)))
        starts = off[:-1] - 2 * np.arange(len(seqs))
        cut = lambda a: [a[s:s + len(q)] for s, q in zip(starts, seqs)]
        return cut(y), (cut(rows) if want_rows else None)

    def landscapes(self, seqs: Sequence[str], want_rows: bool = False, max_residues: int = MAX_RESIDUES_PER_CALL):
        """[y float32 [L_i, 20]] of every sequence (and their residue rows), one device call per group of call_groups."""
        ys, rows = [None] * len(seqs), [None] * len(seqs)
        for group in call_groups([len(s) for s in seqs], max_residues):
            y, r = self._call_landscapes([seqs[j] for j in group], want_rows)
            for k, j in enumerate(group):
                ys[j] = y[k]
                if want_rows:
                    rows[j] = r[k]
        return (ys, rows) if want_rows else ys

    def head(self, rows: np.ndarray, wt_cols: np.ndarray) -> np.ndarray:
        """y float32 [R, 20] of pre-computed rows [R, input_dim]."""
        x, wt = _lib.as_f32(rows), _lib.as_i32(wt_cols)
        if x.ndim != 2 or x.shape[1] != self.D or wt.shape != (x.shape[0],):
            raise ValueError(f"rows {x.shape}, wt_cols {wt.shape}: expected [R, {self.D}] and [R]")
        y = np.empty((x.shape[0], OUT), np.float32)
        _lib.check(_lib.load().pgmi_vespag_head(self._h, _lib.ptr(x, _lib._f32p), _lib.ptr(wt, _lib._i32p), x.shape[0], _lib.ptr(y, _lib._f32p)))
        return y


def from_state_dict(sd, **kw) -> VespaG:
    input_dim, hidden = check_state_dict(sd)
    return VespaG(pack(sd), input_dim, hidden, **kw)


def op_vespag_head(sd, rows, wt_cols, precision: str = "f16x3", slope: float = NEGATIVE_SLOPE, device: int = 0) -> np.ndarray:
    """The head alone through pgmi_op_vespag_head: y float32 [R, 20]."""
    input_dim, hidden = check_state_dict(sd)
    x, wt = _lib.as_f32(rows), _lib.as_i32(wt_cols)
    w1, b1, w2, b2 = (_lib.as_f32(_to_np(sd[k])) for k in KEYS)
    y = np.empty((x.shape[0], OUT), np.float32)
    f = _lib._f32p
    _lib.check(_lib.load().pgmi_op_vespag_head(device, _lib.PRECISIONS[precision], _lib.ptr(x, f), _lib.ptr(w1, f), _lib.ptr(b1, f),
                                               _lib.ptr(w2, f), _lib.ptr(b2, f), _lib.ptr(wt, _lib._i32p), x.shape[0], input_dim, hidden,
                                               slope, _lib.ptr(y, f)))
    return y
