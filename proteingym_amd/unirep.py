"""UniRep on libpgmi (include/pgmi.h, UniRep section): the checkpoint loader, the float64 folding of weight normalisation and of the
input-side products into per-token tables, the prefix planner and the device-resident model.  Host code here is numpy only.

Reference: proteingym/baselines/unirep/unirep.py (mLSTMCell1900, babbler1900), unirep_inference.py, utils/data_utils.py,
utils/io_utils.py.  A mutant's recurrent state equals the target sequence's up to its first changed residue, so the target runs once
(``UniRepModel.set_target``) and every mutant starts from the state stored at its join step: the same bits as a run from the zero
state, for fewer cell steps."""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _lib

# utils/data_utils.py:16-45 ('-' never reaches the model: unirep_inference.py:44 replaces it by 'X')
AA_TO_INT = {'M': 1, 'R': 2, 'H': 3, 'K': 4, 'D': 5, 'E': 6, 'S': 7, 'T': 8, 'N': 9, 'Q': 10, 'C': 11, 'U': 12, 'G': 13, 'P': 14, 'A': 15,
             'V': 16, 'I': 17, 'F': 18, 'Y': 19, 'W': 20, 'L': 21, 'O': 22, 'X': 23, 'Z': 23, 'B': 23, 'J': 23}
TOK_PAD, TOK_START, TOK_STOP = 0, 24, 25
VOCAB, N_OUT = 26, 25
VALID_AAS = "MRHKDESTNQCUGPAVIFYWLO"          # utils/data_utils.py:115, the filter io_utils.load_and_filter_seqs applies
MAX_LEN = 4000

_CELL = {"wx": "rnn_mlstm_mlstm_wx:0.npy", "wh": "rnn_mlstm_mlstm_wh:0.npy", "wmx": "rnn_mlstm_mlstm_wmx:0.npy",
         "wmh": "rnn_mlstm_mlstm_wmh:0.npy", "b": "rnn_mlstm_mlstm_b:0.npy", "gx": "rnn_mlstm_mlstm_gx:0.npy",
         "gh": "rnn_mlstm_mlstm_gh:0.npy", "gmx": "rnn_mlstm_mlstm_gmx:0.npy", "gmh": "rnn_mlstm_mlstm_gmh:0.npy"}    # unirep.py:89-97
_DENSE = (("fully_connected_weights:0.npy", "fully_connected_biases:0.npy"), ("dense_kernel:0.npy", "dense_bias:0.npy"))  # unirep.py:386-391


class UniRepConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("abi_version", "hidden", "vocab", "precision", "max_rows")]


# ---- tokens and sequences ----------------------------------------------------------------------------------------------------------
def format_seq(seq: str) -> np.ndarray:
    """data_utils.format_seq(stop=False): [start] + residues, after unirep_inference.py:44's '-' -> 'X'."""
    try:
        return np.array([TOK_START] + [AA_TO_INT[a] for a in seq.strip().replace('-', 'X')], dtype=np.int32)
    except KeyError as e:
        raise ValueError(f"letter {e.args[0]!r} is not in UniRep's alphabet") from None


def is_valid_seq(seq: str, max_len: int = MAX_LEN) -> bool:
    """utils/data_utils.py:110-119."""
    return len(seq) <= max_len and set(seq) <= set(VALID_AAS)


def load_and_filter_seqs(df) -> List[str]:
    """io_utils.load_and_filter_seqs (:157-180) in ProteinGym mode: np.unique of ``mutated_sequence`` (``mutant`` when that column is
    absent) -- sorted and de-duplicated --, '*' stripped from both ends, sequences that fail is_valid_seq dropped."""
    col = "mutated_sequence" if "mutated_sequence" in df.columns.values else "mutant"
    out = []
    for seq in np.unique(df[col].values):
        seq = seq.strip('*')
        if is_valid_seq(seq):
            out.append(seq)
    return out


def evotune_path(model_path: str, msa_filename: str) -> str:
    """unirep_inference.py:104-105."""
    return model_path + os.sep + msa_filename.split('.a2m')[0]


# ---- checkpoint --------------------------------------------------------------------------------------------------------------------
def load_arrays(path: str) -> Dict[str, np.ndarray]:
    """The checkpoint directory's arrays under short names (wx, wh, wmx, wmh, b, gx, gh, gmx, gmh, embed, dense_w, dense_b), with the
    reference's file names and its choice between the two names of the dense layer; names and shapes are checked."""
    if not os.path.isdir(path):
        raise _lib.PgmiError(f"UniRep checkpoint {path!r} is not a directory of .npy arrays")

    def get(fn):
        p = os.path.join(path, fn)
        if not os.path.exists(p):
            raise _lib.PgmiError(f"UniRep checkpoint {path!r} has no array {fn!r}")
        return np.load(p)

    a = {k: get(fn) for k, fn in _CELL.items()}
    a["embed"] = get("embed_matrix:0.npy")
    wn, bn = _DENSE[0] if os.path.exists(os.path.join(path, _DENSE[0][0])) else _DENSE[1]
    a["dense_w"], a["dense_b"] = get(wn), get(bn)
    check_arrays(a)
    return a


def arrays_from_files(files: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    """The same from a dict keyed by the reference's file names (tests, synthetic checkpoints)."""
    a = {}
    for k, fn in _CELL.items():
        if fn not in files:
            raise _lib.PgmiError(f"UniRep checkpoint has no array {fn!r}")
        a[k] = files[fn]
    if "embed_matrix:0.npy" not in files:
        raise _lib.PgmiError("UniRep checkpoint has no array 'embed_matrix:0.npy'")
    a["embed"] = files["embed_matrix:0.npy"]
    wn, bn = _DENSE[0] if _DENSE[0][0] in files else _DENSE[1]
    for fn in (wn, bn):
        if fn not in files:
            raise _lib.PgmiError(f"UniRep checkpoint has no array {fn!r}")
    a["dense_w"], a["dense_b"] = files[wn], files[bn]
    check_arrays(a)
    return a


def check_arrays(a: Dict[str, np.ndarray]) -> None:
    if a["wmh"].ndim != 2 or a["wmh"].shape[0] != a["wmh"].shape[1]:
        raise _lib.PgmiError(f"wmh: shape {a['wmh'].shape}, expected a square [H, H]")
    if a["embed"].ndim != 2:
        raise _lib.PgmiError(f"embed_matrix: shape {a['embed'].shape}, expected [vocab, embed]")
    H, (V, E) = a["wmh"].shape[0], a["embed"].shape
    if V != VOCAB:
        raise _lib.PgmiError(f"embed_matrix: {V} rows, the tokeniser has {VOCAB}")
    want = {"wx": (E, 4 * H), "wh": (H, 4 * H), "wmx": (E, H), "wmh": (H, H), "b": (4 * H,), "gx": (4 * H,), "gh": (4 * H,), "gmx": (H,),
            "gmh": (H,), "dense_w": (H, V - 1), "dense_b": (V - 1,)}
    for k, shape in want.items():
        if tuple(a[k].shape) != shape:
            raise _lib.PgmiError(f"{k}: shape {tuple(a[k].shape)}, expected {shape} (H = {H}, vocab = {V}, embed = {E})")
    for k, v in a.items():
        if not np.isfinite(v).all():
            raise _lib.PgmiError(f"{k}: non-finite values")


def fold(a: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    """Float64: weight normalisation applied once (unirep.py:119-122: tf.nn.l2_normalize(w, axis=0) * g = w * rsqrt(max(sum over rows
    of w^2, 1e-12)) * g per column), and the two input-side products of a step (unirep.py:123-124) as per-token tables:
    Tmx = E wmx' [26, H], Tx = E wx' + b [26, 4 H]."""
    def wn(w, g):
        w = w.astype(np.float64)
        return w / np.sqrt(np.maximum((w * w).sum(0, keepdims=True), 1e-12)) * g.astype(np.float64)

    E = a["embed"].astype(np.float64)
    return {"Tmx": E @ wn(a["wmx"], a["gmx"]), "Tx": E @ wn(a["wx"], a["gx"]) + a["b"].astype(np.float64),
            "wmh": wn(a["wmh"], a["gmh"]), "wh": wn(a["wh"], a["gh"]),
            "dense_w": a["dense_w"].astype(np.float64), "dense_b": a["dense_b"].astype(np.float64)}


BLOB_ORDER = ("Tmx", "Tx", "wmh", "wh", "dense_w", "dense_b")


def blob_from_arrays(a: Dict[str, np.ndarray]) -> np.ndarray:
    f = fold(a)
    return np.concatenate([f[k].astype(np.float32).ravel() for k in BLOB_ORDER])


# ---- planner -----------------------------------------------------------------------------------------------------------------------
@dataclass
class Plan:
    """How a call will run.  ``join[i]``: the residues sequence i shares with the target from the left (0 without a target);
    ``order``: the run order (by length, then by join step, so that the active rows of a step are a leading range of their chunk);
    ``chunks``: (first, last + 1) positions of ``order``, each of one length and at most max_rows rows; ``row_steps``: the cell
    evaluations the run executes = sum of len_i - join_i."""
    lens: np.ndarray
    join: np.ndarray
    order: np.ndarray
    chunks: List[tuple]
    row_steps: int


def join_step(tokens: np.ndarray, target: Optional[np.ndarray]) -> int:
    """Common prefix, in residues, of two formatted sequences (0 when there is no target or the first tokens differ)."""
    if target is None or tokens[0] != target[0]:
        return 0
    n = min(len(tokens), len(target)) - 1
    neq = np.nonzero(tokens[1:1 + n] != target[1:1 + n])[0]
    return int(neq[0]) if len(neq) else n


def plan(token_rows: Sequence[np.ndarray], target: Optional[np.ndarray] = None, max_rows: int = 8192) -> Plan:
    lens = np.array([len(t) - 1 for t in token_rows], dtype=np.int64)
    join = np.array([join_step(t, target) for t in token_rows], dtype=np.int64)
    order = np.lexsort((join, lens))                 # stable: by length, then by join step, then by position
    chunks, i0, n = [], 0, len(order)
    while i0 < n:
        i1 = i0
        while i1 < n and i1 - i0 < max_rows and lens[order[i1]] == lens[order[i0]]:
            i1 += 1
        chunks.append((i0, i1))
        i0 = i1
    return Plan(lens, join, order, chunks, int((lens - join).sum()))


# ---- the model ---------------------------------------------------------------------------------------------------------------------
class UniRepModel(_lib.SideHandle):
    """A device-resident UniRep."""

    PREFIX, CREATE = "unirep", "pgmi_unirep_model_create"

    def __init__(self, arrays: Dict[str, np.ndarray], device: int = 0, precision: str = "f16x3", max_rows: int = 0):
        if precision not in _lib.PRECISIONS:
            raise _lib.PgmiError(f"unknown precision {precision!r}")
        check_arrays(arrays)
        self.H = int(arrays["wmh"].shape[0])
        self.Hp = (self.H + 31) // 32 * 32
        c = UniRepConfig(abi_version=_lib.ABI_VERSION, hidden=self.H, vocab=VOCAB, precision=_lib.PRECISIONS[precision], max_rows=max_rows)
        self._create(c, blob_from_arrays(arrays), device)
        self.max_rows = max_rows or 8192
        self.target: Optional[np.ndarray] = None
        self.last_row_steps = 0

    def set_target(self, seq: Optional[str]):
        """Runs the target sequence once; later ``nll`` calls start every sequence from the state stored at its join step."""
        self.target = None
        if not seq:
            _lib.check(_lib.load().pgmi_unirep_set_target(self._h, None, 0))
            return
        t = format_seq(seq)
        _lib.check(_lib.load().pgmi_unirep_set_target(self._h, _lib.ptr(t, _lib._i32p), len(t) - 1))
        self.target = t

    def nll_tokens(self, token_rows: Sequence[np.ndarray], from_scratch: bool = False) -> np.ndarray:
        rows = [_lib.as_i32(t) for t in token_rows]
        off = np.zeros(len(rows) + 1, dtype=np.int64)
        np.cumsum([len(t) for t in rows], out=off[1:])
        tok = _lib.as_i32(np.concatenate(rows)) if rows else np.zeros(0, np.int32)
        out = np.empty(len(rows), dtype=np.float64)
        steps = C.c_int64(0)
        _lib.check(_lib.load().pgmi_unirep_sequence_nll(self._h, _lib.ptr(tok, _lib._i32p), _lib.ptr(off, _lib._i64p), len(rows),
                                                        int(bool(from_scratch)), _lib.ptr(out, _lib._f64p), C.byref(steps)))
        self.last_row_steps = int(steps.value)
        return out

    def nll(self, seqs: Sequence[str], from_scratch: bool = False) -> np.ndarray:
        """Unirep_score of every sequence: the mean negative log-likelihood (lower is fitter)."""
        return self.nll_tokens([format_seq(s) for s in seqs], from_scratch)

    def plan(self, seqs: Sequence[str], from_scratch: bool = False) -> Plan:
        return plan([format_seq(s) for s in seqs], None if from_scratch else self.target, self.max_rows)

    def token_logprobs(self, x_tokens) -> np.ndarray:
        x = _lib.as_i32(x_tokens)
        out = np.empty((len(x), N_OUT), dtype=np.float32)
        _lib.check(_lib.load().pgmi_unirep_token_logprobs(self._h, _lib.ptr(x, _lib._i32p), len(x), _lib.ptr(out, _lib._f32p)))
        return out

    def step(self, h_prev, c_prev, tokens):
        """One cell step (pgmi_op_mlstm_step): (h, c [rows, Hp], z [rows, 4, Hp]), padding included."""
        h_prev, c_prev, tok = _lib.as_f32(h_prev), _lib.as_f32(c_prev), _lib.as_i32(tokens)
        rows = len(tok)
        if h_prev.shape != (rows, self.H) or c_prev.shape != (rows, self.H):
            raise _lib.PgmiError(f"h_prev and c_prev must be [{rows}, {self.H}]")
        h = np.empty((rows, self.Hp), dtype=np.float32)
        c = np.empty((rows, self.Hp), dtype=np.float32)
        z = np.empty((rows, 4, self.Hp), dtype=np.float32)
        p = _lib._f32p
        _lib.check(_lib.load().pgmi_op_mlstm_step(self._h, _lib.ptr(h_prev, p), _lib.ptr(c_prev, p), _lib.ptr(tok, _lib._i32p), rows,
                                                  _lib.ptr(h, p), _lib.ptr(c, p), _lib.ptr(z, p)))
        return h, c, z


def from_pretrained(path: str, device: int = 0, precision: str = "f16x3", max_rows: int = 0) -> UniRepModel:
    return UniRepModel(load_arrays(path), device=device, precision=precision, max_rows=max_rows)


def random_arrays(seed: int, H: int, gain: float = 1.0, embed: int = 10) -> Dict[str, np.ndarray]:
    """Seeded arrays in the checkpoint's shapes for benches (short names)."""
    rng = np.random.default_rng(seed)
    f = np.float32

    def g(n):
        return (gain * (1.0 + 0.2 * rng.normal(0, 1.0, (n,)))).astype(f)

    return {"embed": rng.normal(0, 1.0, (VOCAB, embed)).astype(f), "wx": rng.normal(0, 1.0, (embed, 4 * H)).astype(f),
            "wh": rng.normal(0, 1.0, (H, 4 * H)).astype(f), "wmx": rng.normal(0, 1.0, (embed, H)).astype(f),
            "wmh": rng.normal(0, 1.0, (H, H)).astype(f), "b": rng.normal(0, 0.3, (4 * H,)).astype(f), "gx": g(4 * H), "gh": g(4 * H),
            "gmx": g(H), "gmh": g(H), "dense_w": rng.normal(0, 2.0 / np.sqrt(H), (H, N_OUT)).astype(f),
            "dense_b": rng.normal(0, 0.3, (N_OUT,)).astype(f)}
