"""CARP on libpgmi (include/pgmi.h, CARP section): the checkpoint reader with its refusals, the float64 fold of the embedding into a
token table, the convolution weight permutation, tokenisation, the device-resident model and the two scoring rules of
proteingym/baselines/carp_mif/compute_fitness.py.

``sequence_models`` (microsoft/protein-sequence-models) is not a dependency: every fact about it that this module relies on is one
named constant or function below, and DESIGN.md 4.6o lists them under "Read from the libraries' documented behaviour, not run here".
MIF and MIF-ST (the structure-conditioned models of the same launcher) are refused by name."""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import Dict, List, Sequence

import numpy as np

from . import _lib

# ---- readings of sequence_models --------------------------------------------------------------------------------
CANONICAL_AAS = "ACDEFGHIKLMNPQRSTVWY"
SPECIALS = "*-#@"                                  # stop, gap (= pad), mask, start
PROTEIN_ALPHABET = CANONICAL_AAS + "BZXJOU" + SPECIALS
MASK = "#"
MASK_ID = PROTEIN_ALPHABET.index(MASK)
D_EMBED, KERNEL_SIZE, R_MAX, ACTIVATION, LN_EPS = 8, 5, 128, "gelu", 1e-5
# published checkpoints: name -> (d_model, n_layers, slim); the only shapes whose parameter count matches the name
CHECKPOINT_SHAPES = {"carp_600k": (128, 16, True), "carp_38M": (1024, 16, True), "carp_76M": (1024, 32, True),
                     "carp_640M": (1280, 56, False)}
# ProteinGym's config.json rows -> checkpoint names
MODEL_NAMES = {"CARP_600K": "carp_600k", "CARP_38M": "carp_38M", "CARP_76M": "carp_76M", "CARP_640M": "carp_640M"}

K_EMBED, K_UP_W, K_UP_B = "embedder.embedder.weight", "embedder.up_embedder.conv.weight", "embedder.up_embedder.conv.bias"
K_LAST_NORM, K_DECODER = "last_norm", "decoder.conv"


def block_keys(n: int) -> Dict[str, str]:
    """State-dict prefixes of block n: LN1, PFF1, LN2 (sequence1.0 / .2.conv / .3), the convolution, LN3, PFF2 (sequence2.0 / .2.conv)."""
    p = f"embedder.layers.{n}."
    return {"ln1": p + "sequence1.0", "pff1": p + "sequence1.2.conv", "ln2": p + "sequence1.3", "conv": p + "conv",
            "ln3": p + "sequence2.0", "pff2": p + "sequence2.2.conv"}


def hidden_width(d_model: int, slim: bool) -> int:
    return d_model // 2 if slim else d_model


def dilation_schedule(n_layers: int, r: int = R_MAX) -> List[int]:
    """Block n has dilation 2^(n mod (log2 r + 1)): 1, 2, .., r, 1, 2, .."""
    n_dil = int(np.log2(r)) + 1
    return [2 ** (n % n_dil) for n in range(n_layers)]


def param_count(d_model: int, n_layers: int, slim: bool, vocab: int = len(PROTEIN_ALPHABET), d_embed: int = D_EMBED,
                kernel_size: int = KERNEL_SIZE) -> int:
    D, H = d_model, hidden_width(d_model, slim)
    block = 2 * D + (D * H + H) + 2 * H + (H * H * kernel_size + H) + 2 * H + (H * D + D)
    return vocab * d_embed + (d_embed * D + D) + n_layers * block + 2 * D + (D * vocab + vocab)


class CarpConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("abi_version", "d_model", "d_hidden", "n_layers", "kernel_size", "r", "vocab", "mask_id",
                                         "precision", "max_rows")] + [("ln_eps", C.c_float)]


@dataclass
class CarpSpec:
    d_model: int
    d_hidden: int
    n_layers: int
    kernel_size: int
    r: int
    vocab: int
    slim: bool


# ---- checkpoint --------------------------------------------------------------------------------------------------------------------
def resolve_checkpoint(model_name: str, model_path: str | None) -> str:
    """``model_name`` is a path ending in .pt, or a name (a config.json row or a checkpoint name) resolved as
    ``{model_path}/{name}.pt``.  Nothing is downloaded: a missing file is an error that names it."""
    if model_name.endswith(".pt"):
        path = model_name
    else:
        low = model_name.lower()
        if "mif" in low:
            raise _lib.PgmiError(f"{model_name!r}: MIF and MIF-ST need the structure GNN and are not supported; CARP checkpoints only")
        if model_path is None:
            raise _lib.PgmiError(f"--model_path is needed to resolve the checkpoint name {model_name!r}")
        path = os.path.join(model_path, MODEL_NAMES.get(model_name, model_name) + ".pt")
    if not os.path.isfile(path):
        raise _lib.PgmiError(f"CARP checkpoint {path!r} not found (no download is attempted)")
    return path


def read_checkpoint(path: str) -> dict:
    """torch.load of a released checkpoint: a dict with ``model`` (the name), the hyper-parameters and ``model_state_dict``."""
    import torch
    ck = torch.load(path, map_location="cpu", weights_only=False)
    if not isinstance(ck, dict) or "model_state_dict" not in ck:
        raise _lib.PgmiError(f"{path!r} is not a CARP checkpoint: no 'model_state_dict'")
    return ck


def _np(t) -> np.ndarray:
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


def check_checkpoint(ck: dict) -> CarpSpec:
    """The shapes come from the tensors; the hyper-parameters are checked against them; anything that is not a plain CARP is refused
    with the cause."""
    name = str(ck.get("model", "carp"))
    low = name.lower()
    if "mif" in low:
        raise _lib.PgmiError(f"checkpoint model {name!r}: MIF and MIF-ST need the structure GNN and are not supported")
    if "carp" not in low:
        raise _lib.PgmiError(f"checkpoint model {name!r} is not a CARP model")
    if "big" in low or ck.get("big"):
        raise _lib.PgmiError(f"checkpoint model {name!r}: the 'big' ByteNet variant is not supported")
    if ck.get("causal"):
        raise _lib.PgmiError("causal convolutions are not supported (CARP is a masked LM)")
    if ck.get("rank") is not None:
        raise _lib.PgmiError(f"factorised feed-forwards (rank = {ck['rank']}) are not supported")
    if ck.get("activation", ACTIVATION) != ACTIVATION:
        raise _lib.PgmiError(f"activation {ck['activation']!r} is not supported (gelu only)")
    sd = {k: _np(v) for k, v in ck["model_state_dict"].items()}

    def need(key, ndim):
        if key not in sd:
            raise _lib.PgmiError(f"CARP checkpoint has no tensor {key!r}")
        if sd[key].ndim != ndim:
            raise _lib.PgmiError(f"{key}: {sd[key].ndim} dimensions, expected {ndim}")
        return sd[key]

    E, up = need(K_EMBED, 2), need(K_UP_W, 3)
    V, d_embed = E.shape
    if V != len(PROTEIN_ALPHABET):
        raise _lib.PgmiError(f"{K_EMBED}: {V} rows, the alphabet has {len(PROTEIN_ALPHABET)} letters")
    D = up.shape[0]
    n_layers = 0
    while block_keys(n_layers)["conv"] + ".weight" in sd:
        n_layers += 1
    if n_layers == 0:
        raise _lib.PgmiError("CARP checkpoint has no tensor 'embedder.layers.0.conv.weight'")
    if any(k.startswith(f"embedder.layers.{n_layers}.") for k in sd):
        raise _lib.PgmiError(f"block {n_layers} has tensors but no convolution")
    conv0 = need(block_keys(0)["conv"] + ".weight", 3)
    H, _, k = conv0.shape
    if H not in (D, D // 2):
        raise _lib.PgmiError(f"hidden width {H} is neither d_model = {D} nor d_model / 2")
    slim = H != D
    spec = CarpSpec(D, H, n_layers, k, int(ck.get("r", R_MAX)), V, slim)
    for key, have in (("d_embed", d_embed), ("d_model", D), ("n_layers", n_layers), ("kernel_size", k), ("slim", slim)):
        if key in ck and ck[key] != have:
            raise _lib.PgmiError(f"hyper-parameter {key} = {ck[key]!r}, the tensors say {have!r}")
    if spec.r < 1 or spec.r & (spec.r - 1):
        raise _lib.PgmiError(f"r = {spec.r} is not a power of two")
    want = {K_EMBED: (V, d_embed), K_UP_W: (D, d_embed, 1), K_UP_B: (D,), K_LAST_NORM + ".weight": (D,), K_LAST_NORM + ".bias": (D,),
            K_DECODER + ".weight": (V, D, 1), K_DECODER + ".bias": (V,)}
    for n in range(n_layers):
        b = block_keys(n)
        for ln, width in (("ln1", D), ("ln2", H), ("ln3", H)):
            want[b[ln] + ".weight"] = want[b[ln] + ".bias"] = (width,)
        want[b["pff1"] + ".weight"], want[b["pff1"] + ".bias"] = (H, D, 1), (H,)
        want[b["conv"] + ".weight"], want[b["conv"] + ".bias"] = (H, H, k), (H,)
        want[b["pff2"] + ".weight"], want[b["pff2"] + ".bias"] = (D, H, 1), (D,)
    for key, shape in want.items():
        if key not in sd:
            raise _lib.PgmiError(f"CARP checkpoint has no tensor {key!r}")
        if tuple(sd[key].shape) != shape:
            raise _lib.PgmiError(f"{key}: shape {tuple(sd[key].shape)}, expected {shape}")
        if not np.isfinite(sd[key]).all():
            raise _lib.PgmiError(f"{key}: non-finite values")
    extra = sorted(set(sd) - set(want))
    if extra:
        raise _lib.PgmiError(f"CARP checkpoint has tensors this model does not have: {extra[:4]}")
    return spec


def fold_token_table(sd: Dict[str, np.ndarray]) -> np.ndarray:
    """Float64: Embedding(V, 8) through the 1x1 up-embedder, [V][D]; row v = W_up E[v] + b_up."""
    E, W, b = (np.asarray(_np(sd[k]), dtype=np.float64) for k in (K_EMBED, K_UP_W, K_UP_B))
    return E @ W[:, :, 0].T + b


def permute_conv_weight(w) -> np.ndarray:
    """conv.weight [out][in][tap] -> [out][tap][in]: row o is the K = taps * in axis of the implicit GEMM, tap-major."""
    return np.ascontiguousarray(np.transpose(_np(w), (0, 2, 1)))


def blob_from_state(sd: Dict[str, np.ndarray], spec: CarpSpec) -> np.ndarray:
    """The weight blob in include/pgmi.h's order."""
    f = np.float32
    parts = [fold_token_table(sd).astype(f).ravel()]

    def get(key):
        return np.asarray(_np(sd[key]), dtype=f)

    for n in range(spec.n_layers):
        b = block_keys(n)
        parts += [get(b["ln1"] + ".weight"), get(b["ln1"] + ".bias"), get(b["pff1"] + ".weight")[:, :, 0].ravel(), get(b["pff1"] + ".bias"),
                  get(b["ln2"] + ".weight"), get(b["ln2"] + ".bias"), permute_conv_weight(get(b["conv"] + ".weight")).ravel(),
                  get(b["conv"] + ".bias"), get(b["ln3"] + ".weight"), get(b["ln3"] + ".bias"),
                  get(b["pff2"] + ".weight")[:, :, 0].ravel(), get(b["pff2"] + ".bias")]
    parts += [get(K_LAST_NORM + ".weight"), get(K_LAST_NORM + ".bias"), get(K_DECODER + ".weight")[:, :, 0].ravel(), get(K_DECODER + ".bias")]
    return np.concatenate(parts)


# ---- tokens and mutants ------------------------------------------------------------------------------------------------------------
def tokenize(seq: str) -> np.ndarray:
    """The collater adds no start or stop token: L letters are L tokens."""
    try:
        return np.array([PROTEIN_ALPHABET.index(a) for a in seq], dtype=np.int32)
    except ValueError:
        bad = next(a for a in seq if a not in PROTEIN_ALPHABET)
        raise ValueError(f"letter {bad!r} is not in CARP's alphabet") from None


def parse_mutant(mutant: str, sequence: str, offset_idx: int = 1) -> List[tuple]:
    """compute_fitness.py:19-26: 'A5C:D7E' -> [(4, 'A', 'C'), (6, 'D', 'E')]; a wild-type letter that is not the sequence's is refused."""
    out = []
    for row in mutant.split(":"):
        wt, idx, mt = row[0], int(row[1:-1]) - offset_idx, row[-1]
        if idx < 0 or idx >= len(sequence) or sequence[idx] != wt:
            raise ValueError(f"{row}: the listed wildtype does not match the provided sequence")
        if mt not in PROTEIN_ALPHABET:
            raise ValueError(f"{row}: letter {mt!r} is not in CARP's alphabet")
        out.append((idx, wt, mt))
    return out


def get_mutated_sequence(focus_seq: str, mutant: str, start_idx: int = 1) -> str:
    """compute_fitness.py:96-111."""
    s = list(focus_seq)
    for idx, _, mt in parse_mutant(mutant, focus_seq, start_idx):
        if mt not in CANONICAL_AAS:
            raise ValueError(f"mutant to_AA is invalid: {mutant}")
        s[idx] = mt
    return "".join(s)


def mean_substitution_score(subs: Sequence[tuple], row_of: Dict[int, np.ndarray]) -> float:
    """compute_fitness.py:27-30: the MEAN over a mutant's substitutions of lp[i, mt] - lp[i, wt] (score / len(rows))."""
    score = 0.0
    for idx, wt, mt in subs:
        lp = row_of[idx]
        score += float(lp[PROTEIN_ALPHABET.index(mt)] - lp[PROTEIN_ALPHABET.index(wt)])
    return score / len(subs)


def masked_marginal_scores(model, target_seq: str, mutants: Sequence[str], offset_idx: int = 1) -> np.ndarray:
    """compute_fitness.py:67-93.  Only the positions some mutant touches are run; there is no context window."""
    subs = [parse_mutant(m, target_seq, offset_idx) for m in mutants]
    positions = sorted({idx for s in subs for idx, _, _ in s})
    if not positions:
        return np.zeros(0, dtype=np.float64)
    lp = model.masked_logprobs(tokenize(target_seq), positions)
    row_of = {p: lp[i] for i, p in enumerate(positions)}
    return np.array([mean_substitution_score(s, row_of) for s in subs], dtype=np.float64)


def pseudo_likelihood_scores(model, seqs: Sequence[str]) -> np.ndarray:
    """compute_fitness.py:52-66: minus CrossEntropyLoss of one unmasked forward = the mean over the L tokens of log p(x_t)."""
    toks = [tokenize(s) for s in seqs]
    if not toks:
        return np.zeros(0, dtype=np.float64)
    return model.sequence_loglik(toks) / np.array([len(t) for t in toks], dtype=np.float64)


# ---- the model ---------------------------------------------------------------------------------------------------------------------
def _pack(token_rows):
    rows = [_lib.as_i32(t) for t in token_rows]
    lens = np.array([len(t) for t in rows], dtype=np.int32)
    tok = _lib.as_i32(np.concatenate(rows)) if rows else np.zeros(0, np.int32)
    return tok, lens


class CarpModel(_lib.SideHandle):
    """A device-resident CARP."""

    PREFIX = "carp"

    def __init__(self, ck: dict, device: int = 0, precision: str = "f16x3", max_rows: int = 0):
        if precision not in _lib.PRECISIONS:
            raise _lib.PgmiError(f"unknown precision {precision!r}")
        self.spec = check_checkpoint(ck)
        s = self.spec
        c = CarpConfig(abi_version=_lib.ABI_VERSION, d_model=s.d_model, d_hidden=s.d_hidden, n_layers=s.n_layers, kernel_size=s.kernel_size,
                       r=s.r, vocab=s.vocab, mask_id=MASK_ID, precision=_lib.PRECISIONS[precision], max_rows=max_rows, ln_eps=LN_EPS)
        self._create(c, blob_from_state(ck["model_state_dict"], s), device)
        self.V = s.vocab

    def token_logprobs(self, token_rows) -> List[np.ndarray]:
        """One [L_i, V] array of log-probabilities per sequence, from one unmasked forward each."""
        tok, lens = _pack(token_rows)
        out = np.empty((int(lens.sum()), self.V), dtype=np.float32)
        _lib.check(_lib.load().pgmi_carp_token_logprobs(self._h, _lib.ptr(tok, _lib._i32p), _lib.ptr(lens, _lib._i32p), len(lens),
                                                        _lib.ptr(out, _lib._f32p)))
        return np.split(out, np.cumsum(lens)[:-1])

    def masked_logprobs(self, wt_tokens, positions) -> np.ndarray:
        """[n_pos, V]: row i = the log-probabilities at positions[i] of the sequence with that token masked."""
        wt, pos = _lib.as_i32(wt_tokens), _lib.as_i32(positions)
        out = np.empty((len(pos), self.V), dtype=np.float32)
        _lib.check(_lib.load().pgmi_carp_masked_logprobs(self._h, _lib.ptr(wt, _lib._i32p), len(wt), _lib.ptr(pos, _lib._i32p), len(pos),
                                                         _lib.ptr(out, _lib._f32p)))
        return out

    def sequence_loglik(self, token_rows) -> np.ndarray:
        """Per sequence, the sum over its tokens of log p(x_t) from one unmasked forward (float64)."""
        tok, lens = _pack(token_rows)
        out = np.empty(len(lens), dtype=np.float64)
        _lib.check(_lib.load().pgmi_carp_sequence_loglik(self._h, _lib.ptr(tok, _lib._i32p), _lib.ptr(lens, _lib._i32p), len(lens),
                                                         _lib.ptr(out, _lib._f64p)))
        return out


def from_pretrained(path: str, device: int = 0, precision: str = "f16x3", max_rows: int = 0) -> CarpModel:
    return CarpModel(read_checkpoint(path), device=device, precision=precision, max_rows=max_rows)


# ---- single ops (tests) ----------------------------------------------------------------------------------------------------------
def op_dilated_conv(x, W, bias, seg_off, dilation: int, precision: str = "f16x3", device: int = 0) -> np.ndarray:
    """x [M, C], W [C, taps, C] (permute_conv_weight's form), bias [C], seg_off [n_seg + 1] -> [M, C]."""
    x, W, bias, seg = _lib.as_f32(x), _lib.as_f32(W), _lib.as_f32(bias), _lib.as_i32(seg_off)
    Cc, taps = W.shape[0], W.shape[1]
    if x.ndim != 2 or x.shape[1] != Cc or W.shape != (Cc, taps, Cc) or bias.shape != (Cc,) or seg[-1] != x.shape[0]:
        raise _lib.PgmiError("op_dilated_conv: inconsistent shapes")
    out = np.empty_like(x)
    p = _lib._f32p
    _lib.check(_lib.load().pgmi_op_dilated_conv(device, _lib.PRECISIONS[precision], _lib.ptr(x, p), _lib.ptr(W, p), _lib.ptr(bias, p),
                                                _lib.ptr(seg, _lib._i32p), len(seg) - 1, Cc, taps, dilation, _lib.ptr(out, p)))
    return out


def op_ln_gelu(x, w, b, eps: float = LN_EPS, precision: str = "f16x3", device: int = 0) -> np.ndarray:
    x, w, b = _lib.as_f32(x), _lib.as_f32(w), _lib.as_f32(b)
    out = np.empty_like(x)
    p = _lib._f32p
    _lib.check(_lib.load().pgmi_op_ln_gelu(device, _lib.PRECISIONS[precision], _lib.ptr(x, p), _lib.ptr(w, p), _lib.ptr(b, p), x.shape[0],
                                           x.shape[1], eps, _lib.ptr(out, p)))
    return out


def random_checkpoint(seed: int, d_model: int, n_layers: int, slim: bool, name: str = "carp_seeded") -> dict:
    """A seeded checkpoint in the released format (numpy tensors) for benches and tests; the mask row of the embedding is zero."""
    rng = np.random.default_rng(seed)
    f = np.float32
    V, D, H, k = len(PROTEIN_ALPHABET), d_model, hidden_width(d_model, slim), KERNEL_SIZE

    def lin(o, i, kk=1):
        return (rng.normal(0, 1.0, (o, i, kk)) / np.sqrt(i * kk)).astype(f), rng.normal(0, 0.1, (o,)).astype(f)

    def ln(n):
        return (1.0 + 0.1 * rng.normal(0, 1.0, (n,))).astype(f), rng.normal(0, 0.1, (n,)).astype(f)

    sd = {K_EMBED: rng.normal(0, 1.0, (V, D_EMBED)).astype(f)}
    sd[K_EMBED][MASK_ID] = 0.0
    sd[K_UP_W], sd[K_UP_B] = lin(D, D_EMBED)
    for n in range(n_layers):
        b = block_keys(n)
        for key, width in (("ln1", D), ("ln2", H), ("ln3", H)):
            sd[b[key] + ".weight"], sd[b[key] + ".bias"] = ln(width)
        sd[b["pff1"] + ".weight"], sd[b["pff1"] + ".bias"] = lin(H, D)
        sd[b["conv"] + ".weight"], sd[b["conv"] + ".bias"] = lin(H, H, k)
        sd[b["pff2"] + ".weight"], sd[b["pff2"] + ".bias"] = lin(D, H)
    sd[K_LAST_NORM + ".weight"], sd[K_LAST_NORM + ".bias"] = ln(D)
    sd[K_DECODER + ".weight"], sd[K_DECODER + ".bias"] = lin(V, D)
    return {"model": name, "d_embed": D_EMBED, "d_model": D, "n_layers": n_layers, "kernel_size": k, "r": R_MAX, "activation": ACTIVATION,
            "slim": slim, "model_state_dict": sd}
