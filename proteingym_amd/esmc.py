"""ESM C (ESM Cambrian) scoring on libpgmi (include/pgmi.h, arch PGMI_ARCH_ESMC).

Replaces the sequence-only path of proteingym/baselines/evoscale/compute_fitness.py: an ``ESMC`` state dict is packed into the C ABI's
blob, the forward runs in HIP (csrc/api_esmc.hip), and ``score_mutations`` reproduces ``score_mutations`` /
``_score_mutations_common`` (:20-143, :292-474) -- the same parsing and skips, one masked forward per unique mutated position with
the ESM C window rule, log-softmax over all 64 columns, scores as Python-float sums of fp32 differences -- with the masked rows of
an assay batched into one call (they all have the same length, so nothing is padded).
"""
from __future__ import annotations

import math
import os
import re
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .esm import VOCABULARY

# EsmSequenceTokenizer: the ids of ESM's 33-symbol alphabet (<cls> 0, <pad> 1, <eos> 2, <unk> 3, <mask> 32); 64 logits columns
CLS, PAD, EOS, UNK, MASK = 0, 1, 2, 3, 32
VOCAB = 64
TOKEN_IDS = {tok: i for i, tok in enumerate(VOCABULARY) if len(tok) == 1}
AMINO_ACIDS = "ACDEFGHIKLMNPQRSTVWY"
AA_TO_TOKEN = {aa: TOKEN_IDS[aa] for aa in AMINO_ACIDS}    # compute_fitness.py:311-320 (aa_to_token)
HEAD_DIM = 64
WINDOW_SIZE = 1024                                         # compute_fitness.py:561 (window_size=1024)
# pretrained.py:65-98: the released configurations
RELEASED = {"esmc_300M": dict(embed_dim=960, heads=15, layers=30), "esmc_600M": dict(embed_dim=1152, heads=18, layers=36)}
SNAPSHOT_FILES = {"esmc_300M": "data/weights/esmc_300m_2024_12_v0.pth", "esmc_600M": "data/weights/esmc_600m_2024_12_v0.pth"}


def swiglu_hidden(d_model: int, expansion_ratio: float = 8 / 3) -> int:
    """blocks.py:15-17 (swiglu_correction_fn)."""
    return int(((expansion_ratio * d_model) + 255) // 256 * 256)


def tokenize(sequence: str) -> np.ndarray:
    """<cls> + residues + <eos> (EsmSequenceTokenizer with special tokens); a character outside the alphabet is <unk>."""
    return np.array([CLS] + [TOKEN_IDS.get(ch, UNK) for ch in sequence] + [EOS], dtype=np.int32)


# -- checkpoint ------------------------------------------------------------------------------------------------------------
def expected_keys(n_layers: int) -> List[str]:
    """ESMC.state_dict() names, in blob order (tests/golden/esmc_state_dict_keys.json holds the reference's own list)."""
    keys = ["embed.weight"]
    for i in range(n_layers):
        p = f"transformer.blocks.{i}."
        keys += [p + "attn.layernorm_qkv.0.weight", p + "attn.layernorm_qkv.0.bias", p + "attn.layernorm_qkv.1.weight",
                 p + "attn.q_ln.weight", p + "attn.k_ln.weight", p + "attn.out_proj.weight",
                 p + "ffn.0.weight", p + "ffn.0.bias", p + "ffn.1.weight", p + "ffn.3.weight"]
    return keys + ["transformer.norm.weight", "sequence_head.0.weight", "sequence_head.0.bias", "sequence_head.2.weight",
                   "sequence_head.2.bias", "sequence_head.3.weight", "sequence_head.3.bias"]


def config_from_state_dict(sd, model_type: Optional[str] = None) -> dict:
    """d from embed.weight, layers from the block count, the SwiGLU width from ffn.1.weight, heads = d / 64."""
    D = int(np.shape(sd["embed.weight"])[1])
    L = 0
    while f"transformer.blocks.{L}.attn.out_proj.weight" in sd:
        L += 1
    F = int(np.shape(sd["transformer.blocks.0.ffn.1.weight"])[0]) // 2 if L else 0
    if L == 0 or D % HEAD_DIM:
        raise ValueError(f"not an ESM C state dict: d_model {D}, {L} blocks (head_dim 64 needs d % 64 == 0)")
    cfg = dict(layers=L, embed_dim=D, heads=D // HEAD_DIM, ffn_dim=F, vocab=VOCAB)
    if model_type is not None:
        if model_type not in RELEASED:
            raise ValueError(f"model_type {model_type!r}: this path scores {sorted(RELEASED)}")
        want = RELEASED[model_type]
        shape = dict(embed_dim=D, heads=D // HEAD_DIM, layers=L)
        other = [k for k, v in RELEASED.items() if k != model_type and v == shape]
        if other:
            raise ValueError(f"--model_type {model_type} but the checkpoint has the {other[0]} configuration (d_model {D}, {L} layers)")
        if shape != want:
            print(f"Warning: checkpoint (d_model {D}, {L} layers) is not the released {model_type} configuration {want}")
    return cfg


def load_state_dict(path: str, model_type: Optional[str] = None) -> Dict[str, np.ndarray]:
    """An ESMC state dict from a .pth file or a snapshot directory (data/weights/esmc_{300m,600m}_2024_12_v0.pth); every float tensor
    upcast to fp32.  Keys must be exactly ESMC.state_dict()'s.  Never downloads."""
    import torch
    if os.path.isdir(path):
        names = [SNAPSHOT_FILES[model_type]] if model_type in SNAPSHOT_FILES else list(SNAPSHOT_FILES.values())
        found = [os.path.join(path, n) for n in names if os.path.isfile(os.path.join(path, n))]
        if not found:
            raise FileNotFoundError(f"{path}: no ESM C weights at {' or '.join(names)}")
        path = found[0]
    raw = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(raw, dict):
        raise ValueError(f"{path}: expected a state dict, got {type(raw).__name__}")
    sd = {k: (v.detach().to(torch.float32).numpy() if v.is_floating_point() else v.numpy()) for k, v in raw.items()}
    cfg = config_from_state_dict(sd, model_type)
    want = expected_keys(cfg["layers"])
    missing, unexpected = sorted(set(want) - set(sd)), sorted(set(sd) - set(want))
    if missing or unexpected:
        raise ValueError(f"{path}: not an ESMC state dict (missing {missing[:5]}, unexpected {unexpected[:5]})")
    return sd


def interleave_w1(w1: np.ndarray) -> np.ndarray:
    """ffn.1.weight [2F, D] (gate rows, then up rows) -> SwiGLU block order: per 32 hidden units, their 32 gate rows then their 32
    up rows (include/pgmi.h, the FC1 epilogue's pairing)."""
    F = w1.shape[0] // 2
    if F % 32:
        raise ValueError(f"SwiGLU hidden width {F} is not a multiple of 32")
    g, u = w1[:F].reshape(F // 32, 32, -1), w1[F:].reshape(F // 32, 32, -1)
    return np.concatenate([g, u], axis=1).reshape(2 * F, -1)


def deinterleave_w1(w: np.ndarray) -> np.ndarray:
    F = w.shape[0] // 2
    b = w.reshape(F // 32, 64, -1)
    return np.concatenate([b[:, :32].reshape(F, -1), b[:, 32:].reshape(F, -1)], axis=0)


def weight_count(cfg: dict) -> int:
    D, F, V, L = cfg["embed_dim"], cfg["ffn_dim"], cfg["vocab"], cfg["layers"]
    return V * D + L * (2 * D + 3 * D * D + 2 * D + D * D + 2 * D + 2 * F * D + D * F) + D + (D * D + D) + 2 * D + V * D + V


def pack(cfg: dict, sd) -> np.ndarray:
    """The blob of include/pgmi.h (PGMI_ARCH_ESMC): the state dict in expected_keys order, ffn.1.weight interleaved."""
    blob = np.empty(weight_count(cfg), dtype=np.float32)
    o = 0
    for k in expected_keys(cfg["layers"]):
        a = np.asarray(sd[k], dtype=np.float32)
        if k.endswith("ffn.1.weight"):
            a = interleave_w1(a)
        blob[o:o + a.size] = a.ravel()
        o += a.size
    assert o == blob.size
    return blob


def unpack(cfg: dict, blob: np.ndarray) -> Dict[str, np.ndarray]:
    """Inverse of pack (the float64 reference forward of the tests reads the blob through it)."""
    D, F, V = cfg["embed_dim"], cfg["ffn_dim"], cfg["vocab"]
    shapes = {"embed.weight": (V, D), "transformer.norm.weight": (D,), "sequence_head.0.weight": (D, D), "sequence_head.0.bias": (D,),
              "sequence_head.2.weight": (D,), "sequence_head.2.bias": (D,), "sequence_head.3.weight": (V, D), "sequence_head.3.bias": (V,)}
    per = {"attn.layernorm_qkv.1.weight": (3 * D, D), "attn.out_proj.weight": (D, D), "ffn.1.weight": (2 * F, D), "ffn.3.weight": (D, F)}
    sd, o = {}, 0
    for k in expected_keys(cfg["layers"]):
        tail = k.split(".", 3)[-1] if k.startswith("transformer.blocks.") else None
        shape = shapes.get(k) or per.get(tail, (D,))
        n = int(np.prod(shape))
        a = blob[o:o + n].reshape(shape)
        sd[k] = deinterleave_w1(a) if k.endswith("ffn.1.weight") else a
        o += n
    assert o == blob.size
    return sd


# -- scoring (compute_fitness.py:20-143, 292-474) -----------------------------------------------------------------------------
Parsed = Tuple[str, List[int], str, List[int], str]


def parse_mutations(sequence: str, mutations: Sequence[str], verbose: bool = False) -> List[Parsed]:
    """compute_fitness.py:64-135: (wt letters, 1-based positions, mt letters, 0-based positions, mutant) per scorable mutant; a part
    that does not re.match ([A-Z])(\\d+)([A-Z]), lies out of range or has the wrong wild type skips the whole mutant."""
    out = []
    for mutation in mutations:
        parts = mutation.split(":") if ":" in mutation else [mutation]
        wt_s, mt_s, pos, seq_pos, ok = "", "", [], [], True
        for part in parts:
            m = re.match(r"([A-Z])(\d+)([A-Z])", part)
            if not m:
                ok = False
                if verbose:
                    print(f"Warning: Could not parse mutation {part}, skipping")
                break
            wt, p, mt = m.group(1), int(m.group(2)), m.group(3)
            if p - 1 < 0 or p - 1 >= len(sequence) or sequence[p - 1] != wt:
                ok = False
                if verbose:
                    print(f"Warning: mutation {part} is out of range or does not match the wild type, skipping")
                break
            wt_s, mt_s = wt_s + wt, mt_s + mt
            pos.append(p)
            seq_pos.append(p - 1)
        if ok:
            out.append((wt_s, pos, mt_s, seq_pos, mutation))
    return out


def window(seq_pos: int, seq_len: int, window_size: int = WINDOW_SIZE) -> Tuple[int, int]:
    """compute_fitness.py:343-368: the residues [start, end) forwarded for a mask at seq_pos (the whole sequence when it fits)."""
    if seq_len <= window_size - 2:
        return 0, seq_len
    half = (window_size - 2) // 2
    start = max(0, seq_pos - half)
    end = min(seq_len, start + window_size - 2)
    if end == seq_len:
        start = max(0, seq_len - (window_size - 2))
    return start, end


def masked_rows(sequence: str, positions: Sequence[int], window_size: int = WINDOW_SIZE):
    """The reference's forwards as rows: tokens [P, T] (<cls> + window + <eos>) and the mask column of each."""
    tok = tokenize(sequence)                      # tok[1 + i] = residue i
    rows, mask = [], []
    for p in positions:
        s, e = window(p, len(sequence), window_size)
        rows.append(np.concatenate([[CLS], tok[1 + s:1 + e], [EOS]]).astype(np.int32))
        mask.append(p - s + 1)
    return np.stack(rows) if rows else np.zeros((0, 0), np.int32), np.array(mask, dtype=np.int32)


def check_letters(parsed: Sequence[Parsed]):
    """aa_to_token holds the 20 standard amino acids only: any other wild-type or mutant letter is the reference's KeyError."""
    for wt, _, mt, _, _ in parsed:
        for ch in wt + mt:
            if ch not in AA_TO_TOKEN:
                raise KeyError(ch)


def combine(parsed: Sequence[Parsed], lp_by_pos: Dict[int, np.ndarray]) -> Dict[str, float]:
    """compute_fitness.py:421-472: (lp[mt] - lp[wt]) in fp32, summed as Python floats from 0.0 for a multi-mutant."""
    scores = {}
    for wt, _, mt, seq_pos, name in parsed:
        if len(seq_pos) > 1:
            score = 0.0
            for i, p in enumerate(seq_pos):
                lp = lp_by_pos[p]
                score += float(lp[AA_TO_TOKEN[mt[i]]] - lp[AA_TO_TOKEN[wt[i]]])
        else:
            lp = lp_by_pos[seq_pos[0]]
            score = float(lp[AA_TO_TOKEN[mt]] - lp[AA_TO_TOKEN[wt]])
        scores[name] = score
    return scores


# -- model -----------------------------------------------------------------------------------------------------------------
class ESMC(_lib.ModelHandle):
    """Device-resident ESM C (f16x3)."""

    def __init__(self, cfg: dict, weights: np.ndarray, device: int = 0, max_rows: int = 0):
        super().__init__(cfg, weights, device, max_rows, arch=_lib.ARCH_ESMC, vocab=VOCAB, ln_eps=1e-5)

    def token_logprobs(self, tokens) -> np.ndarray:
        """log_softmax(model(tokens).sequence_logits) over all 64 columns: [B,T] -> [B,T,64]."""
        t = _lib.as_i32(np.atleast_2d(np.asarray(tokens)))
        B, T = t.shape
        out = np.empty((B, T, VOCAB), dtype=np.float32)
        _lib.check(_lib.load().pgmi_token_logprobs(self._h, _lib.ptr(t, _lib._i32p), B, T, _lib.ptr(out, _lib._f32p)))
        return out

    def masked_logprobs(self, tokens, mask_pos) -> np.ndarray:
        """Row b forwarded with tokens[b, mask_pos[b]] = <mask>; the log-softmax of that row: [B,T], [B] -> [B,64]."""
        t = _lib.as_i32(np.atleast_2d(np.asarray(tokens)))
        mp = _lib.as_i32(mask_pos)
        out = np.empty((t.shape[0], VOCAB), dtype=np.float32)
        _lib.check(_lib.load().pgmi_masked_logprobs(self._h, _lib.ptr(t, _lib._i32p), _lib.ptr(mp, _lib._i32p), t.shape[0], t.shape[1],
                                                    _lib.ptr(out, _lib._f32p)))
        return out

    def score_mutations(self, sequence: str, mutations: Sequence[str], window_size: int = WINDOW_SIZE) -> Dict[str, float]:
        """compute_fitness.py score_mutations (sequence only): {mutant: score} for the scorable mutants."""
        if len(sequence) == 0:
            raise ValueError("Empty sequence provided")
        parsed = parse_mutations(sequence, mutations)
        if not parsed:
            print("No valid mutations to score")
            return {}
        check_letters(parsed)
        positions = sorted({p for _, _, _, sp, _ in parsed for p in sp})
        tokens, mask = masked_rows(sequence, positions, window_size)
        lp = self.masked_logprobs(tokens, mask)
        return combine(parsed, dict(zip(positions, lp)))


def from_state_dict(sd, device: int = 0, max_rows: int = 0, model_type: Optional[str] = None) -> ESMC:
    cfg = config_from_state_dict(sd, model_type)
    return ESMC(cfg, pack(cfg, sd), device=device, max_rows=max_rows)


def from_pretrained(path: str, model_type: Optional[str] = None, device: int = 0, max_rows: int = 0) -> ESMC:
    return from_state_dict(load_state_dict(path, model_type), device=device, max_rows=max_rows, model_type=model_type)
