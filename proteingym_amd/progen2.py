"""ProGen2 scoring on libpgmi (include/pgmi.h, arch PGMI_ARCH_PROGEN2).

Replaces proteingym/baselines/progen2/compute_fitness.py: the checkpoint is packed into the C ABI's blob, the forward runs in
HIP (csrc/api_progen2.hip on the causal decoder of csrc/api_gpt.hip), and ``calc_fitness`` reproduces the reference's per-sequence
loop -- chunks of n_positions characters, each scored in both reading directions, a terminal last target dropped, log-softmax over
the 25 amino-acid columns, -mean CE summed, halved and divided by the sequence length -- with the equal-length (chunk, direction) rows
of all sequences batched together.
"""
from __future__ import annotations

import json
import os
from collections import defaultdict
from typing import Sequence

import numpy as np

from . import _lib
from .causal_lm import DecoderHandle, chunks        # chunks: compute_fitness.py:44-53 splits as RITA's does

# progen2/tokenizer.json: one id per character
PAD, BOS, EOS = 0, 1, 2
TOKENS = {"1": 3, "2": 4, **{ch: 5 + i for i, ch in enumerate("ABCDEFGHIJKLMNOPQRSTUVWXYZ".replace("J", ""))}}
VOCAB_SIZE = 32
FIRST_AA, LAST_AA = 5, 29                 # compute_fitness.py:67-70: the log-softmax covers these logits columns
TERMINALS = (3, 4)                        # '1' and '2' (compute_fitness.py:59-64)
MP_NUM = 8                                # modeling_progen.py:157-168


def encode(seq: str) -> np.ndarray:
    try:
        return np.array([TOKENS[ch] for ch in seq], dtype=np.int32)
    except KeyError as e:
        raise ValueError(f"character {e.args[0]!r} is not in the ProGen2 vocabulary") from None


def get_mutated_sequence(focus_seq, mutant, start_idx=1, AA_vocab="ACDEFGHIKLMNPQRSTVWY"):
    """compute_fitness.py:84-103: the substituted sequence between the '1' ... '2' terminals."""
    mutated = list(focus_seq)
    for mutation in mutant.split(":"):
        from_AA, position, to_AA = mutation[0], int(mutation[1:-1]), mutation[-1]
        rel = position - start_idx
        assert from_AA == focus_seq[rel], f"Invalid from_AA or mutant position: {mutation}"
        assert to_AA in AA_vocab, f"Mutant to_AA is invalid: {mutation}"
        mutated[rel] = to_AA
    return "1" + "".join(mutated) + "2"


def sequences_to_score(DMS_data, target_seq: str, indel_mode: bool):
    """compute_fitness.py:143-144: terminals are added only when the file has no mutated_sequence column and indel mode is off;
    a mutated_sequence column is scored as it is."""
    if not indel_mode and "mutated_sequence" not in DMS_data.columns:
        return [get_mutated_sequence(target_seq, m) for m in DMS_data["mutant"]]
    return list(DMS_data["mutated_sequence"])


def scoring_plan(prots: Sequence[str], model_context_len: int):
    """The reference's forwards as (sequence index, token ids) rows: every chunk, then its reverse."""
    plan = []
    for i, prot in enumerate(prots):
        for chunk in chunks(prot, model_context_len):
            for p in (chunk, chunk[::-1]):
                ids = encode(p)
                if ids.size < 2:
                    raise ValueError(f"sequence {i} (length {len(prot)}): a chunk of {ids.size} token(s) at n_positions = "
                                     f"{model_context_len} leaves the model no input/target pair (the reference fails on it too)")
                # compute_fitness.py:59-64: after the terminal strip every target must be an amino acid (the reference asserts it)
                bad = [t for t in range(1, ids.size - (1 if ids[-1] in TERMINALS else 0)) if not FIRST_AA <= ids[t] <= LAST_AA]
                if bad:
                    raise ValueError(f"sequence {i}: a '1' / '2' terminal at position {bad[0]} of a scored chunk "
                                     f"({'reversed ' if p is not chunk else ''}chunk of {ids.size} tokens): the reference's assertion "
                                     f"that no target is a terminal fails on it too")
                plan.append((i, ids))
    return plan


def kept_targets(ids: np.ndarray) -> int:
    """Targets scored for one row: ids[1:] minus a terminal last target."""
    return ids.size - 1 - (1 if ids[-1] in TERMINALS else 0)


def combine(prots: Sequence[str], plan, sums, n_kept, reduction="mean") -> np.ndarray:
    """-mean CE per row summed per sequence, halved, / len (compute_fitness.py:72-80).  0 kept targets: NaN, as torch's mean."""
    out = np.zeros(len(prots), dtype=np.float64)
    for (i, _), s, n in zip(plan, sums, n_kept):
        out[i] += float(np.float32(s) / np.float32(n)) if n > 0 else float("nan")
    out /= 2.0
    if reduction == "mean":
        out /= np.array([len(p) for p in prots], dtype=np.float64)
    return out


# -- checkpoint ------------------------------------------------------------------------------------------------------------
def config_from_json(c: dict) -> dict:
    D, H, L = int(c["n_embd"]), int(c["n_head"]), int(c["n_layer"])
    if c.get("activation_function", "gelu_new") != "gelu_new":
        raise ValueError("only the gelu_new activation of the released ProGen2 checkpoints is supported")
    dh = D // H
    rd = c.get("rotary_dim")
    return dict(layers=L, embed_dim=D, heads=H, ffn_dim=int(c["n_inner"]) if c.get("n_inner") else 4 * D,
                vocab=int(c.get("vocab_size", VOCAB_SIZE)), max_positions=int(c["n_positions"]),
                rotary_dim=int(rd) if rd is not None else dh, ln_eps=float(c.get("layer_norm_epsilon", 1e-5)))


def expected_keys(n_layer):
    keys = ["transformer.wte.weight"]
    for i in range(n_layer):
        p = f"transformer.h.{i}."
        keys += [p + "ln_1.weight", p + "ln_1.bias", p + "attn.qkv_proj.weight", p + "attn.out_proj.weight",
                 p + "mlp.fc_in.weight", p + "mlp.fc_in.bias", p + "mlp.fc_out.weight", p + "mlp.fc_out.bias"]
    return keys + ["transformer.ln_f.weight", "transformer.ln_f.bias", "lm_head.weight", "lm_head.bias"]


def qkv_to_qkv_order(w: np.ndarray, heads: int) -> np.ndarray:
    """qkv_proj.weight [3D, D] as stored -- mp_num = 8 blocks of [q | v | k] rows, D/8 each (modeling_progen.py:157-168) -- reordered
    to [q | k | v], each block head-major (row h*dh + j = dim j of head h).  A pure row permutation: exact."""
    D = w.shape[1]
    blk = w.reshape(MP_NUM, 3, D // MP_NUM, D)
    return np.concatenate([blk[:, 0].reshape(D, D), blk[:, 2].reshape(D, D), blk[:, 1].reshape(D, D)])


def weight_count(cfg: dict) -> int:
    D, F, V, L = cfg["embed_dim"], cfg["ffn_dim"], cfg["vocab"], cfg["layers"]
    return V * D + L * (2 * D + 3 * D * D + D * D + F * D + F + D * F + D) + 2 * D + V * D + V


def pack(cfg: dict, sd) -> np.ndarray:
    """The C ABI's blob (include/pgmi.h, ProGen2) from a state dict of numpy arrays or torch tensors, written into ONE preallocated
    fp32 array tensor by tensor (progen2-xlarge is 25.6 GB in fp32: no intermediate concatenation)."""
    keys = expected_keys(cfg["layers"])
    missing = [k for k in keys if k not in sd]
    if missing:
        raise RuntimeError(f"Missing key(s) in ProGen2 state_dict: {missing[:8]}...")
    blob = np.empty(weight_count(cfg), dtype=np.float32)
    o = 0
    for k in keys:
        a = sd[k]
        if hasattr(a, "detach"):
            a = a.detach().float().numpy()
        a = np.asarray(a, dtype=np.float32)
        if k.endswith("attn.qkv_proj.weight"):
            a = qkv_to_qkv_order(a, cfg["heads"])
        blob[o:o + a.size] = a.ravel()
        o += a.size
    assert o == blob.size
    return blob


def load_checkpoint(checkpoint_dir: str):
    """config.json + pytorch_model.bin (the state-dict keys of modeling_progen.py).  Returns (cfg dict, blob)."""
    cfg = config_from_json(json.load(open(os.path.join(checkpoint_dir, "config.json"))))
    import torch
    path = os.path.join(checkpoint_dir, "pytorch_model.bin")
    try:
        sd = torch.load(path, map_location="cpu", mmap=True, weights_only=True)
    except Exception:            # an old (non-zip) serialization cannot be memory-mapped
        sd = torch.load(path, map_location="cpu", weights_only=True)
    blob = pack(cfg, sd)
    del sd
    return cfg, blob


# -- model -----------------------------------------------------------------------------------------------------------------
class ProGen2Model(DecoderHandle):
    """Device-resident ProGen2 (f16x3)."""
    ARCH, CREATE, TOKEN_LOGPROBS = _lib.ARCH_PROGEN2, "pgmi_pg2_model_create", "pgmi_pg2_token_logprobs"

    def __init__(self, cfg: dict, weights: np.ndarray, device: int = 0, max_rows: int = 0):
        super().__init__(cfg, weights, int(cfg["rotary_dim"]), device, max_rows)
        self.n_positions = cfg["max_positions"]

    def sequence_loglik(self, rows):
        """rows int32 [B,L] of whole (chunk, direction) id rows -> (sum of the kept targets' 25-column log-probs, kept count)."""
        t = _lib.as_i32(np.atleast_2d(np.asarray(rows)))
        B, L = t.shape
        out = np.empty(B, dtype=np.float32)
        kept = np.empty(B, dtype=np.int32)
        _lib.check(_lib.load().pgmi_pg2_sequence_loglik(self._h, _lib.ptr(t, _lib._i32p), B, L, _lib.ptr(out, _lib._f32p),
                                                         _lib.ptr(kept, _lib._i32p)))
        return out, kept

    def calc_fitness(self, prots: Sequence[str], model_context_len: int = None, reduction: str = "mean") -> np.ndarray:
        """compute_fitness.py:35-82 with the (chunk, direction) rows of equal length batched."""
        ctx = int(model_context_len or self.n_positions)
        plan = scoring_plan(prots, ctx)
        sums = np.zeros(len(plan), dtype=np.float32)
        kept = np.zeros(len(plan), dtype=np.int32)
        by_len = defaultdict(list)
        for j, (_, ids) in enumerate(plan):
            by_len[ids.size].append(j)
        for L, idx in by_len.items():
            s, k = self.sequence_loglik(np.stack([plan[j][1] for j in idx]))
            sums[idx] = s
            kept[idx] = k
        return combine(prots, plan, sums, kept, reduction)


def from_pretrained(checkpoint_dir: str, device: int = 0, max_rows: int = 0) -> ProGen2Model:
    cfg, blob = load_checkpoint(checkpoint_dir)
    model = ProGen2Model(cfg, blob, device=device, max_rows=max_rows)
    del blob
    return model
