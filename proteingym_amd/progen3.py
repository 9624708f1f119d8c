"""ProGen3 scoring on libpgmi (include/pgmi.h, arch PGMI_ARCH_PROGEN3).

Replaces proteingym/baselines/progen3/progen3/scorer.py (ProGen3Scorer) and batch_preparer.py (prepare_clm): every sequence is scored
twice, ``<bos> 1 SEQ 2 <eos>`` and the same string with ``1 SEQ 2`` reversed character by character; a pass contributes the mean over its
T - 1 targets of log p(tok[t+1] | tok[<=t]) as an fp32 value, and the sequence's log-likelihood is (forward + reverse) / 2 in fp32,
its perplexity exp(-log-likelihood).  The forward is HIP (csrc/api_progen3.hip on csrc/api_gpt.hip's decoder loop; the routed expert
block in csrc/moe.hip).

Checkpoints are Hugging Face directories (config.json + model.safetensors / pytorch_model.bin).  Both expert layouts load: the eager one
(``block_sparse_moe.experts.E.w1|w2|w3.weight``, ``block_sparse_moe.gate.weight``) and the megablocks one that published checkpoints are
saved from (stacked ``block_sparse_moe.experts.mlp.w1 / v1 / w2`` of E * F rows, ``block_sparse_moe.router.layer.weight``).  The
megablocks mapping is worked out from model/mb_wrapper.py and megablocks' public layout (w2 stored as [E * F, D], the transpose of an
nn.Linear weight) and has NOT been checked against a published checkpoint: scripts/accept_real_weights.py --progen3 is where it
is first proven.
"""
from __future__ import annotations

import ctypes as C
import json
import os
import re
from typing import Sequence

import numpy as np

from . import _lib
from .causal_lm import DecoderHandle
from .tranception import load_hf_directory

MAX_BATCH_TOKENS = 65536                   # scorer.py:23
MAX_POSITIONS = 16384                      # rotary table rows built at creation (config.max_position_embeddings is 65536)

# progen3/tokenizer.json: the base vocabulary (ids 0 .. 33); ids 34 .. 133 are the <span_i> tokens of the infilling inputs, which
# scoring never produces
SPECIALS = {"<pad>": 0, "<bos>": 1, "<eos>": 2, "<bos_glm>": 3, "<eos_span>": 4, "<mask>": 5}
TOKENS = dict(SPECIALS, **{"1": 6, "2": 7}, **{chr(ord("A") + i): 8 + i for i in range(26)})
PAD_ID, BOS_ID, EOS_ID = 0, 1, 2
TOKENIZER_VOCAB = 134                      # tokenizer.get_vocab_size(): config.vocab_size is never smaller
CLM_PATTERN = re.compile(r"^[A-Z]+$")      # batch_preparer.py:14


# -- tokenisation ----------------------------------------------------------------------------------------------------------
def encode(sequence: str, reverse: bool = False) -> np.ndarray:
    """batch_preparer.py prepare_clm: ids of ``<bos>`` + s + ``<eos>`` with s = "1" + sequence + "2", reversed character by character
    for the C -> N pass."""
    if not CLM_PATTERN.match(sequence):
        raise ValueError(f"not an upper-case amino-acid sequence (infilling inputs are not scored): {sequence[:40]!r}")
    s = "1" + sequence + "2"
    if reverse:
        s = s[::-1]
    return np.array([BOS_ID] + [TOKENS[ch] for ch in s] + [EOS_ID], dtype=np.int32)


# -- scoring plan ----------------------------------------------------------------------------------------------------------
def group_by_length(sequences: Sequence[str], max_batch_tokens: int = MAX_BATCH_TOKENS):
    """scorer.py group_by_length: indices sorted by (length, index), a batch closed when length * (batch size + 1) would pass the
    token budget."""
    batches = [[]]
    for idx in sorted(range(len(sequences)), key=lambda i: (len(sequences[i]), i)):
        if batches[-1] and len(sequences[idx]) * (len(batches[-1]) + 1) > max_batch_tokens:
            batches.append([])
        batches[-1].append(idx)
    return batches


def scoring_plan(sequences: Sequence[str]):
    """The reference's forwards as (sequence index, direction, token ids) rows: N -> C, then C -> N."""
    return [(i, rev, encode(s, rev)) for i, s in enumerate(sequences) for rev in (False, True)]


def combine(n_seq: int, plan, sums, n_targets):
    """scorer.py _log_likelihoods / score_batch: a pass's -nll = sum / count formed in fp32, log_likelihood = (fwd + rev) / 2 in fp32,
    perplexity = exp(-log_likelihood) in fp32.  Returns (log_likelihood, perplexity) as float64 arrays of fp32 values (``.item()``)."""
    ll = np.zeros((n_seq, 2), dtype=np.float32)
    for (i, rev, _), s, n in zip(plan, sums, n_targets):
        ll[i, int(rev)] = np.float32(s) / np.float32(n)
    out = (ll[:, 0] + ll[:, 1]) / np.float32(2)
    return out.astype(np.float64), np.exp(-out).astype(np.float64)


# -- checkpoints -----------------------------------------------------------------------------------------------------------
def config_from_json(c: dict, max_positions: int = None) -> dict:
    """Model dims from a ProGen3 config.json (config.py ProGen3Config's defaults for what is absent); refuses what the forward does
    not implement."""
    act = c.get("hidden_act", "silu")
    if act != "silu":
        raise ValueError(f"ProGen3 hidden_act {act!r}: only silu is supported")
    if c.get("clip_qkv") is not None:
        raise ValueError(f"ProGen3 clip_qkv = {c['clip_qkv']}: not supported (the clamp sits between the fused QKV projection and the rotary)")
    if c.get("moe_expert_selection", "switch") != "switch":
        raise ValueError(f"ProGen3 moe_expert_selection {c['moe_expert_selection']!r}: only switch (softmax) is supported")
    if c.get("tie_word_embeddings", False):
        raise ValueError("ProGen3 config ties lm_head to the embedding: not supported (the released models do not)")
    D, H = int(c.get("hidden_size", 4096)), int(c.get("num_attention_heads", 32))
    dh = D // H
    if D % H or dh not in (64, 80, 96, 128, 256):
        raise ValueError(f"unsupported head_dim {D / H:g} (hidden_size {D} / num_attention_heads {H}): ProGen3 runs head dims 64, 80, 96, 128, 256")
    gated = bool(c.get("gated_mlp", False))
    F = c.get("intermediate_size")
    F = int(F) if F is not None else (3 * D if gated else 4 * D)
    E = int(c.get("num_experts", 8))
    KV = c.get("num_key_value_heads")
    P = int(c.get("max_position_embeddings", 65536))
    return dict(layers=int(c.get("num_hidden_layers", 40)), embed_dim=D, heads=H, ffn_dim=F,
                vocab=max(int(c.get("vocab_size") or 0), TOKENIZER_VOCAB), max_positions=int(max_positions or min(P, MAX_POSITIONS)),
                ln_eps=float(c.get("rms_norm_eps", 1e-5)), kv_heads=int(KV) if KV is not None else H, n_experts=E,
                top_k=min(int(c.get("num_experts_per_tok", 2)), E), gated=gated, rope_theta=float(c.get("rope_theta", 100000.0)),
                fused_attention_norm=bool(c.get("fused_attention_norm", False)))


def weight_count(cfg: dict) -> int:
    D, F, V, L, E = cfg["embed_dim"], cfg["ffn_dim"], cfg["vocab"], cfg["layers"], cfg["n_experts"]
    kvd = cfg["kv_heads"] * (D // cfg["heads"])
    layer = D + D * D + 2 * kvd * D + D * D + D + (E * D if E > 1 else 0) + E * ((2 if cfg["gated"] else 1) * F * D + D * F)
    return V * D + D + L * layer + D + V * D


def expert_layout(sd, layer: int = 0) -> str:
    """"eager" or "megablocks", from the names of layer `layer`'s expert tensors."""
    p = f"model.layers.{layer}.block_sparse_moe."
    if p + "experts.0.w1.weight" in sd:
        return "eager"
    if p + "experts.mlp.w1" in sd:
        return "megablocks"
    found = sorted(k for k in sd if k.startswith(p))[:6]
    raise ValueError(f"unrecognised ProGen3 expert layout under {p}: found {found}; known are the eager names (experts.E.w1|w2|w3.weight, "
                     f"gate.weight) and the megablocks names (experts.mlp.w1|v1|w2, router.layer.weight) -- the megablocks mapping itself "
                     f"is unproven against a published checkpoint (scripts/accept_real_weights.py --progen3)")


def _tensors(cfg: dict, sd):
    D, F, E, gated = cfg["embed_dim"], cfg["ffn_dim"], cfg["n_experts"], cfg["gated"]
    layout = expert_layout(sd)
    yield sd["model.embed_tokens.weight"]
    yield np.asarray(sd["model.embed_seq_id.weight"])[0]
    for i in range(cfg["layers"]):
        p = f"model.layers.{i}."
        a = p + ("norm_attn_norm." if cfg["fused_attention_norm"] else "")       # the same arithmetic under another prefix
        yield sd[a + "input_layernorm.weight"]
        for name in ("q_proj", "k_proj", "v_proj", "o_proj"):
            yield sd[a + f"self_attn.{name}.weight"]
        yield sd[a + "post_attention_layernorm.weight"]
        m = p + "block_sparse_moe."
        if layout == "eager":
            if E > 1:
                yield sd[m + "gate.weight"]
            for e in range(E):
                yield sd[m + f"experts.{e}.w1.weight"]
                if gated:
                    yield sd[m + f"experts.{e}.w3.weight"]
                yield sd[m + f"experts.{e}.w2.weight"]
        else:
            # megablocks: w1 / v1 [E * F, D] are the experts' nn.Linear weights stacked; w2 [E * F, D] holds every expert's
            # down-projection as [F, D], the transpose of nn.Linear's [D, F]
            if E > 1:
                yield sd[m + "router.layer.weight"]
            w1 = np.asarray(sd[m + "experts.mlp.w1"]).reshape(E, F, D)
            v1 = np.asarray(sd[m + "experts.mlp.v1"]).reshape(E, F, D) if gated else None
            w2 = np.asarray(sd[m + "experts.mlp.w2"]).reshape(E, F, D)
            for e in range(E):
                yield w1[e]
                if gated:
                    yield v1[e]
                yield w2[e].T
    yield sd["model.norm.weight"]
    yield sd["lm_head.weight"]


def pack(cfg: dict, sd) -> np.ndarray:
    """The C ABI's blob (include/pgmi.h, ProGen3) from a state dict of numpy arrays or torch tensors in either expert layout."""
    sd = {k: (v.detach().float().numpy() if hasattr(v, "detach") else np.asarray(v, dtype=np.float32)) for k, v in sd.items()}
    V = sd["lm_head.weight"].shape[0] if "lm_head.weight" in sd else cfg["vocab"]
    cfg["vocab"] = int(V)                                   # the checkpoint's own embedding rows (config.vocab_size, never below the tokenizer's)
    blob = np.empty(weight_count(cfg), dtype=np.float32)
    o = 0
    try:
        for a in _tensors(cfg, sd):
            a = np.asarray(a, dtype=np.float32)
            if o + a.size > blob.size:
                raise ValueError(f"ProGen3 state dict holds more weights than its config describes ({blob.size})")
            blob[o:o + a.size] = a.ravel()
            o += a.size
    except KeyError as e:
        raise RuntimeError(f"Missing key in ProGen3 state_dict: {e.args[0]}") from None
    if o != blob.size:
        raise ValueError(f"ProGen3 state dict holds {o} weights, its config describes {blob.size}")
    return blob


def load_directory(checkpoint_dir: str):
    """load_hf_directory, and the sharded form the larger checkpoints are published in: model.safetensors.index.json naming
    model-0000i-of-0000n.safetensors files."""
    index = os.path.join(checkpoint_dir, "model.safetensors.index.json")
    if not os.path.exists(index) or any(os.path.exists(os.path.join(checkpoint_dir, f)) for f in ("model.safetensors", "pytorch_model.bin")):
        return load_hf_directory(checkpoint_dir)
    from safetensors.numpy import load_file
    sd = {}
    for fn in sorted(set(json.load(open(index))["weight_map"].values())):
        sd.update(load_file(os.path.join(checkpoint_dir, fn)))
    return json.load(open(os.path.join(checkpoint_dir, "config.json"))), sd


def load_checkpoint(checkpoint_dir: str, max_positions: int = None):
    """config.json + model.safetensors (one file or shards) / pytorch_model.bin.  Returns (cfg dict, blob)."""
    c, sd = load_directory(checkpoint_dir)
    cfg = config_from_json(c, max_positions)
    return cfg, pack(cfg, sd)


# -- model -----------------------------------------------------------------------------------------------------------------
class ProGen3Model(DecoderHandle):
    """Device-resident ProGen3 (f16x3)."""
    ARCH, CREATE, TOKEN_LOGPROBS = _lib.ARCH_PROGEN3, "pgmi_pg3_model_create", "pgmi_pg3_token_logprobs"

    def __init__(self, cfg: dict, weights: np.ndarray, device: int = 0, max_rows: int = 0):
        params = _lib.Pg3Params(kv_heads=cfg["kv_heads"], n_experts=cfg["n_experts"], top_k=cfg["top_k"], gated=int(cfg["gated"]),
                                rope_theta=cfg["rope_theta"], clip_qkv=float(cfg.get("clip_qkv") or 0.0))
        self._params = params
        super().__init__(cfg, weights, C.byref(params), device, max_rows)

    @staticmethod
    def _weight_count(lib, c, params):
        n = lib.pgmi_pg3_weight_count(C.byref(c), params)
        if n < 0:                                           # let the library say what it refuses
            h = C.c_void_p()
            _lib.check(lib.pgmi_pg3_model_create(C.byref(c), params, None, 0, 0, C.byref(h)))
        return n

    def sequence_loglik(self, rows: Sequence[np.ndarray]):
        """Whole id rows of any lengths, right-padded with <pad> to the longest -> (sum of log p(ids[t+1] | ids[<=t]) as float64,
        target count)."""
        lens = np.array([len(r) for r in rows], dtype=np.int32)
        T = int(lens.max())
        t = np.full((len(rows), T), PAD_ID, dtype=np.int32)
        for j, r in enumerate(rows):
            t[j, :len(r)] = r
        out = np.empty(len(rows), dtype=np.float64)
        n = np.empty(len(rows), dtype=np.int32)
        _lib.check(_lib.load().pgmi_pg3_sequence_loglik(self._h, _lib.ptr(t, _lib._i32p), _lib.ptr(lens, _lib._i32p), len(rows), T,
                                                         _lib.ptr(out, _lib._f64p), _lib.ptr(n, _lib._i32p)))
        return out, n

    def routing(self, layer: int, rows: int):
        """The experts and weights layer `layer` chose for the first `rows` token rows of the last device chunk: ([rows, top_k] int32,
        [rows, top_k] float32)."""
        k = self.cfg["top_k"]
        ids = np.empty((rows, k), dtype=np.int32)
        w = np.empty((rows, k), dtype=np.float32)
        _lib.check(_lib.load().pgmi_pg3_routing(self._h, layer, rows, _lib.ptr(ids, _lib._i32p), _lib.ptr(w, _lib._f32p)))
        return ids, w

    def score(self, sequences: Sequence[str], max_batch_tokens: int = MAX_BATCH_TOKENS):
        """ProGen3Scorer.evaluate: (log_likelihood, perplexity) per sequence.  The reference's length-sorted batches under the token
        budget, both directions of a batch in one device call."""
        sequences = list(sequences)
        plan = scoring_plan(sequences)
        sums = np.zeros(len(plan), dtype=np.float64)
        n = np.zeros(len(plan), dtype=np.int32)
        for batch in group_by_length(sequences, max_batch_tokens):
            idx = [2 * i + d for i in batch for d in (0, 1)]
            s, k = self.sequence_loglik([plan[j][2] for j in idx])
            sums[idx] = s
            n[idx] = k
        return combine(len(sequences), plan, sums, n)


def from_pretrained(checkpoint_dir: str, device: int = 0, max_rows: int = 0, max_positions: int = None) -> ProGen3Model:
    cfg, blob = load_checkpoint(checkpoint_dir, max_positions)
    model = ProGen3Model(cfg, blob, device=device, max_rows=max_rows)
    del blob
    return model
