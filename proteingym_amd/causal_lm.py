"""RITA and ProtGPT2 scoring on libpgmi (include/pgmi.h, arch PGMI_ARCH_GPT).

Replaces proteingym/baselines/rita/compute_fitness.py and proteingym/baselines/protgpt2/compute_fitness.py.  Both run the same
``calc_fitness`` loop: chunks of 1023 characters, every chunk and its character-reversed copy tokenized and scored separately, each
forward contributing -mean CE over ids[1:] given ids[:-1].  RITA sums the contributions; ProtGPT2 divides the sum by 2 * n_chunks.
Here the (sequence, chunk, direction) rows of all sequences are sorted by token count, right-padded and batched through
``pgmi_gpt_sequence_loglik``; the forward is HIP (csrc/api_gpt.hip).

RITA is a pre-LN causal decoder with rotate-half rotary (rita_modeling.py); ProtGPT2 is a GPT-2 (transformers GPT2LMHeadModel,
what the reference's AutoModelForCausalLM returns) with learned positions and a head tied to wte.  The host packs both into one blob
layout: GPT-2's Conv1D weights are transposed and its fused c_attn split into q / k / v.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Callable, Sequence

import numpy as np

from . import _lib
from .tranception import load_hf_directory

MODEL_CONTEXT_LEN = 1023                   # compute_fitness.py:13 (both): the chunk length in characters
FAMILIES = ("rita", "gpt2")
POS_KIND = {"rita": _lib.GPT_POS_ROTARY, "gpt2": _lib.GPT_POS_LEARNED}


# -- tokenizer -------------------------------------------------------------------------------------------------------------
def load_tokenizer(path: str):
    """The tokenizer the reference's AutoTokenizer wraps, from the `tokenizers` library: ``tokenizer.json`` (a file, or a directory
    holding one), else a byte-level BPE from ``vocab.json`` + ``merges.txt``.  ``encode(p).ids`` then carries the post-processor's
    special tokens, exactly as ``tokenizer.encode(p)`` does in the reference.  Returns a callable str -> int32 ids."""
    try:
        import tokenizers
    except ImportError as e:
        raise ImportError("scoring RITA / ProtGPT2 needs the `tokenizers` package (the backend of the reference's "
                          "AutoTokenizer): pip install tokenizers") from e
    if os.path.isdir(path):
        tj = os.path.join(path, "tokenizer.json")
        if os.path.exists(tj):
            tok = tokenizers.Tokenizer.from_file(tj)
        elif os.path.exists(os.path.join(path, "vocab.json")) and os.path.exists(os.path.join(path, "merges.txt")):
            tok = tokenizers.ByteLevelBPETokenizer(os.path.join(path, "vocab.json"), os.path.join(path, "merges.txt"))
        else:
            raise FileNotFoundError(f"{path}: no tokenizer.json, and no vocab.json + merges.txt")
    else:
        tok = tokenizers.Tokenizer.from_file(path)

    def encode(p: str) -> np.ndarray:
        return np.asarray(tok.encode(p).ids, dtype=np.int32)
    encode.vocab_size = tok.get_vocab_size()
    return encode


# -- scoring plan ----------------------------------------------------------------------------------------------------------
def chunks(prot: str, model_context_len: int = MODEL_CONTEXT_LEN):
    """compute_fitness.py:19-30 (and progen2/compute_fitness.py:44-53): one chunk below the context length, else 1 + int(len / n)
    windows (the last one empty when the length is a multiple of n)."""
    if len(prot) < model_context_len:
        return [prot]
    n = 1 + int(len(prot) / model_context_len)
    return [prot[i * model_context_len:(i + 1) * model_context_len] for i in range(n)]


def scoring_plan(prots: Sequence[str], encode: Callable[[str], np.ndarray], model_context_len: int = MODEL_CONTEXT_LEN):
    """The reference's forwards as (sequence index, token ids) rows: every chunk, then its reverse (compute_fitness.py:32-39)."""
    plan = []
    for i, prot in enumerate(prots):
        for chunk in chunks(prot, model_context_len):
            for p in (chunk, chunk[::-1]):
                ids = encode(p)
                if ids.size < 2:
                    raise ValueError(f"sequence {i} (length {len(prot)}): a chunk of {len(p)} character(s) encodes to {ids.size} "
                                     f"token(s) at a context of {model_context_len}: no input/target pair (the reference's mean "
                                     f"over zero targets is NaN)")
                plan.append((i, ids))
    return plan


def combine(n_prots: int, plan, sums, n_targets, family: str) -> np.ndarray:
    """-mean CE per row (an fp32 value, as loss.item()) summed per sequence; ProtGPT2 divides by the row count 2 * n_chunks."""
    out = np.zeros(n_prots, dtype=np.float64)
    rows = np.zeros(n_prots, dtype=np.int64)
    for (i, _), s, n in zip(plan, sums, n_targets):
        out[i] += float(np.float32(s / n))
        rows[i] += 1
    return out / rows if family == "gpt2" else out


def batches(lengths: Sequence[int], tile: int = 32):
    """Row indices sorted by token count and cut where the model's input length (count - 1) enters another 32-token tile: each
    batch pads to its own longest row."""
    order = sorted(range(len(lengths)), key=lambda j: lengths[j])
    out, cur, band = [], [], None
    for j in order:
        b = (lengths[j] - 2) // tile
        if cur and b != band:
            out.append(cur)
            cur = []
        cur.append(j)
        band = b
    if cur:
        out.append(cur)
    return out


# -- checkpoints -----------------------------------------------------------------------------------------------------------
def config_from_json(c: dict) -> dict:
    """Model dims from a RITA (model_type "rita") or GPT-2 config.json; refuses GPT-2 options the forward does not implement."""
    if c.get("model_type") == "rita" or "d_model" in c:
        D = int(c.get("d_model", 768))
        return dict(family="rita", layers=int(c.get("num_layers", 12)), embed_dim=D, heads=int(c.get("num_heads", 12)),
                    ffn_dim=int(c.get("d_feedforward") or D * int(c.get("ff_ratio", 4))), vocab=int(c.get("vocab_size", 26)),
                    max_positions=int(c.get("max_seq_len", 1024)), ln_eps=1e-5)       # nn.LayerNorm's default eps
    if c.get("activation_function", "gelu_new") != "gelu_new":
        raise ValueError(f"GPT-2 activation {c['activation_function']!r}: only gelu_new (ProtGPT2) is supported")
    for flag in ("scale_attn_by_inverse_layer_idx", "reorder_and_upcast_attn"):
        if c.get(flag, False):
            raise ValueError(f"GPT-2 config sets {flag}: not supported (ProtGPT2 does not)")
    if not c.get("scale_attn_weights", True):
        raise ValueError("GPT-2 config clears scale_attn_weights: not supported (ProtGPT2 scales by head_dim^-1/2)")
    if c.get("tie_word_embeddings", True) is False:
        raise ValueError("GPT-2 config unties lm_head from wte: not supported (ProtGPT2 ties them)")
    D = int(c["n_embd"])
    return dict(family="gpt2", layers=int(c["n_layer"]), embed_dim=D, heads=int(c["n_head"]),
                ffn_dim=int(c["n_inner"]) if c.get("n_inner") else 4 * D, vocab=int(c["vocab_size"]),
                max_positions=int(c["n_positions"]), ln_eps=float(c.get("layer_norm_epsilon", 1e-5)))


def weight_count(cfg: dict) -> int:
    D, F, V, L, P = cfg["embed_dim"], cfg["ffn_dim"], cfg["vocab"], cfg["layers"], cfg["max_positions"]
    layer = 2 * D + 3 * (D * D + D) + (D * D + D) + 2 * D + (F * D + F) + (D * F + D)
    return V * D + (P * D if cfg["family"] == "gpt2" else 0) + L * layer + 2 * D + (V * D if cfg["family"] == "rita" else 0)


def _rita_tensors(cfg, sd):
    D, H = cfg["embed_dim"], cfg["heads"]
    dh = D // H
    inv = (1.0 / (10000 ** (np.arange(0, dh, 2, dtype=np.float32) / np.float32(dh)))).astype(np.float32)
    yield sd["transformer.embedding.weight"]
    for i in range(cfg["layers"]):
        p = f"transformer.layers.{i}."
        f = sd.get(p + "self_attention.rotary_embedding.inv_freq")
        if f is not None and not np.allclose(np.asarray(f, dtype=np.float32), inv, rtol=1e-6, atol=0):
            raise ValueError(f"{p}self_attention.rotary_embedding.inv_freq differs from 10000^(-arange(0, {dh}, 2) / {dh})")
        yield sd[p + "attn_norm.weight"]
        yield sd[p + "attn_norm.bias"]
        for name in ("query", "key", "value", "proj"):
            yield sd[p + f"self_attention.{name}.weight"]
            yield sd[p + f"self_attention.{name}.bias"]
        yield sd[p + "mlp_norm.weight"]
        yield sd[p + "mlp_norm.bias"]
        for name in ("mlp.0", "mlp.2"):
            yield sd[p + name + ".weight"]
            yield sd[p + name + ".bias"]
    yield sd["transformer.final_norm.weight"]
    yield sd["transformer.final_norm.bias"]
    yield sd["lm_head.weight"]


def _gpt2_tensors(cfg, sd):
    D = cfg["embed_dim"]
    yield sd["transformer.wte.weight"]
    yield sd["transformer.wpe.weight"]
    for i in range(cfg["layers"]):
        p = f"transformer.h.{i}."
        yield sd[p + "ln_1.weight"]
        yield sd[p + "ln_1.bias"]
        w, b = sd[p + "attn.c_attn.weight"], sd[p + "attn.c_attn.bias"]          # Conv1D: y = x W + b, W [D, 3D] = q | k | v columns
        for k in range(3):
            yield w[:, k * D:(k + 1) * D].T
            yield b[k * D:(k + 1) * D]
        yield sd[p + "attn.c_proj.weight"].T
        yield sd[p + "attn.c_proj.bias"]
        yield sd[p + "ln_2.weight"]
        yield sd[p + "ln_2.bias"]
        yield sd[p + "mlp.c_fc.weight"].T
        yield sd[p + "mlp.c_fc.bias"]
        yield sd[p + "mlp.c_proj.weight"].T
        yield sd[p + "mlp.c_proj.bias"]
    yield sd["transformer.ln_f.weight"]
    yield sd["transformer.ln_f.bias"]


def pack(cfg: dict, sd) -> np.ndarray:
    """The C ABI's blob (include/pgmi.h, causal decoder) from a RITA or GPT-2 state dict of numpy arrays or torch tensors, written
    into one preallocated fp32 array.  RITA's inv_freq buffers are checked against the formula and dropped; GPT-2's attn.bias /
    attn.masked_bias buffers and a tied lm_head.weight are ignored."""
    sd = {k: (v.detach().float().numpy() if hasattr(v, "detach") else np.asarray(v, dtype=np.float32)) for k, v in sd.items()}
    blob = np.empty(weight_count(cfg), dtype=np.float32)
    o = 0
    try:
        for a in (_rita_tensors if cfg["family"] == "rita" else _gpt2_tensors)(cfg, sd):
            blob[o:o + a.size] = np.asarray(a, dtype=np.float32).ravel()
            o += a.size
    except KeyError as e:
        raise RuntimeError(f"Missing key in {cfg['family']} state_dict: {e.args[0]}") from None
    assert o == blob.size
    return blob


def load_checkpoint(checkpoint_dir: str):
    """config.json + pytorch_model.bin / model.safetensors.  Returns (cfg dict, blob)."""
    c, sd = load_hf_directory(checkpoint_dir)
    cfg = config_from_json(c)
    return cfg, pack(cfg, sd)


# -- model -----------------------------------------------------------------------------------------------------------------
class DecoderHandle(_lib.ModelHandle):
    """A device-resident causal decoder (f16x3) and its token_logprobs.  Subclasses (CausalLM, progen2.ProGen2Model) name their arch
    and C entries."""
    ARCH: int
    CREATE = TOKEN_LOGPROBS = ""            # pgmi_*_model_create(cfg, arch_arg, ...), pgmi_*_token_logprobs

    def __init__(self, cfg: dict, weights: np.ndarray, arch_arg: int, device: int = 0, max_rows: int = 0):
        super().__init__(cfg, weights, device, max_rows, arch_arg, arch=self.ARCH, vocab=cfg["vocab"],
                         max_positions=cfg["max_positions"], ln_eps=cfg.get("ln_eps", 1e-5))

    def token_logprobs(self, input_ids) -> np.ndarray:
        """log_softmax(model(input_ids).logits) over all V columns: [B,T] -> [B,T,V]."""
        t = _lib.as_i32(np.atleast_2d(np.asarray(input_ids)))
        B, T = t.shape
        out = np.empty((B, T, self.cfg["vocab"]), dtype=np.float32)
        _lib.check(getattr(_lib.load(), self.TOKEN_LOGPROBS)(self._h, _lib.ptr(t, _lib._i32p), B, T, _lib.ptr(out, _lib._f32p)))
        return out


class CausalLM(DecoderHandle):
    """Device-resident RITA or ProtGPT2 (f16x3)."""
    ARCH, CREATE, TOKEN_LOGPROBS = _lib.ARCH_GPT, "pgmi_gpt_model_create", "pgmi_gpt_token_logprobs"

    def __init__(self, cfg: dict, weights: np.ndarray, device: int = 0, max_rows: int = 0):
        self.family = cfg["family"]
        super().__init__(cfg, weights, POS_KIND[self.family], device, max_rows)

    @staticmethod
    def _weight_count(lib, c, pos_kind):
        return lib.pgmi_gpt_weight_count(C.byref(c), pos_kind)

    def sequence_loglik(self, rows: Sequence[np.ndarray]):
        """Whole (chunk, direction) id rows of any lengths -> (sum of log p(ids[t+1] | ids[<=t]) as float64, target count), in one
        call: right-padded to the longest row."""
        lens = np.array([len(r) for r in rows], dtype=np.int32)
        T = int(lens.max())
        t = np.zeros((len(rows), T), dtype=np.int32)
        for j, r in enumerate(rows):
            t[j, :len(r)] = r
        out = np.empty(len(rows), dtype=np.float64)
        n = np.empty(len(rows), dtype=np.int32)
        _lib.check(_lib.load().pgmi_gpt_sequence_loglik(self._h, _lib.ptr(t, _lib._i32p), _lib.ptr(lens, _lib._i32p), len(rows), T,
                                                         _lib.ptr(out, _lib._f64p), _lib.ptr(n, _lib._i32p)))
        return out, n

    def calc_fitness(self, prots: Sequence[str], encode: Callable[[str], np.ndarray],
                     model_context_len: int = MODEL_CONTEXT_LEN) -> np.ndarray:
        """compute_fitness.py:13-44 (RITA) / :13-46 (ProtGPT2) with the rows of all sequences batched."""
        plan = scoring_plan(prots, encode, model_context_len)
        sums = np.zeros(len(plan), dtype=np.float64)
        n = np.zeros(len(plan), dtype=np.int32)
        for idx in batches([ids.size for _, ids in plan]):
            s, k = self.sequence_loglik([plan[j][1] for j in idx])
            sums[idx] = s
            n[idx] = k
        return combine(len(prots), plan, sums, n, self.family)


def from_pretrained(checkpoint_dir: str, device: int = 0, max_rows: int = 0) -> CausalLM:
    cfg, blob = load_checkpoint(checkpoint_dir)
    model = CausalLM(cfg, blob, device=device, max_rows=max_rows)
    del blob
    return model


# -- assay CLIs (score_rita_proteingym.py, score_protgpt2_proteingym.py; the assay I/O of score_progen2_proteingym.py) -----
def get_mutated_sequence(focus_seq, mutant, start_idx=1, AA_vocab="ACDEFGHIKLMNPQRSTVWY"):
    """compute_fitness.py:46-61: the substituted sequence (substitutions only)."""
    mutated = list(focus_seq)
    for mutation in mutant.split(":"):
        from_AA, position, to_AA = mutation[0], int(mutation[1:-1]), mutation[-1]
        rel = position - start_idx
        assert from_AA == focus_seq[rel], f"Invalid from_AA or mutant position: {mutation}"
        assert to_AA in AA_vocab, f"Mutant to_AA is invalid: {mutation}"
        mutated[rel] = to_AA
    return "".join(mutated)


def add_common_flags(p, model_flag: str, model_help: str):
    p.add_argument(model_flag, type=str, required=True, help=model_help)
    p.add_argument("--DMS_reference_file_path", type=str, help="reference CSV listing the assays (DMS_id, DMS_filename, target_seq)")
    p.add_argument("--DMS_data_folder", type=str, help="folder holding the assay CSVs")
    p.add_argument("--DMS_index", type=int, help="row of the reference CSV to score")
    p.add_argument("--output_scores_folder", type=str, default=None, help="where <DMS_id>.csv is written")
    p.add_argument("--indel_mode", action="store_true", help="score the mutated_sequence column as it is (insertions / deletions)")
    p.add_argument("--tokenizer_path", type=str, default=None,
                   help="tokenizer.json, or a directory with tokenizer.json or vocab.json + merges.txt (default: the model directory)")
    p.add_argument("--device", type=int, default=0, help="HIP device")
    p.add_argument("--max_rows", type=int, default=0, help="workspace rows per device call (0 = library default)")


def load_assay(args, name: str, model_path: str):
    """compute_fitness.py main()'s assay resolution (all three causal-LM scorers): row --DMS_index of the reference file ->
    (DMS_id, upper-case target_seq, the assay's rows), after the reference's "Computing scores for" line."""
    import pandas as pd
    mapping = pd.read_csv(args.DMS_reference_file_path)
    DMS_id = mapping["DMS_id"][args.DMS_index]
    print("Computing scores for: {} with {}: {}".format(DMS_id, name, model_path))
    row = mapping[mapping["DMS_id"] == DMS_id]
    DMS_file_name = row["DMS_filename"].values[0]
    target_seq = row["target_seq"].values[0].upper()
    return DMS_id, target_seq, pd.read_csv(os.path.join(args.DMS_data_folder, DMS_file_name), low_memory=False)


def write_scores(args, DMS_id: str, DMS_data, out_cols) -> str:
    """The columns out_cols of the scored assay to <output_scores_folder>/<DMS_id>.csv; returns the path."""
    os.makedirs(args.output_scores_folder, exist_ok=True)
    out = os.path.join(args.output_scores_folder, DMS_id + ".csv")
    DMS_data[out_cols].to_csv(out, index=False)
    return out


def score_assay(args, model_path: str, name: str, score_col: str, out_cols):
    """compute_fitness.py main() of both scorers: resolve assay --DMS_index, build mutated_sequence only when the column is missing
    and --indel_mode is off, score, write <output_scores_folder>/<DMS_id>.csv."""
    encode = load_tokenizer(args.tokenizer_path or model_path)
    model = from_pretrained(model_path, device=args.device, max_rows=args.max_rows)
    DMS_id, target_seq, DMS_data = load_assay(args, name, model_path)
    if not args.indel_mode and "mutated_sequence" not in DMS_data.columns:
        DMS_data["mutated_sequence"] = DMS_data["mutant"].apply(lambda x: get_mutated_sequence(target_seq, x))
    DMS_data[score_col] = model.calc_fitness(list(DMS_data["mutated_sequence"]), encode)
    out = write_scores(args, DMS_id, DMS_data, out_cols)
    model.close()
    return out
