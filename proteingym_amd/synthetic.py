"""Synthetic inputs of the reference's shapes (no network: no real checkpoints or DMS files).

* random-weight ESM-1v / ESM2 models of a given architecture, as the flat ABI blob
  (include/pgmi.h) or as a fair-esm ``.pt`` file (layouts: SURVEY.md Appendix A,
  /root/reference/proteingym/baselines/esm/esm/pretrained.py:85-99,162-181);
* DMS assays shaped like rows of reference_files/DMS_substitutions.csv
  (``data/dms_substitutions_shapes.csv`` holds seq_len and mutant counts of the 217 assays;
  SURVEY.md section 8d describes the generator: positions uniform over [1,L], target amino acid
  uniform over the 19 non-wild-type letters, multi-mutants of depth 2-5).
"""
from __future__ import annotations

import argparse
import os
from typing import Dict, List, Tuple

import numpy as np

from . import _lib
from .esm import expected_keys

AA = "ACDEFGHIKLMNPQRSTVWY"

ESM1V_650M = dict(arch=_lib.ARCH_ESM1B, layers=33, embed_dim=1280, heads=20, ffn_dim=5120,
                  max_positions=1024, token_dropout=1, emb_layer_norm_before=0)
ESM2_650M = dict(arch=_lib.ARCH_ESM2, layers=33, embed_dim=1280, heads=20, ffn_dim=5120,
                 max_positions=0, token_dropout=1, emb_layer_norm_before=0)
ESM2_3B = dict(arch=_lib.ARCH_ESM2, layers=36, embed_dim=2560, heads=40, ffn_dim=10240,
               max_positions=0, token_dropout=1, emb_layer_norm_before=0)
ESM2_35M = dict(arch=_lib.ARCH_ESM2, layers=12, embed_dim=480, heads=20, ffn_dim=1920,        # head_dim 24, embed_dim not a multiple of 64
                max_positions=0, token_dropout=1, emb_layer_norm_before=0)                       # (pretrained.py:355-360; /root/reference/config.json:18)
ESM2_15B = dict(arch=_lib.ARCH_ESM2, layers=48, embed_dim=5120, heads=40, ffn_dim=20480,      # head_dim 128 (pretrained.py:387-394)
                max_positions=0, token_dropout=1, emb_layer_norm_before=0)


def key_shapes(cfg) -> List[Tuple[str, Tuple[int, ...]]]:
    D, F, V = cfg["embed_dim"], cfg["ffn_dim"], 33
    out = []
    for k in expected_keys(cfg):
        leaf = k.split(".")[-2] + "." + k.split(".")[-1]
        if k == "embed_tokens.weight":
            s = (V, D)
        elif k == "embed_positions.weight":
            s = (cfg["max_positions"] + 2, D)
        elif k == "lm_head.bias":
            s = (V,)
        elif leaf == "fc1.weight":
            s = (F, D)
        elif leaf == "fc1.bias":
            s = (F,)
        elif leaf == "fc2.weight":
            s = (D, F)
        elif k.endswith("_proj.weight") or k == "lm_head.dense.weight":
            s = (D, D)
        else:
            s = (D,)
        out.append((k, s))
    return out


def random_weights(cfg, seed: int, embed_std: float = 0.25) -> np.ndarray:
    """Flat fp32 blob in ABI order.  Linear layers U(-1/sqrt(fan_in), 1/sqrt(fan_in)) (the
    nn.Linear default scale), LayerNorm gamma 1+0.1N / beta 0.05N, embeddings N(0, embed_std^2)."""
    rng = np.random.default_rng(seed)
    n = sum(int(np.prod(s)) for _, s in key_shapes(cfg))
    blob = np.empty(n, dtype=np.float32)
    o = 0
    for k, s in key_shapes(cfg):
        m = int(np.prod(s))
        v = blob[o:o + m]
        if "layer_norm" in k:
            v[:] = rng.standard_normal(m, dtype=np.float32)
            if k.endswith("weight"):
                v *= 0.1
                v += 1.0
            else:
                v *= 0.05
        elif k.startswith("embed_"):
            v[:] = rng.standard_normal(m, dtype=np.float32)
            v *= embed_std
        else:
            fan_in = s[-1] if len(s) == 2 else {"fc1.bias": cfg["embed_dim"], "fc2.bias": cfg["ffn_dim"]}.get(
                k.split(".")[-2] + ".bias", cfg["embed_dim"])
            b = 1.0 / np.sqrt(fan_in)
            v[:] = rng.random(m, dtype=np.float32)
            v *= 2 * b
            v -= b
        o += m
    return blob


def outlier_weights(cfg, seed: int, n_outlier: int = 6, magnitude: float = 3000.0, max_ln_gain: float = 30.0,
                    tail_df: float = 3.0, embed_std: float = 0.15, inject_layer: int = 2) -> np.ndarray:
    """A checkpoint with the features real ESM / LLM checkpoints are known for and ``random_weights`` lacks (flat ABI blob):
    * heavy-tailed Linear weights: Student-t(tail_df) scaled to nn.Linear's default variance (max / median of a matrix ~ 10^2-10^3,
      so the per-tensor power-of-two pre-scale of the f16x3 weight planes leaves most entries far below the largest);
    * ``n_outlier`` "massive" residual channels: the learned positions (ESM-1b/1v) carry +-magnitude there from the first layer on,
      and layer ``inject_layer``'s FC2 bias adds +-magnitude as the feed-forward of real models does -- every LayerNorm after that
      sees a row whose variance is a few channels, every residual add works at fp32's resolution AT that magnitude;
    * LayerNorm gains up to ``max_ln_gain`` on a handful of channels of every LayerNorm (the outlier channels among them).
    The tied embedding / LM-head rows stay N(0, embed_std^2): the log-likelihood ratios keep the size real checkpoints produce."""
    rng = np.random.default_rng(seed)
    blob = random_weights(cfg, seed=seed, embed_std=embed_std)
    arrs = blob_to_arrays(cfg, blob)                       # views into blob
    D = cfg["embed_dim"]
    chans = rng.choice(D, size=n_outlier, replace=False)
    signs = rng.choice([-1.0, 1.0], size=n_outlier)
    for k, v in arrs.items():
        if k == "lm_head.weight" or k.startswith("embed_tokens"):
            continue
        if v.ndim == 2 and not k.startswith("embed_"):
            b = 1.0 / np.sqrt(v.shape[1])                  # U(-b, b) has variance b^2 / 3; t(df) has df / (df - 2)
            v[:] = (rng.standard_t(tail_df, size=v.shape) * (b / np.sqrt(3.0) / np.sqrt(tail_df / (tail_df - 2.0)))).astype(np.float32)
        elif "layer_norm" in k and k.endswith("weight"):
            hot = np.concatenate([chans[:3], rng.choice(D, size=5, replace=False)])
            v[hot] = rng.uniform(0.3 * max_ln_gain, max_ln_gain, size=hot.size).astype(np.float32)
    if "embed_positions.weight" in arrs:
        pe = arrs["embed_positions.weight"]
        pe[:, chans] = (signs * magnitude * (1.0 + 0.1 * rng.standard_normal((pe.shape[0], n_outlier)))).astype(np.float32)
    arrs[f"layers.{inject_layer}.fc2.bias"][chans] += (signs * magnitude).astype(np.float32)
    return blob


def blob_to_arrays(cfg, blob: np.ndarray) -> Dict[str, np.ndarray]:
    out, o = {}, 0
    for k, s in key_shapes(cfg):
        m = int(np.prod(s))
        out[k] = blob[o:o + m].reshape(s)
        o += m
    assert o == blob.size
    out["lm_head.weight"] = out["embed_tokens.weight"]     # tied (esm1.py:101-105)
    return out


def save_fair_esm_checkpoint(path: str, cfg, blob: np.ndarray):
    """Write the blob as a fair-esm v1 (ESM-1b/1v) or v2 (ESM2; file stem must start with
    'esm2') checkpoint that both the reference loader and this package read."""
    import torch
    arrs = blob_to_arrays(cfg, blob)
    model = {}
    for k, v in arrs.items():
        pref = "encoder." if k.startswith("lm_head") else "encoder.sentence_encoder."
        model[pref + k] = torch.from_numpy(np.ascontiguousarray(v)).clone()
    # like real fair-esm files, the tied tensors share storage
    model["encoder.lm_head.weight"] = model["encoder.sentence_encoder.embed_tokens.weight"]
    stem = os.path.basename(path).split(".")[0]
    if cfg["arch"] == _lib.ARCH_ESM2:
        assert stem.startswith("esm2"), "ESM2 checkpoints are dispatched by file stem (pretrained.py:187)"
        dh = cfg["embed_dim"] // cfg["heads"]                                          # rotary_embedding.py:39-41: one frequency per pair of head dims
        inv = (1.0 / (10000 ** (np.arange(0, dh, 2, dtype=np.float32) / dh))).astype(np.float32)
        for i in range(cfg["layers"]):
            model[f"encoder.sentence_encoder.layers.{i}.self_attn.rot_emb.inv_freq"] = torch.from_numpy(inv.copy())
        c = argparse.Namespace(encoder_layers=cfg["layers"], encoder_embed_dim=cfg["embed_dim"],
                               encoder_attention_heads=cfg["heads"], token_dropout=bool(cfg["token_dropout"]))
        torch.save({"cfg": {"model": c}, "model": model}, path)
    else:
        assert not stem.startswith("esm2")
        a = argparse.Namespace(arch="roberta_large", encoder_layers=cfg["layers"],
                               encoder_embed_dim=cfg["embed_dim"], encoder_ffn_embed_dim=cfg["ffn_dim"],
                               encoder_attention_heads=cfg["heads"], max_positions=cfg["max_positions"],
                               token_dropout=bool(cfg["token_dropout"]))
        torch.save({"args": a, "model": model}, path)
    return path


def random_sequence(rng, L: int) -> str:
    return "".join(rng.choice(list(AA), size=L))


def random_assay(seed: int, L: int, n_single: int, n_multi: int, offset: int = 1):
    """(sequence, mutants list, DMS_score) shaped like one DMS_substitutions row."""
    rng = np.random.default_rng(seed)
    seq = random_sequence(rng, L)
    aa = np.array(list(AA))
    seq_arr = np.array(list(seq))

    def one(p):
        choices = aa[aa != seq_arr[p]]
        return f"{seq_arr[p]}{p + offset}{choices[rng.integers(0, 19)]}"

    muts = [one(int(p)) for p in rng.integers(0, L, size=n_single)]
    for _ in range(n_multi):
        k = int(rng.integers(2, 6))
        ps = np.sort(rng.choice(L, size=min(k, L), replace=False))
        muts.append(":".join(one(int(p)) for p in ps))
    score = rng.standard_normal(len(muts))
    return seq, muts, score


def dms_shapes():
    import csv
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "dms_substitutions_shapes.csv")
    with open(path) as f:
        return [dict(DMS_index=i, DMS_id=r["DMS_id"], seq_len=int(r["seq_len"]),
                     n_total=int(r["DMS_total_number_mutants"]), n_single=int(r["DMS_number_single_mutants"]),
                     n_multi=int(r["DMS_number_multiple_mutants"])) for i, r in enumerate(csv.DictReader(f))]


def indel_shapes():
    """seq_len and mutant count of the 66 indel assays (reference_files/DMS_indels.csv; 287 207 mutants)."""
    import csv
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "dms_indels_shapes.csv")
    with open(path) as f:
        return [dict(DMS_index=i, DMS_id=r["DMS_id"], seq_len=int(r["seq_len"]), n_total=int(r["DMS_total_number_mutants"]))
                for i, r in enumerate(csv.DictReader(f))]


def random_indel_library(seed: int, L: int, n: int, max_edit: int = 3):
    """(wild type, n mutated sequences): each member deletes or inserts 1..max_edit residues at a random site, like the
    single-event indel libraries of DMS_indels.csv; lengths spread over L-max_edit .. L+max_edit."""
    rng = np.random.default_rng(seed)
    wt = random_sequence(rng, L)
    out = []
    for _ in range(n):
        k = int(rng.integers(1, max_edit + 1))
        if rng.random() < 0.5 and L - k > 4:
            p = int(rng.integers(0, L - k + 1))
            out.append(wt[:p] + wt[p + k:])
        else:
            p = int(rng.integers(0, L + 1))
            out.append(wt[:p] + random_sequence(rng, k) + wt[p:])
    return wt, out


# ---- Tranception ------------------------------------------------------------------------------------
TRANCEPTION_L = dict(arch=_lib.ARCH_TRANCEPTION, layers=36, embed_dim=1280, heads=20, ffn_dim=5120, vocab=25,
                     max_positions=1024, ln_eps=1e-5)     # paper "Large"; real dims come from the checkpoint's config.json


def tranception_key_shapes(cfg):
    from .tranception import expected_keys
    D, F, V = cfg["embed_dim"], cfg["ffn_dim"], cfg["vocab"]
    out = []
    for k in expected_keys(cfg["layers"]):
        if k in ("transformer.wte.weight", "lm_head.weight"):
            s = (V, D)
        elif k.endswith("c_attn.weight"):
            s = (D, 3 * D)
        elif k.endswith("c_attn.bias"):
            s = (3 * D,)
        elif "depthwiseconv" in k:
            ksz = (3, 5, 7)[int(k.split("depthwiseconv.")[1][0])]
            s = (64, ksz) if k.endswith("weight") else (64,)
        elif k.endswith("attn.c_proj.weight"):
            s = (D, D)
        elif k.endswith("mlp.c_fc.weight"):
            s = (D, F)
        elif k.endswith("mlp.c_fc.bias"):
            s = (F,)
        elif k.endswith("mlp.c_proj.weight"):
            s = (F, D)
        else:
            s = (D,)
        out.append((k, s))
    return out


def random_tranception_weights(cfg, seed: int, embed_std: float = 0.3) -> np.ndarray:
    """Flat fp32 blob in the Tranception ABI order; Conv1D weights N(0, 1/fan_in), tied lm_head."""
    rng = np.random.default_rng(seed)
    parts = []
    wte = None
    for k, s in tranception_key_shapes(cfg):
        m = int(np.prod(s))
        if k == "lm_head.weight":
            v = wte.copy()
        elif k.endswith("wte.weight"):
            v = rng.standard_normal(m, dtype=np.float32) * embed_std
            wte = v
        elif "ln_" in k:
            v = rng.standard_normal(m, dtype=np.float32) * (0.1 if k.endswith("weight") else 0.05)
            if k.endswith("weight"):
                v += 1.0
        elif "depthwiseconv" in k:
            v = rng.standard_normal(m, dtype=np.float32) * (0.4 if k.endswith("weight") else 0.05)
        elif k.endswith(".bias"):
            v = rng.standard_normal(m, dtype=np.float32) * 0.02
        else:
            v = rng.standard_normal(m, dtype=np.float32) / np.float32(np.sqrt(s[0]))
        parts.append(v.astype(np.float32))
    return np.concatenate(parts)


def tranception_blob_to_arrays(cfg, blob):
    out, o = {}, 0
    for k, s in tranception_key_shapes(cfg):
        m = int(np.prod(s))
        a = blob[o:o + m].reshape(s)
        if k.endswith("conv.weight"):
            a = a.reshape(s[0], 1, s[1])
        out[k] = a
        o += m
    assert o == blob.size
    return out


# ---- MSA Transformer (esm_msa1b_t12_100M_UR50S shape: 12 x 768, 12 heads, F = 3072) ------------------
MSA_1B = dict(arch=4, layers=12, embed_dim=768, heads=12, ffn_dim=3072, max_positions=1024, embed_positions_msa=True)


def random_msa_transformer_arrays(cfg, seed: int, embed_std: float = 0.25) -> Dict[str, np.ndarray]:
    """State-dict-keyed random arrays (names after the loader's row/column swap) for
    ``msa_transformer.pack_state_dict`` and the oracle's ``from_arrays``."""
    from . import msa_transformer as pmsa
    rng = np.random.default_rng(seed)
    D, F = cfg["embed_dim"], cfg["ffn_dim"]
    out = {}
    for k in pmsa.expected_keys(cfg):
        if k == "embed_tokens.weight":
            out[k] = (rng.standard_normal((33, D)) * embed_std).astype(np.float32)
        elif k == "embed_positions.weight":
            out[k] = (rng.standard_normal((cfg["max_positions"] + 2, D)) * embed_std).astype(np.float32)
        elif k == "msa_position_embedding":
            out[k] = (rng.standard_normal((1, 1024, 1, D)) * 0.1).astype(np.float32)
        elif "layer_norm" in k:
            out[k] = (1.0 + 0.1 * rng.standard_normal(D)).astype(np.float32) if k.endswith("weight") \
                else (0.05 * rng.standard_normal(D)).astype(np.float32)
        elif k == "lm_head.bias":
            out[k] = (0.1 * rng.standard_normal(33)).astype(np.float32)
        else:
            if "fc1" in k:
                shape, fan = ((F, D) if k.endswith("weight") else (F,)), D
            elif "fc2" in k:
                shape, fan = ((D, F) if k.endswith("weight") else (D,)), F
            else:
                shape, fan = ((D, D) if k.endswith("weight") else (D,)), D
            b = 1.0 / np.sqrt(fan)
            out[k] = ((rng.random(shape) * 2 - 1) * b).astype(np.float32)
    out["lm_head.weight"] = out["embed_tokens.weight"]
    return out


# ProGen2 (proteingym_amd/progen2.py).  Widths of the released checkpoints (ProGen2 paper, Table 1); rotary_dim here is a test value --
# the product reads every dimension from the checkpoint's config.json.
PROGEN2_WIDTHS = {
    "small": dict(embed_dim=1024, heads=16, rotary_dim=32),
    "medium": dict(embed_dim=1536, heads=16, rotary_dim=48),
    "large": dict(embed_dim=2560, heads=32, rotary_dim=32),
    "xlarge": dict(embed_dim=4096, heads=16, rotary_dim=64),
}


def progen2_config(layers: int, embed_dim: int, heads: int, rotary_dim: int, n_positions: int = 1024, ffn_dim: int = 0) -> dict:
    return dict(layers=layers, embed_dim=embed_dim, heads=heads, ffn_dim=ffn_dim or 4 * embed_dim, vocab=32,
                max_positions=n_positions, rotary_dim=rotary_dim, ln_eps=1e-5)


def progen2_state_dict(cfg: dict, seed: int) -> Dict[str, np.ndarray]:
    """Seeded random ProGen2 weights under the HF state-dict keys of modeling_progen.py (qkv_proj.weight in its stored mp_num = 8
    q | v | k block order).  Linear weights ~ N(0, 1/fan_in), LayerNorm gains 1 + N(0, 0.1^2), biases N(0, 0.02^2), wte N(0, 1),
    the LM head 3x wider so that the log-probabilities are far from uniform."""
    rng = np.random.default_rng(seed)
    D, F, V = cfg["embed_dim"], cfg["ffn_dim"], cfg["vocab"]

    def normal(shape, std):
        return (rng.standard_normal(shape, dtype=np.float32) * np.float32(std)).astype(np.float32)
    sd = {"transformer.wte.weight": normal((V, D), 1.0)}
    for i in range(cfg["layers"]):
        p = f"transformer.h.{i}."
        sd[p + "ln_1.weight"] = 1.0 + normal((D,), 0.1)
        sd[p + "ln_1.bias"] = normal((D,), 0.02)
        sd[p + "attn.qkv_proj.weight"] = normal((3 * D, D), D ** -0.5)
        sd[p + "attn.out_proj.weight"] = normal((D, D), D ** -0.5)
        sd[p + "mlp.fc_in.weight"] = normal((F, D), D ** -0.5)
        sd[p + "mlp.fc_in.bias"] = normal((F,), 0.02)
        sd[p + "mlp.fc_out.weight"] = normal((D, F), F ** -0.5)
        sd[p + "mlp.fc_out.bias"] = normal((D,), 0.02)
    sd["transformer.ln_f.weight"] = 1.0 + normal((D,), 0.1)
    sd["transformer.ln_f.bias"] = normal((D,), 0.02)
    sd["lm_head.weight"] = normal((V, D), 3.0 * D ** -0.5)
    sd["lm_head.bias"] = normal((V,), 0.1)
    return sd


def save_progen2_checkpoint(path: str, cfg: dict, sd: Dict[str, np.ndarray]):
    """config.json + pytorch_model.bin in the layout of the released ProGen2 checkpoints."""
    import json
    import torch
    os.makedirs(path, exist_ok=True)
    c = dict(model_type="progen", vocab_size=cfg["vocab"], n_positions=cfg["max_positions"], n_ctx=cfg["max_positions"],
             n_embd=cfg["embed_dim"], n_layer=cfg["layers"], n_head=cfg["heads"], rotary_dim=cfg["rotary_dim"],
             n_inner=cfg["ffn_dim"] if cfg["ffn_dim"] != 4 * cfg["embed_dim"] else None, activation_function="gelu_new",
             layer_norm_epsilon=cfg["ln_eps"], resid_pdrop=0.0, embd_pdrop=0.0, attn_pdrop=0.0, bos_token_id=1, eos_token_id=2)
    json.dump(c, open(os.path.join(path, "config.json"), "w"), indent=1)
    torch.save({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}, os.path.join(path, "pytorch_model.bin"))


# Causal decoders (proteingym_amd/causal_lm.py): RITA (rita_modeling.py) and ProtGPT2 (GPT-2).  Shapes of the released checkpoints;
# the product reads every dimension from the checkpoint's config.json.
RITA_WIDTHS = {
    "s": dict(embed_dim=768, heads=12, layers=12),
    "m": dict(embed_dim=1024, heads=16, layers=24),
    "l": dict(embed_dim=1536, heads=24, layers=24),
    "xl": dict(embed_dim=2048, heads=16, layers=24),
}
PROTGPT2_SHAPE = dict(embed_dim=1280, heads=20, layers=36, vocab=50257, max_positions=1024)


def rita_config(layers: int, embed_dim: int, heads: int, vocab: int = 26, max_positions: int = 1024) -> dict:
    return dict(family="rita", layers=layers, embed_dim=embed_dim, heads=heads, ffn_dim=4 * embed_dim, vocab=vocab,
                max_positions=max_positions, ln_eps=1e-5)


def gpt2_config(layers: int, embed_dim: int, heads: int, vocab: int, max_positions: int = 1024) -> dict:
    return dict(family="gpt2", layers=layers, embed_dim=embed_dim, heads=heads, ffn_dim=4 * embed_dim, vocab=vocab,
                max_positions=max_positions, ln_eps=1e-5)


def _causal_normal(seed):
    rng = np.random.default_rng(seed)

    def normal(shape, std):
        return (rng.standard_normal(shape, dtype=np.float32) * np.float32(std)).astype(np.float32)
    return normal


def rita_state_dict(cfg: dict, seed: int) -> Dict[str, np.ndarray]:
    """Seeded random RITA weights under the state-dict keys of rita_modeling.py (RITAModelForCausalLM), the rotary inv_freq buffers
    included.  Linear weights ~ N(0, 1/fan_in), LayerNorm gains 1 + N(0, 0.1^2), biases N(0, 0.02^2), embedding N(0, 1), the LM head 3x
    wider so that the log-probabilities are far from uniform."""
    normal = _causal_normal(seed)
    D, F, V, H = cfg["embed_dim"], cfg["ffn_dim"], cfg["vocab"], cfg["heads"]
    dh = D // H
    inv_freq = (1.0 / (10000 ** (np.arange(0, dh, 2, dtype=np.float32) / np.float32(dh)))).astype(np.float32)
    sd = {"transformer.embedding.weight": normal((V, D), 1.0)}
    for i in range(cfg["layers"]):
        p = f"transformer.layers.{i}."
        for name in ("key", "query", "value", "proj"):
            sd[p + f"self_attention.{name}.weight"] = normal((D, D), D ** -0.5)
            sd[p + f"self_attention.{name}.bias"] = normal((D,), 0.02)
        sd[p + "self_attention.rotary_embedding.inv_freq"] = inv_freq.copy()
        sd[p + "attn_norm.weight"] = 1.0 + normal((D,), 0.1)
        sd[p + "attn_norm.bias"] = normal((D,), 0.02)
        sd[p + "mlp.0.weight"] = normal((F, D), D ** -0.5)
        sd[p + "mlp.0.bias"] = normal((F,), 0.02)
        sd[p + "mlp.2.weight"] = normal((D, F), F ** -0.5)
        sd[p + "mlp.2.bias"] = normal((D,), 0.02)
        sd[p + "mlp_norm.weight"] = 1.0 + normal((D,), 0.1)
        sd[p + "mlp_norm.bias"] = normal((D,), 0.02)
    sd["transformer.final_norm.weight"] = 1.0 + normal((D,), 0.1)
    sd["transformer.final_norm.bias"] = normal((D,), 0.02)
    sd["lm_head.weight"] = normal((V, D), 3.0 * D ** -0.5)
    return sd


def gpt2_state_dict(cfg: dict, seed: int) -> Dict[str, np.ndarray]:
    """Seeded random GPT-2 weights under transformers' GPT2LMHeadModel keys (Conv1D weights [in, out], lm_head tied to wte and not
    stored).  wte ~ N(0, 3/D) doubles as the head, so logits have std ~3 as in the other families."""
    normal = _causal_normal(seed)
    D, F, V, P = cfg["embed_dim"], cfg["ffn_dim"], cfg["vocab"], cfg["max_positions"]
    sd = {"transformer.wte.weight": normal((V, D), 3.0 * D ** -0.5), "transformer.wpe.weight": normal((P, D), 0.3)}
    for i in range(cfg["layers"]):
        p = f"transformer.h.{i}."
        sd[p + "ln_1.weight"] = 1.0 + normal((D,), 0.1)
        sd[p + "ln_1.bias"] = normal((D,), 0.02)
        sd[p + "attn.c_attn.weight"] = normal((D, 3 * D), D ** -0.5)
        sd[p + "attn.c_attn.bias"] = normal((3 * D,), 0.02)
        sd[p + "attn.c_proj.weight"] = normal((D, D), D ** -0.5)
        sd[p + "attn.c_proj.bias"] = normal((D,), 0.02)
        sd[p + "ln_2.weight"] = 1.0 + normal((D,), 0.1)
        sd[p + "ln_2.bias"] = normal((D,), 0.02)
        sd[p + "mlp.c_fc.weight"] = normal((D, F), D ** -0.5)
        sd[p + "mlp.c_fc.bias"] = normal((F,), 0.02)
        sd[p + "mlp.c_proj.weight"] = normal((F, D), F ** -0.5)
        sd[p + "mlp.c_proj.bias"] = normal((D,), 0.02)
    sd["transformer.ln_f.weight"] = 1.0 + normal((D,), 0.1)
    sd["transformer.ln_f.bias"] = normal((D,), 0.02)
    return sd


def save_causal_lm_checkpoint(path: str, cfg: dict, sd: Dict[str, np.ndarray]):
    """config.json + pytorch_model.bin in the layout of the released RITA / ProtGPT2 checkpoints."""
    import json
    import torch
    os.makedirs(path, exist_ok=True)
    if cfg["family"] == "rita":
        c = dict(model_type="rita", vocab_size=cfg["vocab"], d_model=cfg["embed_dim"], num_layers=cfg["layers"],
                 num_heads=cfg["heads"], max_seq_len=cfg["max_positions"], ff_ratio=cfg["ffn_dim"] // cfg["embed_dim"],
                 d_feedforward=cfg["ffn_dim"], dropout=0.0, eos_token_id=2)
    else:
        c = dict(model_type="gpt2", architectures=["GPT2LMHeadModel"], vocab_size=cfg["vocab"], n_positions=cfg["max_positions"],
                 n_ctx=cfg["max_positions"], n_embd=cfg["embed_dim"], n_layer=cfg["layers"], n_head=cfg["heads"], n_inner=None,
                 activation_function="gelu_new", layer_norm_epsilon=cfg["ln_eps"], resid_pdrop=0.0, embd_pdrop=0.0, attn_pdrop=0.0,
                 scale_attn_weights=True, scale_attn_by_inverse_layer_idx=False, reorder_and_upcast_attn=False,
                 bos_token_id=0, eos_token_id=0)
    json.dump(c, open(os.path.join(path, "config.json"), "w"), indent=1)
    torch.save({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}, os.path.join(path, "pytorch_model.bin"))


def esmc_config(embed_dim: int = 960, layers: int = 30) -> dict:
    """An ESM C configuration (esm/pretrained.py:65-98): head_dim 64, SwiGLU width swiglu_correction_fn(8/3, d), 64-column head."""
    return dict(layers=layers, embed_dim=embed_dim, heads=embed_dim // 64, ffn_dim=int(((8 / 3 * embed_dim) + 255) // 256 * 256), vocab=64)


def esmc_state_dict(cfg: dict, seed: int) -> Dict[str, np.ndarray]:
    """Seeded random ESM C weights under ESMC.state_dict()'s keys.  Linear weights ~ N(0, 1/fan_in), LayerNorm gains 1 + N(0, 0.1^2)
    (q_ln / k_ln and the bias-free final norm included), biases N(0, 0.02^2), embedding N(0, 1); the output layer 3x wider so that the
    log-probabilities are far from uniform, its untrained rows 33..63 non-zero like the rest."""
    normal = _causal_normal(seed)
    D, F, V = cfg["embed_dim"], cfg["ffn_dim"], cfg["vocab"]
    sd = {"embed.weight": normal((V, D), 1.0)}
    for i in range(cfg["layers"]):
        p = f"transformer.blocks.{i}."
        sd[p + "attn.layernorm_qkv.0.weight"] = 1.0 + normal((D,), 0.1)
        sd[p + "attn.layernorm_qkv.0.bias"] = normal((D,), 0.02)
        sd[p + "attn.layernorm_qkv.1.weight"] = normal((3 * D, D), D ** -0.5)
        sd[p + "attn.out_proj.weight"] = normal((D, D), D ** -0.5)
        sd[p + "attn.q_ln.weight"] = 1.0 + normal((D,), 0.1)
        sd[p + "attn.k_ln.weight"] = 1.0 + normal((D,), 0.1)
        sd[p + "ffn.0.weight"] = 1.0 + normal((D,), 0.1)
        sd[p + "ffn.0.bias"] = normal((D,), 0.02)
        sd[p + "ffn.1.weight"] = normal((2 * F, D), D ** -0.5)
        sd[p + "ffn.3.weight"] = normal((D, F), F ** -0.5)
    sd["transformer.norm.weight"] = 1.0 + normal((D,), 0.1)
    sd["sequence_head.0.weight"] = normal((D, D), D ** -0.5)
    sd["sequence_head.0.bias"] = normal((D,), 0.02)
    sd["sequence_head.2.weight"] = 1.0 + normal((D,), 0.1)
    sd["sequence_head.2.bias"] = normal((D,), 0.02)
    sd["sequence_head.3.weight"] = normal((V, D), 3.0 * D ** -0.5)
    sd["sequence_head.3.bias"] = normal((V,), 0.02)
    return sd


def saprot_config(embed_dim: int = 1280, heads: int = 20, layers: int = 33, ffn_dim: int = 0) -> dict:
    """A SaProt configuration (SaProt-650M by default; SaProt-35M: 480, 20, 12): ESM2's shape with the 446-token vocabulary, token
    dropout, rotary positions, no LayerNorm before the encoder, <mask> at id 4."""
    return dict(arch=_lib.ARCH_SAPROT, layers=layers, embed_dim=embed_dim, heads=heads, ffn_dim=ffn_dim or 4 * embed_dim, vocab=446,
                max_positions=0, token_dropout=1, emb_layer_norm_before=0, mask_token_id=4)


def saprot_state_dict(cfg: dict, seed: int, embed_std: float = 0.15) -> Dict[str, np.ndarray]:
    """Seeded random SaProt weights under Hugging Face EsmForMaskedLM's keys (the tied lm_head.decoder.weight is not stored).  Linear
    weights ~ N(0, 1/fan_in), LayerNorm gains 1 + N(0, 0.1^2), biases N(0, 0.02^2); the tied embedding N(0, embed_std^2) so that the
    log-ratios stay in the range real checkpoints produce."""
    normal = _causal_normal(seed)
    D, F, V = cfg["embed_dim"], cfg["ffn_dim"], cfg["vocab"]
    sd = {"esm.embeddings.word_embeddings.weight": normal((V, D), embed_std)}

    def ln(p):
        sd[p + ".weight"] = 1.0 + normal((D,), 0.1)
        sd[p + ".bias"] = normal((D,), 0.02)

    def linear(p, n_out, n_in):
        sd[p + ".weight"] = normal((n_out, n_in), n_in ** -0.5)
        sd[p + ".bias"] = normal((n_out,), 0.02)
    if cfg["emb_layer_norm_before"]:
        ln("esm.embeddings.layer_norm")
    for i in range(cfg["layers"]):
        p = f"esm.encoder.layer.{i}."
        ln(p + "attention.LayerNorm")
        for n in ("query", "key", "value"):
            linear(p + "attention.self." + n, D, D)
        linear(p + "attention.output.dense", D, D)
        ln(p + "LayerNorm")
        linear(p + "intermediate.dense", F, D)
        linear(p + "output.dense", D, F)
    ln("esm.encoder.emb_layer_norm_after")
    linear("lm_head.dense", D, D)
    ln("lm_head.layer_norm")
    sd["lm_head.bias"] = normal((V,), 0.02)
    return sd


def mulan_config(embed_dim: int = 320, heads: int = 20, layers: int = 6, ffn_dim: int = 0, use_foldseek: bool = False) -> dict:
    """A MULAN configuration (MULAN-small by default: ESM2 8M's shape): ESM2's alphabet (<mask> 32), or SaProt's 446 tokens (<mask> 4,
    21 amino-acid groups) with use_foldseek; token dropout, rotary positions, no LayerNorm before the encoder."""
    return dict(arch=_lib.ARCH_MULAN, layers=layers, embed_dim=embed_dim, heads=heads, ffn_dim=ffn_dim or 4 * embed_dim,
                vocab=446 if use_foldseek else 33, max_positions=0, token_dropout=1, emb_layer_norm_before=0,
                mask_token_id=4 if use_foldseek else 32, groups=21 if use_foldseek else 0)


def mulan_state_dict(cfg: dict, seed: int, embed_std: float = 0.15, adapter_scale: float = 1.0) -> Dict[str, np.ndarray]:
    """Seeded random MULAN weights under StructEsmForMaskedLM's keys: saprot_state_dict's main stack, then the structure adapter --
    MLP [D,7], one layer whose feed-forward width is 4 D whatever the main stack's, and its final LayerNorm, whose gain and bias are
    multiplied by adapter_scale (0: the adapter adds exactly nothing)."""
    sd = saprot_state_dict(cfg, seed, embed_std)
    normal = _causal_normal(seed + 7919)
    D = cfg["embed_dim"]
    p = "esm.embeddings.struct_embeddings."

    def ln(k, scale=1.0, spread=0.1):
        sd[k + ".weight"] = ((1.0 + normal((D,), spread)) * scale).astype(np.float32)
        sd[k + ".bias"] = (normal((D,), 0.02) * scale).astype(np.float32)

    def linear(k, n_out, n_in):
        sd[k + ".weight"] = normal((n_out, n_in), n_in ** -0.5)
        sd[k + ".bias"] = normal((n_out,), 0.02)
    linear(p + "MLP", D, 7)
    q = p + "encoder.layer.0."
    ln(q + "attention.LayerNorm")
    for n in ("query", "key", "value"):
        linear(q + "attention.self." + n, D, D)
    linear(q + "attention.output.dense", D, D)
    ln(q + "LayerNorm")
    linear(q + "intermediate.dense", 4 * D, D)
    linear(q + "output.dense", D, 4 * D)
    # the adapter's output is a LayerNorm row (unit variance times the gain) added to embeddings of std embed_std
    ln(p + "encoder.emb_layer_norm_after", embed_std * adapter_scale)
    return sd


def esm3_config(embed_dim: int = 1536, layers: int = 48, v_heads: int = 256) -> dict:
    """An ESM3 configuration (esm/pretrained.py:101-117 by default): ESM C's block shape plus the geometric attention's v_heads."""
    return dict(esmc_config(embed_dim, layers), v_heads=v_heads)


ESM3_HEADS = (("sequence_head", 64), ("structure_head", 4096), ("ss8_head", 11), ("sasa_head", 19), ("function_head", 260 * 8),
              ("residue_head", 1478))


def esm3_state_dict(cfg: dict, seed: int) -> Dict[str, np.ndarray]:
    """Seeded random ESM3 weights under every key of ESM3.state_dict() (the five output heads this project does not pack included, so
    that the reference loads it strictly).  Blocks as esmc_state_dict; the track embeddings N(0, 0.3^2 .. 1), the padding rows of the
    function and residue tables zero as nn.Embedding(padding_idx=0) leaves them; both per-head scales of the geometric attention
    N(0, 1), so non-zero: the rotation and the distance term both carry weight."""
    normal = _causal_normal(seed)
    D, F, Hv = cfg["embed_dim"], cfg["ffn_dim"], cfg["v_heads"]
    sd = {"encoder.sequence_embed.weight": normal((64, D), 1.0)}
    for n in ("plddt_projection", "structure_per_res_plddt_projection"):
        sd[f"encoder.{n}.weight"] = normal((D, 16), 0.25)
        sd[f"encoder.{n}.bias"] = normal((D,), 0.02)
    sd["encoder.structure_tokens_embed.weight"] = normal((4096 + 5, D), 0.5)
    sd["encoder.ss8_embed.weight"] = normal((11, D), 0.3)
    sd["encoder.sasa_embed.weight"] = normal((19, D), 0.3)
    for k in range(8):
        w = normal((260, D // 8), 0.3)
        w[0] = 0.0
        sd[f"encoder.function_embed.{k}.weight"] = w
    w = normal((1478, D), 0.3)
    w[0] = 0.0
    sd["encoder.residue_embed.weight"] = w
    for i in range(cfg["layers"]):
        p = f"transformer.blocks.{i}."
        sd[p + "attn.layernorm_qkv.0.weight"] = 1.0 + normal((D,), 0.1)
        sd[p + "attn.layernorm_qkv.0.bias"] = normal((D,), 0.02)
        sd[p + "attn.layernorm_qkv.1.weight"] = normal((3 * D, D), D ** -0.5)
        sd[p + "attn.out_proj.weight"] = normal((D, D), D ** -0.5)
        sd[p + "attn.q_ln.weight"] = 1.0 + normal((D,), 0.1)
        sd[p + "attn.k_ln.weight"] = 1.0 + normal((D,), 0.1)
        if i == 0:
            sd[p + "geom_attn.distance_scale_per_head"] = normal((Hv,), 1.0)
            sd[p + "geom_attn.rotation_scale_per_head"] = normal((Hv,), 1.0)
            sd[p + "geom_attn.s_norm.weight"] = 1.0 + normal((D,), 0.1)
            sd[p + "geom_attn.proj.weight"] = normal((15 * Hv, D), D ** -0.5)
            sd[p + "geom_attn.out_proj.weight"] = normal((D, 3 * Hv), (3 * Hv) ** -0.5)
        sd[p + "ffn.0.weight"] = 1.0 + normal((D,), 0.1)
        sd[p + "ffn.0.bias"] = normal((D,), 0.02)
        sd[p + "ffn.1.weight"] = normal((2 * F, D), D ** -0.5)
        sd[p + "ffn.3.weight"] = normal((D, F), F ** -0.5)
    sd["transformer.norm.weight"] = 1.0 + normal((D,), 0.1)
    for name, n_out in ESM3_HEADS:
        p = f"output_heads.{name}."
        sd[p + "0.weight"] = normal((D, D), D ** -0.5)
        sd[p + "0.bias"] = normal((D,), 0.02)
        sd[p + "2.weight"] = 1.0 + normal((D,), 0.1)
        sd[p + "2.bias"] = normal((D,), 0.02)
        sd[p + "3.weight"] = normal((n_out, D), 3.0 * D ** -0.5)
        sd[p + "3.bias"] = normal((n_out,), 0.02)
    return sd


def esm3_encoder_config(d_model: int = 1024, v_heads: int = 128, layers: int = 2, d_out: int = 128, n_codes: int = 4096) -> dict:
    """A StructureTokenEncoder configuration (esm/pretrained.py:30-34 by default; n_heads is unused: its blocks have no plain
    attention)."""
    return dict(d_model=d_model, v_heads=v_heads, layers=layers, d_out=d_out, n_codes=n_codes, ffn_dim=int(((4 * d_model) + 255) // 256 * 256))


def esm3_encoder_state_dict(cfg: dict, seed: int) -> Dict[str, np.ndarray]:
    """Seeded random StructureTokenEncoder weights under its state-dict keys (vqvae.py:182-194; the codebook's three buffers
    included).  Every Linear and LayerNorm has a bias (bias=True blocks); the relative-position table N(0, 1) rather than the 0.02 of
    its initialiser, so that neighbourhoods differ visibly; both per-head scales N(0, 1)."""
    normal = _causal_normal(seed)
    D, F, Hv, O, K = cfg["d_model"], cfg["ffn_dim"], cfg["v_heads"], cfg["d_out"], cfg["n_codes"]
    sd = {}
    for i in range(cfg["layers"]):
        p = f"transformer.blocks.{i}."
        sd[p + "geom_attn.distance_scale_per_head"] = normal((Hv,), 1.0)
        sd[p + "geom_attn.rotation_scale_per_head"] = normal((Hv,), 1.0)
        sd[p + "geom_attn.s_norm.weight"] = 1.0 + normal((D,), 0.1)
        sd[p + "geom_attn.s_norm.bias"] = normal((D,), 0.02)
        sd[p + "geom_attn.proj.weight"] = normal((15 * Hv, D), D ** -0.5)
        sd[p + "geom_attn.proj.bias"] = normal((15 * Hv,), 0.02)
        sd[p + "geom_attn.out_proj.weight"] = normal((D, 3 * Hv), (3 * Hv) ** -0.5)
        sd[p + "geom_attn.out_proj.bias"] = normal((D,), 0.02)
        sd[p + "ffn.0.weight"] = 1.0 + normal((D,), 0.1)
        sd[p + "ffn.0.bias"] = normal((D,), 0.02)
        sd[p + "ffn.1.weight"] = normal((2 * F, D), D ** -0.5)
        sd[p + "ffn.1.bias"] = normal((2 * F,), 0.02)
        sd[p + "ffn.3.weight"] = normal((D, F), F ** -0.5)
        sd[p + "ffn.3.bias"] = normal((D,), 0.02)
    sd["pre_vq_proj.weight"] = normal((O, D), D ** -0.5)
    sd["pre_vq_proj.bias"] = normal((O,), 0.02)
    sd["codebook.embeddings"] = normal((K, O), 1.0)
    sd["codebook.N"] = np.zeros((K,), np.float32)
    sd["codebook.z_avg"] = sd["codebook.embeddings"].copy()
    sd["relative_positional_embedding.embedding.weight"] = normal((2 * 32 + 2, D), 1.0)
    return sd
