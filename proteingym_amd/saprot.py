"""SaProt scoring on libpgmi (include/pgmi.h, arch PGMI_ARCH_SAPROT).

Replaces proteingym/baselines/saprot/compute_fitness.py's model side: a Hugging Face ``EsmForMaskedLM`` checkpoint directory
(config.json, vocab.txt, model.safetensors or pytorch_model.bin) is packed into ESM2's blob with the 446-token structure-aware
vocabulary, the forward runs in HIP (csrc/api_saprot.hip on the ESM2 encoder), and ``score_chunk`` reproduces ``calc_fitness`` /
``predict_mut`` (:17-75) for one structure chunk.  The reference runs one forward per mutant; its masked input depends only on the
SET of mutated positions, so every distinct position set is forwarded once and its rows are batched.  foldseek_util.py's Foldseek
call and pLDDT parser are restated here as well.  Nothing is downloaded.
"""
from __future__ import annotations

import json
import os
import re
import subprocess
import tempfile
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from . import esm as pesm

# the tokenizer's vocabulary (vocab.txt): 5 specials, then amino-acid letter x Foldseek 3Di letter, the amino-acid letter major
SPECIALS = ("<cls>", "<pad>", "<eos>", "<unk>", "<mask>")
CLS, PAD, EOS, UNK, MASK = range(5)
AA_LETTERS = "ACDEFGHIKLMNPQRSTVWY#"
STRUC_LETTERS = "pynwrqhgdlvtmfsaeikc#"                    # compute_fitness.py:14 (foldseek_struc_vocab)
FIRST, GROUPS, WIDTH = len(SPECIALS), len(AA_LETTERS), len(STRUC_LETTERS)
VOCAB = FIRST + GROUPS * WIDTH
assert VOCAB == 446
LN_EPS = 1e-5                                              # the kernels' constant
PLDDT_THRESHOLD = 70.0                                     # compute_fitness.py:60
# ESM alphabet id (what pgmi_parse_mutants returns for a letter) -> amino-acid group; -1: not one of the 20 (get_mutated_sequence)
_ESM_TO_GROUP = np.full(len(pesm.VOCABULARY), -1, dtype=np.int32)
for _g, _a in enumerate(AA_LETTERS[:20]):
    _ESM_TO_GROUP[pesm.VOCABULARY.index(_a)] = _g


def vocabulary() -> List[str]:
    return list(SPECIALS) + [a + s for a in AA_LETTERS for s in STRUC_LETTERS]


def check_vocabulary(tokens: Sequence[str]):
    """The kernels address a residue token as 5 + 21 * amino-acid index + structure index: anything else is refused."""
    want = vocabulary()
    tokens = list(tokens)
    if tokens != want:
        n = next((i for i, (a, b) in enumerate(zip(tokens, want)) if a != b), min(len(tokens), len(want)))
        raise ValueError(f"vocab.txt is not SaProt's layout (5 specials, then for each letter of {AA_LETTERS} the 21 tokens in "
                         f"{STRUC_LETTERS} order): {len(tokens)} tokens, first difference at id {n} "
                         f"({tokens[n] if n < len(tokens) else 'end'!r}, expected {want[n] if n < len(want) else 'end'!r})")


def read_vocab(path: str) -> List[str]:
    with open(path) as f:
        return [line.rstrip("\n") for line in f if line.rstrip("\n")]


def tokenize(sequence: str, structure: str) -> np.ndarray:
    """<cls> + one token per residue (amino-acid letter + 3Di letter, compute_fitness.py:62) + <eos>, as EsmTokenizer numbers them."""
    if len(sequence) != len(structure):
        raise ValueError(f"structure string has {len(structure)} letters, the sequence {len(sequence)}")
    ids = np.empty(len(sequence) + 2, dtype=np.int32)
    ids[0], ids[-1] = CLS, EOS
    for i, (a, s) in enumerate(zip(sequence, structure)):
        ai, si = AA_LETTERS.find(a), STRUC_LETTERS.find(s)
        if ai < 0 or si < 0:
            raise ValueError(f"residue {i + 1}: {a + s!r} is not a SaProt token (amino acid in {AA_LETTERS}, structure in {STRUC_LETTERS})")
        ids[i + 1] = FIRST + WIDTH * ai + si
    return ids


def masked_ids() -> np.ndarray:
    """id -> the '#' amino-acid group's token with the same structure letter ("#" + token[-1], compute_fitness.py:33); specials stay."""
    ids = np.arange(VOCAB, dtype=np.int32)
    ids[FIRST:] = FIRST + (GROUPS - 1) * WIDTH + (ids[FIRST:] - FIRST) % WIDTH
    return ids


# -- Foldseek and pLDDT (foldseek_util.py) -----------------------------------------------------------------------------------
def foldseek_command(foldseek: str, pdb_path: str, tsv_path: str) -> str:
    """foldseek_util.py:34."""
    return f"{foldseek} structureto3didescriptor -v 0 --threads 1 --chain-name-mode 1 {pdb_path} {tsv_path}"


def extract_plddt(pdb_path: str) -> np.ndarray:
    """foldseek_util.py:67-100: mean B-factor per residue number, in order of first appearance.  ATOM lines are split on runs of
    blanks; the residue number is field 5, or field 4 without its first character when chain and number have fused (>= 1000)."""
    by_pos: Dict[int, List[float]] = {}
    with open(pdb_path) as f:
        for line in f:
            splits = re.sub(" +", " ", line).strip().split(" ")
            if splits[0] == "ATOM":
                pos = int(splits[5]) if len(splits[4]) == 1 else int(splits[4][1:])
                by_pos.setdefault(pos, []).append(float(splits[-2]))
    return np.array([np.mean(v) for v in by_pos.values()])


def structure_sequence(foldseek: str, pdb_path: str, chain: str = "A") -> str:
    """get_struc_seq(foldseek, pdb, [chain], plddt_mask=True, plddt_threshold=70)[chain][1].lower() (compute_fitness.py:60): the 3Di
    string of the chain's first record, '#' where the residue's mean pLDDT is below 70.  Foldseek writes into a temporary directory
    (the reference writes get_struc_seq_0.tsv into the working directory)."""
    assert os.path.exists(foldseek), f"Foldseek not found: {foldseek}"
    assert os.path.exists(pdb_path), f"Pdb file not found: {pdb_path}"
    name = os.path.basename(pdb_path)
    found = None
    with tempfile.TemporaryDirectory(prefix="pgmi_saprot_") as tmp:
        tsv = os.path.join(tmp, "get_struc_seq.tsv")
        subprocess.run(foldseek_command(foldseek, pdb_path, tsv), shell=True)          # os.system in the reference: status not checked
        with open(tsv) as f:
            for line in f:
                desc, _seq, struc_seq = line.split("\t")[:3]
                plddts = extract_plddt(pdb_path)
                assert len(plddts) == len(struc_seq), f"Length mismatch: {len(plddts)} != {len(struc_seq)}"
                np_seq = np.array(list(struc_seq))
                np_seq[np.where(plddts < PLDDT_THRESHOLD)[0]] = "#"
                this_chain = desc.split(" ")[0].replace(name, "").split("_")[-1]
                if this_chain == chain and found is None:
                    found = "".join(np_seq)
    if found is None:
        raise KeyError(chain)
    return found.lower()


# -- checkpoint --------------------------------------------------------------------------------------------------------------
def hf_keys(cfg: dict) -> List[Tuple[str, str]]:
    """(ESM blob key, HF EsmForMaskedLM key) in blob order (include/pgmi.h pgmi_weight_count)."""
    out = [("embed_tokens.weight", "esm.embeddings.word_embeddings.weight")]
    if cfg["emb_layer_norm_before"]:
        out += [(f"emb_layer_norm_before.{x}", f"esm.embeddings.layer_norm.{x}") for x in ("weight", "bias")]
    for i in range(cfg["layers"]):
        e, h = f"layers.{i}.", f"esm.encoder.layer.{i}."
        pairs = [("self_attn_layer_norm", "attention.LayerNorm"), ("self_attn.q_proj", "attention.self.query"),
                 ("self_attn.k_proj", "attention.self.key"), ("self_attn.v_proj", "attention.self.value"),
                 ("self_attn.out_proj", "attention.output.dense"), ("final_layer_norm", "LayerNorm"),
                 ("fc1", "intermediate.dense"), ("fc2", "output.dense")]
        out += [(e + a + "." + x, h + b + "." + x) for a, b in pairs for x in ("weight", "bias")]
    out += [(f"emb_layer_norm_after.{x}", f"esm.encoder.emb_layer_norm_after.{x}") for x in ("weight", "bias")]
    out += [(f"lm_head.dense.{x}", f"lm_head.dense.{x}") for x in ("weight", "bias")]
    out += [(f"lm_head.layer_norm.{x}", f"lm_head.layer_norm.{x}") for x in ("weight", "bias")]
    return out + [("lm_head.bias", "lm_head.bias")]


def _ignored(key: str) -> bool:
    return (key.startswith("esm.contact_head.") or key.endswith("rotary_embeddings.inv_freq") or key.endswith("position_ids")
            or key == "esm.embeddings.position_embeddings.weight" or key == "lm_head.decoder.weight")


def config_from_hf(c: dict, sd=None) -> dict:
    """The model dimensions from config.json; refuses what the kernels do not compute."""
    if c.get("position_embedding_type", "absolute") != "rotary":
        raise ValueError(f"position_embedding_type {c.get('position_embedding_type')!r}: this path runs rotary positions only")
    if float(c.get("layer_norm_eps", 1e-12)) != LN_EPS:
        raise ValueError(f"layer_norm_eps {c.get('layer_norm_eps')}: the kernels' LayerNorm epsilon is {LN_EPS}")
    if int(c["vocab_size"]) != VOCAB:
        raise ValueError(f"vocab_size {c['vocab_size']}: SaProt's vocabulary has {VOCAB} tokens")
    if int(c.get("pad_token_id", PAD)) != PAD or int(c.get("mask_token_id", MASK)) != MASK:
        raise ValueError(f"pad_token_id {c.get('pad_token_id')} / mask_token_id {c.get('mask_token_id')}: expected {PAD} / {MASK}")
    if c.get("hidden_act", "gelu") != "gelu":
        raise ValueError(f"hidden_act {c.get('hidden_act')!r}: this path runs erf-GELU only")
    if c.get("tie_word_embeddings", True) is False:
        raise ValueError("tie_word_embeddings false: the LM head of this path is the embedding table")
    lnb = bool(c.get("emb_layer_norm_before", False))
    if lnb and sd is not None and "esm.embeddings.layer_norm.weight" not in sd:
        raise ValueError("emb_layer_norm_before is true but the checkpoint has no esm.embeddings.layer_norm weights")
    return dict(arch=_lib.ARCH_SAPROT, layers=int(c["num_hidden_layers"]), embed_dim=int(c["hidden_size"]),
                heads=int(c["num_attention_heads"]), ffn_dim=int(c["intermediate_size"]), vocab=VOCAB, max_positions=0,
                token_dropout=int(bool(c.get("token_dropout", False))), emb_layer_norm_before=int(lnb),
                mask_token_id=int(c.get("mask_token_id", MASK)))


def weight_count(cfg: dict) -> int:
    D, F, V, L = cfg["embed_dim"], cfg["ffn_dim"], cfg["vocab"], cfg["layers"]
    return V * D + (2 * D if cfg["emb_layer_norm_before"] else 0) + L * (2 * D + 4 * (D * D + D) + 2 * D + F * D + F + D * F + D) \
        + 2 * D + D * D + D + 2 * D + V


def pack(cfg: dict, sd) -> np.ndarray:
    """The HF state dict in ESM2's blob order.  lm_head.bias may be stored as lm_head.decoder.bias; the tied decoder weight, the contact
    head, the rotary inv_freq buffers and an unused position table are ignored; anything else missing or unexpected is an error."""
    sd = dict(sd)
    if "lm_head.bias" not in sd and "lm_head.decoder.bias" in sd:
        sd["lm_head.bias"] = sd.pop("lm_head.decoder.bias")
    sd.pop("lm_head.decoder.bias", None)
    keys = hf_keys(cfg)
    want = {h for _, h in keys}
    missing = sorted(h for h in want if h not in sd)
    unexpected = sorted(k for k in sd if k not in want and not _ignored(k))
    if missing or unexpected:
        raise ValueError(f"not a SaProt (EsmForMaskedLM) state dict: missing {missing[:5]}, unexpected {unexpected[:5]}")
    blob = np.empty(weight_count(cfg), dtype=np.float32)
    o = 0
    for _, h in keys:
        t = sd[h]
        a = t.detach().to("cpu").float().numpy() if hasattr(t, "detach") else np.asarray(t, dtype=np.float32)
        blob[o:o + a.size] = a.ravel()
        o += a.size
    if o != blob.size:
        raise ValueError(f"state dict holds {o} weights, the configuration needs {blob.size}")
    return blob


def load_checkpoint(path: str):
    """(cfg, state dict) of a local checkpoint directory."""
    if not os.path.isdir(path):
        raise ValueError(f"{path!r} is not a local directory (config.json, vocab.txt, model.safetensors): this path never downloads")
    for n in ("config.json", "vocab.txt"):
        if not os.path.isfile(os.path.join(path, n)):
            raise FileNotFoundError(f"{path}: no {n}")
    check_vocabulary(read_vocab(os.path.join(path, "vocab.txt")))
    with open(os.path.join(path, "config.json")) as f:
        c = json.load(f)
    st, pt = os.path.join(path, "model.safetensors"), os.path.join(path, "pytorch_model.bin")
    if os.path.isfile(st):
        from safetensors.numpy import load_file
        sd = {k: np.asarray(v, dtype=np.float32) for k, v in load_file(st).items() if np.issubdtype(v.dtype, np.floating)}
    elif os.path.isfile(pt):
        import torch
        sd = {k: v.float().numpy() for k, v in torch.load(pt, map_location="cpu", weights_only=True).items() if v.is_floating_point()}
    else:
        raise FileNotFoundError(f"{path}: no model.safetensors or pytorch_model.bin")
    return config_from_hf(c, sd), sd


# -- an assay chunk: position sets ---------------------------------------------------------------------------------------------
def position_sets(sub_pos: np.ndarray, mut_off: np.ndarray):
    """Unique position sets of the mutants (sub_pos: token positions per sub-mutation, mut_off [n+1]) in order of first appearance, as
    CSR (set_off, set_pos; positions ascending, a repeated position once), and entry [n_sub]: the row of the group table that
    (mutant, sub-mutation) reads -- set_off[set of the mutant] + rank of the position inside the set."""
    n = len(mut_off) - 1
    sub_pos = np.asarray(sub_pos, dtype=np.int64)
    entry = np.empty(len(sub_pos), dtype=np.int32)
    if n and np.all(np.diff(mut_off) == 1):                # singles: one set per distinct position
        _, first, inv = np.unique(sub_pos, return_index=True, return_inverse=True)
        order = np.argsort(first, kind="stable")           # sets in order of first appearance
        rank = np.empty(len(order), dtype=np.int64)
        rank[order] = np.arange(len(order))
        entry[:] = rank[inv]
        return np.arange(len(order) + 1, dtype=np.int32), sub_pos[np.sort(first)].astype(np.int32), entry
    index: Dict[Tuple[int, ...], int] = {}
    set_off, set_pos = [0], []
    for i in range(n):
        ps = sub_pos[mut_off[i]:mut_off[i + 1]].tolist()
        key = tuple(sorted(set(ps)))
        s = index.get(key)
        if s is None:
            s = index[key] = len(set_off) - 1
            set_pos.extend(key)
            set_off.append(len(set_pos))
        base = set_off[s]
        for k, p in enumerate(ps):
            entry[mut_off[i] + k] = base + key.index(p)
    return np.array(set_off, dtype=np.int32), np.array(set_pos, dtype=np.int32), entry


def parse_chunk(mutants: Sequence[str], target_seq: str, range_start: int, chunk_len: int):
    """The mutants of one structure chunk: parsed against the whole target sequence with the existing parser (the wild-type assertion of
    get_mutated_sequence), their letters mapped to amino-acid groups (its to_AA assertion), positions rebased to the chunk's tokens
    (pos - range_start + 1, compute_fitness.py:68; <cls> is token 0).  A sub-mutation outside the chunk is a ValueError naming the
    mutant: the reference's negative or overlong index would silently read another token."""
    sub_pos, sub_wt, sub_mt, mut_off = pesm.parse_mutants(mutants, target_seq, 1)
    wt_g, mt_g = _ESM_TO_GROUP[sub_wt], _ESM_TO_GROUP[sub_mt]
    if (mt_g < 0).any() or (wt_g < 0).any():
        k = int(np.flatnonzero((mt_g < 0) | (wt_g < 0))[0])
        raise AssertionError("Mutant to_AA is invalid: " + str(mutants[int(np.searchsorted(mut_off, k, side="right")) - 1]))
    pos = sub_pos.astype(np.int64) - range_start + 1
    bad = np.flatnonzero((pos < 1) | (pos > chunk_len))
    if bad.size:
        i = int(np.searchsorted(mut_off, bad[0], side="right")) - 1
        raise ValueError(f"mutant {mutants[i]}: position {int(sub_pos[bad[0]])} lies outside its structure chunk "
                         f"{range_start}-{range_start + chunk_len - 1}")
    return pos.astype(np.int32), wt_g.astype(np.int32), mt_g.astype(np.int32), mut_off


# -- model -------------------------------------------------------------------------------------------------------------------
class SaProt(_lib.ModelHandle):
    """Device-resident SaProt (ESM2 encoder, 446-token vocabulary)."""
    CREATE = "pgmi_saprot_model_create"

    def __init__(self, cfg: dict, weights: np.ndarray, device: int = 0, precision: str = "f16x3", max_rows: int = 0):
        self.precision = precision
        super().__init__(cfg, weights, device, max_rows, arch_arg=int(cfg.get("mask_token_id", MASK)),
                         precision=_lib.PRECISIONS[precision], arch=_lib.ARCH_SAPROT, vocab=VOCAB, max_positions=0,
                         token_dropout=cfg["token_dropout"], emb_layer_norm_before=cfg["emb_layer_norm_before"])

    def token_logprobs(self, tokens) -> np.ndarray:
        """log_softmax(model(input_ids).logits) over all 446 columns: [B,T] -> [B,T,446]."""
        t = _lib.as_i32(np.atleast_2d(np.asarray(tokens)))
        B, T = t.shape
        out = np.empty((B, T, VOCAB), dtype=np.float32)
        _lib.check(_lib.load().pgmi_saprot_token_logprobs(self._h, _lib.ptr(t, _lib._i32p), B, T, _lib.ptr(out, _lib._f32p)))
        return out

    def group_logprobs(self, wt_tokens, set_off, set_pos) -> np.ndarray:
        """One forward per position set (CSR), the set's tokens masked; [n_entries, 21]: log of the summed probability of each
        amino-acid group at every (set, position)."""
        wt, so, sp = _lib.as_i32(wt_tokens), _lib.as_i32(set_off), _lib.as_i32(set_pos)
        out = np.empty((int(so[-1]), GROUPS), dtype=np.float32)
        _lib.check(_lib.load().pgmi_saprot_group_logprobs(self._h, _lib.ptr(wt, _lib._i32p), wt.size, _lib.ptr(so, _lib._i32p),
                                                          _lib.ptr(sp, _lib._i32p), so.size - 1, _lib.ptr(out, _lib._f32p)))
        return out

    def score_chunk(self, wt_tokens, pos, wt_group, mt_group, mut_off) -> np.ndarray:
        """calc_fitness for the parsed mutants of one chunk (parse_chunk): float64 [n_mut]."""
        if len(mut_off) <= 1:
            return np.zeros(0, dtype=np.float64)
        set_off, set_pos, entry = position_sets(pos, mut_off)
        table = self.group_logprobs(wt_tokens, set_off, set_pos)
        return pesm.score_parsed(table, entry, wt_group, mt_group, mut_off)

    profile_enable = pesm.EsmModel.profile_enable
    profile_reset = pesm.EsmModel.profile_reset
    profile = pesm.EsmModel.profile


def from_state_dict(cfg: dict, sd, device: int = 0, precision: str = "f16x3", max_rows: int = 0) -> SaProt:
    return SaProt(cfg, pack(cfg, sd), device=device, precision=precision, max_rows=max_rows)


def from_pretrained(path: str, device: int = 0, precision: str = "f16x3", max_rows: int = 0) -> SaProt:
    cfg, sd = load_checkpoint(path)
    return from_state_dict(cfg, sd, device=device, precision=precision, max_rows=max_rows)
