"""PoET scoring on libpgmi (include/pgmi.h, arch PGMI_ARCH_POET).

Replaces proteingym/baselines/PoET/scripts/score.py: the checkpoint is packed into the C ABI's blob, the tiered forward over the prompt
and the variants runs in HIP (csrc/api_poet.hip on csrc/attention_prefix.hip), and this module restates the host side -- the Uniprot21
encoding, the a3m handling, the similarity filter, the homology weights (neighbour counts from pgmi_msa_neighbor_counts, once per MSA:
the reference recomputes them for each of its 15 ensemble members), the numpy sampling and permutation with the reference's generator
calls in the reference's order, and the ensemble arithmetic in the reference's order and dtype.
"""
from __future__ import annotations

import ctypes as C
import io
import itertools
import os
from typing import Optional, Sequence

import numpy as np

from . import _lib

# poet/alphabets.py Uniprot21(include_gap=True, include_startstop=True, distinct_startstop=True)
CHARS = b"ARNDCQEGHILKMFPSTWYV-*$XOUBZ"
GAP, START, STOP, MASK = 20, 21, 22, 23
N_VOCAB = 24
ENCODING = np.full(256, MASK, dtype=np.uint8)
ENCODING[np.frombuffer(CHARS, dtype=np.uint8)] = list(range(24)) + [11, 4, MASK, MASK]          # O, U, B, Z are synonyms
ASCII_LOWERCASE = bytes(range(ord("a"), ord("z") + 1))
SIMILARITY_CUTOFFS = (1.0, 0.95, 0.90, 0.70, 0.50)
CONTEXT_LENGTHS = (6144, 12288, 24576)
THETA = 0.2
SEED = 188257
INIT_ARGS = {"n_vocab", "hidden_dim", "ff_dim", "num_layers", "nhead", "dropout", "use_multi_rotary", "norm", "mask_token"}


def encode(seq: bytes) -> np.ndarray:
    """Alphabet.encode: one uint8 id per byte, anything unknown is the mask token."""
    return ENCODING[np.frombuffer(bytes(seq), dtype=np.uint8)]


def append_startstop(x: np.ndarray) -> np.ndarray:
    out = np.empty(x.size + 2, dtype=x.dtype)
    out[0], out[-1] = START, STOP
    out[1:-1] = x
    return out


def frame(seq) -> np.ndarray:
    """A sequence (str or bytes) as the model reads it: start + ids + stop."""
    return append_startstop(encode(seq.encode() if isinstance(seq, str) else seq))


# -- MSA -------------------------------------------------------------------------------------------------------------------
def parse_a3m(data: bytes) -> list:
    """poet/fasta.py parse_stream(upper=False): the sequences of a fasta-like file, lower-case kept, '#' lines skipped."""
    seqs, cur, named = [], [], False
    for line in io.BytesIO(data):
        if line.startswith(b"#"):
            continue
        line = line.strip()
        if line.startswith(b">"):
            if named:
                seqs.append(b"".join(cur))
            named, cur = True, []
        else:
            cur.append(line)
    if named:
        seqs.append(b"".join(cur))
    return seqs


def _zstd_decompress(data: bytes, path: str) -> bytes:
    try:
        import pyzstd
        return pyzstd.decompress(data)
    except ImportError:
        pass
    try:
        import zstandard
        return zstandard.ZstdDecompressor().decompressobj().decompress(data)
    except ImportError:
        pass
    try:
        from compression import zstd            # Python 3.14
        return zstd.decompress(data)
    except ImportError:
        raise RuntimeError(f"{path}: no zstd module is importable (pyzstd, zstandard or compression.zstd); install one or put the "
                           f"decompressed {os.path.basename(path)[:-4]} beside it") from None


def read_msa(msa_folder: str, dms_filename: str) -> list:
    """<stem>.a3m.zst as the reference names it, else <stem>.a3m from the same folder."""
    stem = os.path.splitext(dms_filename)[0]
    zst, plain = os.path.join(msa_folder, stem + ".a3m.zst"), os.path.join(msa_folder, stem + ".a3m")
    problem = None
    if os.path.isfile(zst):
        try:
            return parse_a3m(_zstd_decompress(open(zst, "rb").read(), zst))
        except RuntimeError as e:
            problem = str(e)
    if os.path.isfile(plain):
        return parse_a3m(open(plain, "rb").read())
    raise FileNotFoundError(problem or f"neither {zst} nor {plain} exists")


def encoded_msa(msa_sequences: Sequence[bytes]) -> np.ndarray:
    """get_encoded_msa_from_a3m_seqs: lower-case (insertion) columns stripped, uint8 [N, L]."""
    rows = [encode(s.translate(None, delete=ASCII_LOWERCASE)) for s in msa_sequences]
    if len({r.size for r in rows}) != 1:
        raise ValueError("the MSA rows differ in length once their lower-case columns are stripped")
    return np.vstack(rows)


def neighbor_counts(msa: np.ndarray, theta: float = THETA, device: int = 0) -> np.ndarray:
    """#{j : 1 - matches(i, j) / nongap(i) <= theta} on the pair-count kernel; equal to the reference's numpy path."""
    m = np.ascontiguousarray(msa, dtype=np.int8)
    out = np.empty(m.shape[0], dtype=np.int32)
    _lib.check(_lib.load().pgmi_msa_neighbor_counts(device, m.ctypes.data_as(C.POINTER(C.c_int8)), m.shape[0], m.shape[1], GAP,
                                                    float(theta), _lib.ptr(out, _lib._i32p), None))
    return out


def homology_weights(neighbors: np.ndarray) -> np.ndarray:
    """compute_homology_weights: p = 1 / neighbors, normalised (float64, the reference's two statements)."""
    p = 1 / np.asarray(neighbors)
    p /= np.sum(p)
    return p


def sim_filtered_idxs(msa: np.ndarray, max_similarity: float, max_dissimilarity: float = 1.0) -> np.ndarray:
    """MSASampler._get_sim_filtered_idxs: similarity to row 0 over all aligned columns."""
    norm_sim = (msa == msa[[0]]).sum(axis=1) / msa.shape[1]
    dsim = 1 - norm_sim
    return np.where((norm_sim <= max_similarity) & (dsim <= max_dissimilarity))[0]


def sample_idxs(msa: np.ndarray, weights: np.ndarray, max_similarity: float, seed: int) -> np.ndarray:
    """MSASampler.get_sample_idxs with NeighborsSampler: filter, then one rng.choice without replacement over the kept rows."""
    keep = sim_filtered_idxs(msa, max_similarity)
    if keep.size == 0:
        return np.array([], dtype=int)
    w = weights[keep]
    rng = np.random.default_rng(seed)
    return np.arange(len(msa))[keep][rng.choice(keep.size, replace=False, size=keep.size, p=w / w.sum())]


def prompt_sequences(msa_sequences: Sequence[bytes], idxs: Sequence[int], max_tokens: int, seed: int) -> list:
    """sample_msa_sequences(shuffle=True, truncate=False): sequences upper-cased and de-gapped, framed, taken until the budget is
    passed, then a seeded permutation; the prompt may overshoot max_tokens by up to one sequence."""
    seqs, total = [], 0
    for i in idxs:
        seqs.append(frame(msa_sequences[i].upper().translate(None, delete=b"-")))
        total += seqs[-1].size
        if total > max_tokens:
            break
    perm = np.random.default_rng(seed).permutation(len(seqs))
    out, total = [], 0
    for s in (seqs[i] for i in perm):
        total += s.size
        out.append(s)
        if total >= max_tokens:
            break
    return out


# -- checkpoint ------------------------------------------------------------------------------------------------------------
def config_from_init_args(a: dict) -> dict:
    unknown = sorted(set(a) - INIT_ARGS)
    if unknown:
        raise ValueError(f"PoET checkpoint: unknown model init args {unknown}")
    if not a.get("use_multi_rotary", True):
        raise ValueError("PoET checkpoint: use_multi_rotary=False (no rotary in the sequence-of-sequences attention) is not supported")
    D = int(a.get("hidden_dim", 768))
    return dict(layers=int(a.get("num_layers", 6)), embed_dim=D, heads=int(a.get("nhead", 12)), ffn_dim=int(a.get("ff_dim") or 4 * D),
                vocab=int(a["n_vocab"]), final_norm=bool(a.get("norm", False)))


def expected_keys(cfg: dict) -> list:
    keys = ["token_embed.weight"]
    for i in range(cfg["layers"]):
        p = f"decoder.layers.{i}."
        for att, norm in (("self_attn", "norm1"), ("multihead_attn", "norm2")):
            keys += [p + norm + ".weight", p + norm + ".bias"]
            keys += [p + att + f".{n}_proj.weight" for n in "qkv"] + [p + att + ".out_proj.weight", p + att + ".out_proj.bias"]
        keys += [p + "norm3.weight", p + "norm3.bias", p + "linear1.weight", p + "linear1.bias", p + "linear2.weight", p + "linear2.bias"]
    if cfg["final_norm"]:
        keys += ["norm.weight", "norm.bias"]
    return keys + ["linear.weight", "linear.bias"]


def weight_count(cfg: dict) -> int:
    D, F, V, L = cfg["embed_dim"], cfg["ffn_dim"], cfg["vocab"], cfg["layers"]
    att = 2 * D + 4 * D * D + D
    return V * D + L * (2 * att + 2 * D + F * D + F + D * F + D) + (2 * D if cfg["final_norm"] else 0) + V * D + V


def pack(cfg: dict, sd) -> np.ndarray:
    """The C ABI's blob (include/pgmi.h, PoET) from a state dict whose keys have lost their leading component."""
    keys = expected_keys(cfg)
    missing = [k for k in keys if k not in sd]
    if missing:
        raise RuntimeError(f"Missing key(s) in PoET state_dict: {missing[:8]}...")
    blob = np.empty(weight_count(cfg), dtype=np.float32)
    o = 0
    for k in keys:
        a = sd[k]
        if hasattr(a, "detach"):
            a = a.detach().float().numpy()
        a = np.asarray(a, dtype=np.float32)
        blob[o:o + a.size] = a.ravel()
        o += a.size
    assert o == blob.size
    return blob


def load_checkpoint(path: str):
    """A .ckpt as scripts/score.py reads it: hyper_parameters.model_spec.init_args and a state_dict whose keys carry one leading
    component.  Returns (cfg, blob)."""
    import torch
    try:
        ckpt = torch.load(path, map_location="cpu", weights_only=True)
    except Exception:            # a Lightning checkpoint may carry objects beside tensors and plain containers
        ckpt = torch.load(path, map_location="cpu", weights_only=False)
    cfg = config_from_init_args(ckpt["hyper_parameters"]["model_spec"]["init_args"])
    sd = {k.split(".", 1)[1]: v for k, v in ckpt["state_dict"].items()}
    extra = sorted(k for k in sd if k not in set(expected_keys(cfg)) and not k.startswith("rotary_emb.") and not k.endswith("rotary_emb.inv_freq"))
    if extra:
        raise RuntimeError(f"Unexpected key(s) in PoET state_dict: {extra[:8]}...")
    return cfg, pack(cfg, sd)


# -- model -----------------------------------------------------------------------------------------------------------------
class PoetModel(_lib.ModelHandle):
    """Device-resident PoET (f16x3).  max_prompt: the largest prompt in tokens (the prefix cache is allocated for it)."""
    CREATE = "pgmi_poet_model_create"

    def __init__(self, cfg: dict, weights: np.ndarray, device: int = 0, max_rows: int = 0, max_prompt: int = 0):
        super().__init__(cfg, weights, device, max_rows, arch_arg=int(bool(cfg["final_norm"])), arch=_lib.ARCH_POET, vocab=cfg["vocab"],
                         max_positions=int(max_prompt))
        self.prompt_tokens = 0

    @staticmethod
    def _weight_count(lib, c, arch_arg):
        return lib.pgmi_poet_weight_count(C.byref(c), arch_arg)

    def set_prompt(self, sequences: Sequence[np.ndarray]):
        """The framed prompt sequences (possibly none: the reference's memory=None)."""
        lens = _lib.as_i32([len(s) for s in sequences])
        toks = _lib.as_i32(np.concatenate(sequences)) if len(sequences) else _lib.as_i32([])
        _lib.check(_lib.load().pgmi_poet_set_prompt(self._h, _lib.ptr(toks, _lib._i32p), _lib.ptr(lens, _lib._i32p), len(sequences)))
        self.prompt_tokens = int(lens.sum())

    def prompt_logprobs(self) -> np.ndarray:
        out = np.empty((self.prompt_tokens, self.cfg["vocab"]), dtype=np.float32)
        _lib.check(_lib.load().pgmi_poet_prompt_logprobs(self._h, _lib.ptr(out, _lib._f32p)))
        return out

    @staticmethod
    def _pad(variants: Sequence[np.ndarray]):
        lens = _lib.as_i32([len(v) for v in variants])
        t = np.full((len(variants), int(lens.max())), MASK, dtype=np.int32)
        for i, v in enumerate(variants):
            t[i, :len(v)] = v
        return t, lens

    def token_logprobs(self, variants: Sequence[np.ndarray]) -> np.ndarray:
        t, lens = self._pad(variants)
        out = np.empty(t.shape + (self.cfg["vocab"],), dtype=np.float32)
        _lib.check(_lib.load().pgmi_poet_token_logprobs(self._h, _lib.ptr(t, _lib._i32p), _lib.ptr(lens, _lib._i32p), t.shape[0], t.shape[1],
                                                        _lib.ptr(out, _lib._f32p)))
        return out

    def sequence_loglik(self, variants: Sequence[np.ndarray]) -> np.ndarray:
        t, lens = self._pad(variants)
        out = np.empty(t.shape[0], dtype=np.float64)
        _lib.check(_lib.load().pgmi_poet_sequence_loglik(self._h, _lib.ptr(t, _lib._i32p), _lib.ptr(lens, _lib._i32p), t.shape[0], t.shape[1],
                                                         _lib.ptr(out, _lib._f64p)))
        return out

    def score(self, variants: Sequence[np.ndarray], max_batch: int = 4096) -> np.ndarray:
        """log p(variant | prompt) for every variant, as float32 (the reference's `.float().sum(dim=1)` leaves float32): variants sorted
        by length and handed over in batches; the library chunks a batch to its row budget.  Neither changes a variant's bits."""
        order = np.argsort([len(v) for v in variants], kind="stable")
        out = np.empty(len(variants), dtype=np.float32)
        for b0 in range(0, len(order), max_batch):
            idx = order[b0:b0 + max_batch]
            out[idx] = self.sequence_loglik([variants[i] for i in idx]).astype(np.float32)
        return out


def from_checkpoint(path: str, device: int = 0, max_rows: int = 0, max_prompt: int = 0) -> PoetModel:
    cfg, blob = load_checkpoint(path)
    return PoetModel(cfg, blob, device=device, max_rows=max_rows, max_prompt=max_prompt)


# -- the ensemble ----------------------------------------------------------------------------------------------------------
def ensemble_members(context_lengths: Sequence[int]):
    return list(itertools.product(context_lengths, SIMILARITY_CUTOFFS))


def member_prompts(msa_sequences: Sequence[bytes], msa: np.ndarray, weights: np.ndarray, context_lengths: Sequence[int], seed: int):
    """For every ensemble member (context length x similarity cut-off, the reference's order): (sampled indices, prompt sequences).  The
    generator is re-seeded for every member, as in the reference."""
    out = []
    for max_tokens, max_similarity in ensemble_members(context_lengths):
        idxs = sample_idxs(msa, weights, max_similarity, seed)
        out.append((idxs, prompt_sequences(msa_sequences, idxs, max_tokens, seed)))
    return out


def max_prompt_tokens(prompts) -> int:
    return max((sum(s.size for s in p) for _, p in prompts), default=0)


def ensemble_scores(model: PoetModel, prompts, variants: Sequence[np.ndarray], relative_to_wt: bool = False,
                    members_out: Optional[list] = None) -> np.ndarray:
    """scripts/score.py main(): per member (forward + backward) / 2 in float32, the members stacked and averaged; with relative_to_wt
    the last variant is the wild type.  The backward pass reverses every token array whole, start and stop tokens included."""
    rev = [np.ascontiguousarray(v[::-1]) for v in variants]
    logps = []
    for _, prompt in prompts:
        model.set_prompt(prompt)
        fwd = model.score(variants)
        model.set_prompt([np.ascontiguousarray(s[::-1]) for s in prompt])
        bwd = model.score(rev)
        logps.append((fwd + bwd) / 2)
        if members_out is not None:
            members_out.append((fwd, bwd))
    out = np.vstack(logps).mean(axis=0)
    return out[:-1] - out[-1] if relative_to_wt else out
