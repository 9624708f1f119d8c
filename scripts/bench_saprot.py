"""Secondary measurement: SaProt scoring throughput on a BLAT_ECOLX-shaped structure chunk (L = 286, T = 288), synthetic weights at
SaProt-650M's shape (proteingym_amd.synthetic.saprot_config) and full depth.  Two legs:

  singles  every single mutant of the assay's size (4 996): at most 286 position sets, one kept row each
  multi    about 5 000 distinct position sets of 2-4 positions (one multi-mutant each)

Per leg one JSON line: position-set forwards per second, mutants per second, the per-class HIP-event breakdown.  The yardstick is
ESM2-650M's pgmi_masked_logprobs at the same B and T on the SAME encoder weights (the embedding and LM-head bias cut to ESM's 33
rows), timed in interleaved rounds -- SaProt, yardstick, yardstick -- so that the ratio and the A/A spread of the yardstick come from
one box and one session.  --yardstick-lib names another build of libpgmi.so (the parent commit's) to take the yardstick from.

    python scripts/bench_saprot.py [--layers 33] [--rounds 3] [--yardstick-lib path/to/libpgmi.so]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.getcwd())
from proteingym_amd import _lib, saprot, synthetic  # noqa: E402
from proteingym_amd import esm as pesm  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--layers", type=int, default=33)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--multi-sets", type=int, default=5000)
ap.add_argument("--yardstick-lib", default=None, help="another libpgmi.so build for the ESM2 yardstick (default: this tree's)")
args = ap.parse_args()
lib = _lib.load()
AA = "ACDEFGHIKLMNPQRSTVWY"
L, N_SINGLES = 286, 4996
rng = np.random.default_rng(29)
seq = "".join(rng.choice(list(AA), L))
struc = "".join(rng.choice(list(saprot.STRUC_LETTERS), L))
wt_ids = saprot.tokenize(seq, struc)
T = wt_ids.size

every = [f"{seq[p]}{p + 1}{a}" for p in range(L) for a in AA if a != seq[p]]
singles = [every[i] for i in sorted(rng.choice(len(every), N_SINGLES, replace=False))]
multi, seen = [], set()
while len(multi) < args.multi_sets:
    ps = tuple(sorted(int(p) for p in rng.choice(L, int(rng.integers(2, 5)), replace=False)))
    if ps not in seen:
        seen.add(ps)
        multi.append(":".join(f"{seq[p]}{p + 1}{rng.choice([a for a in AA if a != seq[p]])}" for p in ps))

cfg = synthetic.saprot_config(layers=args.layers)
sd = synthetic.saprot_state_dict(cfg, seed=5)
model = saprot.from_state_dict(cfg, sd)
# the yardstick: the same encoder under ESM2's 33-token vocabulary
esm_cfg = dict(synthetic.ESM2_650M, layers=args.layers)
esm_sd = dict(sd)
esm_sd["esm.embeddings.word_embeddings.weight"] = sd["esm.embeddings.word_embeddings.weight"][:33]
esm_sd["lm_head.bias"] = sd["lm_head.bias"][:33]
esm_blob = saprot.pack(dict(cfg, vocab=33), esm_sd)
del sd, esm_sd


class Yardstick:
    """ESM2 pgmi_masked_logprobs through a libpgmi.so of its own (ctypes keeps two builds apart)."""

    def __init__(self, path, cfg, blob):
        self.lib = C.CDLL(path)
        for name, res, argtypes in _lib.SIGNATURES:
            if name in ("pgmi_model_create", "pgmi_masked_logprobs", "pgmi_model_destroy", "pgmi_last_error", "pgmi_profile_enable",
                        "pgmi_profile_get", "pgmi_profile_reset"):
                fn = getattr(self.lib, name)
                fn.restype, fn.argtypes = res, argtypes
        c = _lib.Config(abi_version=self.lib.pgmi_abi_version(), arch=cfg["arch"], layers=cfg["layers"], embed_dim=cfg["embed_dim"],
                        heads=cfg["heads"], ffn_dim=cfg["ffn_dim"], vocab=33, max_positions=0, token_dropout=cfg["token_dropout"],
                        emb_layer_norm_before=0, precision=_lib.PREC_F16X3, max_rows=0)
        self.h = C.c_void_p()
        if self.lib.pgmi_model_create(C.byref(c), _lib.ptr(blob, _lib._f32p), blob.size, 0, C.byref(self.h)):
            raise RuntimeError(self.lib.pgmi_last_error().decode())

    def run(self, B):
        tokens = _lib.as_i32(np.tile(np.concatenate([[0], rng.integers(4, 24, T - 2), [2]]), (B, 1)))
        mask = _lib.as_i32(1 + np.arange(B) % (T - 2))
        out = np.empty((B, 33), dtype=np.float32)
        t0 = time.perf_counter()
        if self.lib.pgmi_masked_logprobs(self.h, _lib.ptr(tokens, _lib._i32p), _lib.ptr(mask, _lib._i32p), B, T, _lib.ptr(out, _lib._f32p)):
            raise RuntimeError(self.lib.pgmi_last_error().decode())
        return time.perf_counter() - t0


def profile_of(plib, handle):
    prof = {}
    for k, kname in enumerate(_lib.K_NAMES):
        ms, n, fl, by = C.c_double(), C.c_int64(), C.c_double(), C.c_double()
        if plib.pgmi_profile_get(handle, k, C.byref(ms), C.byref(n), C.byref(fl), C.byref(by)) == 0 and n.value:
            prof[kname] = dict(ms=round(ms.value, 2), calls=n.value)
    return prof


yard = Yardstick(args.yardstick_lib or _lib.LIB_PATH, esm_cfg, esm_blob)
del esm_blob
for leg, muts in (("singles", singles), ("multi", multi)):
    pos, wt, mt, off = saprot.parse_chunk(muts, seq, 1, L)
    set_off, set_pos, entry = saprot.position_sets(pos, off)
    n_sets = len(set_off) - 1

    def score():
        t0 = time.perf_counter()
        table = model.group_logprobs(wt_ids, set_off, set_pos)
        pesm.score_parsed(table, entry, wt, mt, off)
        return time.perf_counter() - t0
    score(), yard.run(n_sets)                                # warm-up: first launches, rotary tables, clocks
    rounds = [(score(), yard.run(n_sets), yard.run(n_sets)) for _ in range(args.rounds)]
    s, a, b = (float(np.median([r[i] for r in rounds])) for i in range(3))
    lib.pgmi_profile_reset(model._h), lib.pgmi_profile_enable(model._h, 1)
    score()
    lib.pgmi_profile_enable(model._h, 0)
    prof = profile_of(lib, model._h)
    yard.lib.pgmi_profile_reset(yard.h), yard.lib.pgmi_profile_enable(yard.h, 1)
    yard.run(n_sets)
    yard.lib.pgmi_profile_enable(yard.h, 0)
    yprof = profile_of(yard.lib, yard.h)
    total = sum(v["ms"] for v in prof.values())
    print(json.dumps(dict(leg=leg, layers=cfg["layers"], T=int(T), mutants=len(muts), position_sets=n_sets, kept_rows=int(set_off[-1]),
                          seconds=round(s, 4), sets_per_s=round(n_sets / s, 1), mutants_per_s=round(len(muts) / s, 1),
                          yardstick_seconds=[round(a, 4), round(b, 4)], yardstick_lib=args.yardstick_lib or "this tree",
                          ratio_to_yardstick=round(s / (0.5 * (a + b)), 4), yardstick_aa_spread=round(abs(a - b) / (0.5 * (a + b)), 4),
                          head_embed_share=round((prof.get("head", {}).get("ms", 0) + prof.get("embed", {}).get("ms", 0)) / total, 4),
                          rounds=[[round(x, 4) for x in r] for r in rounds], kernels_profiled=prof, yardstick_profiled=yprof)), flush=True)
model.close()
yard.lib.pgmi_model_destroy(yard.h)
