"""Secondary measurement: RITA / ProtGPT2 scoring throughput, end to end from an assay CSV to the scores CSV.
BLAT_ECOLX-shaped assay (L = 286 single mutants, no mutated_sequence column), every sequence in both reading directions as the
reference's calc_fitness does, synthetic weights at a released shape (proteingym_amd.synthetic.RITA_WIDTHS / PROTGPT2_SHAPE).
No real tokenizer file is available: RITA runs on the character-level stand-in of tests/golden/rita_toy_tokenizer (one id per
residue, as RITA's own), ProtGPT2 on the toy byte-level BPE of tests/golden/protgpt2_toy_tokenizer (~0.9 tokens per residue; the
real ProtGPT2 BPE packs ~4 residues per token, so its rows are ~3.5x shorter than here).  Prints mutants/s and the per-kernel
HIP-event breakdown; for the wide head (V > 64) "head" is the logits GEMM and "score" the wide log-softmax with its GB/s.

    python scripts/bench_causal_lm.py --model rita-s --mutants 2000
    python scripts/bench_causal_lm.py --model protgpt2 --layers 8
"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import pandas as pd

sys.path.insert(0, os.getcwd())
from proteingym_amd import _lib, causal_lm as clm, synthetic  # noqa: E402

GOLDEN = os.path.join(os.getcwd(), "tests", "golden")
ap = argparse.ArgumentParser()
ap.add_argument("--model", choices=["rita-" + k for k in synthetic.RITA_WIDTHS] + ["protgpt2"], default="rita-s")
ap.add_argument("--layers", type=int, default=0, help="0 = the released depth")
ap.add_argument("--mutants", type=int, default=1000)
ap.add_argument("--no-profile", action="store_true", help="time without HIP events")
args = ap.parse_args()
if args.model == "protgpt2":
    sh = synthetic.PROTGPT2_SHAPE
    cfg = synthetic.gpt2_config(args.layers or sh["layers"], sh["embed_dim"], sh["heads"], sh["vocab"], sh["max_positions"])
    sd, tok = synthetic.gpt2_state_dict(cfg, seed=3), os.path.join(GOLDEN, "protgpt2_toy_tokenizer")
else:
    w = synthetic.RITA_WIDTHS[args.model[5:]]
    cfg = synthetic.rita_config(args.layers or w["layers"], w["embed_dim"], w["heads"])
    sd, tok = synthetic.rita_state_dict(cfg, seed=3), os.path.join(GOLDEN, "rita_toy_tokenizer")
model = clm.CausalLM(cfg, clm.pack(cfg, sd))
del sd
encode = clm.load_tokenizer(tok)
seq, muts, _ = synthetic.random_assay(seed=23, L=286, n_single=args.mutants, n_multi=0)
with tempfile.TemporaryDirectory() as d:
    src, dst = os.path.join(d, "BLAT.csv"), os.path.join(d, "BLAT_scores.csv")
    pd.DataFrame({"mutant": muts, "DMS_score": 0.0}).to_csv(src, index=False)
    model.calc_fitness([clm.get_mutated_sequence(seq, m) for m in muts[:8]], encode)          # warm-up
    lib = _lib.load()
    lib.pgmi_profile_enable(model._h, 0 if args.no_profile else 1)
    t0 = time.perf_counter()
    df = pd.read_csv(src)
    df["mutated_sequence"] = df["mutant"].apply(lambda x: clm.get_mutated_sequence(seq, x))
    df["score"] = model.calc_fitness(list(df["mutated_sequence"]), encode)
    df[["mutant", "score", "DMS_score"]].to_csv(dst, index=False)
    dt = time.perf_counter() - t0
prof = {}
for k, name in enumerate(_lib.K_NAMES):
    ms, n, fl, by = C.c_double(), C.c_int64(), C.c_double(), C.c_double()
    if lib.pgmi_profile_get(model._h, k, C.byref(ms), C.byref(n), C.byref(fl), C.byref(by)) == 0 and n.value:
        prof[name] = dict(ms=round(ms.value, 2), calls=n.value,
                          tflops=round(fl.value / ms.value / 1e9, 1) if ms.value and fl.value else None,
                          gbps=round(by.value / ms.value / 1e6, 1) if ms.value and by.value else None)
print(json.dumps(dict(model=args.model, layers=cfg["layers"], embed_dim=cfg["embed_dim"], head_dim=cfg["embed_dim"] // cfg["heads"],
                      vocab=cfg["vocab"], L=286, tokens_per_row=int(encode(seq).size), mutants=len(muts), seconds=round(dt, 3),
                      mutants_per_s=round(len(muts) / dt, 1), profiled=not args.no_profile, kernels=prof)))
model.close()
