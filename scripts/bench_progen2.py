"""Secondary measurement: ProGen2 scoring throughput, end to end from an assay CSV to the scores CSV.
BLAT_ECOLX-shaped assay (L = 286 single mutants between the '1' ... '2' terminals, no mutated_sequence column), every sequence in
both reading directions as compute_fitness.py does, synthetic weights at a released width (proteingym_amd.synthetic.PROGEN2_WIDTHS
plus the released depths).  Prints mutants/s (and, with --profile, the per-kernel HIP-event breakdown of the scoring pass).

    python scripts/bench_progen2.py --width small --mutants 2000
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
from proteingym_amd import _lib, progen2 as pg, synthetic  # noqa: E402

DEPTH = {"small": 12, "medium": 27, "large": 32, "xlarge": 32}
ap = argparse.ArgumentParser()
ap.add_argument("--width", choices=list(synthetic.PROGEN2_WIDTHS), default="small")
ap.add_argument("--layers", type=int, default=0, help="0 = the released depth of that width")
ap.add_argument("--mutants", type=int, default=1000)
ap.add_argument("--profile", action="store_true", help="HIP-event breakdown per kernel class (adds event overhead to the timing)")
args = ap.parse_args()
w = synthetic.PROGEN2_WIDTHS[args.width]
cfg = synthetic.progen2_config(args.layers or DEPTH[args.width], w["embed_dim"], w["heads"], w["rotary_dim"])
model = pg.ProGen2Model(cfg, pg.pack(cfg, synthetic.progen2_state_dict(cfg, seed=3)))
seq, muts, _ = synthetic.random_assay(seed=23, L=286, n_single=args.mutants, n_multi=0)
with tempfile.TemporaryDirectory() as d:
    src, dst = os.path.join(d, "BLAT.csv"), os.path.join(d, "BLAT_scores.csv")
    pd.DataFrame({"mutant": muts, "DMS_score": 0.0}).to_csv(src, index=False)
    model.calc_fitness(pg.sequences_to_score(pd.read_csv(src).head(8), seq, False))         # warm-up (kernels loaded, workspace touched)
    lib = _lib.load()
    lib.pgmi_profile_enable(model._h, 1 if args.profile else 0)
    t0 = time.perf_counter()
    df = pd.read_csv(src)
    df["Progen2_score"] = model.calc_fitness(pg.sequences_to_score(df, seq, False), model_context_len=cfg["max_positions"])
    df[["mutant", "Progen2_score", "DMS_score"]].to_csv(dst, index=False)
    dt = time.perf_counter() - t0
prof = {}
for k, name in enumerate(_lib.K_NAMES):
    ms, n, fl, by = C.c_double(), C.c_int64(), C.c_double(), C.c_double()
    if lib.pgmi_profile_get(model._h, k, C.byref(ms), C.byref(n), C.byref(fl), C.byref(by)) == 0 and n.value:
        prof[name] = dict(ms=round(ms.value, 2), calls=n.value, tflops=round(fl.value / ms.value / 1e9, 1) if ms.value and fl.value else None)
print(json.dumps(dict(width=args.width, layers=cfg["layers"], head_dim=cfg["embed_dim"] // cfg["heads"], L=286, mutants=len(muts),
                      seconds=round(dt, 3), mutants_per_s=round(len(muts) / dt, 1), kernels=prof)))
model.close()
