"""Secondary measurement: ESM C scoring throughput, end to end from an assay CSV to the scores CSV (the CLI's score_csv).
BLAT_ECOLX-shaped assay (L = 286, every single mutant), synthetic weights at a released shape (proteingym_amd.synthetic.esmc_config)
and full depth.  Prints one JSON line per model: mutants/s and the per-class HIP-event breakdown ("attention" includes the QK-LayerNorm
prep pass that produces its operands), then the two new kernels on their own: the SwiGLU FC1 against ESM's GELU FC1 at the same
M, N = 2F and K (TFLOP/s), and the QK-LayerNorm prep pass at the forward's M (TB/s, 8 B per element of the fp32 [M, 3D] input).

    python scripts/bench_esmc.py --model 300M 600M
"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np
import pandas as pd

sys.path.insert(0, os.getcwd())
from proteingym_amd import _lib, esmc, synthetic  # noqa: E402
from proteingym_amd.score_esmc_proteingym import score_csv  # noqa: E402

SHAPES = {"300M": (960, 30), "600M": (1152, 36)}
ap = argparse.ArgumentParser()
ap.add_argument("--model", nargs="+", choices=list(SHAPES), default=list(SHAPES))
ap.add_argument("--layers", type=int, default=0, help="0 = the released depth")
ap.add_argument("--iters", type=int, default=50, help="launches per kernel timing")
args = ap.parse_args()
lib = _lib.load()
AA = "ACDEFGHIKLMNPQRSTVWY"
rng = np.random.default_rng(23)
seq = "".join(rng.choice(list(AA), 286))
muts = [f"{seq[p]}{p + 1}{a}" for p in range(len(seq)) for a in AA if a != seq[p]]


def gemm_tflops(M, N, K, epi):
    ms = C.c_double()
    _lib.check(lib.pgmi_bench_gemm(0, _lib.PREC_F16X3, M, N, K, epi, 1, 0, args.iters, C.byref(ms)))
    return round(2.0 * M * N * K / ms.value / 1e9, 1), round(ms.value, 4)


for name in args.model:
    D, L = SHAPES[name]
    cfg = synthetic.esmc_config(D, args.layers or L)
    model = esmc.ESMC(cfg, esmc.pack(cfg, synthetic.esmc_state_dict(cfg, seed=3)))
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "BLAT.csv"), os.path.join(d, "BLAT_scores.csv")
        pd.DataFrame({"mutant": muts, "DMS_score": rng.standard_normal(len(muts))}).to_csv(src, index=False)
        score_csv(model, src, seq, f"esmc_{name}", dst)                                # warm-up (first scipy import, first launches)
        t0 = time.perf_counter()
        score_csv(model, src, seq, f"esmc_{name}", dst)
        dt = time.perf_counter() - t0
        lib.pgmi_profile_enable(model._h, 1)
        score_csv(model, src, seq, f"esmc_{name}", dst)
        lib.pgmi_profile_enable(model._h, 0)
    prof = {}
    for k, kname in enumerate(_lib.K_NAMES):
        ms, n, fl, by = C.c_double(), C.c_int64(), C.c_double(), C.c_double()
        if lib.pgmi_profile_get(model._h, k, C.byref(ms), C.byref(n), C.byref(fl), C.byref(by)) == 0 and n.value:
            prof[kname] = dict(ms=round(ms.value, 2), calls=n.value,
                               tflops=round(fl.value / ms.value / 1e9, 1) if ms.value and fl.value else None,
                               gbps=round(by.value / ms.value / 1e6, 1) if ms.value and by.value else None)
    model.close()
    F, T = cfg["ffn_dim"], 288
    rows_per_call = max(1, 98304 // T)                      # masked rows of one device chunk (library default workspace)
    M = min(len(seq), rows_per_call) * T
    swiglu, gelu = gemm_tflops(M, 2 * F, D, 4), gemm_tflops(M, 2 * F, D, 1)
    qkv = rng.standard_normal((M, 3 * D), dtype=np.float32)
    w = (1.0 + 0.1 * rng.standard_normal(D)).astype(np.float32)
    ms = C.c_double()
    _lib.check(lib.pgmi_op_qkln_prep(0, _lib.ptr(qkv, _lib._f32p), _lib.ptr(w, _lib._f32p), _lib.ptr(w, _lib._f32p), M // T, T, D // 64,
                                     args.iters, None, None, C.byref(ms)))
    print(json.dumps(dict(model=f"esmc_{name}", layers=cfg["layers"], embed_dim=D, ffn_dim=F, L=len(seq), mutants=len(muts),
                          forwards=len(seq), seconds=round(dt, 3), mutants_per_s=round(len(muts) / dt, 1), kernels_profiled=prof,
                          fc1_M=M, fc1_swiglu_tflops=swiglu[0], fc1_swiglu_ms=swiglu[1], fc1_gelu_tflops=gelu[0], fc1_gelu_ms=gelu[1],
                          qkln_prep_ms=round(ms.value, 4), qkln_prep_tbps=round(M * 3 * D * 8 / ms.value / 1e9, 2))), flush=True)
