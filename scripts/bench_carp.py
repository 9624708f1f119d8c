#!/usr/bin/env python
"""CARP scoring at a BLAT-shaped assay: seeded carp_640M-shaped weights (D = d_h = 1280, 56 blocks), L = 286, 4 996 seeded single and
multiple mutants (synthetic.random_assay), masked marginals.

    python scripts/bench_carp.py [--layers 56] [--L 286] [--mutants 4996] [--repeats 2] [--torch_forwards 8] [--iters 5]

Reports (one JSON line):
  * mutants/s and ms per assay of carp.masked_marginal_scores (host clock around calls that end in a device synchronise; one warm-up
    first), and the per-kernel split of a second, profiled pass (pgmi_profile_* on pgmi_carp_profile_model's handle: HIP events on the
    stream, so the classes do not overlap) with the convolution's share of the device time;
  * the convolution kernel alone at M = L x L rows in L segments, C = 1280, dilation 1 and 128 (pgmi_bench_dilated_conv), as
    algorithmic TFLOP/s = 2 M C 5 C / t -- every tap counted, also those that fall outside a segment;
  * the yardsticks, measured on the same GPU in the same run: the dense f16x3 GEMM at M x 1280 x 6400 (pgmi_bench_gemm: the same
    FLOPs without the gather) and the fp32 torch restatement's forwards per second at batch 1, as the reference runs it (a child
    process of its own before this one opens the GPU: torch brings its own HIP runtime).
Arithmetic: a block costs 2 (2 D d_h + 5 d_h^2) FLOP per token."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from proteingym_amd import _lib, carp, synthetic  # noqa: E402

CLASSES = {"embed": 0, "ln_gelu": 1, "pff1": 5, "dilated_conv": 3, "pff2": 6, "head": 7}


def torch_forwards_per_sec(ck, tokens, n, device="cuda"):
    """fp32 torch at batch 1 on the GPU: the block of the reference's ByteNet as F.layer_norm / F.gelu / F.conv1d, weights resident."""
    import torch
    import torch.nn.functional as F
    sd = {k: torch.as_tensor(np.asarray(v), dtype=torch.float32, device=device) for k, v in ck["model_state_dict"].items()}
    dil = carp.dilation_schedule(ck["n_layers"], ck["r"])
    tok = torch.as_tensor(np.asarray(tokens, dtype=np.int64), device=device)[None]

    def ln(v, key):
        return F.layer_norm(v.transpose(1, 2), (v.shape[1],), sd[key + ".weight"], sd[key + ".bias"], 1e-5).transpose(1, 2)

    def forward():
        x = F.conv1d(F.embedding(tok, sd[carp.K_EMBED]).transpose(1, 2), sd[carp.K_UP_W], sd[carp.K_UP_B])
        for n_, d in enumerate(dil):
            b = carp.block_keys(n_)
            h = F.conv1d(F.gelu(ln(x, b["ln1"])), sd[b["pff1"] + ".weight"], sd[b["pff1"] + ".bias"])
            h = F.conv1d(F.gelu(ln(h, b["ln2"])), sd[b["conv"] + ".weight"], sd[b["conv"] + ".bias"], dilation=d, padding=2 * d)
            x = x + F.conv1d(F.gelu(ln(h, b["ln3"])), sd[b["pff2"] + ".weight"], sd[b["pff2"] + ".bias"])
        x = F.layer_norm(x.transpose(1, 2), (x.shape[1],), sd["last_norm.weight"], sd["last_norm.bias"], 1e-5).transpose(1, 2)
        return torch.log_softmax(F.conv1d(x, sd["decoder.conv.weight"], sd["decoder.conv.bias"]), dim=1)

    with torch.no_grad():
        forward()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            forward()
        torch.cuda.synchronize()
    return n / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=56)
    ap.add_argument("--d_model", type=int, default=1280)
    ap.add_argument("--L", type=int, default=286)
    ap.add_argument("--mutants", type=int, default=4996)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--iters", type=int, default=5, help="launches per kernel timing")
    ap.add_argument("--max_rows", type=int, default=0)
    ap.add_argument("--torch_forwards", type=int, default=8, help="forwards of the torch baseline (0: skip it)")
    ap.add_argument("--torch_only", action="store_true", help="(internal) run the torch baseline alone and print its JSON")
    a = ap.parse_args()
    n_multi = a.mutants // 4
    target, muts, _ = synthetic.random_assay(3, a.L, a.mutants - n_multi, n_multi)
    ck = carp.random_checkpoint(1, a.d_model, a.layers, False, name="carp_640M_shaped")
    if a.torch_only:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("the torch baseline needs the GPU")
        print(json.dumps({"forwards_per_sec": torch_forwards_per_sec(ck, carp.tokenize(target), a.torch_forwards)}))
        return
    base = None
    if a.torch_forwards > 0:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--torch_only", "--layers", str(a.layers), "--d_model", str(a.d_model),
                            "--L", str(a.L), "--mutants", str(a.mutants), "--torch_forwards", str(a.torch_forwards)],
                           capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise RuntimeError(f"torch baseline failed:\n{r.stderr[-2000:]}")
        base = json.loads(r.stdout.strip().splitlines()[-1])
    lib = _lib.load()
    D, M = a.d_model, a.L * a.L
    flop_token_layer = 2.0 * (2 * D * D + 5 * D * D)
    res = {"config": {"d_model": D, "layers": a.layers, "L": a.L, "mutants": len(muts), "flop_per_token_and_layer": flop_token_layer}}

    # the kernels alone
    ms = C.c_double()
    conv_flop = 2.0 * M * D * 5 * D
    res["conv_alone"] = {}
    for d in (1, 128):
        _lib.check(lib.pgmi_bench_dilated_conv(0, M, a.L, D, 5, d, a.iters, C.byref(ms)))
        res["conv_alone"][f"dilation_{d}"] = {"ms": ms.value, "tflops": conv_flop / ms.value / 1e9}
    _lib.check(lib.pgmi_bench_gemm(0, _lib.PREC_F16X3, M, D, 5 * D, 0, 0, 0, a.iters, C.byref(ms)))
    res["dense_gemm_same_flops"] = {"M": M, "N": D, "K": 5 * D, "ms": ms.value, "tflops": conv_flop / ms.value / 1e9}
    for d in (1, 128):
        res["conv_alone"][f"dilation_{d}"]["ratio_to_dense_gemm"] = res["conv_alone"][f"dilation_{d}"]["tflops"] / res["dense_gemm_same_flops"]["tflops"]

    # the assay
    model = carp.CarpModel(ck, max_rows=a.max_rows)
    positions = sorted({i for m in muts for i, _, _ in carp.parse_mutant(m, target)})
    carp.masked_marginal_scores(model, target, muts[:64])                  # warm-up: code objects, workspace
    times = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        scores = carp.masked_marginal_scores(model, target, muts)
        times.append(time.perf_counter() - t0)
    best = min(times)
    fl = len(positions) * a.L * a.layers * flop_token_layer
    res["masked_marginals"] = {"sec": times, "ms_per_assay": best * 1e3, "mutants_per_sec": len(muts) / best, "positions_run": len(positions),
                               "tflops_executed": fl / best / 1e12, "finite": bool(np.isfinite(scores).all())}
    ph = model.profile_handle()
    _lib.check(lib.pgmi_profile_reset(ph))
    _lib.check(lib.pgmi_profile_enable(ph, 1))
    t0 = time.perf_counter()
    carp.masked_marginal_scores(model, target, muts)
    wall = time.perf_counter() - t0
    _lib.check(lib.pgmi_profile_enable(ph, 0))
    split = {}
    for cname, k in CLASSES.items():
        t, n, f, by = C.c_double(), C.c_int64(), C.c_double(), C.c_double()
        _lib.check(lib.pgmi_profile_get(ph, k, C.byref(t), C.byref(n), C.byref(f), C.byref(by)))
        split[cname] = {"ms": t.value, "launches": n.value, "tflops": f.value / t.value / 1e9 if t.value > 0 and f.value > 0 else None}
    dev = sum(v["ms"] for v in split.values())
    res["masked_marginals"]["profiled"] = {"wall_sec": wall, "device_sec": dev / 1e3, "classes": split,
                                           "conv_share_of_device_time": split["dilated_conv"]["ms"] / dev,
                                           "gaps_sec_vs_unprofiled_best": best - dev / 1e3}
    model.close()
    if base:
        res["torch_fp32_batch1"] = {"forwards_per_sec": base["forwards_per_sec"], "library_forwards_per_sec": len(positions) / best}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
