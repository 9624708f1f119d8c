#!/usr/bin/env python
"""ProteinMPNN scoring at a BLAT-shaped assay: L = 286 residues (a seeded random-walk backbone, 4 residues masked), K = 48 neighbours,
4 996 seeded single and double mutants, seeded random weights.

    python scripts/bench_mpnn.py [--mutants 4996] [--L 286] [--torch_mutants 20] [--max_rows 0]

Times one pgmi_mpnn_set_structure (graph, features, encoder, hoisted tables) and pgmi_mpnn_scores over all mutants (host clock around the
calls, which end in a device synchronise; the rank computation on the host is inside).  A second, profiled run splits the decoder time
per kernel class (pgmi_profile_* on pgmi_mpnn_profile_model's handle; HIP events, so the classes do not overlap) and gives the edge
kernel's share of the 157.3 TFLOP/s fp32 MFMA peak, counted on the 16-row tiles it issues.  The baseline is the fp32 torch restatement
of the reference's loop on the same GPU: featuriser, encoder and decoder per mutant, batch 1 (tests/mpnn_ref.py's arithmetic moved to
the device by importing it; --torch_mutants of them, after two warm-up forwards, in a child process of its own).  Prints one JSON line.

Derived cost per mutant: 3 x 286 x 48 x 128 x 128 x 2 = 1.35 GFLOP in the W2 GEMMs, about 0.3 GFLOP on the node side,
3 x 286 x 48 x 256 = 1.05e7 erf-GELUs."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

from proteingym_amd import _lib, mpnn  # noqa: E402

CLASSES = {"edge_kernel": 3, "w3_gemm": 4, "layernorm": 1, "ffn_in": 5, "ffn_out": 6, "next_AP_gemm": 2, "head": 7, "score": 8}
PEAK_F32_MFMA = 157.3e12


def torch_baseline(sd, case, S, rank, n, device):
    """seconds per mutant of the reference's loop restated in fp32 torch on ``device``: everything per mutant, batch 1"""
    import torch
    import mpnn_ref
    w = mpnn_ref._t(sd, torch.float32, device)
    X, mask = (torch.as_tensor(case[k], dtype=torch.float32, device=device) for k in ("X", "mask"))
    ridx, chain = (torch.as_tensor(case[k], dtype=torch.long, device=device) for k in ("residue_idx", "chain_encoding"))
    St, Rt = torch.as_tensor(S.astype(np.int64), device=device), torch.as_tensor(rank.astype(np.int64), device=device)

    def one(b):
        E, E_idx = mpnn_ref.features(w, X, mask, ridx, chain, 48)
        h_V, h_E = mpnn_ref.encoder(w, E, E_idx, mask)
        lp = mpnn_ref.decoder(w, h_V, h_E, E_idx, mask, St[b:b + 1], Rt[b:b + 1])
        nll = -lp[0].gather(1, St[b][:, None])[:, 0]
        return -(nll * mask).sum() / mask.sum()

    with torch.no_grad():
        for b in range(n, n + 2):                                   # warm-up on mutants outside the timed ones
            one(b).item()
        t0 = time.perf_counter()
        vals = [one(b).item() for b in range(n)]
        sec = (time.perf_counter() - t0) / n
    return sec, vals


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mutants", type=int, default=4996)
    ap.add_argument("--L", type=int, default=286)
    ap.add_argument("--torch_mutants", type=int, default=20)
    ap.add_argument("--max_rows", type=int, default=0, help="(mutant, residue) rows per device chunk; 0: the default 32768")
    ap.add_argument("--torch_only", action="store_true", help="(internal) run the torch baseline alone and print its JSON")
    a = ap.parse_args()
    import mpnn_cases as mc
    case = mc.make_case(a.L, seed=9, n_masked=4)
    rng = np.random.default_rng(4)
    S = np.tile(case["S"], (a.mutants, 1)).astype(np.uint8)
    for m in range(a.mutants):
        pos = rng.choice(a.L, size=1 + m % 2, replace=False)
        S[m, pos] = (S[m, pos] + rng.integers(1, 20, size=len(pos))) % 20
    randn = rng.standard_normal((a.mutants, a.L)).astype(np.float32)
    sd = mpnn.random_state_dict(7)
    if a.torch_only:
        import torch
        n = a.torch_mutants
        sec, vals = torch_baseline(sd, case, S[:n + 2], mpnn.rank_from_randn(randn[:n + 2], case["mask"]), n, torch.device("cuda:0"))
        print(json.dumps({"sec": sec, "vals": vals}))
        return
    if a.torch_mutants > 0:
        # the baseline runs in a child process of its own, before this one opens the GPU: torch brings its own HIP runtime, and the
        # two do not share a process here; it also has the GPU to itself while it is timed
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--torch_only", "--L", str(a.L), "--mutants", str(a.mutants),
                            "--torch_mutants", str(a.torch_mutants)], capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise RuntimeError(f"torch baseline failed:\n{r.stderr[-2000:]}")
        base = json.loads(r.stdout.strip().splitlines()[-1])
    lib = _lib.load()
    if lib.pgmi_device_count() <= 0:
        raise RuntimeError("bench_mpnn.py needs a GPU: libpgmi has no CPU fallback")
    model = mpnn.MpnnModel(mpnn.blob_from_state_dict(sd), num_edges=48)
    _lib.check(lib.pgmi_set_option(b"mpnn_max_rows", a.max_rows))
    model.set_structure(case["X"], case["mask"], case["residue_idx"], case["chain_encoding"])
    model.scores(S[:256], randn=randn[:256])                                        # warm-up
    t0 = time.perf_counter()
    model.set_structure(case["X"], case["mask"], case["residue_idx"], case["chain_encoding"])
    t_struct = time.perf_counter() - t0
    t0 = time.perf_counter()
    scores = model.scores(S, randn=randn)
    wall = time.perf_counter() - t0
    h = model.profile_handle()
    _lib.check(lib.pgmi_profile_enable(h, 1))
    _lib.check(lib.pgmi_profile_reset(h))
    model.scores(S, randn=randn)
    split, total_ms = {}, 0.0
    for name, k in CLASSES.items():
        ms, n, fl = C.c_double(), C.c_int64(), C.c_double()
        _lib.check(lib.pgmi_profile_get(h, k, C.byref(ms), C.byref(n), C.byref(fl), None))
        split[name] = {"ms_per_1000_mutants": 1e3 * ms.value / a.mutants, "launches": n.value,
                       "tflops": fl.value / ms.value / 1e9 if ms.value > 0 and fl.value > 0 else None}
        total_ms += ms.value
    _lib.check(lib.pgmi_profile_enable(h, 0))
    model.close()
    edge = split["edge_kernel"]
    K = min(48, a.L)
    out = {"bench": "mpnn", "L": a.L, "K": K, "mutants": a.mutants, "max_rows": a.max_rows, "set_structure_ms": 1e3 * t_struct,
           "scores_seconds": wall, "mutants_per_s": a.mutants / wall, "kernel_ms_total_per_1000_mutants": 1e3 * total_ms / a.mutants,
           "split": split, "edge_kernel_share_of_fp32_mfma_peak": edge["tflops"] * 1e12 / PEAK_F32_MFMA if edge["tflops"] else None,
           "derived_gflop_per_mutant": {"w2": 3 * a.L * K * 128 * 128 * 2 / 1e9, "node_side": 3 * a.L * (128 * 128 + 2 * 128 * 512 + 256 * 128) * 2 / 1e9},
           "derived_gelus_per_mutant": 3 * a.L * K * 256, "score_first": float(scores[0])}
    if a.torch_mutants > 0:
        out.update(torch_fp32_same_gpu_seconds_per_mutant=base["sec"], torch_fp32_same_gpu_mutants_per_s=1.0 / base["sec"],
                   speedup_vs_torch_same_gpu=(a.mutants / wall) * base["sec"],
                   max_abs_diff_vs_torch_on_its_mutants=float(np.abs(np.array(base["vals"]) - scores[:a.torch_mutants]).max()))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
