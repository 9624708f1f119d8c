#!/usr/bin/env python
"""UniRep scoring at a BLAT-shaped assay: H = 1900, L = 286, 4 996 seeded single and multiple mutants (synthetic.random_assay), seeded
random weights (unirep.random_arrays, gain 1.5).

    python scripts/bench_unirep.py [--mutants 4996] [--L 286] [--H 1900] [--precision f16x3] [--repeats 3] [--torch_seqs 64]

Times (host clock around calls that end in a device synchronise; one warm-up of every timed shape first) the target's pass
(pgmi_unirep_set_target) and pgmi_unirep_sequence_nll over all mutants, with the prefix start and from scratch, `--repeats` times each,
alternating; checks that both give the same bits and that the executed row-steps equal the planner's count.  A second, profiled pass of
each mode splits the device time per kernel class (pgmi_profile_* on pgmi_unirep_profile_model's handle: HIP events on the stream, so
the classes do not overlap); "gaps" is the unprofiled wall time minus that sum: launch gaps, the host's planning and the copies.  The
baseline is the fp32 torch restatement of the reference's loop on the same GPU (tests/unirep_ref.py's arithmetic as torch ops, every
sequence from its first token): batch 8 as the reference's launcher runs it, and one batch of all mutants; it runs in a child process
of its own before this one opens the GPU (torch brings its own HIP runtime).  Prints one JSON line.

Arithmetic: a row-step is 2 x 1900 x (1900 + 7600) = 36.1 MFLOP."""
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

from proteingym_amd import _lib, synthetic, unirep as ur  # noqa: E402
from proteingym_amd.causal_lm import get_mutated_sequence  # noqa: E402

CLASSES = {"product1_h_wmh": 5, "multiply_Tmx": 1, "product2_m_wh": 6, "gates": 3, "head": 7, "init": 0, "score": 8}


def torch_baseline(arrays, seqs, batch, device="cuda"):
    """seconds for ``seqs`` through the fp32 torch restatement of babbler1900's loop in batches of ``batch`` (unirep.py:118-132, :396-408)"""
    import torch
    f = ur.fold(arrays)                       # the same normalised weights, fp32 on the device; the loop itself is the reference's
    t = lambda a: torch.as_tensor(a, dtype=torch.float32, device=device)
    E = t(arrays["embed"].astype(np.float64))
    wn = lambda w, g: w.astype(np.float64) / np.sqrt(np.maximum((w.astype(np.float64) ** 2).sum(0, keepdims=True), 1e-12)) * g
    wx, wmx, b = t(wn(arrays["wx"], arrays["gx"])), t(wn(arrays["wmx"], arrays["gmx"])), t(arrays["b"])
    wh, wmh, Wd, bd = t(f["wh"]), t(f["wmh"]), t(f["dense_w"]), t(f["dense_b"])
    toks = np.stack([ur.format_seq(s) for s in seqs])
    H = wmh.shape[0]
    out = []

    def run(tk):
        x, y = torch.as_tensor(tk[:, :-1].astype(np.int64), device=device), torch.as_tensor(tk[:, 1:].astype(np.int64), device=device)
        c = torch.zeros(len(tk), H, device=device)
        h = torch.zeros(len(tk), H, device=device)
        nll = torch.zeros(len(tk), device=device)
        for s in range(x.shape[1]):
            inp = E[x[:, s]]
            m = (inp @ wmx) * (h @ wmh)
            z = inp @ wx + m @ wh + b
            i, fg, o, u = z.split(H, dim=1)
            c = torch.sigmoid(fg) * c + torch.sigmoid(i) * torch.tanh(u)
            h = torch.sigmoid(o) * torch.tanh(c)
            lp = torch.log_softmax(h @ Wd + bd, -1)
            nll -= lp.gather(1, (y[:, s] - 1)[:, None])[:, 0]
        return (nll / x.shape[1]).cpu().numpy()

    with torch.no_grad():
        run(toks[:batch])                                             # warm-up of the shape
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(0, len(toks), batch):
            out.append(run(toks[i:i + batch]))
        torch.cuda.synchronize()
        sec = time.perf_counter() - t0
    return sec, np.concatenate(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mutants", type=int, default=4996)
    ap.add_argument("--L", type=int, default=286)
    ap.add_argument("--H", type=int, default=1900)
    ap.add_argument("--precision", default="f16x3", choices=["f16x3", "fp32"])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--torch_seqs", type=int, default=64, help="sequences of the batch-8 torch baseline (0: skip both baselines)")
    ap.add_argument("--max_rows", type=int, default=0)
    ap.add_argument("--torch_only", action="store_true", help="(internal) run the torch baselines alone and print their JSON")
    a = ap.parse_args()
    n_multi = a.mutants // 4
    target, muts, _ = synthetic.random_assay(3, a.L, a.mutants - n_multi, n_multi)
    seqs = [get_mutated_sequence(target, m) for m in muts]
    arrays = ur.random_arrays(1, a.H, gain=1.5)
    if a.torch_only:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("the torch baseline needs the GPU")
        n8 = min(a.torch_seqs, len(seqs))
        sec8, v8 = torch_baseline(arrays, seqs[:n8], 8)
        secN, vN = torch_baseline(arrays, seqs, len(seqs))
        print(json.dumps({"n8": n8, "sec8": sec8, "v8": v8.tolist(), "secN": secN, "vN": vN.tolist()}))
        return
    base = None
    if a.torch_seqs > 0:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--torch_only", "--L", str(a.L), "--mutants", str(a.mutants),
                            "--H", str(a.H), "--torch_seqs", str(a.torch_seqs)], capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise RuntimeError(f"torch baseline failed:\n{r.stderr[-2000:]}")
        base = json.loads(r.stdout.strip().splitlines()[-1])
    lib = _lib.load()
    model = ur.UniRepModel(arrays, precision=a.precision, max_rows=a.max_rows)
    rows = [ur.format_seq(s) for s in seqs]
    plans = {False: ur.plan(rows, ur.format_seq(target), model.max_rows), True: ur.plan(rows, None, model.max_rows)}
    flop_step = 2.0 * a.H * 5 * a.H

    t0 = time.perf_counter()
    model.set_target(target)
    first_target = time.perf_counter() - t0
    model.nll(seqs[:64])                                              # warm-up: code objects, workspace
    model.nll(seqs, from_scratch=True)
    t0 = time.perf_counter()
    model.set_target(target)
    target_sec = time.perf_counter() - t0
    res = {"config": {"H": a.H, "L": a.L, "mutants": len(seqs), "precision": a.precision, "rows_per_chunk": model.max_rows,
                      "flop_per_row_step": flop_step},
           "set_target_sec": target_sec, "set_target_first_call_sec": first_target}
    times, scores, steps = {False: [], True: []}, {}, {}
    for _ in range(a.repeats):
        for scratch in (False, True):
            t0 = time.perf_counter()
            scores[scratch] = model.nll(seqs, from_scratch=scratch)
            times[scratch].append(time.perf_counter() - t0)
            steps[scratch] = model.last_row_steps
    for scratch, name in ((False, "prefix_start"), (True, "from_scratch")):
        best = min(times[scratch])
        res[name] = {"sec": times[scratch], "mutants_per_sec": len(seqs) / best, "row_steps": steps[scratch],
                     "planner_row_steps": plans[scratch].row_steps, "tflops_executed": steps[scratch] * flop_step / best / 1e12}
        assert steps[scratch] == plans[scratch].row_steps, (steps[scratch], plans[scratch].row_steps)
    res["same_bits"] = bool(np.array_equal(scores[False], scores[True]))
    assert res["same_bits"]

    ph = model.profile_handle()
    for scratch, name in ((False, "prefix_start"), (True, "from_scratch")):
        _lib.check(lib.pgmi_profile_reset(ph))
        _lib.check(lib.pgmi_profile_enable(ph, 1))
        t0 = time.perf_counter()
        model.nll(seqs, from_scratch=scratch)
        wall = time.perf_counter() - t0
        _lib.check(lib.pgmi_profile_enable(ph, 0))
        split = {}
        for cname, k in CLASSES.items():
            ms, n, fl, by = C.c_double(), C.c_int64(), C.c_double(), C.c_double()
            _lib.check(lib.pgmi_profile_get(ph, k, C.byref(ms), C.byref(n), C.byref(fl), C.byref(by)))
            split[cname] = {"ms": ms.value, "launches": n.value}
        dev = sum(v["ms"] for v in split.values()) / 1e3
        res[name]["profiled"] = {"wall_sec": wall, "device_sec": dev, "classes": split,
                                 "gaps_sec_vs_unprofiled_best": min(times[scratch]) - dev}
    model.close()

    if base:
        n8, v8, vN = base["n8"], np.array(base["v8"]), np.array(base["vN"])
        res["torch_fp32_batch8"] = {"sequences": n8, "sec": base["sec8"], "mutants_per_sec": n8 / base["sec8"],
                                    "max_abs_diff_vs_library": float(np.abs(v8 - scores[True][:n8]).max())}
        res["torch_fp32_one_batch"] = {"sequences": len(seqs), "sec": base["secN"], "mutants_per_sec": len(seqs) / base["secN"],
                                       "max_abs_diff_vs_library": float(np.abs(vN - scores[True]).max())}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
