#!/usr/bin/env python
"""ProtSSN's EGNN at a BLAT-shaped structure: L = 286 residues on the seeded serpentine backbone, seeded checkpoints (Xavier-normal
times 0.5) of the shapes k30_h1280 and k20_h512 on seeded unit-variance residue rows of width 1280.

    python scripts/bench_protssn.py [--L 286] [--models k30_h1280 k20_h512] [--precision f16x3] [--out bench_protssn.json]

Per checkpoint: the time of pgmi_protssn_set_graph and of pgmi_protssn_forward (host clock around the calls, which end in a device
synchronise; set_graph per call, forward as --repeats groups of --reps calls; every group listed, the best reported, after one
warm-up call), a profiled forward split by kernel class (pgmi_protssn_profile_model's view; HIP events on one stream, so the classes do not overlap), two FLOP counts -- `flop_algorithmic`,
what this path computes with the per-node tables, and `flop_reference_unsplit`, the reference's 2654-wide first Linear on every edge --
and the W2 product's profiled time against the dense f16x3 GEMM of the same shape (pgmi_bench_gemm, M = E rows, at most one chunk's
worth per launch as the forward launches it).  The baseline is the fp32 torch restatement (tests/protssn_ref.py, float32) on the same
GPU, in a child process of its own: the graph is built and uploaded outside the timed window, two warm-up forwards, then --torch_groups
groups of --torch_reps forwards, each group between device synchronises.  Prints one JSON line."""
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

import protssn_ref as R  # noqa: E402
from proteingym_amd import _lib, protssn  # noqa: E402

D = protssn.NODE_IN
NORM = os.path.join(ROOT, "tests", "golden", "ProtSSN_toy")


def case(L, k):
    n, ca, c = R.toy_backbone(R.serpentine(L, seed=1), seed=2)
    x = np.random.default_rng(13).standard_normal((L, D)).astype(np.float32)
    return protssn.build_graph(n, ca, c, k, protssn.load_norm(k, norm_dir=NORM)), x


def state_dict(h):
    return protssn.random_state_dict(5, D, h, gain=0.5)


def flops(L, E, h):
    d = protssn.dims(D, h)
    node = 2.0 * L * (2 * D * (D + h) + D * 2 * D)
    alg = 2.0 * L * D * 2 * d["Hh"] + 2.0 * E * 94 * d["Hh"] + 2.0 * E * d["Hh"] * h + node
    ref = 2.0 * E * (2 * D + 94) * d["Hh"] + 2.0 * E * d["Hh"] * h + node
    return 6 * alg + 2.0 * L * D * 20, 6 * ref + 2.0 * L * D * 20


def torch_baseline(L, k, h, reps, groups):
    import torch
    (pos, centre, nb, ea), x = case(L, k)
    W = R.tensors(state_dict(h), torch.float32, "cuda")
    dev = lambda a, t: torch.as_tensor(np.array(a)).to(device="cuda", dtype=t)
    args = (dev(x, torch.float32), dev(pos, torch.float32), dev(centre, torch.long), dev(nb, torch.long), dev(ea, torch.float32))

    def run():
        xx, p, c, n, e = args
        with torch.no_grad():
            return R.forward(None, xx, p, c, n, e, dtype=torch.float32, device="cuda", W=W)[0]
    for _ in range(2):
        lp = run()
    torch.cuda.synchronize()
    secs = []
    for _ in range(groups):
        t0 = time.perf_counter()
        for _ in range(reps):
            lp = run()
        torch.cuda.synchronize()
        secs.append((time.perf_counter() - t0) / reps)
    return dict(torch_forward_sec=float(np.median(secs)), torch_forward_sec_groups=secs, torch_lp=lp.cpu().numpy().tolist())


def bench_model(name, L, precision, repeats, reps, iters, torch_reps, torch_groups):
    k, h = protssn.parse_model_name(name)
    (pos, centre, nb, ea), x = case(L, k)
    E = len(centre)
    model = protssn.from_state_dict(state_dict(h), D, h, precision=precision)
    model.set_graph(pos, centre, nb, ea)                    # warm-up: workspaces
    t_graph = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        model.set_graph(pos, centre, nb, ea)
        t_graph.append(time.perf_counter() - t0)
    lp = model.forward(x)
    t_fwd = []
    for _ in range(repeats):                                # groups of `reps` forwards: one forward is a few milliseconds
        t0 = time.perf_counter()
        for _ in range(reps):
            lp = model.forward(x)
        t_fwd.append((time.perf_counter() - t0) / reps)
    view = model.profile_view()
    view.profile_enable(True)
    view.profile_reset()
    model.forward(x)
    prof = view.profile()
    view.profile_enable(False)
    model.close()
    d = protssn.dims(D, h)
    chunk = min(E, 8192)
    ms = C.c_double()
    _lib.check(_lib.load().pgmi_bench_gemm(0, _lib.PRECISIONS[precision], chunk, d["hp"], d["Hp"], 0, 0, 0, iters, C.byref(ms)))
    dense_ms = ms.value * E / chunk * 6                     # the same rows, six layers
    alg, ref = flops(L, E, h)
    sec = min(t_fwd)
    out = dict(model=name, L=L, edges=E, max_in_degree=int(np.bincount(nb, minlength=L).max()), min_in_degree=int(np.bincount(nb, minlength=L).min()),
               precision=precision, set_graph_sec=min(t_graph), set_graph_sec_runs=t_graph, forward_sec=sec, forward_sec_runs=t_fwd,
               flop_algorithmic=alg, flop_reference_unsplit=ref, tflops_algorithmic=alg / sec / 1e12,
               classes_ms={c: round(v["ms"], 3) for c, v in prof.items() if v["launches"]},
               w2_ms=prof["gemm_out"]["ms"], w2_dense_gemm_ms=dense_ms, w2_dense_share=dense_ms / prof["gemm_out"]["ms"],
               edge_share_bytes_per_chunk=chunk * d["Hp"] * 4)
    if torch_reps > 0:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--torch_only", name, "--L", str(L), "--torch_reps", str(torch_reps),
                            "--torch_groups", str(torch_groups)], capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise RuntimeError(f"torch baseline failed:\n{r.stderr[-2000:]}")
        base = json.loads(r.stdout.strip().splitlines()[-1])
        out["max_abs_diff_vs_torch_fp32"] = float(np.abs(np.array(base.pop("torch_lp")) - lp).max())
        out.update(base)
        out["speedup_vs_torch_fp32"] = base["torch_forward_sec"] / sec
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=286)
    ap.add_argument("--models", nargs="+", default=["k30_h1280", "k20_h512"])
    ap.add_argument("--precision", default="f16x3")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--torch_reps", type=int, default=20)
    ap.add_argument("--torch_groups", type=int, default=5)
    ap.add_argument("--torch_only", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.torch_only:
        k, h = protssn.parse_model_name(args.torch_only)
        print(json.dumps(torch_baseline(args.L, k, h, args.torch_reps, args.torch_groups)))
        return
    out = dict(models=[bench_model(m, args.L, args.precision, args.repeats, args.reps, args.iters, args.torch_reps, args.torch_groups) for m in args.models])
    out["forward_faster_than_torch_fp32"] = all(m.get("speedup_vs_torch_fp32", 0) > 1 for m in out["models"])
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if args.torch_reps > 0 and not out["forward_faster_than_torch_fp32"]:
        sys.exit("the device forward is not faster than the fp32 torch restatement")


if __name__ == "__main__":
    main()
