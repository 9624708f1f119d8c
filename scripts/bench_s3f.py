#!/usr/bin/env python
"""S3F scoring at a BLAT-shaped assay: L = 286 residues on bench_s2f.py's compact toy backbone, a seeded synthetic surface of --points
points around it, one masked copy per position for the first --sets positions, seeded ESM-2-650M-shaped, GVP and surface weights.

    python scripts/bench_s3f.py --points 5000 [--sets 32] [--batch_size 2] [--torch_sets 3] [--out bench_s3f.json]

Times pgmi_s3f_set_structure once and pgmi_s3f_set_logprobs over the sets (host clock around the calls, which end in a device
synchronise; best of --repeats after one warm-up call).  A second, profiled run splits the time between ESM2 (the ESM2 model's view),
the residue GNN (view 0) and the surface half (view 1: the surface MLP, the surface message kernel, the rest); HIP events on one
stream, so the classes do not overlap.  The surface message kernel is reported in ns per edge and layer, next to s2f_message_kernel's
figure in profiles/s2f/README.md, and its MFMA FLOPs (the two 272 -> 256 products and the three 256 -> 16 gates per edge row) as time
at the 157.3 TFLOP/s fp32 matrix peak.  The baseline is the fp32 torch restatement (tests/s3f_ref.py) on the same GPU, one masked
copy at a time with both graphs and their edge features built once outside the timed window; the k-NN lists are the device's (the
restatement's brute force is quadratic in memory).  It runs in a child process of its own.  Prints one JSON line."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import bench_s2f  # noqa: E402
from proteingym_amd import s2f, s3f, synthetic  # noqa: E402

ESM_CFG = dict(synthetic.ESM2_650M)
PEAK_F32_MATRIX = 157.3e12
LAYERS = 5


def surface(pos, n, seed=11):
    """n points 3 .. 7 A from randomly chosen C-alpha atoms, seeded 42-wide features."""
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    pts = pos[rng.integers(0, len(pos), n)].astype(np.float64) + u * rng.uniform(3.0, 7.0, (n, 1))
    return pts.astype(np.float32), rng.standard_normal((n, 42)).astype(np.float32)


def state_dict():
    return s3f.random_state_dict(5, ESM_CFG, esm_blob=synthetic.random_weights(ESM_CFG, seed=3))


def torch_baseline(L, points, n, groups, lists):
    import torch
    import s2f_ref
    import s3f_ref
    seq, pos, plddt, _, _ = bench_s2f.case(L)
    pts, feat = surface(pos, points)
    g = np.load(lists)
    W = s2f_ref.tensors(state_dict(), torch.float32, "cuda")
    like = W["linear.weight"]
    base = [0] + [s2f_ref.ESM_TOKENS.index(a) for a in seq] + [2]
    cols = [s2f_ref.ESM_TOKENS.index(a) for a in s2f_ref.ORDER]
    with torch.no_grad():
        graph = s2f_ref.structure_graph(W, pos, like)
        edges = s3f_ref.surface_edges(g["src"].astype(np.int64)).to("cuda")
        es, ev = s3f_ref.surface_edge_features(W, torch.as_tensor(pts).to(like), edges)
        st = dict(src=g["src"], res=g["res"].astype(np.int64), res_dist=g["res_dist"], edges=edges, e_s=es, e_v=ev)

        def run(i):
            tok = list(base)
            tok[1 + i] = s2f_ref.ESM_TOKENS.index("<mask>")
            rep, logits = s2f_ref.esm2(W, tok, ESM_CFG["heads"], ESM_CFG["layers"])
            out = s3f_ref.surf_gvp(W, pos, pts, feat, [rep[1:-1]], LAYERS, graph, st)
            return s2f_ref.head_logprobs(W, out["node_feature"][0], logits[1:-1][:, cols], plddt)[i].cpu().numpy()

        run(L - 1)
        torch.cuda.synchronize()
        secs = []
        for _ in range(groups):
            t0 = time.perf_counter()
            rows = [run(i) for i in range(n)]
            torch.cuda.synchronize()
            secs.append((time.perf_counter() - t0) / n)
    return dict(torch_sec_per_set=float(np.median(secs)), torch_sec_per_set_groups=secs, torch_rows=[r.tolist() for r in rows])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=286)
    ap.add_argument("--points", type=int, default=5000)
    ap.add_argument("--sets", type=int, default=32)
    ap.add_argument("--batch_size", type=int, default=2, help="the loader batch that shares a pooled row (s3f.yaml: 2)")
    ap.add_argument("--torch_sets", type=int, default=3)
    ap.add_argument("--torch_groups", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--precision", default="f16x3")
    ap.add_argument("--out", default="")
    ap.add_argument("--torch_only", default="", help="(child process) the npz of the device's k-NN lists")
    args = ap.parse_args()
    L, ns = args.L, args.points
    if args.torch_only:
        print(json.dumps(torch_baseline(L, ns, args.torch_sets, args.torch_groups, args.torch_only)))
        return
    seq, pos, plddt, _, _ = bench_s2f.case(L)
    pts, feat = surface(pos, ns)
    n = min(args.sets, L)
    set_off, set_pos = np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32)
    pools = s3f.pool_groups(n, args.batch_size)
    model = s3f.from_state_dict(state_dict(), ESM_CFG, precision=args.precision)
    model.set_structure(pos, plddt, pts, feat)                  # warm-up: allocations
    t0 = time.perf_counter()
    model.set_structure(pos, plddt, pts, feat)
    t_struct = time.perf_counter() - t0
    g = model.graph()
    E = len(g["src"])
    tok = s2f.tokenize(seq)
    model.set_logprobs(tok, set_off, set_pos, pools)            # warm-up: workspaces
    times = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        model.set_logprobs(tok, set_off, set_pos, pools)
        times.append(time.perf_counter() - t0)
    sec = min(times)
    table = model.set_logprobs(tok, set_off, set_pos)           # batch_size 1: what the torch baseline computes
    views = (model.esm, model.profile_view(0), model.profile_view(1))
    for v in views:
        v.profile_enable(True)
        v.profile_reset()
    model.set_logprobs(tok, set_off, set_pos, pools)
    esm_prof, res_prof, surf_prof = (v.profile() for v in views)
    for v in views:
        v.profile_enable(False)
    ms = lambda prof, keys=None: sum(c["ms"] for k, c in prof.items() if k != "embed" and (keys is None or k in keys))
    esm_ms, res_ms, surf_ms = sum(c["ms"] for c in esm_prof.values()), ms(res_prof), ms(surf_prof)      # "embed" of a GNN view: the structure pass
    mlp_ms, msg_ms = ms(surf_prof, ("gemm_out",)), ms(surf_prof, ("attention",))
    total = esm_ms + res_ms + surf_ms
    rows = n * 16.0 * ns * LAYERS                               # edge rows through the surface message kernel
    mfma_flops = rows * 2.0 * 256 * (2 * 272 + 3 * 16)
    out = dict(L=L, points=ns, residue_edges=E, surface_edges=16 * ns, sets=n, batch_size=args.batch_size, mutants=19 * n,
               precision=args.precision, structure_sec=t_struct, sec_all_sets=sec, sec_runs=times, sets_per_sec=n / sec,
               mutants_per_sec=19 * n / sec, profiled_ms=dict(esm2=esm_ms, residue_gnn=res_ms, surface_mlp=mlp_ms, surface_message=msg_ms,
                                                              surface_rest=surf_ms - mlp_ms - msg_ms),
               shares=dict(esm2=esm_ms / total, residue_gnn=res_ms / total, surface_mlp=mlp_ms / total, surface_message=msg_ms / total,
                           surface_rest=(surf_ms - mlp_ms - msg_ms) / total),
               surface_message_ns_per_edge_layer=msg_ms * 1e6 / rows, s2f_message_ns_per_edge_layer=7.2,
               surface_message_mfma_flops=mfma_flops, surface_message_mfma_ms_at_peak=mfma_flops / PEAK_F32_MATRIX * 1e3,
               surface_classes_ms={k: round(c["ms"], 3) for k, c in surf_prof.items() if c["launches"]},
               residue_classes_ms={k: round(c["ms"], 3) for k, c in res_prof.items() if c["launches"]},
               esm2_classes_ms={k: round(c["ms"], 3) for k, c in esm_prof.items() if c["launches"]})
    model.close()
    model.esm.close()
    if args.torch_sets > 0:
        with tempfile.TemporaryDirectory() as tmp:
            lists = os.path.join(tmp, "lists.npz")
            np.savez(lists, src=g["surf_src"], res=g["surf_res"], res_dist=g["surf_res_dist"])
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--torch_only", lists, "--L", str(L), "--points", str(ns),
                                "--torch_sets", str(args.torch_sets), "--torch_groups", str(args.torch_groups)],
                               capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise RuntimeError(f"torch baseline failed:\n{r.stderr[-2000:]}")
        base = json.loads(r.stdout.strip().splitlines()[-1])
        trows = np.array(base.pop("torch_rows"))
        out.update(base)
        out["torch_sets_per_sec"] = 1.0 / base["torch_sec_per_set"]
        out["speedup_vs_torch_fp32"] = base["torch_sec_per_set"] / (sec / n)
        out["max_abs_diff_vs_torch_fp32_rows"] = float(np.abs(trows - table[:args.torch_sets]).max())
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
