#!/usr/bin/env python
"""ProSST structure tokens at a BLAT-sized protein (L = 286) and a longer one: seeded compact backbones (bench_s2f.py's serpentine
lattice, 5 x 5 in cross-section at 4.6 A, with N, C, O at seeded offsets), seeded AutoGraphEncoder weights, seeded codebooks.

    python scripts/bench_prosst_tokens.py [--L 286 1000] [--K 2048 20] [--repeats 3] [--torch 1] [--out bench_prosst_tokens.json]

Per length: E_global, the node copies and the subgraph edges; the time per structure = pgmi_prosst_set_structure (the host graph pass
in float64 and the device structure pass) + pgmi_prosst_embed + one pgmi_prosst_assign per K, each timed with the host clock around
calls that end in a device synchronise (one warm-up, then --repeats runs, every one listed, the best reported); pgmi_prosst_embed with
and without the layer-0 sharing (pgmi_set_option("prosst_share_layer0")); a profiled run split by kernel class (HIP events on one
stream, so the classes do not overlap).  The yardstick, on the same GPU and in a child process of its own: the fp32 torch
restatement's GNN (tests/prosst_ref.py) batched over all subgraphs as one disjoint graph, as the reference's collate function batches
them, with the graph and the input features built outside the timed window; two warm-up forwards, then --repeats timed ones.
Prints one JSON line."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from proteingym_amd import _lib, prosst  # noqa: E402


def say(*a):
    print(*a, file=sys.stderr, flush=True)


def backbone(L, seed=1):
    rng = np.random.default_rng(seed)
    pts = []
    for t in range(L):
        z, r = divmod(t, 25)
        y, x = divmod(r, 5)
        if y % 2:
            x = 4 - x
        if z % 2:
            y, x = 4 - y, 4 - x
        pts.append((4.6 * x, 4.6 * y, 4.6 * z))
    ca = np.array(pts) + 0.3 * rng.standard_normal((L, 3))
    X = np.empty((L, 4, 3))
    X[:, 1] = ca
    for atom, length, base in ((0, 1.46, 1), (2, 1.52, 1), (3, 1.23, 2)):
        u = rng.standard_normal((L, 3))
        X[:, atom] = X[:, base] + length * u / np.linalg.norm(u, axis=1, keepdims=True)
    return np.round(X, 3).astype(np.float32)


def best(fn, repeats):
    fn()
    runs = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        runs.append(time.perf_counter() - t0)
    return min(runs), runs


def torch_yardstick(L, repeats):
    import torch
    import prosst_ref as R
    sd, X = prosst.random_state_dict(11), backbone(L)
    W = R.tensors(sd, torch.float32, "cuda")
    d = R.distances(X)
    edges = R.global_edges(d)
    subs = [R.subgraph_nodes(d, i) for i in range(L)]
    sube = [R.subgraph_edges(d, edges, n) for n in subs]
    off = np.concatenate([[0], np.cumsum([len(n) for n in subs])])
    node_v, edge_s, edge_v = R.features(X, edges, torch.float32, "cuda")
    nodes = torch.as_tensor(np.concatenate(subs)).cuda()
    e = torch.as_tensor(np.concatenate([se + off[k] for k, (se, _) in enumerate(sube)], 1)).cuda()
    gid = torch.as_tensor(np.concatenate([g for _, g in sube])).cuda()
    batch = torch.as_tensor(np.repeat(np.arange(L), np.diff(off))).cuda()
    nv, es, ev = node_v[nodes], edge_s[gid], edge_v[gid]

    def fwd():
        with torch.no_grad():
            o, _, _ = R.encode(W, nv, e, es, ev)
            cnt = o.new_zeros(L).index_add_(0, batch, o.new_ones(len(batch)))
            p = o.new_zeros(L, o.shape[1]).index_add_(0, batch, o) / cnt[:, None]
            out = torch.nn.functional.normalize(p, p=2, dim=1)
        torch.cuda.synchronize()
        return out
    fwd()
    sec, runs = best(fwd, repeats)
    return dict(L=L, gnn_sec=sec, gnn_sec_runs=runs, peak_mem_gb=torch.cuda.max_memory_allocated() / 2 ** 30)


def bench_length(m, L, Ks, repeats):
    X = backbone(L)
    lib = _lib.load()
    rng = np.random.default_rng(5)
    books = {K: rng.standard_normal((K, 256)).astype(np.float32) / 16 for K in Ks}
    out = dict(L=L)
    sec, runs = best(lambda: m.set_structure(X), repeats)
    out.update(set_structure_sec=sec, set_structure_sec_runs=runs)
    g = m.subgraphs()
    out.update(E_global=int(g["edges"].shape[1]), node_copies=int(len(g["nodes"])), E_sub=int(len(g["edge_gid"])),
               max_nodes=int(np.diff(g["node_off"]).max()))
    for share in (1, 0):
        _lib.check(lib.pgmi_set_option(b"prosst_share_layer0", share))
        sec, runs = best(m.embed, repeats)
        out["embed_sec" if share else "embed_no_layer0_sharing_sec"] = sec
        out["embed_sec_runs" if share else "embed_no_layer0_sharing_sec_runs"] = runs
    _lib.check(lib.pgmi_set_option(b"prosst_share_layer0", 1))
    emb = m.embed()
    out["assign_sec"] = {str(K): best(lambda c=c: m.assign(c), repeats)[0] for K, c in books.items()}
    out["per_structure_sec"] = out["set_structure_sec"] + out["embed_sec"] + sum(out["assign_sec"].values())
    out["emb_norm_range"] = [float(np.linalg.norm(emb, axis=1).min()), float(np.linalg.norm(emb, axis=1).max())]
    view = m.profile_view()
    view.profile_enable(True)
    view.profile_reset()
    m.set_structure(X)
    m.embed()
    for c in books.values():
        m.assign(c)
    out["classes_ms"] = {c: round(v["ms"], 3) for c, v in view.profile().items() if v["launches"]}
    out["classes_tflops"] = {c: round(v["flops"] / v["ms"] / 1e9, 2) for c, v in view.profile().items() if v["launches"] and v["flops"] and v["ms"]}
    view.profile_enable(False)
    say(f"[L {L}] {out}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, nargs="+", default=[286, 1000])
    ap.add_argument("--K", type=int, nargs="+", default=[2048, 20])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--torch", type=int, default=1)
    ap.add_argument("--torch_only", type=int, default=0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.torch_only:
        print(json.dumps(torch_yardstick(args.torch_only, args.repeats)))
        return
    m = prosst.Quantizer(prosst.pack(prosst.random_state_dict(11)))
    try:
        out = dict(runs=[bench_length(m, L, args.K, args.repeats) for L in args.L])
    finally:
        m.close()
    out["torch_fp32_batched"] = []
    for L in args.L if args.torch else []:
        say(f"torch yardstick: L {L}")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--torch_only", str(L), "--repeats", str(args.repeats)], capture_output=True,
                           text=True, timeout=600)
        if r.returncode != 0:
            raise RuntimeError(f"torch yardstick L {L} failed:\n{r.stderr[-2000:]}")
        out["torch_fp32_batched"].append(json.loads(r.stdout.strip().splitlines()[-1]))
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
