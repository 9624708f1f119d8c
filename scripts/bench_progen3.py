"""Secondary measurement: ProGen3 scoring throughput, end to end from sequences to (log_likelihood, perplexity), both reading
directions as ProGen3Scorer does, on seeded weights.

The shape is ASSUMED, not a released checkpoint's (their config.json files are not available here): hidden 1024, 16 heads on 4 K/V
heads (head_dim 64), 10 layers, 8 gated experts of width 2048, top-2, vocab 134 -- about 0.54 B parameters, between the 339m and 762m
classes.  BLAT_ECOLX-shaped assay: L = 286 single mutants.

Prints one JSON line: mutants/s of the timed pass (profiler off, host clock around calls that end in a device synchronise, every shape
warmed up first); the per-kernel-class HIP-event breakdown of a separate profiled pass; from it, per layer, the share of router +
permutation + gather + combine against the expert GEMMs; and mutants/s of the same model as a torch fp32 restatement of the reference's
eager block on the same GPU, run in a child process of its own.

    python scripts/bench_progen3.py [--mutants 1000] [--torch-mutants 300] > profiles/progen3/bench_progen3.json
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.getcwd())

SHAPE = dict(layers=10, embed_dim=1024, heads=16, kv_heads=4, ffn_dim=2048, n_experts=8, top_k=2, gated=True, vocab=134,
             max_positions=512, ln_eps=1e-5, rope_theta=100000.0, fused_attention_norm=False)
L_ASSAY = 286


def sequences(n):
    from proteingym_amd import synthetic
    from proteingym_amd.causal_lm import get_mutated_sequence
    seq, muts, _ = synthetic.random_assay(seed=23, L=L_ASSAY, n_single=n, n_multi=0)
    return [get_mutated_sequence(seq, m) for m in muts]


def torch_child(n):
    """The reference's forward restated in torch fp32 (eager expert loop, SDPA attention) on cuda:0; prints mutants/s."""
    import torch
    import torch.nn.functional as F
    from proteingym_amd import progen3 as pg3
    dev = torch.device("cuda:0")
    c = SHAPE
    D, H, KV, Fh, E, k = c["embed_dim"], c["heads"], c["kv_heads"], c["ffn_dim"], c["n_experts"], c["top_k"]
    dh = D // H
    g = torch.Generator(device="cpu").manual_seed(3)
    rnd = lambda *s: (torch.randn(*s, generator=g) * 0.02).to(dev)   # noqa: E731
    emb, head = rnd(c["vocab"], D), rnd(c["vocab"], D)
    layers = [dict(n1=torch.ones(D, device=dev), n2=torch.ones(D, device=dev), q=rnd(D, D), k=rnd(KV * dh, D), v=rnd(KV * dh, D), o=rnd(D, D),
                   gate=rnd(E, D), w1=[rnd(Fh, D) for _ in range(E)], w3=[rnd(Fh, D) for _ in range(E)], w2=[rnd(D, Fh) for _ in range(E)])
              for _ in range(c["layers"])]
    nf = torch.ones(D, device=dev)
    inv = c["rope_theta"] ** -(torch.arange(0, dh, 2, dtype=torch.float32) / dh)
    ang = torch.outer(torch.arange(c["max_positions"], dtype=torch.float32), inv)
    cos, sin = torch.cat([ang, ang], 1).cos().to(dev), torch.cat([ang, ang], 1).sin().to(dev)
    rms = lambda x, w: x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + c["ln_eps"]) * w   # noqa: E731
    rot = lambda x: torch.cat((-x[..., dh // 2:], x[..., :dh // 2]), -1)                      # noqa: E731

    def forward(ids):
        B, T = ids.shape
        x = emb[ids]
        for Lw in layers:
            h = rms(x, Lw["n1"])
            q, kk, v = (h @ Lw["q"].T).view(B, T, H, dh), (h @ Lw["k"].T).view(B, T, KV, dh), (h @ Lw["v"].T).view(B, T, KV, dh)
            cs, sn = cos[:T, None], sin[:T, None]
            q, kk = q * cs + rot(q) * sn, kk * cs + rot(kk) * sn
            kk, v = kk.repeat_interleave(H // KV, 2), v.repeat_interleave(H // KV, 2)
            a = F.scaled_dot_product_attention(q.transpose(1, 2), kk.transpose(1, 2), v.transpose(1, 2), is_causal=True)
            x = x + a.transpose(1, 2).reshape(B, T, D) @ Lw["o"].T
            h = rms(x, Lw["n2"]).view(-1, D)
            p = F.softmax(h @ Lw["gate"].T, dim=-1, dtype=torch.float32)
            w, sel = torch.topk(p, k, dim=-1)
            w = w / w.sum(-1, keepdim=True)
            out = torch.zeros_like(h)
            mask = F.one_hot(sel, num_classes=E).permute(2, 1, 0)
            for e in range(E):
                idx, top_x = torch.where(mask[e])
                if top_x.shape[0]:
                    he = h[top_x]
                    out.index_add_(0, top_x, ((F.silu(he @ Lw["w1"][e].T) * (he @ Lw["w3"][e].T)) @ Lw["w2"][e].T) * w[top_x, idx, None])
            x = x + out.view(B, T, D)
        return rms(x, nf) @ head.T

    def score(seqs):
        out = []
        with torch.no_grad():
            for batch in pg3.group_by_length(seqs, 16384):                       # fp32 activations of the eager block: a smaller budget than the scorer's default
                for rev in (False, True):
                    ids = torch.from_numpy(np.stack([pg3.encode(seqs[i], rev) for i in batch]).astype(np.int64)).to(dev)
                    logits = forward(ids)
                    nll = F.cross_entropy(logits[:, :-1].reshape(-1, c["vocab"]), ids[:, 1:].reshape(-1), reduction="none").view(len(batch), -1)
                    out.append(nll.mean(1).cpu())
        return out
    seqs = sequences(n)
    score(seqs[:57])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    score(seqs)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(json.dumps(dict(torch_fp32_mutants=n, torch_fp32_seconds=round(dt, 3), torch_fp32_mutants_per_s=round(n / dt, 1))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mutants", type=int, default=1000)
    ap.add_argument("--torch-mutants", type=int, default=300, help="0: skip the torch fp32 baseline")
    ap.add_argument("--torch-child", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.torch_child:
        return torch_child(args.torch_child)
    from proteingym_amd import _lib, progen3 as pg3
    lib = _lib.load()
    if lib.pgmi_device_count() <= 0:
        raise SystemExit("bench_progen3 needs a GPU: nothing is measured without one")
    cfg = dict(SHAPE)
    rng = np.random.default_rng(3)
    blob = rng.standard_normal(pg3.weight_count(cfg), dtype=np.float32) * np.float32(0.02)
    D = cfg["embed_dim"]
    # the norm weights are ones, as initialised: walk the blob's layout (include/pgmi.h) to find them
    kvd = cfg["kv_heads"] * (D // cfg["heads"])
    o = cfg["vocab"] * D + D
    per_expert = 3 * cfg["ffn_dim"] * D
    for _ in range(cfg["layers"]):
        blob[o:o + D] = 1.0
        o += D + 2 * D * D + 2 * kvd * D
        blob[o:o + D] = 1.0
        o += D + cfg["n_experts"] * D + cfg["n_experts"] * per_expert
    blob[o:o + D] = 1.0
    model = pg3.ProGen3Model(cfg, blob)
    params = blob.size
    del blob
    seqs = sequences(args.mutants)
    model.score(seqs)                                                            # warm-up: every shape of the timed pass
    lib.pgmi_synchronize(model._h)
    t0 = time.perf_counter()
    model.score(seqs)                                                            # sequence_loglik returns after the device synchronise
    dt = time.perf_counter() - t0
    lib.pgmi_profile_enable(model._h, 1)                                         # the profiled pass: separate, not timed end to end
    lib.pgmi_profile_reset(model._h)
    model.score(seqs)
    prof = {}
    for kk, name in enumerate(_lib.K_NAMES):
        ms, n, fl, by = C.c_double(), C.c_int64(), C.c_double(), C.c_double()
        if lib.pgmi_profile_get(model._h, kk, C.byref(ms), C.byref(n), C.byref(fl), C.byref(by)) == 0 and n.value:
            prof[name] = dict(ms=round(ms.value, 2), calls=n.value, tflops=round(fl.value / ms.value / 1e9, 1) if ms.value and fl.value else None)
    lib.pgmi_profile_enable(model._h, 0)
    model.close()
    gemm = prof.get("gemm_fc1", {}).get("ms", 0.0) + prof.get("gemm_fc2", {}).get("ms", 0.0)
    route = prof.get("moe_route", {}).get("ms", 0.0)
    out = dict(shape=SHAPE, shape_is="assumed (no released config.json at hand)", parameters=params, L=L_ASSAY, mutants=len(seqs), seconds=round(dt, 3),
               mutants_per_s=round(len(seqs) / dt, 1), kernels=prof,
               expert_block=dict(permute_gather_combine_ms=route, expert_gemms_ms=round(gemm, 2), router_in="layernorm (fused into the second RMSNorm)",
                                 share_of_permute_gather_combine=round(route / (route + gemm), 4) if route + gemm else None,
                                 expert_gemm_launches=prof.get("gemm_fc1", {}).get("calls", 0) + prof.get("gemm_fc2", {}).get("calls", 0)))
    if args.torch_mutants:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--torch-child", str(args.torch_mutants)], capture_output=True, text=True)
        line = next((ln for ln in reversed(r.stdout.splitlines()) if ln.startswith("{")), None)
        out.update(json.loads(line) if r.returncode == 0 and line else dict(torch_fp32_error=(r.stderr or r.stdout)[-400:]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
