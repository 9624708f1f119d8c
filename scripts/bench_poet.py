#!/usr/bin/env python
"""PoET scoring at a BLAT-shaped assay: variants of L = 286 residues (288 tokens with start and stop), seeded random weights at the
dimensions the published checkpoint is believed to have (D = 1024, 16 heads, 12 layers, FFN 4096, final norm), prompts of 6 144 /
12 288 / 24 576 tokens made of seeded sequences of the same length.

    python scripts/bench_poet.py [--variants 4996] [--contexts 6144 12288 24576] [--torch_variants 64] [--layers 12]

Per context length: the time of one pgmi_poet_set_prompt (the tiered forward over the prompt, which fills the prefix cache) and of
pgmi_poet_sequence_loglik over all variants (host clock around calls that end in a device synchronise, after a warm-up of both at the
same shapes), variants/s, and from a second, profiled run the split per kernel class (HIP events: the classes do not overlap) with the
prefix-attention kernel's share of the scoring time and its fraction of the fp16 MFMA rate.  That fraction counts the MFMAs the kernel
issues -- three 16-bit products per f16x3 product, whole 32 x 32 tiles including the masked half of a diagonal tile and prefix tails --
against the MI355X's 2.5 PFLOP/s dense fp16 peak (spec); the algorithmic rate (4 * visible pairs * 64 * heads FLOP) is printed beside it.
The baseline is a torch restatement of the reference's cached-memory loop (scripts/score.py _get_logps_tiered_fast: batch 8, the
prompt's per-layer keys and values computed once, variants padded to one length) on the same GPU in fp16 and in fp32, in a child process
of its own.  The reference itself runs flash-attn kernels in fp16; torch's scaled_dot_product_attention stands in for them.
Prints one JSON line."""
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

from proteingym_amd import _lib, poet  # noqa: E402

CLASSES = {"embed_gather": 0, "layernorm": 1, "gemm_qkv": 2, "attention": 3, "gemm_out": 4, "gemm_fc1": 5, "gemm_fc2": 6, "head": 7, "score": 8}
PEAK_F16_MFMA = 2.5e15


def config(layers):
    return dict(layers=layers, embed_dim=1024, heads=16, ffn_dim=4096, vocab=24, final_norm=True)


def random_state_dict(cfg, seed):
    rng = np.random.default_rng(seed)
    D, F, V = cfg["embed_dim"], cfg["ffn_dim"], cfg["vocab"]
    sd = {}
    for k in poet.expected_keys(cfg):
        shape = {"token_embed.weight": (V, D), "linear.weight": (V, D), "linear.bias": (V,)}.get(k)
        if shape is None:
            shape = (F, D) if k.endswith("linear1.weight") else (D, F) if k.endswith("linear2.weight") else (F,) if k.endswith("linear1.bias") \
                else (D, D) if k.endswith("_proj.weight") else (D,)
        if len(shape) == 2:
            sd[k] = (rng.standard_normal(shape, dtype=np.float32) * (0.5 / np.sqrt(shape[1]))).astype(np.float32)
        elif "norm" in k and k.endswith("weight"):
            sd[k] = (1.0 + 0.05 * rng.standard_normal(shape, dtype=np.float32)).astype(np.float32)
        else:
            sd[k] = (0.02 * rng.standard_normal(shape, dtype=np.float32)).astype(np.float32)
    return sd


def assay(L, n_variants, contexts, seed=5):
    rng = np.random.default_rng(seed)
    wt = rng.integers(0, 20, L).astype(np.uint8)
    variants = []
    for i in range(n_variants):
        v = wt.copy()
        pos = rng.choice(L, 1 + i % 2, replace=False)
        v[pos] = (v[pos] + rng.integers(1, 20, len(pos))) % 20
        variants.append(poet.append_startstop(v))
    prompts = {}
    for P in contexts:
        seqs, total = [], 0
        while total < P:                                           # truncate=False: the last sequence overshoots the budget
            s = wt.copy()
            pos = rng.choice(L, L // 3, replace=False)
            s[pos] = rng.integers(0, 20, len(pos))
            seqs.append(poet.append_startstop(s))
            total += L + 2
        prompts[P] = seqs
    return variants, prompts


def torch_baseline(cfg, sd, prompt, variants, dtype_name, batch=8, device="cuda:0"):
    """seconds per variant of the reference's cached-memory loop restated in torch on the GPU: memory once, then batches of 8"""
    import torch
    import torch.nn.functional as F
    dev, dtype = torch.device(device), getattr(torch, dtype_name)
    w = {k: torch.as_tensor(v).to(dev, dtype) for k, v in sd.items()}
    H, dh = cfg["heads"], cfg["embed_dim"] // cfg["heads"]
    inv = (1.0 / (10000 ** (torch.div(torch.arange(dh), 2, rounding_mode="floor") * 2.0 / dh))).float().to(dev)

    def rot(x, pos):                                               # x [..., n, H, dh]
        f = torch.outer(pos.float(), inv)
        cos, sin = torch.cos(f).to(dtype)[:, None, :], torch.sin(f).to(dtype)[:, None, :]
        return x * cos + torch.stack((-x[..., 1::2], x[..., 0::2]), dim=-1).flatten(-2) * sin

    def ln(x, name):
        return F.layer_norm(x, (x.shape[-1],), w[name + ".weight"], w[name + ".bias"], 1e-5)

    def proj(h, p, pos):
        q = rot((h @ w[p + "q_proj.weight"].T).unflatten(-1, (H, dh)), pos)
        k = rot((h @ w[p + "k_proj.weight"].T).unflatten(-1, (H, dh)), pos)
        return q, k, (h @ w[p + "v_proj.weight"].T).unflatten(-1, (H, dh))

    def out(ctx, p):
        return ctx.flatten(-2) @ w[p + "out_proj.weight"].T + w[p + "out_proj.bias"]

    def mlp(x, p):
        return x + F.gelu(ln(x, p + "norm3") @ w[p + "linear1.weight"].T + w[p + "linear1.bias"]) @ w[p + "linear2.weight"].T + w[p + "linear2.bias"]

    def sdpa(q, k, v, mask=None, causal=False):                    # [b, n, H, dh] -> the same
        return F.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), attn_mask=mask, is_causal=causal).transpose(1, 2)

    with torch.no_grad():
        # the prompt's memory: per sequence tier 1 (equal lengths here: one batch), tier 2 causal over the concatenation
        n_seq, n = len(prompt), len(prompt[0])
        tok = torch.as_tensor(np.stack(prompt).astype(np.int64), device=dev)
        pos = torch.arange(n, device=dev)
        x = w["token_embed.weight"][tok]
        memory = []
        for l in range(cfg["layers"]):
            p = f"decoder.layers.{l}."
            q, k, v = proj(ln(x, p + "norm1"), p + "self_attn.", pos)
            x = x + out(sdpa(q, k, v, causal=True), p + "self_attn.")
            q, k, v = proj(ln(x, p + "norm2"), p + "multihead_attn.", pos)
            qf, kf, vf = (t.reshape(1, n_seq * n, H, dh) for t in (q, k, v))
            x = x + out(sdpa(qf, kf, vf, causal=True).reshape(n_seq, n, H, dh), p + "multihead_attn.")
            memory.append((kf, vf))
            x = mlp(x, p)
        P = n_seq * n
        T = len(variants[0]) - 1
        mask = torch.cat([torch.ones(T, P, dtype=torch.bool, device=dev), torch.tril(torch.ones(T, T, dtype=torch.bool, device=dev))], dim=1)
        vpos = torch.arange(T, device=dev)

        def score(batch_variants):
            t = torch.as_tensor(np.stack(batch_variants).astype(np.int64), device=dev)
            b = t.shape[0]
            x = w["token_embed.weight"][t[:, :-1]]
            for l in range(cfg["layers"]):
                p = f"decoder.layers.{l}."
                q, k, v = proj(ln(x, p + "norm1"), p + "self_attn.", vpos)
                x = x + out(sdpa(q, k, v, causal=True), p + "self_attn.")
                q, k, v = proj(ln(x, p + "norm2"), p + "multihead_attn.", vpos)
                km, vm = memory[l]
                ka, va = torch.cat([km.expand(b, -1, -1, -1), k], dim=1), torch.cat([vm.expand(b, -1, -1, -1), v], dim=1)
                x = x + out(sdpa(q, ka, va, mask=mask), p + "multihead_attn.")
                x = mlp(x, p)
            lp = torch.log_softmax((ln(x, "norm") @ w["linear.weight"].T + w["linear.bias"]).float(), dim=-1)
            return lp.gather(2, t[:, 1:, None])[..., 0].sum(dim=1)

        score(variants[:batch]).cpu()                              # warm-up at the timed shape
        if dev.type == "cuda":
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        vals = [score(variants[i:i + batch]).cpu().numpy() for i in range(0, len(variants), batch)]
        if dev.type == "cuda":
            torch.cuda.synchronize()
        sec = (time.perf_counter() - t0) / len(variants)
    return sec, np.concatenate(vals).tolist()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", type=int, default=4996)
    ap.add_argument("--L", type=int, default=286)
    ap.add_argument("--contexts", type=int, nargs="+", default=[6144, 12288, 24576])
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--torch_variants", type=int, default=64)
    ap.add_argument("--torch_only", type=str, default="", help="(internal) run the torch baseline alone in this dtype and print its JSON")
    a = ap.parse_args()
    cfg = config(a.layers)
    sd = random_state_dict(cfg, 7)
    variants, prompts = assay(a.L, a.variants, a.contexts)
    if a.torch_only:
        res = {}
        for P in a.contexts:
            sec, vals = torch_baseline(cfg, sd, prompts[P], variants[:a.torch_variants], a.torch_only)
            res[str(P)] = {"sec": sec, "vals": vals}
        print(json.dumps(res))
        return
    base = {}
    if a.torch_variants > 0:
        # the baselines run in child processes of their own, one after the other, before this process opens the GPU
        for dt in ("float16", "float32"):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--torch_only", dt, "--L", str(a.L), "--variants", str(a.variants),
                                "--torch_variants", str(a.torch_variants), "--layers", str(a.layers), "--contexts", *map(str, a.contexts)],
                               capture_output=True, text=True, timeout=1500)
            if r.returncode != 0:
                raise RuntimeError(f"torch baseline ({dt}) failed:\n{r.stderr[-2000:]}")
            base[dt] = json.loads(r.stdout.strip().splitlines()[-1])
    lib = _lib.load()
    if lib.pgmi_device_count() <= 0:
        raise RuntimeError("bench_poet.py needs a GPU: libpgmi has no CPU fallback")
    longest = max(sum(len(s) for s in p) for p in prompts.values())
    padded = max(sum((len(s) + 31) // 32 * 32 for s in p) for p in prompts.values())
    model = poet.PoetModel(cfg, poet.pack(cfg, sd), max_rows=max(padded + 32, 32768), max_prompt=longest)
    H, T = cfg["heads"], a.L + 1                                   # T input rows per variant
    out = {"bench": "poet", "L": a.L, "variants": a.variants, "layers": a.layers, "dims": cfg, "contexts": {}}
    for P in a.contexts:
        prompt = prompts[P]
        Pt = sum(len(s) for s in prompt)
        model.set_prompt(prompt)                                   # warm-up of both calls at the timed shapes
        model.sequence_loglik(variants[:256])
        t0 = time.perf_counter()
        model.set_prompt(prompt)
        t_prompt = time.perf_counter() - t0
        t0 = time.perf_counter()
        scores = model.score(variants)
        wall = time.perf_counter() - t0
        _lib.check(lib.pgmi_profile_enable(model._h, 1))
        _lib.check(lib.pgmi_profile_reset(model._h))
        model.score(variants)
        split, total_ms = {}, 0.0
        for name, k in CLASSES.items():
            ms, n, fl = C.c_double(), C.c_int64(), C.c_double()
            _lib.check(lib.pgmi_profile_get(model._h, k, C.byref(ms), C.byref(n), C.byref(fl), None))
            split[name] = {"ms": ms.value, "launches": n.value, "algorithmic_tflops": fl.value / ms.value / 1e9 if ms.value > 0 and fl.value > 0 else None}
            total_ms += ms.value
        _lib.check(lib.pgmi_profile_enable(model._h, 0))
        # MFMAs issued by the two attention launches of a layer, per variant: query tiles x key tiles x (32 x 32 x 64 x 2 FLOP x 2 products
        # (scores, context) x 3 split terms); the class's time also holds the two prep passes
        qt = (T + 31) // 32
        own_tiles = qt * (qt + 1) // 2
        issued = a.layers * H * (2 * own_tiles + qt * ((Pt + 31) // 32)) * (32 * 32 * 64 * 2 * 2 * 3) * a.variants
        att = split["attention"]
        res = {"prompt_tokens": Pt, "prompt_sequences": len(prompt), "set_prompt_seconds": t_prompt, "score_seconds": wall,
               "variants_per_s": a.variants / wall, "prompt_share_of_total": t_prompt / (t_prompt + wall),
               "kernel_ms_total": total_ms, "split": split, "attention_share_of_kernel_time": att["ms"] / total_ms,
               "attention_issued_mfma_tflops": issued / att["ms"] / 1e9, "attention_fraction_of_fp16_mfma_rate": issued / (att["ms"] * 1e-3) / PEAK_F16_MFMA,
               "score_first": float(scores[0])}
        for dt, b in base.items():
            sec = b[str(P)]["sec"]
            res[f"torch_{dt}_same_gpu_variants_per_s"] = 1.0 / sec
            res[f"speedup_vs_torch_{dt}"] = (a.variants / wall) * sec
            res[f"max_abs_diff_vs_torch_{dt}"] = float(np.abs(np.array(b[str(P)]["vals"]) - scores[:a.torch_variants]).max())
        out["contexts"][str(P)] = res
    model.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
