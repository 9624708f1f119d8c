#!/usr/bin/env python
"""ESM-IF1 scoring at a BLAT-shaped assay: L = 286 residues (a seeded random-walk backbone), 4 996 seeded single substitutions, seeded
random weights of the released widths (esm_if1_gvp4_t16_142M_UR50: 4 GVP layers of 1024 / 256 channels, 8 + 8 transformer layers of
width 512, 8 heads).

    python scripts/bench_esmif1.py [--mutants 4996] [--L 286] [--torch_mutants 20] [--max_rows 0]

Times the one encoder forward (torch restatement on the GPU), pgmi_esmif1_set_memory, and pgmi_esmif1_sequence_loglik over all mutants
(host clock around the calls, which end in a device synchronise).  A second, profiled run splits the decoder time per kernel class
(pgmi_profile_*; HIP events, so the classes do not overlap): self-attention (prep + kernel), cross-attention (q prep + kernel) and the
GEMMs.  The baseline is the fp32 torch restatement of the reference's per-mutant loop on the same GPU: encoder AND decoder per batch of
one mutant, as compute_fitness_esm_if1.py runs them at its default --batch_size 1 (--torch_mutants of them, after two warm-up forwards,
in a child process of its own).  Prints one JSON line.

Derived cost per decoder row and layer: QKV 3 D^2 + out D^2 + cross q D^2 + cross out D^2 + FFN 2 D F multiply-adds = 2 x (6 x 512^2 +
2 x 512 x 2048) = 7.3 MFLOP in the GEMMs; self-attention 4 x 64 x 8 x (t + 1) and cross-attention 4 x 64 x 8 x S FLOP."""
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

from proteingym_amd import _lib, esmif1  # noqa: E402

CLASSES = {"embed": 0, "layernorm": 1, "gemm_qkv_and_cross_q": 2, "self_attention": 3, "gemm_out": 4, "gemm_fc1": 5, "gemm_fc2": 6, "head": 7,
           "score": 8, "cross_attention": 12}


def torch_decoder(cfg, w, enc, tokens):
    """transformer_decoder.py / transformer_layer.py restated in torch for one sequence: mean log p of tokens[1:] given tokens[:-1]"""
    import torch
    F = torch.nn.functional
    D, H = cfg["embed_dim"], cfg["heads"]
    t = torch.as_tensor(tokens[:-1].astype(np.int64), device=enc.device)
    T = t.shape[0]
    x = D ** 0.5 * w["decoder.embed_tokens.weight"][t] + esmif1._sinusoid(torch.arange(T) + esmif1.PAD + 1, D, esmif1.PAD).to(enc.device)

    def lin(n, v):
        return F.linear(v, w[n + ".weight"], w[n + ".bias"])

    def ln(n, v):
        return F.layer_norm(v, v.shape[-1:], w[n + ".weight"], w[n + ".bias"])

    def att(p, q_in, kv, causal):
        dh = D // H
        q = (lin(p + "q_proj", q_in) * dh ** -0.5).reshape(T, H, dh).transpose(0, 1)
        k = lin(p + "k_proj", kv).reshape(-1, H, dh).transpose(0, 1)
        v = lin(p + "v_proj", kv).reshape(-1, H, dh).transpose(0, 1)
        a = q @ k.transpose(-1, -2)
        if causal:
            a = a.masked_fill(torch.triu(torch.ones(T, T, dtype=torch.bool, device=a.device), 1), float("-inf"))
        return lin(p + "out_proj", (torch.softmax(a, -1) @ v).transpose(0, 1).reshape(T, D))

    for i in range(cfg["layers"]):
        p = f"decoder.layers.{i}."
        h = ln(p + "self_attn_layer_norm", x)
        x = x + att(p + "self_attn.", h, h, True)
        x = x + att(p + "encoder_attn.", ln(p + "encoder_attn_layer_norm", x), enc, False)
        x = x + lin(p + "fc2", torch.relu(lin(p + "fc1", ln(p + "final_layer_norm", x))))
    lp = torch.log_softmax(F.linear(ln("decoder.layer_norm", x), w["decoder.output_projection.weight"]), -1)
    tgt = torch.as_tensor(tokens[1:].astype(np.int64), device=enc.device)
    return lp.gather(1, tgt[:, None]).mean()


def torch_baseline(cfg, sd, coords, seqs, n):
    """seconds per mutant of the reference's loop restated in fp32 torch on the GPU: encoder and decoder per mutant, batch 1"""
    import torch
    dev = torch.device("cuda:0")
    enc = esmif1.Encoder(cfg, sd, dev, torch.float32)
    w = {k: torch.as_tensor(v).to(dev) for k, v in sd.items() if k.startswith("decoder.")}

    def one(b):
        with torch.no_grad():
            e = torch.as_tensor(enc.encode(coords), dtype=torch.float32, device=dev)
            return float(torch_decoder(cfg, w, e, esmif1.tokenize(seqs[b])))
    for b in range(n, n + 2):
        one(b)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    vals = [one(b) for b in range(n)]
    return (time.perf_counter() - t0) / n, vals


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mutants", type=int, default=4996)
    ap.add_argument("--L", type=int, default=286)
    ap.add_argument("--torch_mutants", type=int, default=20)
    ap.add_argument("--max_rows", type=int, default=0, help="decoder rows per device chunk; 0: the library's default")
    ap.add_argument("--torch_only", action="store_true", help="(internal) run the torch baseline alone and print its JSON")
    a = ap.parse_args()
    import esmif1_cases as K
    cfg = esmif1.config_from_args(K.RELEASED_ARGS)
    sd = K.state_dict(cfg, seed=7)
    coords = K.backbone(9, a.L)
    wt = K.sequence_of(10, a.L)
    rng = np.random.default_rng(4)
    seqs = []
    for _ in range(a.mutants):
        p = int(rng.integers(a.L))
        seqs.append(wt[:p] + str(rng.choice([c for c in K.AA if c != wt[p]])) + wt[p + 1:])
    if a.torch_only:
        sec, vals = torch_baseline(cfg, sd, coords, seqs, a.torch_mutants)
        print(json.dumps({"sec": sec, "vals": vals}))
        return
    if a.torch_mutants > 0:
        # the baseline runs in a child process of its own, before this one opens the GPU, and has the GPU to itself while it is timed
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--torch_only", "--L", str(a.L), "--mutants", str(a.mutants),
                            "--torch_mutants", str(a.torch_mutants)], capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise RuntimeError(f"torch baseline failed:\n{r.stderr[-2000:]}")
        base = json.loads(r.stdout.strip().splitlines()[-1])
    # the model puts its encoder on the torch device before it creates the decoder: torch's HIP runtime has to come up before libpgmi's
    model = esmif1.EsmIf1Model(cfg, sd, device=0, max_rows=a.max_rows, max_memory=a.L + 2)
    lib = _lib.load()
    model.set_structure(coords)
    model.score(seqs[:256])                                                          # warm-up
    t0 = time.perf_counter()
    enc = model.encoder.encode(coords)
    t_enc = time.perf_counter() - t0
    t0 = time.perf_counter()
    model.decoder.set_memory(enc)
    t_mem = time.perf_counter() - t0
    t0 = time.perf_counter()
    scores = model.score(seqs, max_batch=a.mutants)
    wall = time.perf_counter() - t0
    h = model.decoder._h
    _lib.check(lib.pgmi_profile_enable(h, 1))
    _lib.check(lib.pgmi_profile_reset(h))
    model.score(seqs, max_batch=a.mutants)
    split, total_ms = {}, 0.0
    for name, k in CLASSES.items():
        ms, n, fl = C.c_double(), C.c_int64(), C.c_double()
        _lib.check(lib.pgmi_profile_get(h, k, C.byref(ms), C.byref(n), C.byref(fl), None))
        split[name] = {"ms": ms.value, "launches": n.value, "tflops": fl.value / ms.value / 1e9 if ms.value > 0 and fl.value > 0 else None}
        total_ms += ms.value
    _lib.check(lib.pgmi_profile_enable(h, 0))
    model.close()
    for v in split.values():
        v["share"] = v["ms"] / total_ms
    rows = a.mutants * a.L
    D, Fd = cfg["embed_dim"], cfg["ffn_dim"]
    out = {"bench": "esmif1", "L": a.L, "S": int(enc.shape[0]), "mutants": a.mutants, "decoder_rows": rows, "max_rows": a.max_rows,
           "encoder_forward_ms": 1e3 * t_enc, "set_memory_ms": 1e3 * t_mem, "scores_seconds": wall, "mutants_per_s": a.mutants / wall,
           "kernel_ms_total": total_ms, "split": split,
           "derived_gemm_mflop_per_row_and_layer": 2 * (6 * D * D + 2 * D * Fd) / 1e6, "score_first": float(scores[0])}
    if a.torch_mutants > 0:
        out.update(torch_fp32_same_gpu_seconds_per_mutant=base["sec"], torch_fp32_same_gpu_mutants_per_s=1.0 / base["sec"],
                   speedup_vs_torch_same_gpu=(a.mutants / wall) * base["sec"],
                   max_abs_diff_vs_torch_on_its_mutants=float(np.abs(np.array(base["vals"]) - scores[:a.torch_mutants]).max()))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
