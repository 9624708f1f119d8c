#!/usr/bin/env python
"""EVE evolutionary indices at a BLAT-shaped assay: L = 286 focus columns, 4 996 mutants + wild type, the default parameter file's
sizes (encoder 2000-1000-300, z 50, decoder 300-1000-2000, conv depth 40, temperature, dropout 0.1), seeded random weights.

    python scripts/bench_eve.py [--samples 300] [--warmup 20] [--cpu_samples 3] [--rows 4997] [--L 286] [--max_rows 0]

Times ``--samples`` Monte-Carlo samples of pgmi_eve_evol_indices (host clock around the call, which ends in a device synchronise)
and extrapolates to the launcher's 20 000 per seed; a second, profiled run splits the time per sample into the weight sampler, the
latent + hidden layers, the final GEMM and the ELBO reduction (pgmi_profile_* on pgmi_eve_profile_model's handle; HIP events, so the
classes do not overlap).  The CPU figure is the same estimator written in fp32 torch (shared weights per sample, the whole assay as
one batch) on the threads torch is given.  Prints one JSON line.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from proteingym_amd import _lib, eve  # noqa: E402

CLASSES = {"sampler": 0, "hidden": 5, "final_gemm": 6, "reduction": 8, "encoder": 7}     # include/pgmi.h PGMI_K_*


def torch_sample(sd, d, onehot, mu, log_var, gen):
    """One sample of the estimator in fp32 torch (tests/eve_ref.py's arithmetic, noise from torch)."""
    import torch
    p, L, H, Cc = d["dropout_p"], d["seq_len"], d["dec_sizes"][-1], d["conv_depth"]
    draw = lambda mean, lv: torch.exp(0.5 * sd[lv]) * torch.randn(sd[mean].shape, generator=gen) + sd[mean]
    drop = lambda x: x * (torch.rand(x.shape, generator=gen) < 1 - p) / (1 - p)
    h = drop(torch.exp(0.5 * log_var) * torch.randn(mu.shape, generator=gen) + mu)
    for i in range(len(d["dec_sizes"])):
        W = draw(f"decoder.hidden_layers_mean.{i}.weight", f"decoder.hidden_layers_log_var.{i}.weight")
        b = draw(f"decoder.hidden_layers_mean.{i}.bias", f"decoder.hidden_layers_log_var.{i}.bias")
        h = drop(torch.relu(h @ W.T + b))
    W = draw("decoder.last_hidden_layer_weight_mean", "decoder.last_hidden_layer_weight_log_var")
    b = draw("decoder.last_hidden_layer_bias_mean", "decoder.last_hidden_layer_bias_log_var")
    conv = draw("decoder.output_convolution_mean.weight", "decoder.output_convolution_log_var.weight")
    W = (W.reshape(L * H, Cc) @ conv.reshape(Cc, 20)).reshape(L * 20, H)
    t = draw("decoder.temperature_scaler_mean", "decoder.temperature_scaler_log_var")
    lp = torch.log_softmax((torch.log(1 + torch.exp(t)) * (h @ W.T + b)).reshape(-1, L, 20), -1)
    bce = (torch.log1p(torch.exp(lp)) - lp * onehot).sum((1, 2))
    kld = -0.5 * (1 + log_var - mu ** 2 - log_var.exp()).sum(1)
    return -(bce + kld)


def cpu_seconds_per_sample(sd_np, d, res, n):
    import torch
    sd = {k: torch.from_numpy(v) for k, v in sd_np.items()}
    onehot = torch.zeros(len(res), d["seq_len"], 20)
    onehot.scatter_(2, torch.from_numpy(res.astype(np.int64))[:, :, None], 1.0)
    h = onehot.reshape(len(res), -1)
    for i in range(len(d["enc_sizes"])):
        h = torch.relu(h @ sd[f"encoder.hidden_layers.{i}.weight"].T + sd[f"encoder.hidden_layers.{i}.bias"])
    mu = h @ sd["encoder.fc_mean.weight"].T + sd["encoder.fc_mean.bias"]
    lv = h @ sd["encoder.fc_log_var.weight"].T + sd["encoder.fc_log_var.bias"]
    gen = torch.Generator().manual_seed(0)
    with torch.no_grad():
        torch_sample(sd, d, onehot, mu, lv, gen)                       # warm-up
        t0 = time.perf_counter()
        for _ in range(n):
            torch_sample(sd, d, onehot, mu, lv, gen)
    return (time.perf_counter() - t0) / n, torch.get_num_threads()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--cpu_samples", type=int, default=3)
    ap.add_argument("--rows", type=int, default=4997)
    ap.add_argument("--L", type=int, default=286)
    ap.add_argument("--max_rows", type=int, default=0, help="rows per device chunk (the CLI's --batch_size); 0: one chunk of up to 256 MB of logits")
    ap.add_argument("--full", type=int, default=20000, help="samples per seed to extrapolate to")
    a = ap.parse_args()
    d = dict(seq_len=a.L, z_dim=50, enc_sizes=[2000, 1000, 300], dec_sizes=[300, 1000, 2000], conv_depth=40, temperature=1,
             sparsity_tiles=0, enc_act="relu", dec_first_act="relu", dec_last_act="relu", dropout_p=0.1)
    sd = eve.random_state_dict(d, seed=1, log_var=(-8.0, -4.0))
    rng = np.random.default_rng(2)
    res = np.tile(rng.integers(0, 20, size=a.L).astype(np.uint8), (a.rows, 1))
    for m in range(1, a.rows):
        res[m, rng.integers(a.L)] = rng.integers(20)
    lib = _lib.load()
    if lib.pgmi_device_count() <= 0:
        raise RuntimeError("bench_eve.py needs a GPU: libpgmi has no CPU fallback")
    model = eve.EveModel(d, eve.blob_from_state_dict(sd, d))
    _lib.check(lib.pgmi_set_option(b"eve_max_rows", a.max_rows))
    model.evol_indices(res, a.warmup, seed=0)
    t0 = time.perf_counter()
    mean, std = model.evol_indices(res, a.samples, seed=0)
    wall = time.perf_counter() - t0
    h = model.profile_handle()
    _lib.check(lib.pgmi_profile_enable(h, 1))
    _lib.check(lib.pgmi_profile_reset(h))
    model.evol_indices(res, a.samples, seed=0)
    split = {}
    for name, k in CLASSES.items():
        ms, n, fl = C.c_double(), C.c_int64(), C.c_double()
        _lib.check(lib.pgmi_profile_get(h, k, C.byref(ms), C.byref(n), C.byref(fl), None))
        split[name] = {"ms_per_sample": ms.value / a.samples, "launch_groups": n.value,
                       "tflops": fl.value / ms.value / 1e9 if ms.value > 0 and fl.value > 0 else None}
    _lib.check(lib.pgmi_profile_enable(h, 0))
    model.close()
    out = {"bench": "eve", "L": a.L, "rows": a.rows, "max_rows": a.max_rows, "samples": a.samples, "gpu_ms_per_sample": 1e3 * wall / a.samples,
           "gpu_seconds_per_seed_extrapolated": wall / a.samples * a.full, "samples_per_seed": a.full, "split": split,
           "elbo_mean_wt": float(mean[0]), "elbo_std_wt": float(std[0])}
    if a.cpu_samples > 0:
        sec, threads = cpu_seconds_per_sample(sd, d, res, a.cpu_samples)
        out.update(cpu_ms_per_sample=1e3 * sec, cpu_threads=threads, cpu_seconds_per_seed_extrapolated=sec * a.full,
                   speedup=sec / (wall / a.samples))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
