#!/usr/bin/env python
"""TranceptEVE's EVE log-prior at a BLAT-shaped family: L = 286 focus columns, the default parameter file's sizes (encoder
2000-1000-300, z 50, decoder 300-1000-2000, conv depth 40, temperature), seeded random weights, one row (the wild type).

    python scripts/bench_trancepteve.py [--samples 2000] [--rounds 5] [--warmup 40] [--parent_samples 200] [--batches 0,1,2]

Times pgmi_eve_log_prior per sample by device events (pgmi_profile_* on pgmi_eve_profile_model's handle: hidden layers, fused final
layer, log-softmax + accumulators; the classes do not overlap) against the route to the same numbers without it: pgmi_eve_elbo at
M = 1, one call per sample (weight sampler into the [20 L][H] matrix, hidden layers, final GEMM, reduction; its encoder time is kept
apart, since pgmi_eve_log_prior encodes once per call).  Both run in the same process in ``--rounds`` alternating rounds; the spread
over the rounds is reported.  ``--batches``: values of the eve_prior_batch option to time as well (0 = default).  Bytes and operations
are derived from the shapes.  Prints one JSON line.
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

NEW = {"hidden": 5, "final_fused": 6, "finish": 8}                                   # include/pgmi.h PGMI_K_*
OLD = {"sampler": 0, "hidden": 5, "final_gemm": 6, "reduction": 8}
ENCODER = 7


def classes(lib, h, names):
    out = {}
    for name, k in names.items():
        ms, n = C.c_double(), C.c_int64()
        _lib.check(lib.pgmi_profile_get(h, k, C.byref(ms), C.byref(n), None, None))
        out[name] = ms.value
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=2000, help="samples of pgmi_eve_log_prior, over all rounds")
    ap.add_argument("--parent_samples", type=int, default=200, help="pgmi_eve_elbo calls (M = 1), over all rounds")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--L", type=int, default=286)
    ap.add_argument("--batches", type=str, default="0,1,2")
    ap.add_argument("--full", type=int, default=200000, help="samples per seed of the reference's launcher")
    ap.add_argument("--seeds", type=int, default=5)
    a = ap.parse_args()
    d = dict(seq_len=a.L, z_dim=50, enc_sizes=[2000, 1000, 300], dec_sizes=[300, 1000, 2000], conv_depth=40, temperature=1,
             sparsity_tiles=0, enc_act="relu", dec_first_act="relu", dec_last_act="relu", dropout_p=0.1)
    sd = eve.random_state_dict(d, seed=1, log_var=(-8.0, -4.0))
    res = np.random.default_rng(2).integers(0, 20, size=(1, a.L)).astype(np.uint8)
    lib = _lib.load()
    if lib.pgmi_device_count() <= 0:
        raise RuntimeError("bench_trancepteve.py needs a GPU: libpgmi has no CPU fallback")
    model = eve.EveModel(d, eve.blob_from_state_dict(sd, d))
    h = model.profile_handle()
    model.log_prior(res[0], a.warmup, seed=0)
    for j in range(4):
        model.elbo(res, seed=0, sample=j)
    _lib.check(lib.pgmi_profile_enable(h, 1))
    per_new, per_old = a.samples // a.rounds, max(1, a.parent_samples // a.rounds)
    batches = [int(b) for b in a.batches.split(",")]
    new = {b: [] for b in batches}
    new_split, old, old_split, old_encoder, wall_new, wall_old = [], [], [], [], [], []
    for r in range(a.rounds):
        for b in batches:
            _lib.check(lib.pgmi_set_option(b"eve_prior_batch", b))
            _lib.check(lib.pgmi_profile_reset(h))
            t0 = time.perf_counter()
            model.log_prior(res[0], per_new, seed=r)
            w = time.perf_counter() - t0
            c = classes(lib, h, NEW)
            new[b].append(sum(c.values()) / per_new)
            if b == batches[0]:
                new_split.append({k: v / per_new for k, v in c.items()})
                wall_new.append(1e3 * w / per_new)
        _lib.check(lib.pgmi_set_option(b"eve_prior_batch", 0))
        _lib.check(lib.pgmi_profile_reset(h))
        t0 = time.perf_counter()
        for j in range(per_old):
            model.elbo(res, seed=r, sample=j)
        wall_old.append(1e3 * (time.perf_counter() - t0) / per_old)
        c = classes(lib, h, OLD)
        old.append(sum(c.values()) / per_old)
        old_split.append({k: v / per_old for k, v in c.items()})
        old_encoder.append(classes(lib, h, {"encoder": ENCODER})["encoder"] / per_old)
    _lib.check(lib.pgmi_profile_enable(h, 0))
    model.close()
    L, H, Cc = a.L, 2000, 40
    weights = Cc * L * H
    hidden = 300 * 50 + 1000 * 300 + 2000 * 1000
    spread = lambda v: {"min": min(v), "median": float(np.median(v)), "max": max(v)}
    mean_split = lambda rows: {k: float(np.mean([x[k] for x in rows])) for k in rows[0]}
    med_new = float(np.median(new[batches[0]]))
    out = {"bench": "trancepteve_log_prior", "L": L, "samples": a.samples, "parent_samples": per_old * a.rounds, "rounds": a.rounds,
           "new_ms_per_sample": {str(b): spread(v) for b, v in new.items()}, "new_split_ms_per_sample": mean_split(new_split),
           "new_wall_ms_per_sample": spread(wall_new),
           "parent_ms_per_sample": spread(old), "parent_split_ms_per_sample": mean_split(old_split),
           "parent_encoder_ms_per_sample": spread(old_encoder), "parent_wall_ms_per_sample": spread(wall_old),
           "speedup_median_device_time": float(np.median(old)) / med_new,
           "projected_hours_for_seeds_x_full": med_new * a.full * a.seeds / 3.6e6, "full": a.full, "seeds": a.seeds,
           "derived": {"final_weights_per_sample": weights, "hidden_weights_per_sample": hidden,
                       "normals_per_sample": weights + hidden, "philox_counters_per_sample": (weights + hidden) // 4,
                       # the fused final kernel shares its read among a launch's samples; the hidden kernels (grid.y = sample) do not
                       "final_mean_sd_bytes_per_launch": 8 * weights, "hidden_mean_sd_bytes_per_sample": 8 * hidden,
                       "conv_flops_per_sample": 2 * 20 * weights,
                       "parent_w_final_bytes_written_and_read_per_sample": 2 * 4 * 20 * L * H}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
