#!/usr/bin/env python
"""Benchmark of the hot path: mutants scored per second, ESM-1v 650M masked-marginals.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--precision fp32] [--dump-outputs DIR] [--full]

One *step* = one pass of the hot path over one assay-shaped batch resident in HBM:
BASELINE.json configs[1] -- ESM-1v 650M (33 x 1280 x 20 heads x 5120), one assay shaped like
BLAT_ECOLX_Stiffler_2015 (L=286 -> T=288 tokens, 4 996 single mutants), ONE checkpoint:
masked windows -> 33-layer forward over every masked position -> LM head on the masked rows
-> log-softmax table -> per-mutant score (label_row).  Synthetic sequence, synthetic
random-init weights (no network), deterministic seeds.

N > 1 (launched by torch.distributed.run, one rank per GPU): the SAME step on every rank -- one BLAT-shaped assay per rank per
step (its own synthetic assay), then the path's one exchange: an RCCL all_gather of the per-mutant score vectors.  Per-GPU work
is fixed ("scaling": "weak"), value = N x 4 996 x K mutants / max-over-ranks seconds, so value(N) / (N x value(1)) is the scaling
efficiency of the step the N = 1 line measures.  With --full, after that timed region the line gains `strong_scaling_217`: ONE pass
over the 217-assay-shaped substitution benchmark (2 465 767 mutants, the north star's workload) with the assays sharded over the ranks by
the product planner (run_benchmark.plan_assays), inputs resident, timed with its own barriers (scripts/bench_scale.py); its
one-GPU point is the N = 1 --full line's `one_gpu_same_workload_mutants_per_s`.

A plain run does only what the headline needs: set-up, W warm-up steps, the K timed steps, the
--dump-outputs arrays, and the JSON line with `roofline` (dominant kernel = the FFN GEMMs, HIP-event
timed inside the timed region, against the MFMA peak of the dtype) and `kernels` from that same
region.  --full adds everything that takes work of its own after the timed region: `box` (clock and
power during extra steps), roofline.traffic from in-run rocprofv3 --pmc passes, the end-to-end
fields, `cpu_baseline` (the oracle's CPU restatement of the reference path timed on this box's host
cores, bounded sample) with `parity`, the `secondary` configurations and, N > 1, `strong_scaling_217`.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
# RCCL / device-tensor sharing between the ranks of one node needs dmabuf IPC handles on this driver (without it:
# `hipIpcGetMemHandle: invalid argument`); exported on the pool's boxes already -- kept here for any other launcher
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

PEAK_TFLOPS = {"fp32": 157.3, "bf16": 2500.0, "f16x3": 2500.0}   # MI355X_MICROARCH.md, dense
L_BLAT, N_MUT_BLAT = 286, 4996
PMC_TRAFFIC = os.path.join(ROOT, "profiles", "r6", "pmc_traffic.json")


def ffn_traffic(precision, M, D, F, live=None):
    """HBM-side bytes per FFN GEMM launch from rocprofv3 --pmc passes of this same command (FETCH_SIZE and WRITE_SIZE in separate
    runs, FETCH_SIZE doubled per MI355X_MICROARCH.md).  ``live``: the passes `live_traffic` collected on THIS box after the timed
    region (preferred); otherwise the committed file of scripts/pmc_profile.sh -- only when it was taken on THIS build: it is
    stamped with build_native._digest() (sha256 over the kernel sources, headers and compiler flags); any other digest, precision
    or shape gives traffic = null and says why."""
    if precision != "f16x3":
        return None, {"unavailable": "PMC passes were taken on the f16x3 kernels only"}
    from proteingym_amd import build_native
    if live is not None and live.get("kernels"):
        doc, where = live, "rocprofv3 --pmc passes run by bench.py itself on this box, after the timed region"
    else:
        why_not_live = (live or {}).get("unavailable", "not attempted")
        if not os.path.exists(PMC_TRAFFIC):
            return None, {"unavailable": f"{os.path.relpath(PMC_TRAFFIC, ROOT)} not found", "in_run_passes": why_not_live}
        doc = json.load(open(PMC_TRAFFIC))
        where = f"{os.path.relpath(PMC_TRAFFIC, ROOT)} (committed passes of scripts/pmc_profile.sh; in-run passes: {why_not_live})"
        if doc.get("lib_digest") != build_native._digest():
            return None, {"unavailable": f"{os.path.relpath(PMC_TRAFFIC, ROOT)} was collected on another build of the kernels "
                                         f"(digest {str(doc.get('lib_digest'))[:12]} != {build_native._digest()[:12]}): re-run scripts/pmc_profile.sh",
                          "in_run_passes": why_not_live}
    if doc.get("rows_per_launch") not in (None, M):
        return None, {"unavailable": f"PMC passes cover launches of {doc.get('rows_per_launch')} rows, this run has {M}"}
    k = doc["kernels"]
    fc1 = next((v for n, v in k.items() if "gemm16x_kernel<1, 1," in n), None)          # FC1 + GELU, split output
    fc2 = next((v for n, v in k.items() if "gemm16x_kernel<0, 0," in n), None)          # FC2 and out-projection share a kernel
    if not fc1 or not fc2:
        return None, {"unavailable": "kernel names not found in the PMC summary"}
    algo = {"fc1": {"read": 4.0 * (M * D + F * D), "write": 4.0 * M * F}, "fc2_and_out_mean": {"read": 4.0 * (M * (F + D) / 2 + (D * F + D * D) / 2) + 4.0 * M * D, "write": 4.0 * M * D}}
    detail = {"fc1": {"fetch_bytes": fc1["fetch_bytes"], "write_bytes": fc1["write_bytes"], "algorithmic_read": algo["fc1"]["read"],
                      "algorithmic_write": algo["fc1"]["write"], "fetch_over_algorithmic": fc1["fetch_bytes"] / algo["fc1"]["read"],
                      "l2_hit_rate": fc1.get("l2_hit_rate")},
              "fc2_and_out_projection_mean": {"fetch_bytes": fc2["fetch_bytes"], "write_bytes": fc2["write_bytes"],
                                              "algorithmic_read": algo["fc2_and_out_mean"]["read"], "algorithmic_write": algo["fc2_and_out_mean"]["write"],
                                              "fetch_over_algorithmic": fc2["fetch_bytes"] / algo["fc2_and_out_mean"]["read"],
                                              "l2_hit_rate": fc2.get("l2_hit_rate")},
              "lib_digest": str(doc.get("lib_digest"))[:16], "git_head": doc.get("git_head"),
              "source": where + "; separate FETCH_SIZE / WRITE_SIZE passes of `bench.py --layers 2..4` (every dispatch at the full row "
                                "count); bytes at the L2<->fabric boundary: requests served by the 256 MB Infinity Cache are counted"}
    return fc1["fetch_bytes"] + fc1["write_bytes"], detail


def live_traffic(precision, timeout_s=90):
    """FETCH_SIZE / WRITE_SIZE of the GEMM launches collected NOW, on this box: two `rocprofv3 --kernel-trace --pmc <counter>` child
    runs of this script (2 layers, one step, every dispatch at the full row count), parsed like scripts/pmc_summarize.py.  Counters
    cannot be read from inside a run, so the children run after the timed region.  Never raises: {"unavailable": reason}."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    from collections import defaultdict
    try:
        exe = shutil.which("rocprofv3") or ("/opt/rocm/bin/rocprofv3" if os.path.exists("/opt/rocm/bin/rocprofv3") else None)
        if precision != "f16x3":
            return {"unavailable": "f16x3 only"}
        if exe is None:
            return {"unavailable": "rocprofv3 not on this box"}
        from proteingym_amd import build_native
        agg = defaultdict(lambda: defaultdict(lambda: [0.0, 0]))
        with tempfile.TemporaryDirectory(dir="/tmp") as d:
            env = dict(os.environ, PGMI_KEEP_ROWS="0", TMPDIR="/tmp")
            for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
                env.pop(k, None)
            for counter in ("FETCH_SIZE", "WRITE_SIZE"):
                cmd = [exe, "--kernel-trace", "--pmc", counter, "--output-format", "csv", "-d", os.path.join(d, counter), "-o", "p", "--",
                       sys.executable, os.path.abspath(__file__), "--steps", "1", "--warmup", "0", "--layers", "2", "--precision", precision]
                done = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout_s, env=env, cwd="/tmp")
                if done.returncode != 0:
                    return {"unavailable": f"rocprofv3 --pmc {counter} exited {done.returncode}: {done.stderr.strip()[-200:]}"}
                for f in glob.glob(os.path.join(d, counter, "**", "*counter_collection.csv"), recursive=True):
                    for r in csv.DictReader(open(f)):
                        a = agg[r["Kernel_Name"].split("(")[0][:60]][r["Counter_Name"]]
                        a[0] += float(r["Counter_Value"])
                        a[1] += 1
        kernels = {}
        for name, c in agg.items():
            if "gemm16x_kernel" not in name or "FETCH_SIZE" not in c or "WRITE_SIZE" not in c:
                continue
            kernels[name] = {"dispatches": c["FETCH_SIZE"][1], "fetch_bytes": c["FETCH_SIZE"][0] / c["FETCH_SIZE"][1] * 1024 * 2,
                             "write_bytes": c["WRITE_SIZE"][0] / c["WRITE_SIZE"][1] * 1024}
        if not kernels:
            return {"unavailable": "no gemm16x_kernel dispatch in the counter files"}
        return {"lib_digest": build_native._digest(), "git_head": os.environ.get("PGMI_GIT_HEAD"), "rows_per_launch": None, "kernels": kernels}
    except Exception as e:                                             # noqa: BLE001 -- a profiler hiccup must never take the line down
        return {"unavailable": repr(e)}


def end_to_end_fields(e2e, b217):
    """Top-level keys that carry the metric SURVEY 8d defines (weights resident -> CSV written) beside the device-only `value`:
    e2e = {"mutants", "seconds", ...} of the BLAT-shaped assay through parse + upload + run + D2H + CSV; b217 = the
    benchmark_217_end_to_end leg (or None)."""
    out = {}
    if e2e and e2e.get("seconds"):
        out["value_end_to_end"] = e2e["mutants"] / e2e["seconds"]
        out["value_end_to_end_detail"] = e2e
    if b217 and b217.get("seconds"):
        out["benchmark_217_end_to_end_mutants_per_s"] = b217["mutants"] / b217["seconds"]
        if b217.get("rank0_wall_clock", {}).get("assay_run_s"):
            # the one-GPU point of the N > 1 line's strong_scaling_217 (same workload, same timed region: mutants / seconds inside the scorer)
            out["one_gpu_same_workload_mutants_per_s"] = b217["mutants"] / b217["rank0_wall_clock"]["assay_run_s"]
            out["one_gpu_same_workload"] = ("the 217-assay-shaped table of the N > 1 lines' strong_scaling_217 on one GPU (secondary."
                                            "benchmark_217_end_to_end: mutants / rank0_wall_clock.assay_run_s); its scaling efficiency at N GPUs = "
                                            "strong_scaling_217.mutants_per_s / (N * this number)")
    return out


def box_state(step, seconds=2.0):
    """Shader clock and socket power WHILE the hot path runs (untimed extra steps in a thread, `rocm-smi` sampled beside them):
    boxes of this pool differ by +-3 % under the 1 400 W cap, and the line should say which kind of box it was measured on.
    Never raises: {"unavailable": reason} instead."""
    import re
    import subprocess
    import threading
    try:
        stop = threading.Event()

        def spin():
            while not stop.is_set():
                step()
        th = threading.Thread(target=spin, daemon=True)
        th.start()
        clocks, watts = [], []
        t_end = time.perf_counter() + seconds
        try:
            while time.perf_counter() < t_end:
                txt = subprocess.run(["rocm-smi", "--showpower", "--showclocks"], capture_output=True, text=True, timeout=10).stdout
                c = re.search(r"sclk clock level:?\s*\d*:?\s*\(?(\d+)\s*Mhz", txt, re.I)
                w = re.search(r"Power \(W\):\s*([\d.]+)", txt)
                if c:
                    clocks.append(int(c.group(1)))
                if w:
                    watts.append(float(w.group(1)))
        finally:
            stop.set()
            th.join()
        if not clocks and not watts:
            return {"unavailable": "rocm-smi printed neither a shader clock nor a socket power"}
        return {"sclk_mhz": round(sum(clocks) / len(clocks)) if clocks else None,
                "socket_power_w": round(sum(watts) / len(watts)) if watts else None, "samples": max(len(clocks), len(watts)),
                "what": "rocm-smi --showpower --showclocks sampled during untimed extra steps of the same assay, after the timed region"}
    except Exception as e:                                             # noqa: BLE001 -- monitoring must never take the line down
        return {"unavailable": repr(e)}


def usable_cores() -> int:
    """Host cores this process may actually use: affinity mask capped by the cgroup CPU quota
    (the GPU box shows 256 logical CPUs but grants a 16-CPU quota; oversubscribing it with 256
    threads is ~1000x slower)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except Exception:
        pass
    return max(1, n)


def cpu_baseline(cfg, blob, seq, n_mut, budget_s, gpu_table=None):
    """The reference algorithm on the host cores: batch-1 masked forwards (compute_fitness.py:
    489-503) through oracle/esm_oracle.py (torch CPU fp32), bounded to ~budget_s seconds: when a
    full 33-layer forward does not fit the budget, k of the 33 (identical-cost) layers are timed
    and scaled by 33/k."""
    import torch
    from oracle import esm_oracle as eo
    from proteingym_amd import synthetic
    cores = usable_cores()
    torch.set_num_threads(cores)
    ocfg, W = eo.from_arrays(arrays=synthetic.blob_to_arrays(cfg, blob), **cfg)
    toks = eo.tokenize(seq)
    n_tok, L = len(toks), ocfg["layers"]

    rows = {}

    def fwd(i, k):
        t = toks.copy()
        t[i] = eo.MASK
        t0 = time.perf_counter()
        with torch.no_grad():
            row = torch.log_softmax(eo.forward_logits(ocfg, W, t[None], n_layers=k), dim=-1)[0, i]
        dt = time.perf_counter() - t0
        if k == L:
            rows[i] = row.numpy()
        return dt

    fwd(1, 2)                                   # warm-up (threads, first-touch of two layers)
    per_layer = fwd(2, 2) / 2
    reps = 3
    k = int(max(2, min(L, budget_s / reps / max(per_layer, 1e-6))))
    if k < L:
        fwd(3, k)                               # first touch of the k layers' weights: not timed
    else:                                       # full-depth forwards fit: as many of them as the budget holds (<= 32)
        reps = int(max(3, min(32, budget_s / max(per_layer * L, 1e-6))))
    ts = [fwd(1 + (3 + r) % (n_tok - 2), k) for r in range(reps)]
    per_fwd = float(np.mean(ts)) * L / k
    assay_s = per_fwd * n_tok                   # the reference runs all L+2 positions, batch 1
    out = {"value": n_mut / assay_s, "unit": "mutants/s", "cores": cores, "kind": "port",
           "sample": f"{reps} batch-1 masked forwards at T={n_tok} through {k} of {L} layers "
                     f"(oracle/esm_oracle.py, torch CPU fp32, {cores} threads), scaled x{L}/{k}: "
                     f"{per_fwd:.3f} s/forward, x{n_tok} forwards for the assay"}
    # the full-depth oracle rows just computed double as a live parity check of the GPU table (checker only)
    parity = None
    if gpu_table is not None:
        common = [i for i in rows if not np.isnan(gpu_table[i, 0])]
        if common:
            parity = {"max_abs_err_vs_oracle": float(max(np.abs(gpu_table[i] - rows[i]).max() for i in common)),
                      "rows_compared": len(common), "tolerance": 1e-4,
                      "what": "log-prob table rows (33 values each) of the timed assay, HIP path vs CPU fp32 oracle"}
    return out, parity


def secondary(precision, budget_note="bounded: every leg is a few seconds of GPU time"):
    """Other BASELINE.json configurations and the ensemble / end-to-end rates, measured on this GPU after the headline
    (never inside its timed region).  Same synthetic conventions as the headline."""
    import tempfile
    import pandas as pd
    from proteingym_amd import esm as pesm, synthetic, dist as pdist
    out = {"note": budget_note}

    def timed(fn, reps=2):
        fn()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        return (time.perf_counter() - t0) / reps

    seq, muts, _ = synthetic.random_assay(seed=23, L=L_BLAT, n_single=N_MUT_BLAT, n_multi=0)
    cfg = dict(synthetic.ESM1V_650M)

    # every leg is independent (own models, closed at its end) and individually guarded: one failing leg costs that leg only
    def leg_ensemble():
        # (1) ESM-1v ensemble rate: five checkpoints per assay, plain mean (compute_fitness.py:532-537)
        cfg = dict(synthetic.ESM1V_650M)
        blob = synthetic.random_weights(cfg, seed=2)
        models = [pesm.EsmModel(cfg, blob, device=0, precision=precision) for _ in range(5)]
        assays = [pesm.Assay(m, seq, muts) for m in models]
        dt = timed(lambda: [a.run_device_only() for a in assays])
        out["esm1v_5_checkpoint_ensemble"] = {"mutants_per_s": len(muts) / dt, "ms_per_assay": dt * 1e3,
                                              "what": "BLAT-shaped assay scored with 5 resident ESM-1v-650M-shaped checkpoints"}
        for a in assays:
            a.close()
        for m in models:
            m.close()

    def leg_bf16():
        # (0) BASELINE configs[1] names "bf16": the plain-bf16 THROUGHPUT mode (one v_mfma_f32_32x32x16_bf16 per product block, fp32 accumulate) on
        #     the headline's assay, with its error MEASURED against the parity-gated f16x3 scores of the same weights -- never assumed: bf16
        #     operands carry 8 bits, the 1e-4 bar needs ~22 (~1 % of the log-prob range)
        from scipy.stats import spearmanr
        cfgb = dict(synthetic.ESM1V_650M)
        blobb = synthetic.random_weights(cfgb, seed=2, embed_std=0.15)
        scores = {}
        rate = {}
        for prec in ("f16x3", "bf16"):
            m = pesm.EsmModel(cfgb, blobb, device=0, precision=prec)
            a = pesm.Assay(m, seq, muts)
            rate[prec] = timed(a.run_device_only)
            scores[prec] = np.asarray(a.run(), dtype=np.float64)
            a.close()
            m.close()
        err = float(np.abs(scores["bf16"] - scores["f16x3"]).max())
        out["bf16_throughput_mode"] = {"mutants_per_s": len(muts) / rate["bf16"], "ms_per_assay": rate["bf16"] * 1e3,
                                       "f16x3_same_weights_mutants_per_s": len(muts) / rate["f16x3"],
                                       "max_abs_score_difference_vs_f16x3": err, "score_range": float(np.ptp(scores["f16x3"])),
                                       "spearman_bf16_vs_f16x3": round(float(spearmanr(scores["bf16"], scores["f16x3"])[0]), 4),
                                       "parity_gated": False,
                                       "what": "BASELINE configs[1] in plain bf16 (--precision bf16; round 6: the persistent ping-pong GEMM kernel in its one-plane "
                                               "form -- 64-deep K tiles, one v_mfma_f32_32x32x16_bf16 per product block --, the attention on the split-fp16 pipe from the "
                                               "fused QKV epilogue, context rows as one bf16 plane): NOT parity-gated -- its distance to the parity-gated f16x3 "
                                               "scores of the same checkpoint is measured here; the headline runs f16x3, which holds the 1e-4 bar"}

    def leg_benchmark_217():
        # (2) the WHOLE 217-assay-shaped substitution benchmark end to end through the product runner: checkpoint read + upload, DMS
        #     files read, mutants parsed + uploaded, masked-marginals with optimal 1024 windows, CSVs written (1 checkpoint)
        sys.path.insert(0, os.path.join(ROOT, "scripts"))
        import bench_217
        from proteingym_amd import run_benchmark
        blob = synthetic.random_weights(cfg, seed=2)
        n_assays = int(os.environ.get("PGMI_BENCH_217_ASSAYS", "217"))
        with tempfile.TemporaryDirectory() as d:
            os.makedirs(os.path.join(d, "dms"))
            shapes = synthetic.dms_shapes()[:n_assays]
            rows = []
            t0 = time.perf_counter()
            for sh in shapes:
                rng = np.random.default_rng(sh["DMS_index"])
                sq, df = bench_217.make_assay(rng, sh["seq_len"], sh["n_single"], sh["n_total"] - sh["n_single"])
                df.to_csv(os.path.join(d, "dms", sh["DMS_id"] + ".csv"), index=False)
                rows.append({"DMS_id": sh["DMS_id"], "DMS_filename": sh["DMS_id"] + ".csv", "target_seq": sq, "DMS_total_number_mutants": len(df)})
            pd.DataFrame(rows).to_csv(os.path.join(d, "map.csv"), index=False)
            ck = synthetic.save_fair_esm_checkpoint(os.path.join(d, "esm1v_synth_1.pt"), cfg, blob)
            gen_s = time.perf_counter() - t0
            a8 = run_benchmark.create_parser().parse_args(["--model-location", ck, "--model_type", "ESM1v", "--dms_mapping", os.path.join(d, "map.csv"),
                                                           "--dms-input", os.path.join(d, "dms"), "--dms-output", os.path.join(d, "out"), "--precision", precision])
            t0 = time.perf_counter()
            st = run_benchmark.main(a8)
            dt = time.perf_counter() - t0
        log = st["rank0_assays"]
        fl = [e["positions_run"] * pdist.forward_flops(e["T"]) for e in log]
        bins = [(0, 60), (60, 100), (100, 200), (200, 400), (400, 1023), (1023, 10 ** 9)]
        hist = []
        for lo, hi in bins:
            sel = [k for k, e in enumerate(log) if lo <= e["seq_len"] < hi]
            if sel:
                t = sum(log[k]["run_s"] for k in sel)
                hist.append({"residues": f"{lo}-{hi - 1}" if hi < 10 ** 9 else f">={lo}", "assays": len(sel), "seconds_in_Assay_run": round(t, 2),
                             "executed_tflops": round(sum(fl[k] for k in sel) / max(t, 1e-9) / 1e12, 1),
                             "min_assay_tflops": round(min(fl[k] / max(log[k]["run_s"], 1e-9) for k in sel) / 1e12, 1),
                             "max_assay_tflops": round(max(fl[k] / max(log[k]["run_s"], 1e-9) for k in sel) / 1e12, 1)})
        clock = {k: round(v, 2) for k, v in st["rank0_wall_clock"].items()}
        out["benchmark_217_end_to_end"] = {
            "mutants_per_s": st["mutants"] / dt, "seconds": dt, "mutants": st["mutants"], "assays": st["assays"],
            "positions_run": int(sum(e["positions_run"] for e in log)), "positions_the_reference_runs": int(sum(e["seq_len"] + 2 for e in log)),
            "executed_algorithmic_pflop": sum(fl) / 1e15, "executed_tflops_over_wall": sum(fl) / dt / 1e12,
            "executed_tflops_inside_Assay_run": sum(fl) / max(clock.get("assay_run_s", 0.0), 1e-9) / 1e12,
            "rank0_wall_clock": clock,
            "wall_split": "checkpoint_load_s = read + split + upload of the 2.6 GB checkpoint; assay_create_s = mutant parse + upload; "
                          "assay_run_s = GPU + 8 bytes per mutant back (the one-GPU point of the N > 1 strong-scaling curve); wait_read_s / "
                          "wait_write_s = time the scoring loop waited for the background DMS reader / CSV writer",
            "per_assay_rate_by_protein_length": hist, "setup_seconds_not_timed": round(gen_s, 1),
            "what": f"the {'whole ' if n_assays >= 217 else 'first ' + str(n_assays) + ' assays of the '}217-assay-shaped benchmark through run_benchmark (1 checkpoint, CSVs written)"}

    def leg_esm2_3b():
        # (3) BASELINE config 3's model: ESM2-3B (36 x 2560 x 40), one BLAT-shaped assay
        cfg3 = dict(synthetic.ESM2_3B)
        n3 = sum(int(np.prod(sh)) for _, sh in synthetic.key_shapes(cfg3))
        block = (np.random.default_rng(3).random(1 << 24, dtype=np.float32) - 0.5) * 0.04      # timing only: a tiled random block
        blob3 = np.tile(block, n3 // block.size + 1)[:n3]
        m3 = pesm.EsmModel(cfg3, blob3, device=0, precision=precision)
        del blob3
        a3 = pesm.Assay(m3, seq, muts)
        dt = timed(a3.run_device_only, reps=1)
        fl = len(a3.positions) * pdist.forward_flops(a3.T, layers=36, D=2560, F=10240)
        out["esm2_3b_one_assay"] = {"mutants_per_s": len(muts) / dt, "ms_per_assay": dt * 1e3, "algorithmic_tflops": fl / dt / 1e12,
                                    "what": "config 3 model shape, BLAT-shaped assay (286 positions x 288 tokens), 1 GPU"}
        a3.close()
        m3.close()

    def leg_pseudo_ppl():
        # (4) BASELINE config 5: pseudo-ppl on a CAPSD_AAV2S-shaped slice (variable-length members, ESM2-650M shape): six members =
        #     4 400 masked forwards of ~737 tokens, several workspace batches -> the steady-state rate of the packed path
        cfg5 = dict(synthetic.ESM2_650M)
        m5 = pesm.EsmModel(cfg5, synthetic.random_weights(cfg5, seed=5), device=0, precision=precision)
        n5 = 6
        lib5 = pesm.SequenceLibrary(m5, synthetic.random_indel_library(7, 735, n5)[1])
        lib5.score(first=0, count=1)                                        # warm-up
        t0 = time.perf_counter()
        lib5.score()
        dt = time.perf_counter() - t0
        st = lib5.stats()
        fl5 = st["rows"] * pdist.forward_flops(737)
        out["esm2_650m_pseudo_ppl_capsd_shaped"] = {"mutants_per_s": n5 / dt, "masked_forwards_per_s": st["rows"] / dt, "tokens_per_s": st["tokens"] / dt,
                                                    "packing_efficiency": st["packing_efficiency"], "batches": st["batches"], "seconds": dt,
                                                    "algorithmic_tflops": fl5 / dt / 1e12,
                                                    "what": f"config 5: {n5} members of a 735-residue indel library = {st['rows']} masked forwards of ~737 tokens"}
        lib5.close()
        m5.close()

    def leg_tranception():
        # (5) BASELINE config 4's model: Tranception-L shape, both directions; one 485-mutant batch without retrieval, then a WHOLE
        #     BLAT-shaped assay (4 996 rows) with inference-time retrieval: alignment parsed, EVE sequence weights counted by the HIP
        #     kernel, prior built and fused on the device
        from proteingym_amd import tranception as ptr
        cfgt = dict(synthetic.TRANCEPTION_L)
        mt = ptr.TranceptionModel(cfgt, synthetic.random_tranception_weights(cfgt, seed=3), device=0)
        sq, mu, _ = synthetic.random_assay(seed=23, L=L_BLAT, n_single=512, n_multi=0)
        df = pd.DataFrame({"mutant": mu})
        df["mutated_sequence"] = df["mutant"].apply(lambda m: ptr.get_mutated_sequence(sq, m))
        df = df.drop_duplicates("mutated_sequence")
        mt.score_mutants(DMS_data=df.iloc[:32], target_seq=sq)
        timing = {}
        for share in (False, True):                 # the reference's loop (every sequence in full), then prefix-shared: same bits
            mt.share_prefix = share
            mt.rows_forwarded = mt.rows_full = 0
            t0 = time.perf_counter()
            mt.score_mutants(DMS_data=df, target_seq=sq, scoring_mirror=True)
            timing[share] = (time.perf_counter() - t0, mt.rows_forwarded, mt.rows_full)
        dt = timing[True][0]
        out["tranception_l_one_batch"] = {"mutants_per_s": len(df) / dt, "seconds": dt, "mutants": len(df),
                                          "full_forward_mutants_per_s": len(df) / timing[False][0],
                                          "rows_forwarded": timing[True][1], "rows_of_the_full_forwards": timing[True][2],
                                          "what": "config 4 model shape (36 x 1280 x 20), 286-residue protein, both directions, no retrieval; "
                                                  "prefix-shared (rows from the first mutated token's tile on; bit-identical to "
                                                  "full_forward_mutants_per_s' path, which forwards every sequence in full like the reference)"}
        # a pairwise double-mutant library of the same protein (the benchmark's largest assay is one; 72 % of its rows are multi-mutants): every
        # sequence in full (the reference's loop) against prefix-shared with intermediate roots ("wild type + first substitution")
        rngd = np.random.default_rng(5)
        first = sorted(int(p) for p in rngd.choice(len(sq) // 2, size=24, replace=False))
        second = sorted(int(p) for p in len(sq) // 2 + rngd.choice(len(sq) // 2, size=12, replace=False))
        other = lambda p, k: [c for c in ptr.AA_vocab if c != sq[p]][k]   # noqa: E731
        dm = [f"{sq[i]}{i + 1}{other(i, a)}:{sq[j]}{j + 1}{other(j, b)}" for i in first for a in range(3) for j in second for b in range(2)]
        dd = pd.DataFrame({"mutant": dm, "mutated_sequence": ptr.mutated_sequences(sq, dm)})
        td = {}
        for share in (False, True):
            mt.share_prefix = share
            mt.rows_forwarded = mt.rows_full = 0
            t0 = time.perf_counter()
            mt.score_mutants(DMS_data=dd, target_seq=sq, scoring_mirror=True)
            td[share] = (time.perf_counter() - t0, mt.rows_forwarded, mt.rows_full)
        out["tranception_l_pairwise_double_mutants"] = {"mutants_per_s": len(dd) / td[True][0], "seconds": td[True][0], "mutants": len(dd),
                                                        "full_forward_mutants_per_s": len(dd) / td[False][0],
                                                        "rows_forwarded": td[True][1], "rows_of_the_full_forwards": td[True][2],
                                                        "what": "config 4 model shape, 1 728 double mutants (24 x 3 first, 12 x 2 second substitutions), both "
                                                                "directions, no retrieval; prefix-shared with intermediate roots; same bits as the full forwards"}
        with tempfile.TemporaryDirectory() as d:
            rng = np.random.default_rng(11)
            n_seq, aa = 4000, np.array(list(synthetic.AA))
            wt_idx = np.array([synthetic.AA.index(c) for c in sq])
            msa = np.tile(wt_idx, (n_seq, 1))
            flip = rng.random(msa.shape) < rng.uniform(0.05, 0.6, size=(n_seq, 1))       # members 5 .. 60 % away from the query
            msa[flip] = rng.integers(0, 20, size=int(flip.sum()))
            msa[0] = wt_idx
            gaps = rng.random(msa.shape) < 0.03
            gaps[0] = False
            with open(os.path.join(d, "synth.a2m"), "w") as f:
                for k in range(n_seq):
                    row = aa[msa[k]]
                    row[gaps[k]] = "-"
                    f.write(f">seq{k}/1-{L_BLAT}\n{''.join(row)}\n")
            sq2, mu2, _ = synthetic.random_assay(seed=23, L=L_BLAT, n_single=N_MUT_BLAT, n_multi=0)
            assert sq2 == sq
            full = pd.DataFrame({"mutant": mu2})
            full["mutated_sequence"] = [ptr.get_mutated_sequence(sq, m) for m in mu2]
            t0 = time.perf_counter()
            wfile = os.path.join(d, "weights.npy")
            ptr.MSA_processing(MSA_location=os.path.join(d, "synth.a2m"), weights_location=wfile, device=0)       # counts on the GPU, saved
            t_w = time.perf_counter() - t0
            mt.retrieval = ptr.build_retrieval(dict(MSA_filename=os.path.join(d, "synth.a2m"), MSA_weight_file_name=wfile, MSA_start=0,
                                                    MSA_end=L_BLAT, full_protein_length=L_BLAT, retrieval_inference_weight=0.6))
            t_p = time.perf_counter() - t0 - t_w
            mt.rows_forwarded = mt.rows_full = 0
            res = mt.score_mutants(DMS_data=full, target_seq=sq, scoring_mirror=True)
            dt = time.perf_counter() - t0
        out["tranception_l_whole_assay_with_retrieval"] = {
            "mutants_per_s": len(full) / dt, "seconds": dt, "mutants": len(full), "scored_sequences": int(len(res)),
            "sequence_weights_s": t_w, "prior_s": t_p, "scoring_s": dt - t_w - t_p,
            "rows_forwarded": mt.rows_forwarded, "rows_of_the_full_forwards": mt.rows_full,
            "tokens_per_s": 2 * len(res) * (L_BLAT + 2) / max(dt - t_w - t_p, 1e-9),
            "what": f"config 4 model shape, BLAT-shaped assay ({len(full)} rows), both directions, inference-time retrieval on a synthetic {n_seq}-sequence "
                    "alignment (weights by the HIP pair-count kernel, prior fused on the device)"}
        mt.close()

    def leg_tranception_217_projection():
        # (6) config 4 AT WORKLOAD SCALE: one synthetic assay per protein-length bin of the 217-assay table (real length, single and
        #     multi-mutant rows scored separately, both directions, prefix-shared) -> seconds per unit of the product planner's cost ->
        #     every row of the real table (scripts/bench_projection.py)
        sys.path.insert(0, os.path.join(ROOT, "scripts"))
        import bench_projection as bp
        from proteingym_amd import tranception as ptr
        cfgt = dict(synthetic.TRANCEPTION_L)
        mt = ptr.TranceptionModel(cfgt, synthetic.random_tranception_weights(cfgt, seed=3), device=0)
        shapes = synthetic.dms_shapes()
        t0 = time.perf_counter()
        unit, detail = bp.measure_tranception(mt, bp.tranception_sample(shapes), ptr)
        measured_s = time.perf_counter() - t0
        mt.close()
        proj = bp.project_tranception(shapes, unit)
        ref_pflop = sum(bp.tranception_flops(s["seq_len"], s["n_total"]) for s in shapes) / 1e15
        out["tranception_217_projection"] = {
            **proj, "reference_loop_algorithmic_pflop": ref_pflop, "reference_loop_tflops_1_gpu": ref_pflop * 1e3 / proj["seconds_1_gpu"],
            "hours_1_gpu": proj["seconds_1_gpu"] / 3600.0, "minutes_8_gpus_planned": proj["seconds_8_gpus_planned"] / 60.0,
            "sample": detail, "sample_seconds": round(measured_s, 1),
            "what": "PROJECTION of config 4 (Tranception-L, the 217-assay substitution table, 2 465 767 mutants, both directions, no retrieval: "
                    "the prior fusion is one elementwise pass) from a stratified sample: per protein-length bin the assay carrying most of the "
                    "bin's planned cost, <= 384 single and <= 384 multi-mutant rows (depth 2-5) scored separately with the product's defaults "
                    "(prefix sharing + intermediate roots); seconds per unit of run_sharded.chunk_cost applied to every row of the table; N = 8 "
                    "through run_sharded.plan_mutant_chunks.  Model resident, no file I/O; SURVEY 8f estimated ~2 700 PFLOP for the reference's loop"}

    def leg_indels_projection():
        # (7) config 5 AT WORKLOAD SCALE: masked forwards per second of ESM2-650M pseudo-ppl libraries at the cost-weighted quantiles of
        #     the 66-assay indel table's lengths -> seconds per forward (interpolated in FLOPs per forward) -> the whole table
        sys.path.insert(0, os.path.join(ROOT, "scripts"))
        import bench_projection as bp
        cfg5 = dict(synthetic.ESM2_650M)
        m5 = pesm.EsmModel(cfg5, synthetic.random_weights(cfg5, seed=5), device=0, precision=precision)
        shapes = synthetic.indel_shapes()
        t0 = time.perf_counter()
        spf, detail = bp.measure_indels(m5, bp.indel_sample_lengths(shapes), pesm)
        measured_s = time.perf_counter() - t0
        m5.close()
        proj = bp.project_indels(shapes, spf)
        out["indels_projection"] = {
            **proj, "algorithmic_tflops_1_gpu": proj["algorithmic_pflop"] * 1e3 / proj["seconds_1_gpu"], "sample": detail, "sample_seconds": round(measured_s, 1),
            "what": "PROJECTION of config 5 (ESM2-650M pseudo-ppl over the 66 indel assays, 287 207 mutants, one masked forward per (mutant, residue)) "
                    "from measured forwards per second at the table's cost-weighted length quantiles, interpolated in FLOPs per forward; N = 8 through "
                    "run_indels.partition_pool (pooled sequences, LPT).  Model resident, no file I/O; SURVEY 8f estimated ~2e5 PFLOP"}

    only = [x for x in os.environ.get("PGMI_BENCH_LEGS", "").split(",") if x]
    for fn in (leg_bf16, leg_ensemble, leg_benchmark_217, leg_esm2_3b, leg_pseudo_ppl, leg_tranception, leg_tranception_217_projection, leg_indels_projection):
        if only and fn.__name__[4:] not in only:
            continue
        t0 = time.perf_counter()
        try:
            fn()
        except Exception as e:
            import traceback
            traceback.print_exc(file=sys.stderr)
            out[fn.__name__[4:] + "_error"] = repr(e)
        out.setdefault("leg_seconds", {})[fn.__name__[4:]] = round(time.perf_counter() - t0, 1)
    return out


def end_to_end_blat(model, seq, muts, reps=3):
    """The BLAT-shaped assay from mutant STRINGS to a CSV on disk with the weights resident ("weights resident" to "all
    CSVs written"): parse + upload (Assay), run, scores to the host, the assay's frame with its score column written like the CLI
    writes it.  Mean of `reps` runs after one untimed run."""
    import tempfile
    import pandas as pd
    from proteingym_amd import compute_fitness as cf, esm as pesm
    rng = np.random.default_rng(0)
    frame = pd.DataFrame({"mutant": muts, "DMS_score": rng.standard_normal(len(muts))})
    frame["DMS_score_bin"] = (frame["DMS_score"] > 0).astype(int)
    parts = {"assay_create_s": 0.0, "run_s": 0.0, "csv_s": 0.0}
    with tempfile.TemporaryDirectory() as d:
        for r in range(reps + 1):
            t0 = time.perf_counter()
            a = pesm.Assay(model, seq, muts, offset_idx=1)
            t1 = time.perf_counter()
            scores = a.run()
            t2 = time.perf_counter()
            df = frame.copy()
            df["esm1v_t33_650M_UR90S_1"] = scores
            cf.write_atomically(df, os.path.join(d, f"BLAT_{r}.csv"))
            t3 = time.perf_counter()
            a.close()
            if r:
                parts["assay_create_s"] += (t1 - t0) / reps
                parts["run_s"] += (t2 - t1) / reps
                parts["csv_s"] += (t3 - t2) / reps
    return {"mutants": len(muts), "seconds": sum(parts.values()), **{k: round(v, 4) for k, v in parts.items()},
            "what": "one BLAT-shaped assay, weights resident: mutant strings parsed + uploaded (pgmi_assay_create), masked-marginals, scores "
                    f"copied to the host, CSV written (all input columns + the score column); mean of {reps} runs"}


def only_json_on_stdout():
    """From here on file descriptor 1 of this process IS its stderr: whatever a library prints on stdout (backend chatter such as
    '[Gloo] Rank 0 is connected ...', the runners' progress lines, rocm-smi) lands there, and the ONE JSON line goes out through
    the returned function on the real stdout -- a driver that parses the stream, not only its last line, reads exactly one line."""
    sys.stdout.flush()
    real = os.dup(1)
    os.dup2(2, 1)

    def emit(line: str):
        sys.stdout.flush()
        os.write(real, (line + "\n").encode())
    return emit


def main(argv=None, make_model=None, make_assay=None):
    """``make_model`` / ``make_assay`` are test seams (the N > 1 branch on two gloo ranks without a GPU, tests/test_dist_cpu.py):
    (cfg, blob, device, precision) -> model with profile_reset / profile_enable / profile / close, and (model, seq, mutants) ->
    assay with run_device_only(ptr), positions, T, close()."""
    emit = only_json_on_stdout()
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--precision", default="f16x3", choices=["fp32", "bf16", "f16x3"],
                    help="f16x3 (default) and fp32 are parity-gated (1e-4 abs vs the reference); bf16 is not")
    ap.add_argument("--full", action="store_true",
                    help="after the timed region also measure and check everything beyond the headline (box state, in-run PMC "
                         "traffic, end-to-end rate, CPU baseline and parity, secondary configurations, N > 1: strong_scaling_217)")
    ap.add_argument("--cpu-seconds", type=float, default=15.0, help="--full: CPU-baseline time budget (0 = skip it and `secondary`)")
    ap.add_argument("--layers", type=int, default=33, help="debug only; the headline config is 33")
    ap.add_argument("--checkpoints", type=int, default=1,
                    help="score with N checkpoints per step and average (ESM-1v ensemble rate; the headline is 1)")
    ap.add_argument("--variant", type=int, default=None, help="debug: PGMI_GEMM_VARIANT tile configuration")
    ap.add_argument("--no-secondary", action="store_true", help="--full: skip the `secondary` object (other configs; minutes after the headline)")
    ap.add_argument("--no-live-traffic", action="store_true", help="--full: do not run the rocprofv3 --pmc child passes for roofline.traffic (the committed file is used)")
    ap.add_argument("--no-box-state", action="store_true", help="--full: skip the `box` object (shader clock / socket power during ~2 s of untimed extra steps)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed as DIR/<name>.npy: scores.npy, the float64 per-mutant scores "
                         "(N > 1: the all_gathered vector of every rank, written by rank 0)")
    args = ap.parse_args(argv)
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    seam = make_model is not None

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            raise SystemExit("launch with: python -m torch.distributed.run --nproc-per-node N bench.py --gpus N")
        raise SystemExit(f"WORLD_SIZE={world} does not match --gpus {args.gpus}")

    if args.variant is not None:
        os.environ["PGMI_GEMM_VARIANT"] = str(args.variant)
    import torch
    from proteingym_amd import build_native, esm as pesm, synthetic
    if not seam:
        build_native.build(verbose=False)
    # PGMI_BENCH_SHARE_GPU=1 (rehearsal only, never a measurement): the ranks share the GPUs that exist (local_rank modulo the device
    # count) and talk over gloo through host memory -- RCCL refuses two ranks on one device -- so that the N > 1 code path can run
    # end to end on a one-GPU box
    share = os.environ.get("PGMI_BENCH_SHARE_GPU") == "1" or seam
    if share and not seam:
        local_rank = local_rank % max(torch.cuda.device_count(), 1)
    if not seam:
        torch.cuda.set_device(local_rank)
    gdev = "cpu" if seam else "cuda"                                  # where the score vectors live
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if share:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world,
                                    device_id=torch.device("cuda", local_rank))
    cdev = "cpu" if share else "cuda"                                 # where collective buffers live

    cfg = dict(synthetic.ESM1V_650M, layers=args.layers)
    blob = synthetic.random_weights(cfg, seed=1)                      # same "checkpoint" on every rank
    model = make_model(cfg, blob, local_rank, args.precision) if seam else pesm.EsmModel(cfg, blob, device=local_rank, precision=args.precision)
    seq, muts, _ = synthetic.random_assay(seed=23 + rank, L=L_BLAT, n_single=N_MUT_BLAT, n_multi=0)
    assay = make_assay(model, seq, muts) if seam else pesm.Assay(model, seq, muts, offset_idx=1)    # uploads: inputs resident in HBM
    n_mut = len(muts)
    scores_dev = torch.zeros(n_mut, dtype=torch.float64, device=gdev)
    gathered = torch.zeros(world * n_mut, dtype=torch.float64, device=cdev) if world > 1 else None
    extra = []                                                        # checkpoints 2..N of an ensemble step
    for c in range(1, args.checkpoints):
        m2 = pesm.EsmModel(cfg, synthetic.random_weights(cfg, seed=1 + c), device=local_rank, precision=args.precision)
        extra.append((m2, pesm.Assay(m2, seq, muts, offset_idx=1), torch.zeros(n_mut, dtype=torch.float64, device="cuda")))

    def step():
        assay.run_device_only(scores_dev.data_ptr())                  # whole hot path, synchronised at return
        if extra:                                                     # compute_fitness.py:532-537: plain mean
            for _, a2, buf in extra:
                a2.run_device_only(buf.data_ptr())
            scores_dev.add_(sum(buf for _, _, buf in extra)).div_(args.checkpoints)
        if world > 1:
            dist.all_gather_into_tensor(gathered, scores_dev if not share else scores_dev.cpu())   # RCCL over xGMI

    def fence():
        if world > 1:
            dist.barrier()
        if not seam:
            torch.cuda.synchronize()

    # every N: W untimed steps, then exactly K timed steps between two fences; N > 1 --full adds the 217-assay pass AFTER this region
    blat_steps = args.steps
    for _ in range(args.warmup):
        step()
    model.profile_reset()
    model.profile_enable(True)
    fence()
    t0 = time.perf_counter()
    for _ in range(blat_steps):
        step()
    fence()
    dt = time.perf_counter() - t0
    model.profile_enable(False)
    if args.dump_outputs and rank == 0:                               # before any untimed step overwrites the buffers
        os.makedirs(args.dump_outputs, exist_ok=True)
        last = gathered if world > 1 else scores_dev
        np.save(os.path.join(args.dump_outputs, "scores.npy"), last.cpu().numpy().astype(np.float64))
    if world > 1:
        tmax = torch.tensor([dt], dtype=torch.float64, device=cdev)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dt = float(tmax.item())

    if world > 1:
        prof = model.profile()
        assay.close()
        st = None
        if args.full:
            sys.path.insert(0, os.path.join(ROOT, "scripts"))
            import bench_scale
            strong_steps = max(1, min(args.steps, 4))
            st = bench_scale.run(model, rank, world, strong_steps, min(args.warmup, 1), torch, dist,
                                 max_assays=int(os.environ.get("PGMI_BENCH_217_ASSAYS", "0")), make_assay=make_assay)
            st["mutants_per_s"] = st["mutants"] / st["seconds"]
            st["what"] = (f"ONE pass over the {st['assays']}-assay-shaped DMS substitution benchmark ({st['mutants']} mutants; real seq_len / mutant "
                          "counts of reference_files/DMS_substitutions.csv, optimal 1024 windows), 1 checkpoint, assays sharded over the ranks by "
                          "run_benchmark.plan_assays, inputs resident in HBM, one all_gather of the per-mutant score vectors; total work fixed; "
                          f"timed between its own barriers as {strong_steps} consecutive slices of each rank's work list, max over ranks")
            st["scaling_efficiency"] = "mutants_per_s / (N * one_gpu_same_workload_mutants_per_s of the N = 1 line)"
        from proteingym_amd import dist as pdist
        rccl = pdist.collective_identity(local_rank)                  # a collective: every rank calls it
        if rank == 0:
            ffn_ms = prof["gemm_fc1"]["ms"] + prof["gemm_fc2"]["ms"]
            ffn_fl = prof["gemm_fc1"]["flops"] + prof["gemm_fc2"]["flops"]
            ffn_n = prof["gemm_fc1"]["launches"] + prof["gemm_fc2"]["launches"]
            achieved = ffn_fl / (ffn_ms * 1e-3) / 1e12 if ffn_ms > 0 else 0.0
            peak = PEAK_TFLOPS[args.precision]
            passes = 3 if args.precision == "f16x3" else 1
            out = {
                "metric": "mutants scored/sec (ESM-1v 650M masked-marginal)",
                "value": world * n_mut * blat_steps / dt, "unit": "mutants/s",
                "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                "ms_per_step": dt / blat_steps * 1e3,
                "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
                "dtype": {"fp32": "f32", "bf16": "bf16",
                          "f16x3": "f16x3 (fp32 operands split into 2 fp16 planes, 3 fp16 MFMAs per product, fp32 accumulate)"}[args.precision],
                "data": "synthetic",
                "config": {"workload": "ESM-1v 650M (33x1280, 20 heads, FFN 5120) masked-marginals, the N = 1 line's step on every rank: one "
                                       f"BLAT_ECOLX_Stiffler_2015-shaped assay per rank per step (BASELINE.json configs[1]: L=286, T=288, {n_mut} single "
                                       f"mutants, inputs resident in HBM, a different synthetic assay per rank), then ONE all_gather of the {world} score vectors "
                                       "(RCCL over xGMI); per-GPU work fixed",
                           "value_is": "all ranks' mutants / max-over-ranks seconds of the K steps; value(N) / (N * value(1)) = scaling efficiency",
                           "north_star_workload": "strong_scaling_217 (the whole 217-assay table sharded over the ranks), timed after this region "
                                                  "with --full",
                           "precision": args.precision, "layers": args.layers},
                "rccl": rccl,
                **({"strong_scaling_217": st} if st is not None else {}),
                **({"REHEARSAL": "PGMI_BENCH_SHARE_GPU=1: ranks share a GPU and use gloo -- not a measurement"} if share else {}),
                "roofline": {"bound": "mfma", "kernel": "gemm (fc1+GELU, fc2+residual), rank 0", "achieved": achieved, "peak": peak,
                             "unit": "TFLOP/s", "frac": achieved / peak, "avg_launch_ms": ffn_ms / max(ffn_n, 1), "traffic": None,
                             "traffic_detail": {"unavailable": "PMC passes are collected on the N = 1 line"},
                             "mfma_passes": passes, "mfma_util": passes * achieved / peak,
                             "note": "achieved = algorithmic FLOPs (2*M*N*K per GEMM) / HIP-event time of rank 0's FFN GEMM launches in the timed steps"},
                "kernels": {k: {"ms_per_step": round(v["ms"] / blat_steps, 3), "launches_per_step": v["launches"] // blat_steps,
                                "tflops": round(v["flops"] / (v["ms"] * 1e-3) / 1e12, 2) if v["ms"] > 0 and v["flops"] > 0 else None}
                            for k, v in prof.items()},
            }
            emit(json.dumps(out))
        model.close()
        dist.barrier()
        dist.destroy_process_group()
        return

    prof = model.profile()
    box = box_state(step) if args.full and not args.no_box_state else None     # after the timed region and the profile read-out
    if rank == 0:
        ffn_ms = prof["gemm_fc1"]["ms"] + prof["gemm_fc2"]["ms"]
        ffn_fl = prof["gemm_fc1"]["flops"] + prof["gemm_fc2"]["flops"]
        ffn_n = prof["gemm_fc1"]["launches"] + prof["gemm_fc2"]["launches"]
        achieved = ffn_fl / (ffn_ms * 1e-3) / 1e12 if ffn_ms > 0 else 0.0
        peak = PEAK_TFLOPS[args.precision]
        passes = 3 if args.precision == "f16x3" else 1          # MFMA FLOPs executed per algorithmic FLOP
        total_fl = sum(v["flops"] for v in prof.values())
        if not args.full:
            live = {"unavailable": "the rocprofv3 --pmc passes run with --full"}
        else:
            live = None if (args.no_live_traffic or args.layers != 33) else live_traffic(args.precision)
        traffic, traffic_detail = ffn_traffic(args.precision, len(assay.positions) * assay.T, cfg["embed_dim"], cfg["ffn_dim"], live=live)
        kern = {k: {"ms_per_step": round(v["ms"] / args.steps, 3), "launches_per_step": v["launches"] // args.steps,
                    "tflops": round(v["flops"] / (v["ms"] * 1e-3) / 1e12, 2) if v["ms"] > 0 and v["flops"] > 0 else None,
                    "gbps": round(v["bytes"] / (v["ms"] * 1e-3) / 1e9, 1) if v["ms"] > 0 and v["bytes"] > 0 else None}
                for k, v in prof.items()}
        out = {
            "metric": "mutants scored/sec (ESM-1v 650M masked-marginal)",
            "value": world * n_mut * args.steps / dt,
            "unit": "mutants/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": dt / args.steps * 1e3,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": {"fp32": "f32", "bf16": "bf16",
                      "f16x3": "f16x3 (fp32 operands split into 2 fp16 planes, 3 fp16 MFMAs per product, fp32 accumulate)"}[args.precision],
            "data": "synthetic",
            "config": {"workload": "ESM-1v 650M (33x1280, 20 heads, FFN 5120) masked-marginals, one "
                                   "BLAT_ECOLX_Stiffler_2015-shaped assay per step (BASELINE.json configs[1]: L=286, T=288, "
                                   f"{len(assay.positions)} masked positions run, {n_mut} single mutants), "
                                   f"{args.checkpoints} checkpoint{'s averaged (ensemble rate)' if args.checkpoints > 1 else ''}; "
                                   "N > 1 runs the same step on every rank + one all_gather (weak scaling) and, with --full, adds strong_scaling_217",
                       "value_is": "DEVICE-ONLY rate of the hot path: inputs resident in HBM when the timed region starts, scores left in HBM "
                                   "(mutants / seconds of the K timed steps).  The metric as SURVEY 8d words it -- weights resident to CSV written -- is, "
                                   "with --full, value_end_to_end (this assay: mutant strings parsed, uploaded, scored, copied back, CSV written) and, for the whole "
                                   "217-assay table, benchmark_217_end_to_end_mutants_per_s",
                       "precision": args.precision, "layers": args.layers,
                       "last_layer": ("after its attention the last layer runs on the masked row of every sequence only -- the one row "
                                      "masked-marginals reads (class kept_rows); scores bit-identical to the full evaluation"
                                      if os.environ.get("PGMI_KEEP_ROWS", "1") != "0" else "all rows (PGMI_KEEP_ROWS=0)"),
                       "positions_run": int(len(assay.positions)), "tokens_per_step": int(len(assay.positions) * assay.T)},
            "roofline": {"bound": "mfma", "kernel": "gemm (fc1+GELU, fc2+residual)", "achieved": achieved,
                         "peak": peak, "unit": "TFLOP/s", "frac": achieved / peak,
                         "avg_launch_ms": ffn_ms / max(ffn_n, 1), "traffic": traffic, "traffic_detail": traffic_detail,
                         "mfma_passes": passes, "mfma_util": passes * achieved / peak,
                         "vs_fp32_mfma_peak": achieved / PEAK_TFLOPS["fp32"],
                         "note": "achieved = algorithmic FLOPs (2*M*N*K per GEMM) / HIP-event time of the FFN GEMM "
                                 "launches in the timed region; f16x3 issues 3 fp16 MFMAs per product block, so MFMA "
                                 "pipe utilisation is mfma_util = 3*achieved/peak",
                         "whole_step_tflops": total_fl / dt / 1e12},
            "kernels": kern,
        }
        if box is not None:
            out["box"] = box
        e2e = None
        if args.full and world == 1 and args.layers == 33:            # SURVEY 8d's wording of the metric on this assay (after the timed region)
            try:
                e2e = end_to_end_blat(model, seq, muts)
            except Exception as e:                                    # noqa: BLE001
                e2e = {"error": repr(e)}
            out.update(end_to_end_fields(e2e, None))
        if args.full and world == 1 and args.cpu_seconds > 0:
            _, gpu_table = assay.run(want_table=True)                 # outside the timed region
            for m2, a2, _ in extra:
                a2.close()
                m2.close()
            assay.close()
            model.close()
            out["cpu_baseline"], out["parity"] = cpu_baseline(cfg, blob, seq, n_mut, args.cpu_seconds, gpu_table)
            out["cpu_baseline"]["reference_vs_port"] = ("kind 'port': /root/reference does not exist on the GPU box; in the build container the "
                                                        "unmodified reference model and this port were timed side by side on the same input "
                                                        "(profiles/r2/cpu_reference_vs_port.json): same s/forward within noise")
            if not args.no_secondary and args.layers == 33:
                del blob
                import contextlib
                try:                                                 # the runner and scorer print progress: keep stdout to the ONE JSON line
                    with contextlib.redirect_stdout(sys.stderr):
                        out["secondary"] = secondary(args.precision)
                except Exception as e:                               # a secondary leg must never take the headline line down
                    out["secondary"] = {"error": repr(e)}
                b217 = out["secondary"].get("benchmark_217_end_to_end") if isinstance(out["secondary"], dict) else None
                out.update(end_to_end_fields(e2e, b217))
        emit(json.dumps(out))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
