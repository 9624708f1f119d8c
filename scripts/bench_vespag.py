#!/usr/bin/env python
"""VespaG at ESM2-3B's shape with seeded weights: a FASTA of 256 seeded sequences whose lengths were drawn from the seq_len column of
ProteinGym's DMS_substitutions.csv (tests/golden/VespaG_bench_seq_lens.csv holds the drawn list), every residue row through
FNN([256], 2560, 20).

    python scripts/bench_vespag.py [--n 256] [--layers 36] [--precisions f16x3 fp32] [--max_rows 98304] [--out bench_vespag.json]

Per precision: pgmi_vespag_landscapes over the whole FASTA (host clock around the calls, which end in a device synchronise; one warm-up
call on the eight shortest sequences, then --repeats calls, every one listed, the best reported) as sequences/s and residues/s, the
share of <pad> tokens in what the chunks ran, and a profiled call split by kernel class (the encoder's classes on the ESM2 model's
profile, the head's on the handle's; HIP events on one stream, so the classes do not overlap) with the head's share of it.  Beside it, on
the same GPU: the path this replaces, one pgmi_esm_residue_rows call per sequence followed by pgmi_vespag_head (f16x3); and, each in a
child process of its own, a Hugging Face EsmModel of the same shape (its own initialisation: timed, not compared) run the reference's
way -- .half(), batches of up to 4 096 residues in FASTA order padded to the longest (data/embeddings.py) -- and in fp32 at batch 1.
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

from proteingym_amd import _lib, protssn, synthetic as S, vespag  # noqa: E402
from proteingym_amd import esm as pesm  # noqa: E402

LENS = os.path.join(ROOT, "tests", "golden", "VespaG_bench_seq_lens.csv")
WORKSPACE_ROWS = 98304                      # --max_rows' default: the models are made with it and the chunk plan reported below is cut for it


def say(*a):
    print(*a, file=sys.stderr, flush=True)


def fasta(n):
    lens = np.loadtxt(LENS, skiprows=1, dtype=np.int64)[:n]
    rng = np.random.default_rng(31)
    return [S.random_sequence(rng, int(L)) for L in lens]


def esm_cfg(layers):
    return dict(S.ESM2_3B, layers=layers)


def reference_batches(seqs, cap=4096):
    """data/embeddings.py's batching: FASTA order; a batch closes when the next sequence would take it past `cap` residues."""
    out, cur, total = [], [], 0
    for s in seqs:
        if total + min(len(s), cap) > cap:
            out.append(cur)
            cur, total = [], 0
        cur.append(s)
        total += len(s)
    return [b for b in out + [cur] if b]


def torch_baseline(mode, n, layers):
    import torch
    from transformers import EsmConfig, EsmModel
    seqs = fasta(n)
    cfg = esm_cfg(layers)
    hc = EsmConfig(vocab_size=33, hidden_size=cfg["embed_dim"], num_hidden_layers=cfg["layers"], num_attention_heads=cfg["heads"],
                   intermediate_size=cfg["ffn_dim"], position_embedding_type="rotary", token_dropout=True, pad_token_id=1, mask_token_id=32,
                   layer_norm_eps=1e-5, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    with torch.device("cuda"):
        model = EsmModel(hc, add_pooling_layer=False)
    model = (model.half() if mode == "half" else model.float()).eval()
    batches = reference_batches(seqs) if mode == "half" else [[s] for s in seqs]

    def run(batch):
        T = max(len(s) for s in batch) + 2
        ids = np.full((len(batch), T), 1, np.int64)
        for i, s in enumerate(batch):
            ids[i, :len(s) + 2] = vespag.tokenize(s)
        t = torch.as_tensor(ids, device="cuda")
        with torch.no_grad():
            h = model(input_ids=t, attention_mask=(t != 1).long()).last_hidden_state
        return [h[i, 1:len(s) + 1].float().cpu() for i, s in enumerate(batch)]
    run(batches[-1])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for b in batches:
        run(b)
    torch.cuda.synchronize()
    sec = time.perf_counter() - t0
    padded = sum(len(b) * (max(len(s) for s in b) + 2) for b in batches)
    tokens = sum(len(s) + 2 for s in seqs)
    return dict(mode=mode, sec=sec, sequences_per_sec=len(seqs) / sec, residues_per_sec=sum(map(len, seqs)) / sec, batches=len(batches),
                pad_share=1 - tokens / padded)


def classes(view):
    return {c: round(v["ms"], 3) for c, v in view.profile().items() if v["launches"]}


def bench_precision(precision, seqs, cfg, blob, sd, repeats, loop, max_rows):
    say(f"[{precision}] creating the models")
    esm = pesm.EsmModel(cfg, blob, precision=precision, max_rows=max_rows)
    head = vespag.from_state_dict(sd, esm=esm, precision=precision)
    residues = sum(map(len, seqs))
    out = dict(precision=precision, max_rows=max_rows, sequences=len(seqs), residues=residues, longest=max(map(len, seqs)))
    try:
        head.landscapes(sorted(seqs, key=len)[:8])                              # warm-up: workspaces, rotary table
        secs = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            ys = head.landscapes(seqs)
            secs.append(time.perf_counter() - t0)
            say(f"[{precision}] landscapes: {secs[-1]:.2f} s")
        sec = min(secs)
        lens = [len(s) for s in seqs]
        groups = vespag.call_groups(lens)
        plans = [vespag.plan_chunks([lens[i] for i in g], max_rows)[1] for g in groups]
        padded = sum(len(c) * (lens[g[c[0]]] + 2) for g, chunks in zip(groups, plans) for c in chunks)
        out.update(landscapes_sec=sec, landscapes_sec_runs=secs, sequences_per_sec=len(seqs) / sec, residues_per_sec=residues / sec,
                   device_calls=len(groups), chunks=sum(map(len, plans)), pad_share=1 - (residues + 2 * len(seqs)) / padded,
                   y_abs_max=float(max(np.abs(y).max() for y in ys)))
        views = (_lib._ProfileView(esm._h), head.profile_view())
        for v in views:
            v.profile_enable(True)
            v.profile_reset()
        head.landscapes(seqs)
        enc, hd = classes(views[0]), classes(views[1])
        for v in views:
            v.profile_enable(False)
        out.update(encoder_classes_ms=enc, head_classes_ms=hd, head_share=sum(hd.values()) / (sum(enc.values()) + sum(hd.values())))
        if loop:
            alone = vespag.from_state_dict(sd, precision=precision)
            protssn.residue_rows(esm, seqs[0])
            t0 = time.perf_counter()
            for s in seqs:
                alone.head(protssn.residue_rows(esm, s), vespag.wt_columns(s))
            out["loop_of_residue_rows_sec"] = time.perf_counter() - t0
            out["packed_speedup_vs_loop"] = out["loop_of_residue_rows_sec"] / sec
            alone.close()
            say(f"[{precision}] loop of pgmi_esm_residue_rows: {out['loop_of_residue_rows_sec']:.2f} s")
    finally:
        head.close()
        esm.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--layers", type=int, default=36)
    ap.add_argument("--precisions", nargs="+", default=["f16x3", "fp32"])
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--max_rows", type=int, default=WORKSPACE_ROWS, help="workspace rows of the ESM2 models (at least 2048)")
    ap.add_argument("--torch", nargs="*", default=["half", "fp32"], help="torch baselines to run (half, fp32)")
    ap.add_argument("--torch_only", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.torch_only:
        print(json.dumps(torch_baseline(args.torch_only, args.n, args.layers)))
        return
    seqs = fasta(args.n)
    cfg = esm_cfg(args.layers)
    say("seeding the ESM2 weights")
    blob = S.random_weights(cfg, seed=7)
    sd = vespag.random_state_dict(21, vespag.INPUT_DIM, vespag.HIDDEN, gain=1.0)
    out = dict(layers=args.layers, runs=[bench_precision(p, seqs, cfg, blob, sd, args.repeats, p == "f16x3", max(args.max_rows, 2048)) for p in args.precisions])
    del blob
    out["torch"] = []
    for mode in args.torch:
        say(f"torch baseline: {mode}")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--torch_only", mode, "--n", str(args.n), "--layers", str(args.layers)],
                           capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise RuntimeError(f"torch baseline {mode} failed:\n{r.stderr[-2000:]}")
        out["torch"].append(json.loads(r.stdout.strip().splitlines()[-1]))
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
