"""Writes tests/golden/PoET_toy/ from the LIVE reference (proteingym/baselines/PoET, driven by tests/poet_reference.py on the CPU):

  poet_toy.ckpt            a seeded toy checkpoint in the reference's .ckpt layout (hyper_parameters.model_spec.init_args + state_dict
                           with one leading key component): D = 128, 2 heads, 2 layers, FFN 256, norm=True; linear2 and the out
                           projections, which the reference zero-initialises, re-initialised; tensors stored as float16 (the file
                           must stay below the repository's size limit; every value is then exactly what any loader reads)
  TOY_POET.a3m             a toy a3m: lower-case insertions, gaps, a near-duplicate cluster, rows above and below every similarity cut-off
  TOY_POET.csv             mutated_sequence / DMS_score: substitutions, insertions, deletions, one sequence with an X
  TOY_POET_REFERENCE.csv   the mapping file (target_seq longer than the MSA window)
  TOY_POET_scores.csv      the reference's output file for the toy context lengths; TOY_POET_scores_relative.csv with --relative_to_wt
  golden_poet.npz          neighbour counts, the sampled indices of all 15 members, per-member forward / backward scores (float64)

    python tests/golden/make_golden_poet.py [out_dir]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]

INIT_ARGS = dict(n_vocab=24, hidden_dim=128, ff_dim=256, num_layers=2, nhead=2, norm=True)
CONTEXT_LENGTHS = (60, 150, 400)
SEED = 188257
AA = "ARNDCQEGHILKMFPSTWYV"
L = 40


def toy_state_dict():
    import torch
    import poet_reference as pr
    torch.manual_seed(20240917)
    model = pr.build_model(INIT_ARGS, {})
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith("linear2.weight") or name.endswith("out_proj.weight"):
                torch.nn.init.normal_(p, std=0.06)
            elif name.endswith("bias") or "norm" in name:
                p.add_(torch.randn_like(p) * 0.05)
    # the rotary inv_freq buffers stay float32, as in a real checkpoint: they are part of the arithmetic, not weights to be rounded
    return {k: v.detach() if k.endswith("inv_freq") else v.detach().half() for k, v in model.state_dict().items()}


def toy_alignment():
    rng = np.random.default_rng(7)
    wt = "".join(rng.choice(list(AA), L))
    rows = [("wt", wt)]

    def mutate(seq, n):
        s = list(seq)
        for p in rng.choice(L, n, replace=False):
            s[p] = rng.choice([a for a in AA if a != s[p]])
        return "".join(s)
    # identities around every cut-off of the ensemble (1.0, 0.95, 0.90, 0.70, 0.50): 40 columns, so n mismatches = 1 - n / 40
    for n in (0, 1, 2, 3, 4, 5, 8, 11, 12, 13, 16, 19, 20, 21, 24, 30):
        rows.append((f"m{n}", mutate(wt, n)))
    base = mutate(wt, 9)                                       # a cluster of near-duplicates
    for i in range(5):
        rows.append((f"c{i}", mutate(base, i % 2)))
    out = []
    for i, (name, s) in enumerate(rows):
        s = list(s)
        if i % 3 == 2:                                         # gaps
            for p in rng.choice(L, 1 + i % 4, replace=False):
                s[p] = "-"
        if i % 4 == 1:                                         # lower-case insertions: not alignment columns
            p = int(rng.integers(1, L - 1))
            s[p:p] = list("".join(rng.choice(list(AA.lower()), 1 + i % 3)))
        out.append((name, "".join(s)))
    out[0] = ("wt", wt)
    return wt, out


def toy_variants(wt):
    rng = np.random.default_rng(11)
    v = []
    for n in (1, 1, 2, 3, 5):
        s = list(wt)
        for p in rng.choice(L, n, replace=False):
            s[p] = rng.choice([a for a in AA if a != s[p]])
        v.append("".join(s))
    v.append(wt[:10] + "GS" + wt[10:])                         # insertions
    v.append(wt[:33] + "A" + wt[33:])
    v.append(wt[:5] + wt[8:])                                  # deletions
    v.append(wt[:-1])
    v.append(wt[:20] + "X" + wt[21:])                          # X is the mask token: its target is not scored
    v.append(wt)
    return v


def generate(out_dir):
    import pandas as pd
    import torch
    import poet_reference as pr
    os.makedirs(out_dir, exist_ok=True)
    sd = toy_state_dict()
    torch.save({"hyper_parameters": {"model_spec": {"init_args": dict(INIT_ARGS)}}, "state_dict": {"model." + k: v for k, v in sd.items()}},
               os.path.join(out_dir, "poet_toy.ckpt"))
    wt, rows = toy_alignment()
    with open(os.path.join(out_dir, "TOY_POET.a3m"), "w") as f:
        f.write("# toy alignment of tests/golden/make_golden_poet.py\n")
        for name, s in rows:
            f.write(f">{name}\n{s}\n")
    variants = toy_variants(wt)
    pd.DataFrame({"mutated_sequence": variants, "DMS_score": np.round(np.random.default_rng(3).normal(size=len(variants)), 3)}).to_csv(
        os.path.join(out_dir, "TOY_POET.csv"), index=False)
    pd.DataFrame([{"DMS_id": "TOY_POET", "DMS_filename": "TOY_POET.csv", "target_seq": "MK" + wt + "GG", "MSA_start": 3, "MSA_end": 2 + L}]).to_csv(
        os.path.join(out_dir, "TOY_POET_REFERENCE.csv"), index=False)

    # -- the reference's own pipeline, scripts/score.py main() statement by statement, with the CPU forward of poet_reference --
    sc, sampling, alphabet = pr.score_module(), pr.sampling(), pr.alphabet()
    model = pr.build_model(INIT_ARGS, {k: v.float().numpy() for k, v in sd.items()}, torch.float64)
    msa_sequences = sc.get_seqs_from_fastalike(__import__("pathlib").Path(os.path.join(out_dir, "TOY_POET.a3m")))
    assert msa_sequences[0].decode() == wt
    msa = sc.get_encoded_msa_from_a3m_seqs(msa_sequences=msa_sequences, alphabet=alphabet)
    framed = [sc.append_startstop(alphabet.encode(v.encode()), alphabet=alphabet) for v in variants]
    framed.append(sc.append_startstop(alphabet.encode(wt.encode()), alphabet=alphabet))       # --relative_to_wt appends the wild type
    rec = {"msa": msa}
    rec["neighbors"] = sampling._compute_homology_weights(ungapped_msa=msa, gap_token=alphabet.gap_token, gap_token_mask=255, theta=0.2,
                                                          hamming_csim_func=sampling.compute_hamming_csim_np, can_use_torch=False).astype(np.int64)
    logps = []
    import itertools
    for k, (max_tokens, max_similarity) in enumerate(itertools.product(CONTEXT_LENGTHS, [1.0, 0.95, 0.90, 0.70, 0.50])):
        sampler = sampling.MSASampler(method=sampling.NeighborsSampler(can_use_torch=False), max_similarity=max_similarity)
        idxs = sampler.get_sample_idxs(msa=msa, gap_token=alphabet.gap_token, seed=SEED)
        prompt = sc.sample_msa_sequences(get_sequence_fn=lambda ii: msa_sequences[ii].upper().translate(None, delete=b"-"),
                                         sample_idxs=idxs, max_tokens=max_tokens, alphabet=alphabet, shuffle_seed=SEED, truncate=False)
        rec[f"idxs_{k}"] = np.asarray(idxs, dtype=np.int64)
        rec[f"prompt_lens_{k}"] = np.array([len(s) for s in prompt], dtype=np.int64)
        rec[f"prompt_tokens_{k}"] = np.concatenate(prompt).astype(np.int64) if prompt else np.zeros(0, dtype=np.int64)
        fwd = np.array([pr.score(model, prompt, v) for v in framed])
        rprompt = [np.ascontiguousarray(s[::-1]) for s in prompt]
        bwd = np.array([pr.score(model, rprompt, np.ascontiguousarray(v[::-1])) for v in framed])
        rec[f"fwd_{k}"], rec[f"bwd_{k}"] = fwd, bwd
        logps.append((fwd + bwd) / 2)
    logps = np.vstack(logps).mean(axis=0)
    rec["scores"], rec["scores_relative"] = logps[:-1], logps[:-1] - logps[-1]
    pd.DataFrame(data={"mutated_sequence": variants, "PoET_score": rec["scores"]}).to_csv(os.path.join(out_dir, "TOY_POET_scores.csv"), index=False)
    pd.DataFrame(data={"mutated_sequence": variants, "PoET_score": rec["scores_relative"]}).to_csv(
        os.path.join(out_dir, "TOY_POET_scores_relative.csv"), index=False)
    np.savez_compressed(os.path.join(out_dir, "golden_poet.npz"), **rec)
    return rec


if __name__ == "__main__":
    generate(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "PoET_toy"))
