"""Drop-in for ``proteingym/baselines/protein_mpnn/compute_fitness.py`` on MI355X.

Same flags and the same file: ``<output_scores_folder>/<DMS_id>.csv`` with the columns ``mutant``, ``mutated_sequence`` and
``pmpnn_ll`` -- minus the mean negative log-likelihood of the mutated sequence over the residues with a complete backbone, from ONE
forward under a random decoding order (with --num_seq_per_target above 1 the reference still reports only its first draw; so does this).
The structure is parsed, featurised and encoded once per assay; a mutant costs the decoder only.

--pdb_path_chains and --fixed_positions_jsonl act through chain_M / chain_M_pos, which change the decoding order only.  The sampling
flags (--sampling_temp, --omit_AAs, --bias_AA_jsonl, --bias_by_res_jsonl, --omit_AA_jsonl, --pssm_*, --tied_positions_jsonl,
--chain_id_jsonl, --batch_size, --pdb_path, --jsonl_path) are accepted and have no effect on the score, as in the reference;
--backbone_noise must be 0.

Seeds: --seed 0 picks a random seed, as the reference does.  A non-zero seed draws the normals of assay row r from a local
torch.Generator seeded with (seed, r), so a row's order depends on (seed, row) only -- not on the batch, the device or what was scored
before.  The reference's global stream is NOT replayed: the reference first spends it on the random initialisation of its model, and on a GPU
it draws from the device generator.  Additive flags: --device, --max_batch."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import pandas as pd

from . import mpnn

NO_EFFECT = "accepted; no effect on the score (sampling only), as in the reference"


def parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="ProteinMPNN log-likelihood scores (HIP, MI355X)",
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("--DMS_reference_file_path", type=str, help="path to DMS reference file")
    p.add_argument("--DMS_data_folder", type=str, help="path to folder containing DMS data")
    p.add_argument("--structure_folder", type=str, help="folder containing pdb files for each DMS")
    p.add_argument("--DMS_index", type=int, help="index of DMS in DMS reference file")
    p.add_argument("--checkpoint", type=str, help="path to model")
    p.add_argument("--suppress_print", type=int, default=0, help="0 for False, 1 for True")
    p.add_argument("--seed", type=int, default=0, help="If set to 0 then a random seed will be picked; otherwise row r's decoding "
                   "order depends on (seed, r) only")
    p.add_argument("--backbone_noise", type=float, default=0.00, help="Must be 0 (the structure is encoded once)")
    p.add_argument("--num_seq_per_target", type=int, default=1, help="Accepted; only the first draw is reported, as in the reference")
    p.add_argument("--batch_size", type=int, default=1, help=NO_EFFECT)
    p.add_argument("--max_length", type=int, default=200000, help="Max sequence length")
    p.add_argument("--sampling_temp", type=str, default="0.1", help=NO_EFFECT)
    p.add_argument("--output_scores_folder", type=str, help="Path to a folder to output scores, e.g. /home/out/")
    p.add_argument("--pdb_path", type=str, default="", help=NO_EFFECT)
    p.add_argument("--pdb_path_chains", type=str, default="", help="Chains to design (space separated); the others are context. "
                   "Changes the decoding order only")
    p.add_argument("--jsonl_path", type=str, help=NO_EFFECT)
    p.add_argument("--chain_id_jsonl", type=str, default="", help=NO_EFFECT + " (the reference overwrites it from --pdb_path_chains)")
    p.add_argument("--fixed_positions_jsonl", type=str, default="", help="Dictionary of fixed positions; changes the decoding order only")
    p.add_argument("--omit_AAs", type=list, default="X", help=NO_EFFECT)
    p.add_argument("--bias_AA_jsonl", type=str, default="", help=NO_EFFECT)
    p.add_argument("--bias_by_res_jsonl", default="", help=NO_EFFECT)
    p.add_argument("--omit_AA_jsonl", type=str, default="", help=NO_EFFECT)
    p.add_argument("--pssm_jsonl", type=str, default="", help=NO_EFFECT)
    p.add_argument("--pssm_multi", type=float, default=0.0, help=NO_EFFECT)
    p.add_argument("--pssm_threshold", type=float, default=0.0, help=NO_EFFECT)
    p.add_argument("--pssm_log_odds_flag", type=int, default=0, help=NO_EFFECT)
    p.add_argument("--pssm_bias_flag", type=int, default=0, help=NO_EFFECT)
    p.add_argument("--tied_positions_jsonl", type=str, default="", help=NO_EFFECT)
    p.add_argument("--device", type=int, default=0, help="HIP device")
    p.add_argument("--max_batch", type=int, default=1024, help="Mutants per call into the library")
    return p


def row_randn(seed: int, row: int, L: int) -> np.ndarray:
    """The normals of assay row ``row``: a local generator, so nothing else that draws random numbers moves them."""
    import torch
    g = torch.Generator(device="cpu")
    g.manual_seed((int(seed) * 1000003 + int(row)) % (2 ** 63))
    return torch.randn(L, generator=g, dtype=torch.float32).numpy()


def main(argv=None, randn=None) -> str:
    """Scores one assay and returns the path of the CSV.  ``randn`` [rows, L] replaces the drawn normals (tests)."""
    args = parser().parse_args(argv)
    if args.backbone_noise != 0.0:
        raise SystemExit("--backbone_noise must be 0: the structure is encoded once for the whole assay")
    seed = args.seed if args.seed else int(np.random.randint(0, high=999, size=1, dtype=int)[0])
    mapping = pd.read_csv(args.DMS_reference_file_path)
    row = mapping.iloc[args.DMS_index]
    out_path = os.path.join(args.output_scores_folder, row["DMS_id"] + ".csv")
    os.makedirs(args.output_scores_folder, exist_ok=True)
    pdb_file = os.path.join(args.structure_folder, row["pdb_file"])
    name = os.path.basename(pdb_file)[:-4]

    chains = mpnn.parse_pdb(pdb_file)
    if sum(len(s) for _, s, _ in chains) > args.max_length:
        raise SystemExit(f"{pdb_file}: longer than --max_length {args.max_length}")
    designed = [str(c) for c in args.pdb_path_chains.split()] if args.pdb_path_chains else None
    fixed = None
    if os.path.isfile(args.fixed_positions_jsonl):
        with open(args.fixed_positions_jsonl) as f:
            for line in f:
                fixed = json.loads(line)          # the reference keeps the last line
        fixed = fixed[name]
    feat = mpnn.featurize(chains, designed, fixed)
    L = len(feat["seq"])
    n_designed = int(feat["chain_M"].sum())      # designed chains come first in the packing

    df = pd.read_csv(os.path.join(args.DMS_data_folder, row["DMS_filename"]))
    names, seqs = df["mutant"].tolist(), df["mutated_sequence"].tolist()
    for r, s in enumerate(seqs):
        if len(s) != n_designed:
            raise SystemExit(f"row {r} ({names[r]}): mutated sequence has {len(s)} residues, the designed chains of {name} have "
                             f"{n_designed} (residue numbers without ATOM records count as one masked X each)")
    # the reference writes each mutated sequence over the first positions of S and keeps the structure's letters behind them
    full = [s + feat["seq"][n_designed:] for s in seqs]
    S = mpnn.encode_sequences(full, L)

    blob, num_edges = mpnn.load_checkpoint(args.checkpoint)
    model = mpnn.MpnnModel(blob, num_edges=num_edges, device=args.device)
    try:
        model.set_structure(feat["X"], feat["mask"], feat["residue_idx"], feat["chain_encoding"], feat["chain_M"], feat["chain_M_pos"])
        if args.suppress_print == 0:
            print(f"{name}: {L} residues, {int(feat['mask'].sum())} with a full backbone, {min(num_edges, L)} neighbours; "
                  f"{len(seqs)} mutants, seed {seed}")
        scores = np.empty(len(seqs), dtype=np.float64)
        for b0 in range(0, len(seqs), args.max_batch):
            b1 = min(len(seqs), b0 + args.max_batch)
            if randn is not None:
                z = np.asarray(randn[b0:b1], dtype=np.float32).reshape(b1 - b0, L)
            else:
                z = np.stack([row_randn(seed, r, L) for r in range(b0, b1)])
            scores[b0:b1] = model.scores(S[b0:b1], randn=z)
    finally:
        model.close()
    pd.DataFrame({"mutant": names, "mutated_sequence": seqs, "pmpnn_ll": scores}).to_csv(out_path, index=False)
    return out_path


if __name__ == "__main__":
    main(sys.argv[1:])
