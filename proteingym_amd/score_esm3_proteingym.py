"""Drop-in for ``proteingym/baselines/evoscale/compute_fitness.py --model_type esm3_open`` on MI355X, with or without ``--use_structure``.

Same flags, same assay loop (:612-740): every assay of --reference_csv (or row --DMS_index; an index out of range scores all of them,
with a warning), ``<output_dir>/<DMS_id>.csv`` = the assay's columns plus ``esm3_open_score`` (NaN for the mutants the reference
skips; the reference spells this one column ``ESM3_open_score``, the ESM C path's ``<model_type>_score`` rule is kept here), written
after the Spearman step, and ``correlation_summary_esm3_open.csv`` appended to (header only when it is created).

With --use_structure the reference CSV needs a ``pdb_file`` column (ValueError otherwise) and may have ``pdb_range``; the sequence is
the PDB chain's (chain A, as the reference passes), positions map through its residue numbers, a PDB file that is not there skips the
assay without a summary row, and an assay that fails -- a mutant letter outside the 20 standard amino acids, a residue with an
insertion code -- gets a NaN summary row and no CSV.  Without it the target sequence is scored through ESM3's embedding with every
structure track at its default.  The model is loaded once from --model_path: a snapshot directory holding
data/weights/esm3_sm_open_v1.pth and esm3_structure_encoder_v0.pth, or the model's .pth with the encoder's next to it; nothing is
downloaded.  Additive flags: --device, --max_rows.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import pandas as pd

from . import esm3
from .score_esmc_proteingym import select_assays

MODEL_TYPE = "esm3_open"


def parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Process DMS assays with ESM3 scoring (HIP, MI355X)")
    p.add_argument("--model_type", choices=["esmc_300M", "esmc_600M", "esm3_open"], default=MODEL_TYPE,
                   help="Model type to use for scoring (esm3_open; the ESM C models are scored by score_esmc_proteingym)")
    p.add_argument("--model_path", type=str, default=None, help="ESM3 snapshot directory or state dict (.pth) (required: nothing is downloaded)")
    p.add_argument("--reference_csv", required=True, help="CSV file with DMS_id and target_seq columns")
    p.add_argument("--dms_dir", required=True, help="Directory containing DMS CSV files")
    p.add_argument("--pdb_dir", required=False, default=None, help="Directory containing PDB files (only needed with --use_structure)")
    p.add_argument("--output_dir", required=True, help="Directory to save output files")
    p.add_argument("--use_structure", action="store_true", default=False, help="Whether to use structure information")
    p.add_argument("--DMS_index", required=False, default=-1, help="Index of DMS to score. If not provided, score all DMS assays")
    p.add_argument("--device", type=int, default=0, help="HIP device")
    p.add_argument("--max_rows", type=int, default=0, help="workspace rows per device call (0 = library default)")
    return p


def score_csv(model, csv_path: str, output_path: str, sequence=None, pdb_path=None, chain_id=None, pdb_range=None) -> float:
    """compute_fitness.py process_csv_and_score_mutations (:477-609) for esm3_open."""
    from scipy.stats import spearmanr
    df = pd.read_csv(csv_path)
    print(f"Loaded {len(df)} mutations from CSV file")
    mutations = df["mutant"].tolist()
    if pdb_path is not None:
        print("Scoring mutations with ESM3_open using structure")
        mutation_scores = model.score_mutations_with_pdb(pdb_path, mutations, chain_id, use_structure=True, pdb_range=pdb_range)
    else:
        print("Scoring mutations with ESM3_open using sequence only")
        mutation_scores = model.score_mutations(sequence, mutations)
    score_column = f"{MODEL_TYPE}_score"
    df[score_column] = df["mutant"].map(lambda x: mutation_scores.get(x, np.nan))
    valid_data = df.dropna(subset=[score_column, "DMS_score"])
    if len(valid_data) > 0:
        correlation, _ = spearmanr(valid_data["DMS_score"], valid_data[score_column])
        print(f"Spearman correlation: {correlation:.4f}, based on {len(valid_data)} valid mutations (out of {len(df)} total)")
    else:
        correlation = np.nan
        print("No valid mutations for correlation calculation")
    df.to_csv(output_path, index=False)
    print(f"Results saved to {output_path}")
    return correlation


def main(argv=None):
    args = parser().parse_args(argv)
    if args.model_type != MODEL_TYPE:
        print(f"--model_type {args.model_type} is scored by proteingym_amd.score_esmc_proteingym; this entry scores esm3_open", file=sys.stderr)
        return 2
    if args.use_structure and not args.pdb_dir:
        print("--pdb_dir must be provided when using structure with esm3_open", file=sys.stderr)
        return 2
    if not args.model_path:
        print("--model_path is required: give the ESM3 snapshot directory or state dict (.pth) (this path never downloads)", file=sys.stderr)
        return 2
    os.makedirs(args.output_dir, exist_ok=True)
    assay_list_df = pd.read_csv(args.reference_csv)
    if "DMS_id" not in assay_list_df.columns:
        raise ValueError("Input CSV must contain a 'DMS_id' column")
    if "target_seq" not in assay_list_df.columns:
        raise ValueError("Input CSV must contain a 'target_seq' column with protein sequences")
    if args.use_structure and "pdb_file" not in assay_list_df.columns:
        raise ValueError("Input CSV must contain a 'pdb_file' column if we use structures for scoring")
    has_pdb_range = "pdb_range" in assay_list_df.columns
    assay_list_df = select_assays(assay_list_df, args.DMS_index)
    print(f"Loading ESM3_open from local path: {args.model_path}")
    model = esm3.from_pretrained(args.model_path, MODEL_TYPE, device=args.device, max_rows=args.max_rows)
    if args.use_structure and model.encoder is None:
        print(f"--use_structure needs the structure encoder's weights ({esm3.SNAPSHOT_ENCODER}) beside the model's", file=sys.stderr)
        model.close()
        return 2
    results = {}
    for idx, row in assay_list_df.iterrows():
        assay = row["DMS_id"]
        print(f"\n=== Processing assay {assay} ({idx+1}/{len(assay_list_df)}) ===")
        input_csv = os.path.join(args.dms_dir, f"{assay}.csv")
        output_csv = os.path.join(args.output_dir, f"{assay}.csv")
        if not os.path.exists(input_csv):
            print(f"Error: Input CSV file {input_csv} not found, skipping")
            continue
        try:
            if args.use_structure:
                pdb_path = os.path.join(args.pdb_dir, row["pdb_file"])
                if not os.path.exists(pdb_path):
                    print(f"Error: PDB file {pdb_path} not found, skipping")
                    continue
                pdb_range = row["pdb_range"] if has_pdb_range else None
                results[assay] = score_csv(model, input_csv, output_csv, pdb_path=pdb_path, chain_id="A", pdb_range=pdb_range)
            else:
                results[assay] = score_csv(model, input_csv, output_csv, sequence=row["target_seq"])
        except Exception as e:                       # compute_fitness.py:724-726: one failing assay does not stop the others
            print(f"Error processing {assay}: {e!r}")
            results[assay] = np.nan
    model.close()
    summary_df = pd.DataFrame({"assay": list(results.keys()), "correlation": list(results.values())})
    summary_file_path = os.path.join(args.output_dir, f"correlation_summary_{MODEL_TYPE}.csv")
    if os.path.exists(summary_file_path):
        summary_df.to_csv(summary_file_path, mode="a", header=False, index=False)
    else:
        summary_df.to_csv(summary_file_path, index=False)
    for assay, correlation in results.items():
        print(f"{assay}: Spearman correlation = {correlation:.4f}" if not np.isnan(correlation) else f"{assay}: Failed to calculate correlation")
    return 0


if __name__ == "__main__":
    sys.exit(main())
