"""Drop-in for ``proteingym/baselines/evoscale/compute_fitness.py`` (ESM C, sequence only) on MI355X.

Same flags, same assay loop (:636-742): every assay of --reference_csv (or row --DMS_index; an index out of range scores all of them,
with a warning), ``<output_dir>/<DMS_id>.csv`` = the assay's columns plus ``<model_type>_score`` (NaN for the mutants the reference
skips), written after the Spearman step, and ``correlation_summary_<model_type>.csv`` appended to (header only when it is created).
A failing assay -- a mutant letter outside the 20 standard amino acids is the reference's KeyError -- gets a NaN summary row and no
CSV.  The model is loaded once from --model_path (a .pth state dict or a snapshot directory); nothing is downloaded.  esm3_open and
--use_structure are not supported on this path (score_esm3_proteingym scores them).  Additive flags: --device, --max_rows.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import pandas as pd

from . import esmc


def parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Process DMS assays with ESM model scoring (HIP, MI355X)")
    p.add_argument("--model_type", choices=["esmc_300M", "esmc_600M", "esm3_open"], default="esmc_300M",
                   help="Model type to use for scoring (esmc_300M, esmc_600M; esm3_open is not supported on this path)")
    p.add_argument("--model_path", type=str, default=None, help="ESMC state dict (.pth) or snapshot directory (required: nothing is downloaded)")
    p.add_argument("--reference_csv", required=True, help="CSV file with DMS_id and target_seq columns")
    p.add_argument("--dms_dir", required=True, help="Directory containing DMS CSV files")
    p.add_argument("--pdb_dir", required=False, default=None, help="accepted for compatibility (structure is esm3_open only)")
    p.add_argument("--output_dir", required=True, help="Directory to save output files")
    p.add_argument("--use_structure", action="store_true", default=False, help="esm3_open only: not supported on this path")
    p.add_argument("--DMS_index", required=False, default=-1, help="Index of DMS to score. If not provided, score all DMS assays")
    p.add_argument("--device", type=int, default=0, help="HIP device")
    p.add_argument("--max_rows", type=int, default=0, help="workspace rows per device call (0 = library default)")
    return p


def select_assays(assay_list_df: pd.DataFrame, dms_index) -> pd.DataFrame:
    """compute_fitness.py:675-685."""
    if dms_index != -1:
        try:
            dms_index = int(dms_index)
            if 0 <= dms_index < len(assay_list_df):
                assay_list_df = assay_list_df.iloc[[dms_index]]
                print(f"Processing only DMS at index {dms_index}: {assay_list_df.iloc[0]['DMS_id']}")
            else:
                print(f"Warning: DMS_index {dms_index} out of range (0-{len(assay_list_df)-1}), processing all assays")
        except ValueError:
            print(f"Warning: Invalid DMS_index '{dms_index}', processing all assays")
    return assay_list_df


def score_csv(model: esmc.ESMC, csv_path: str, sequence: str, model_type: str, output_path: str) -> float:
    """compute_fitness.py process_csv_and_score_mutations (:495-617) for the ESM C models."""
    from scipy.stats import spearmanr
    df = pd.read_csv(csv_path)
    print(f"Loaded {len(df)} mutations from CSV file")
    mutation_scores = model.score_mutations(sequence, df["mutant"].tolist())
    score_column = f"{model_type}_score"
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
    if args.model_type == "esm3_open" or args.use_structure:
        print("esm3_open / --use_structure (ESM3 with structure tracks) is not supported on this path: "
              "use proteingym_amd.score_esm3_proteingym", file=sys.stderr)
        return 2
    if not args.model_path:
        print("--model_path is required: give the ESMC state dict (.pth) or its snapshot directory (this path never downloads)",
              file=sys.stderr)
        return 2
    os.makedirs(args.output_dir, exist_ok=True)
    assay_list_df = pd.read_csv(args.reference_csv)
    if "DMS_id" not in assay_list_df.columns:
        raise ValueError("Input CSV must contain a 'DMS_id' column")
    if "target_seq" not in assay_list_df.columns:
        raise ValueError("Input CSV must contain a 'target_seq' column with protein sequences")
    assay_list_df = select_assays(assay_list_df, args.DMS_index)
    print(f"Loading {args.model_type} from local path: {args.model_path}")
    model = esmc.from_pretrained(args.model_path, args.model_type, device=args.device, max_rows=args.max_rows)
    results = {}
    for idx, row in assay_list_df.iterrows():
        assay = row["DMS_id"]
        print(f"\n=== Processing assay {assay} ({idx+1}/{len(assay_list_df)}) ===")
        input_csv = os.path.join(args.dms_dir, f"{assay}.csv")
        if not os.path.exists(input_csv):
            print(f"Error: Input CSV file {input_csv} not found, skipping")
            continue
        try:
            results[assay] = score_csv(model, input_csv, row["target_seq"], args.model_type, os.path.join(args.output_dir, f"{assay}.csv"))
        except Exception as e:                       # compute_fitness.py:724-726: one failing assay does not stop the others
            print(f"Error processing {assay}: {e!r}")
            results[assay] = np.nan
    model.close()
    summary_df = pd.DataFrame({"assay": list(results.keys()), "correlation": list(results.values())})
    summary_file_path = os.path.join(args.output_dir, f"correlation_summary_{args.model_type}.csv")
    if os.path.exists(summary_file_path):
        summary_df.to_csv(summary_file_path, mode="a", header=False, index=False)
    else:
        summary_df.to_csv(summary_file_path, index=False)
    for assay, correlation in results.items():
        print(f"{assay}: Spearman correlation = {correlation:.4f}" if not np.isnan(correlation) else f"{assay}: Failed to calculate correlation")
    return 0


if __name__ == "__main__":
    sys.exit(main())
