"""UniRep assay scoring on MI355X: what ProteinGym's ``Unirep`` and ``Unirep_evotune`` rows read.

The flags are proteingym/baselines/unirep/unirep_inference.py's: the assay is row --DMS_index of --mapping_path, its CSV is read from
--data_path, and ``<output_dir>/<DMS_id>.csv`` gets the columns mutated_sequence, Unirep_score -- the mean negative log-likelihood
(lower is fitter; proteingym/merge.py reads it with directionality -1).  As in the reference the sequences are np.unique of the
``mutated_sequence`` column (``mutant`` when it is absent), '*' stripped, invalid ones dropped.  --evotune appends the assay's
MSA_filename stem to --model_path.  --batch_size changes no result in the reference (a row's value does not depend on its batch) and
none here; --save_hidden saves nothing in the reference (the lines are commented out) and nothing here.  When the mapping has a
target_seq column the target runs once and every sequence starts from the state at its first difference (the same bits as a run from
the zero state; --from_scratch runs every step of every sequence).  Additive flags: --device, --precision, --max_rows, --from_scratch.
"""
from __future__ import annotations

import argparse
import os
import pathlib

from . import unirep as ur


def parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="UniRep scoring (HIP, MI355X)")
    p.add_argument("--model_path", type=str, required=True, help="directory of the checkpoint's .npy arrays")
    p.add_argument("--data_path", type=str, required=True, help="folder holding the assay CSVs")
    p.add_argument("--mapping_path", type=str, required=True, help="reference CSV listing the assays (DMS_id, DMS_filename, MSA_filename)")
    p.add_argument("--output_dir", type=str, required=True)
    p.add_argument("--DMS_index", type=int, required=True)
    p.add_argument("--batch_size", type=int, default=64, help="accepted; changes no result")
    p.add_argument("--evotune", action="store_true", help="score with the weights evotuned on the assay's MSA: <model_path>/<MSA stem>")
    p.add_argument("--save_hidden", dest="save_hidden", action="store_true", help="accepted; saves nothing, as in the reference")
    p.add_argument("--device", type=int, default=0, help="HIP device")
    p.add_argument("--precision", type=str, default="f16x3", choices=["f16x3", "fp32"])
    p.add_argument("--max_rows", type=int, default=0, help="rows per device chunk (0 = library default)")
    p.add_argument("--from_scratch", action="store_true", help="run every sequence from the zero state (no shared prefix)")
    return p


def main(argv=None):
    import pandas as pd
    args = parser().parse_args(argv)
    pathlib.Path(args.output_dir).mkdir(parents=True, exist_ok=True)
    mapping = pd.read_csv(args.mapping_path)
    DMS_id = mapping["DMS_id"][args.DMS_index]
    row = mapping[mapping["DMS_id"] == DMS_id]
    DMS_file_name = row["DMS_filename"].values[0]
    model_path = args.model_path
    if args.evotune:
        model_path = ur.evotune_path(model_path, row["MSA_filename"].values[0])
    print(f"Computing scores for: {DMS_id} with Unirep {model_path}")
    seqs = ur.load_and_filter_seqs(pd.read_csv(args.data_path + os.sep + DMS_file_name, low_memory=False))
    model = ur.from_pretrained(model_path, device=args.device, precision=args.precision, max_rows=args.max_rows)
    target = row["target_seq"].values[0] if "target_seq" in mapping.columns else None
    if isinstance(target, str) and not args.from_scratch:
        model.set_target(target.strip('*'))
    scores = model.nll(seqs, from_scratch=args.from_scratch) if seqs else []
    out = args.output_dir + os.sep + str(DMS_id) + ".csv"
    pd.DataFrame({"mutated_sequence": seqs, "Unirep_score": scores}).to_csv(out, index=False)
    print(f"Ran inference on {len(seqs)} sequences ({model.last_row_steps} cell row-steps). Saved results to {args.output_dir}.")
    model.close()
    return out


if __name__ == "__main__":
    main()
