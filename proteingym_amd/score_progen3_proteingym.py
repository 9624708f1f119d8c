"""ProGen3 assay scoring on MI355X: what ProteinGym's ``Progen3_*`` rows read.

The reference checkout has no launcher of its own for this family (its zero_shot/run.sh calls a score.py that is not in it), so the flags
are ProteinGym's usual ones: the assay is row --DMS_index of the reference file, the output ``<output_scores_folder>/<DMS_id>.csv`` with
the columns mutant, log_likelihood, perplexity and DMS_score where the assay has one -- ``log_likelihood`` keyed by ``mutant`` is what
proteingym/merge.py reads for Progen3_112m .. Progen3_3b.  Scores are ProGen3Scorer's (proteingym_amd/progen3.py): both directions, the
mean over the targets, (forward + reverse) / 2.  Without --indel_mode and without a mutated_sequence column the mutants are applied to
the target sequence; with --indel_mode the mutated_sequence column is scored as it is.  Additive flags: --device, --max_rows.
"""
from __future__ import annotations

import argparse

from . import causal_lm as clm, progen3 as pg3


def parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="ProGen3 scoring (HIP, MI355X)")
    p.add_argument("--Progen3_model_name_or_path", type=str, required=True,
                   help="ProGen3 checkpoint directory (config.json + model.safetensors / pytorch_model.bin)")
    p.add_argument("--DMS_reference_file_path", type=str, help="reference CSV listing the assays (DMS_id, DMS_filename, target_seq)")
    p.add_argument("--DMS_data_folder", type=str, help="folder holding the assay CSVs")
    p.add_argument("--DMS_index", type=int, help="row of the reference CSV to score")
    p.add_argument("--output_scores_folder", type=str, default=None, help="where <DMS_id>.csv is written")
    p.add_argument("--indel_mode", action="store_true", help="score the mutated_sequence column as it is (insertions / deletions)")
    p.add_argument("--max_batch_tokens", type=int, default=pg3.MAX_BATCH_TOKENS, help="token budget of a batch (ProGen3Scorer's default)")
    p.add_argument("--device", type=int, default=0, help="HIP device")
    p.add_argument("--max_rows", type=int, default=0, help="workspace rows per device call (0 = library default)")
    return p


def main(argv=None):
    args = parser().parse_args(argv)
    model = pg3.from_pretrained(args.Progen3_model_name_or_path, device=args.device, max_rows=args.max_rows)
    DMS_id, target_seq, DMS_data = clm.load_assay(args, "Progen3", args.Progen3_model_name_or_path)
    if not args.indel_mode and "mutated_sequence" not in DMS_data.columns:
        DMS_data["mutated_sequence"] = DMS_data["mutant"].apply(lambda x: clm.get_mutated_sequence(target_seq, x))
    ll, ppl = model.score(list(DMS_data["mutated_sequence"]), max_batch_tokens=args.max_batch_tokens)
    DMS_data["log_likelihood"] = ll
    DMS_data["perplexity"] = ppl
    cols = ["mutant", "log_likelihood", "perplexity"] + (["DMS_score"] if "DMS_score" in DMS_data.columns else [])
    out = clm.write_scores(args, DMS_id, DMS_data, cols)
    model.close()
    return out


if __name__ == "__main__":
    main()
