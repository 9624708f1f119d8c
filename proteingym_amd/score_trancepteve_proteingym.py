"""Drop-in for ``proteingym/baselines/trancepteve/score_trancepteve.py`` on MI355X.

Same flags, defaults and input resolution (reference file row or manual fields), same output file
``<output_scores_folder>/<DMS_id>.csv`` with Tranception's columns plus, for substitutions, the ``mutant`` column the reference merges
back (with ``--clinvar_scoring`` left-merged with the input on ``mutant``), and the same line appended to ``TranceptEVE_aggregation_coefficients_log`` in the working directory -- seven values under
the reference's six-name header (score_trancepteve.py:200-206).  ``--model_framework``, ``--num_workers`` and
``--batch_size_inference`` are accepted; the device batches on its own.  Additive flags: ``--device``, ``--EVE_ignore_log_prior_cache``.
"""
from __future__ import annotations

import argparse
import os

import pandas as pd

from . import tranception as ptr, trancepteve as tte

# (flag, argparse keywords): names, types and defaults are the reference's CLI contract (score_trancepteve.py:19-60); help texts are ours
_FLAGS = [
    ("--checkpoint", dict(type=str, help="Tranception checkpoint directory (HuggingFace layout)")),
    ("--model_framework", dict(default="pytorch", type=str, help="kept for compatibility")),
    ("--batch_size_inference", dict(default=20, type=int, help="kept for compatibility")),
    ("--DMS_reference_file_path", dict(default=None, type=str, help="reference CSV listing the assays")),
    ("--DMS_index", dict(default=0, type=int, help="row of the reference CSV to score")),
    ("--target_seq", dict(default=None, type=str, help="wild-type sequence (manual mode)")),
    ("--DMS_file_name", dict(default=None, type=str, help="assay CSV inside --DMS_data_folder (manual mode)")),
    ("--MSA_filename", dict(default=None, type=str, help="alignment (a2m) inside --MSA_folder (manual mode)")),
    ("--MSA_weight_file_name", dict(default=None, type=str, help="sequence-weight .npy inside --MSA_weights_folder (manual mode)")),
    ("--MSA_start", dict(default=None, type=int, help="first target position covered by the alignment, 1-indexed (manual mode)")),
    ("--MSA_end", dict(default=None, type=int, help="last target position covered by the alignment, 1-indexed (manual mode)")),
    ("--UniprotID", dict(default=None, type=str, help="UniProt id naming the EVE checkpoints (manual mode)")),
    ("--MSA_threshold_sequence_frac_gaps", dict(default=None, type=float, help="alignment processing: sequence gap threshold")),
    ("--MSA_threshold_focus_cols_frac_gaps", dict(default=None, type=float, help="alignment processing: focus-column gap threshold")),
    ("--DMS_data_folder", dict(type=str, help="folder holding the assay CSVs")),
    ("--output_scores_folder", dict(default="./", type=str, help="where <DMS_id>.csv is written")),
    ("--deactivate_scoring_mirror", dict(action="store_true", help="score left-to-right only")),
    ("--indel_mode", dict(action="store_true", help="the assay holds insertions / deletions")),
    ("--scoring_window", dict(default="optimal", type=str, help="optimal | sliding")),
    ("--num_workers", dict(default=8, type=int, help="kept for compatibility")),
    ("--inference_time_retrieval_type", dict(default=None, type=str, help="None | Tranception | TranceptEVE")),
    ("--retrieval_weights_manual", dict(action="store_true", help="take the two weights from the flags below")),
    ("--retrieval_inference_MSA_weight", dict(default=0.5, type=float, help="alpha")),
    ("--retrieval_inference_EVE_weight", dict(default=0.5, type=float, help="beta")),
    ("--MSA_folder", dict(default=".", type=str, help="folder holding the alignments")),
    ("--MSA_weights_folder", dict(default=None, type=str, help="folder holding the sequence-weight files")),
    ("--clustal_omega_location", dict(default=None, type=str, help="Clustal Omega executable (indels with retrieval)")),
    ("--EVE_model_folder", dict(type=str, help="folder holding the EVE checkpoints")),
    ("--EVE_seeds", dict(nargs="*", help="seeds of the EVE checkpoints")),
    ("--EVE_num_samples_log_proba", dict(default=10, type=int, help="Monte-Carlo samples of the EVE log-prior")),
    ("--EVE_model_parameters_location", dict(default=None, type=str, help="EVE parameter JSON")),
    ("--MSA_recalibrate_probas", dict(action="store_true", help="match the MSA prior's temperature to the transformer's")),
    ("--EVE_recalibrate_probas", dict(action="store_true", help="match the EVE prior's temperature to the transformer's")),
    ("--clinvar_scoring", dict(action="store_true", help="ClinVar input: merge the scores with the input on `mutant`")),
    ("--device", dict(type=int, default=int(os.environ.get("LOCAL_RANK", "0")), help="[additive] GPU index")),
    ("--EVE_ignore_log_prior_cache", dict(action="store_true", help="[additive] neither read nor write <EVE_model_folder>/log_prior")),
]

LOG_NAME = "TranceptEVE_aggregation_coefficients_log"
LOG_HEADER = "DMS_id,num_mutants_scored,num_mutants_scored_no_na,processed_MSA_depth,retrieval_inference_MSA_weight,retrieval_inference_EVE_weight\n"


def create_parser():
    parser = argparse.ArgumentParser(description="TranceptEVE scoring on MI355X")
    for flag, kw in _FLAGS:
        parser.add_argument(flag, **kw)
    return parser


def resolve_inputs(args):
    """score_trancepteve.py:73-104: (DMS_id, target_seq, DMS_file_name, UniProt_ID, msa) with msa = dict(file, weights, start
    (0-based), end, thr_seq, thr_cols) or None without retrieval."""
    msa = None
    if args.DMS_reference_file_path:
        table = pd.read_csv(args.DMS_reference_file_path)
        dms_id = table["DMS_id"][args.DMS_index]
        print("Compute scores for DMS: " + str(dms_id))
        row = table[table["DMS_id"] == dms_id]
        target_seq = row["target_seq"].values[0].upper()
        file_name = row["DMS_filename"].values[0]
        uniprot = row["UniProt_ID"].values[0] if "UniProt_ID" in table else "No ID"
        if args.inference_time_retrieval_type is not None:
            def column(name, default):
                return float(row[name].values[0]) if name in table else default
            msa = dict(file=args.MSA_folder + os.sep + table["MSA_filename"][args.DMS_index] if args.MSA_folder is not None else None,
                       weights=args.MSA_weights_folder + os.sep + row["weight_file_name"].values[0] if args.MSA_weights_folder else None,
                       start=int(row["MSA_start"].values[0]) - 1, end=int(row["MSA_end"].values[0]),
                       thr_seq=column("MSA_threshold_sequence_frac_gaps", 0.5), thr_cols=column("MSA_threshold_focus_cols_frac_gaps", 1.0))
            print("Sequence (fragment) gap threshold: " + str(msa["thr_seq"]))
            print("Focus column gap threshold: " + str(msa["thr_cols"]))
    else:
        target_seq, file_name, uniprot = args.target_seq, args.DMS_file_name, args.UniprotID
        dms_id = file_name.split(".")[0]
        if args.inference_time_retrieval_type is not None:
            msa = dict(file=args.MSA_folder + os.sep + args.MSA_filename if args.MSA_folder is not None else None,
                       weights=args.MSA_weights_folder + os.sep + args.MSA_weight_file_name if args.MSA_weights_folder is not None else None,
                       start=args.MSA_start - 1, end=args.MSA_end, thr_seq=args.MSA_threshold_sequence_frac_gaps,
                       thr_cols=args.MSA_threshold_focus_cols_frac_gaps)
    return dms_id, target_seq, file_name, uniprot, msa


def main(argv=None):
    args = create_parser().parse_args(argv)
    print(args)
    dms_id, target_seq, file_name, uniprot, msa = resolve_inputs(args)
    model = ptr.from_pretrained(args.checkpoint, device=args.device, scoring_window=args.scoring_window)
    state = None
    if msa is not None:
        kind = args.inference_time_retrieval_type
        thr_seq = 0.5 if msa["thr_seq"] is None else msa["thr_seq"]
        thr_cols = 1.0 if msa["thr_cols"] is None else msa["thr_cols"]
        eve_table = eve_msa = None
        if "TranceptEVE" in kind:
            seeds = args.EVE_seeds or []
            print("Number of distinct EVE models to be leveraged: {}".format(len(seeds)))
            paths = tte.eve_model_paths(args.EVE_model_folder, msa["file"], uniprot, seeds)
            assert len(paths) >= 1, "Could not find a reference for EVE model"
            if thr_cols != 1.0:
                print("threshold_focus_cols_frac_gaps not 1.0. Only well-covered positions are factored in the EVE retrieval aggregation.")
            eve_msa = tte.EveMSA(msa["file"], thr_seq, thr_cols)
            eve_table = tte.eve_log_prior(paths, args.EVE_model_parameters_location, eve_msa, len(target_seq), msa["start"],
                                          num_samples=args.EVE_num_samples_log_proba, use_cache=not args.EVE_ignore_log_prior_cache,
                                          device=args.device)
        state = tte.build_state(model, target_seq, msa["file"], msa["weights"], msa["start"], msa["end"], indel_mode=args.indel_mode,
                                threshold_sequence_frac_gaps=thr_seq, threshold_focus_cols_frac_gaps=thr_cols, retrieval_type=kind,
                                eve_table=eve_table, eve_msa=eve_msa, manual_weights=args.retrieval_weights_manual,
                                manual_msa_weight=args.retrieval_inference_MSA_weight, manual_eve_weight=args.retrieval_inference_EVE_weight,
                                MSA_recalibrate=args.MSA_recalibrate_probas and "TranceptEVE" in kind,
                                EVE_recalibrate=args.EVE_recalibrate_probas and "TranceptEVE" in kind,
                                clustal_omega_location=args.clustal_omega_location)
        model.retrieval = state
    else:
        print("Model only uses autoregressive inference")
    os.makedirs(args.output_scores_folder, exist_ok=True)
    out_csv = args.output_scores_folder + os.sep + dms_id + ".csv"
    assay = pd.read_csv(args.DMS_data_folder + os.sep + file_name, low_memory=False)
    scores = model.score_mutants(DMS_data=assay, target_seq=target_seq, scoring_mirror=not args.deactivate_scoring_mirror,
                                 batch_size_inference=args.batch_size_inference, num_workers=args.num_workers, indel_mode=args.indel_mode)
    if args.indel_mode and "mutant" in scores:              # Tranception writes the wild type's zero row under 'mutant' in indel mode
        scores["mutated_sequence"] = scores["mutated_sequence"].fillna(scores["mutant"])      # (tranception model_pytorch.py:918-927);
        scores = scores.drop(columns=["mutant"])                                                # TranceptEVE under 'mutated_sequence' (:1215-1220)
    if len(scores) > 0 and not args.indel_mode:             # model_pytorch.py:1192-1197, :1221: the mutation triplet comes back (substitutions)
        df = assay.copy()
        if "mutated_sequence" not in df:
            df["mutated_sequence"] = df["mutant"].apply(lambda x: ptr.get_mutated_sequence(target_seq, x))
        if "mutant" not in df:
            df["mutant"] = df["mutated_sequence"]
        scores = pd.merge(scores, df[["mutated_sequence", "mutant"]], how="left", on="mutated_sequence")
    if len(scores) > 0 and args.clinvar_scoring:
        scores = pd.merge(scores, assay, how="left", on="mutant")
    scores.to_csv(out_csv + ".tmp", index=False)
    os.replace(out_csv + ".tmp", out_csv)
    model.close()
    s = state or {}
    log = "ClinVar_scoring_Tranception_20221130" if args.clinvar_scoring else LOG_NAME
    with open(log, "a+") as f:
        if os.stat(log).st_size == 0:
            f.write(LOG_HEADER)
        values = [dms_id, len(scores), len(scores.dropna()), s.get("MSA_processed_depth", 0), s.get("EVE_processed_depth", 0),
                  s.get("weight"), s.get("eve_weight")]
        f.write(",".join(str(x) for x in values) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
