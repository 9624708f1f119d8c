#!/bin/bash
# MI355X drop-in for ProteinGym's scripts/scoring_DMS_zero_shot/scoring_PoET_substitutions.sh (same zero_shot_config.sh, same CSVs, same
# MSAs).  checkpoint: the PoET .ckpt file (nothing is downloaded); DMS_MSA_data_folder comes from zero_shot_config.sh and holds
# <DMS_filename stem>.a3m.zst (or .a3m).  Scores assay DMS_index (0 .. 216) into <output_scores_folder>/<DMS_filename> with the column
# PoET_score.  --batch_size is passed as the reference passes it; it does not change the scores here.
source "$(dirname "${BASH_SOURCE[0]}")/_pgmi_env.sh"
: "${checkpoint:=/path/to/poet.ckpt}"
: "${output_scores_folder:=${DMS_output_score_folder_subs}/PoET}"
pgmi_run proteingym_amd.score_poet_proteingym --checkpoint "${checkpoint}" --DMS_reference_file_path "${DMS_reference_file_path_subs}" \
    --DMS_data_folder "${DMS_data_folder_subs}" --DMS_index "${DMS_index:=0}" --output_scores_folder "${output_scores_folder}" \
    --MSA_folder "${DMS_MSA_data_folder}" --context_lengths 6144 12288 24576 --batch_size 8
