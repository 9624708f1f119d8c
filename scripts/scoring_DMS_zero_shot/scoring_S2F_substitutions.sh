#!/bin/bash
# MI355X drop-in for ProteinGym's scripts/scoring_DMS_zero_shot/scoring_S2F_substitutions.sh (same zero_shot_config.sh, same CSVs).
# S2F_model_checkpoint: the local S2F task checkpoint (nothing is downloaded); S2F_config: the reference's config/evaluate/s2f.yaml;
# DMS_structure_folder comes from zero_shot_config.sh.  Scores assay DMS_index (0 .. 216).  EVE_scores_folder (optional): a folder of
# EVE score files, which adds the S2F-MSA column.
source "$(dirname "${BASH_SOURCE[0]}")/_pgmi_env.sh"
: "${S2F_model_checkpoint:=/path/to/s2f.pth}"
: "${S2F_config:=../../proteingym/baselines/S3F/config/evaluate/s2f.yaml}"
: "${S2F_output_scores_folder:=${DMS_output_score_folder_subs}/S2F}"
pgmi_run proteingym_amd.score_s2f_proteingym -c "${S2F_config}" --datadir "${DMS_data_folder_subs}" \
    --ProteinGym_reference_file "${DMS_reference_file_path_subs}" --structdir "${DMS_structure_folder}" --ckpt "${S2F_model_checkpoint}" \
    --output_scores_folder "${S2F_output_scores_folder}" --DMS_index "${DMS_index:=0}" \
    ${EVE_scores_folder:+--MSA_retrieval_location "${EVE_scores_folder}"}
