#!/bin/bash
# MI355X drop-in for ProteinGym's scripts/scoring_DMS_zero_shot/scoring_S3F_substitutions.sh (same zero_shot_config.sh, same CSVs).
# S3F_model_checkpoint: the local S3F task checkpoint (nothing is downloaded); S3F_config: the reference's config/evaluate/s3f.yaml;
# S3F_surfdir: the folder of processed surfaces, one <pdb stem>.pkl per pdb file; DMS_structure_folder comes from zero_shot_config.sh.
# Scores assay DMS_index (0 .. 216).  EVE_scores_folder (optional): a folder of EVE score files, which adds the S3F-MSA column.
source "$(dirname "${BASH_SOURCE[0]}")/_pgmi_env.sh"
: "${S3F_model_checkpoint:=/path/to/s3f.pth}"
: "${S3F_config:=../../proteingym/baselines/S3F/config/evaluate/s3f.yaml}"
: "${S3F_surfdir:=/path/to/processed_surfaces}"
: "${S3F_output_scores_folder:=${DMS_output_score_folder_subs}/S3F}"
pgmi_run proteingym_amd.score_s3f_proteingym -c "${S3F_config}" --datadir "${DMS_data_folder_subs}" \
    --ProteinGym_reference_file "${DMS_reference_file_path_subs}" --structdir "${DMS_structure_folder}" --ckpt "${S3F_model_checkpoint}" \
    --output_scores_folder "${S3F_output_scores_folder}" --surfdir "${S3F_surfdir}" --DMS_index "${DMS_index:=0}" \
    ${EVE_scores_folder:+--MSA_retrieval_location "${EVE_scores_folder}"}
