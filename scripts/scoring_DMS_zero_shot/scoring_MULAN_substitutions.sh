#!/bin/bash
# MI355X drop-in for ProteinGym's scripts/scoring_DMS_zero_shot/scoring_MULAN_substitutions.sh (same zero_shot_config.sh, same CSVs).
# MULAN_model_path: a local directory with MULAN's config.json and model.safetensors (nothing is downloaded); foldseek_path: the
# Foldseek executable, read only with MULAN_use_foldseek=1 (a SaProt-based MULAN); MULAN_dataset_folder: the reference's preprocessed
# dataset folder, read when it exists (else the angles are taken from the structure files); DMS_structure_folder comes from
# zero_shot_config.sh.  Scores assay DMS_index (0 .. 216).
source "$(dirname "${BASH_SOURCE[0]}")/_pgmi_env.sh"
: "${MULAN_model_path:=/path/to/MULAN-small}"
: "${foldseek_path:=/path/to/foldseek}"
: "${MULAN_dataset_folder:=}"
: "${output_scores_folder:=${DMS_output_score_folder_subs}/MULAN/MULAN_small}"
pgmi_run proteingym_amd.score_mulan_proteingym --MULAN_model_name_or_path "${MULAN_model_path}" \
    --DMS_reference_file_path "${DMS_reference_file_path_subs}" --DMS_data_folder "${DMS_data_folder_subs}" \
    --structure_data_folder "${DMS_structure_folder}" --DMS_index "${DMS_index:=0}" --foldseek_path "${foldseek_path}" \
    --output_dataset_folder "${MULAN_dataset_folder}" --output_scores_folder "${output_scores_folder}" \
    ${MULAN_use_foldseek:+--use_foldseek}
