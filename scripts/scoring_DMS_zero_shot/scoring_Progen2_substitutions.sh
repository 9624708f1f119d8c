#!/bin/bash
# MI355X drop-in for ProteinGym's scripts/scoring_DMS_zero_shot/scoring_Progen2_substitutions.sh (same zero_shot_config.sh, same variables, same CSVs).
# Progen2_model_name_or_path: a progen2-small / -medium / -base / -large / -xlarge checkpoint directory.
source "$(dirname "${BASH_SOURCE[0]}")/_pgmi_env.sh"
: "${output_scores_folder:=${DMS_output_score_folder_subs}/Progen2/small}"
pgmi_progen2 "${DMS_reference_file_path_subs}" "${DMS_data_folder_subs}"
