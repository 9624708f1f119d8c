#!/bin/bash
# MI355X drop-in for ProteinGym's scripts/scoring_DMS_zero_shot/scoring_Progen2_indels.sh (same zero_shot_config.sh, same variables, same CSVs).
source "$(dirname "${BASH_SOURCE[0]}")/_pgmi_env.sh"
: "${output_scores_folder:=${DMS_output_score_folder_indels}/Progen2/small}"
pgmi_progen2 "${DMS_reference_file_path_indels}" "${DMS_data_folder_indels}" --indel_mode
