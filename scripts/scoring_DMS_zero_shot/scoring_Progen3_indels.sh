#!/bin/bash
# MI355X launcher for ProteinGym's Progen3_* rows, indels (same zero_shot_config.sh, same variables, same CSVs as the other families).
source "$(dirname "${BASH_SOURCE[0]}")/_pgmi_env.sh"
: "${output_scores_folder:=${DMS_output_score_folder_indels}/Progen3/${Progen3_size:-339m}}"
pgmi_progen3 "${DMS_reference_file_path_indels}" "${DMS_data_folder_indels}" --indel_mode
