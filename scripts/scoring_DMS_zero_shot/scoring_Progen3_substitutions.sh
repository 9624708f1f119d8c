#!/bin/bash
# MI355X launcher for ProteinGym's Progen3_* rows, substitutions (same zero_shot_config.sh, same variables, same CSVs as the other families;
# ProteinGym ships no launcher of its own for ProGen3).
# Progen3_model_name_or_path: a ProGen3 checkpoint directory (112m / 219m / 339m / 762m / 1b / 3b); Progen3_size names the output subfolder.
source "$(dirname "${BASH_SOURCE[0]}")/_pgmi_env.sh"
: "${output_scores_folder:=${DMS_output_score_folder_subs}/Progen3/${Progen3_size:-339m}}"
pgmi_progen3 "${DMS_reference_file_path_subs}" "${DMS_data_folder_subs}"
