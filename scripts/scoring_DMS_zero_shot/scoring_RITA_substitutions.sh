#!/bin/bash
# MI355X drop-in for ProteinGym's scripts/scoring_DMS_zero_shot/scoring_RITA_substitutions.sh (same zero_shot_config.sh, same variables, same CSVs).
# RITA_model_name_or_path: a RITA_s / _m / _l / _xl checkpoint directory; RITA_tokenizer_path: its tokenizer (default: the model directory).
source "$(dirname "${BASH_SOURCE[0]}")/_pgmi_env.sh"
: "${RITA_model_name_or_path:=/path/to/RITA_s}"
: "${output_scores_folder:=${DMS_output_score_folder_subs}/RITA/small}"
pgmi_causal_lm proteingym_amd.score_rita_proteingym --RITA_model_name_or_path "${RITA_model_name_or_path}" "${DMS_reference_file_path_subs}" "${DMS_data_folder_subs}" \
    ${RITA_tokenizer_path:+--tokenizer_path "${RITA_tokenizer_path}"}
