#!/bin/bash
# MI355X drop-in for ProteinGym's scripts/scoring_DMS_zero_shot/scoring_ProtGPT2_indels.sh (same zero_shot_config.sh, same variables, same CSVs).
# ProtGPT2_model_name_or_path: the ProtGPT2 checkpoint directory; ProtGPT2_tokenizer_path: its tokenizer (default: the model directory).
source "$(dirname "${BASH_SOURCE[0]}")/_pgmi_env.sh"
: "${ProtGPT2_model_name_or_path:=/path/to/ProtGPT2}"
: "${output_scores_folder:=${DMS_output_score_folder_indels}/ProtGPT2}"
pgmi_causal_lm proteingym_amd.score_protgpt2_proteingym --ProtGPT2_model_name_or_path "${ProtGPT2_model_name_or_path}" "${DMS_reference_file_path_indels}" "${DMS_data_folder_indels}" --indel_mode \
    ${ProtGPT2_tokenizer_path:+--tokenizer_path "${ProtGPT2_tokenizer_path}"}
