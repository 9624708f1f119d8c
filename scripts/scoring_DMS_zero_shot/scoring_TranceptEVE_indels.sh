#!/bin/bash
# MI355X drop-in for ProteinGym's scripts/scoring_DMS_zero_shot/scoring_TranceptEVE_indels.sh (same zero_shot_config.sh, same variables, same CSVs):
# every scored sequence is re-aligned to the family alignment by the Clustal Omega executable you point at, and both priors go through those rows.
source "$(dirname "${BASH_SOURCE[0]}")/_pgmi_env.sh"
: "${output_scores_folder:=${DMS_output_score_folder_indels}/TranceptEVE/TranceptEVE_L}" "${EVE_num_samples_log_proba:=200000}" "${EVE_seeds:=0 1 2 3 4}"
: "${EVE_model_parameters_location:=/path/to/ProteinGym/proteingym/baselines/trancepteve/trancepteve/utils/eve_model_default_params.json}" "${clustal_omega_location:=/path/to/clustalo}"
pgmi_run proteingym_amd.score_trancepteve_proteingym --checkpoint "${checkpoint:=/path/to/Tranception_Large}" --DMS_index "${DMS_index:=0}" \
    --DMS_reference_file_path "${DMS_reference_file_path_indels}" --DMS_data_folder "${DMS_data_folder_indels}" --output_scores_folder "${output_scores_folder}" \
    --indel_mode --clustal_omega_location "${clustal_omega_location}" --inference_time_retrieval_type TranceptEVE --MSA_folder "${DMS_MSA_data_folder}" \
    --MSA_weights_folder "${DMS_MSA_weights_folder}" --EVE_num_samples_log_proba "${EVE_num_samples_log_proba}" \
    --EVE_model_parameters_location "${EVE_model_parameters_location}" --EVE_model_folder "${DMS_EVE_model_folder}" --scoring_window optimal \
    --EVE_seeds ${EVE_seeds} --EVE_recalibrate_probas
