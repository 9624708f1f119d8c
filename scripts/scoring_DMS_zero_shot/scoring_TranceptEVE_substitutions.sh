#!/bin/bash
# MI355X drop-in for ProteinGym's scripts/scoring_DMS_zero_shot/scoring_TranceptEVE_substitutions.sh (same zero_shot_config.sh, same variables, same CSVs).
# checkpoint: a Tranception S / M / L directory; the EVE checkpoints <MSA stem>_seed_<s> (or <UniProt_ID>_seed_<s>) are looked up in DMS_EVE_model_folder,
# and each seed's log-prior is cached under <DMS_EVE_model_folder>/log_prior in the reference's format.
source "$(dirname "${BASH_SOURCE[0]}")/_pgmi_env.sh"
: "${output_scores_folder:=${DMS_output_score_folder_subs}/TranceptEVE/TranceptEVE_L}" "${EVE_num_samples_log_proba:=200000}" "${EVE_seeds:=0 1 2 3 4}"
: "${EVE_model_parameters_location:=/path/to/ProteinGym/proteingym/baselines/trancepteve/trancepteve/utils/eve_model_default_params.json}" "${scoring_window:=optimal}"
pgmi_run proteingym_amd.score_trancepteve_proteingym --checkpoint "${checkpoint:=/path/to/Tranception_Large}" --DMS_index "${DMS_index:=0}" \
    --DMS_reference_file_path "${DMS_reference_file_path_subs}" --DMS_data_folder "${DMS_data_folder_subs}" --output_scores_folder "${output_scores_folder}" \
    --inference_time_retrieval_type TranceptEVE --MSA_folder "${DMS_MSA_data_folder}" --MSA_weights_folder "${DMS_MSA_weights_folder}" \
    --EVE_num_samples_log_proba "${EVE_num_samples_log_proba}" --EVE_model_parameters_location "${EVE_model_parameters_location}" \
    --EVE_model_folder "${DMS_EVE_model_folder}" --scoring_window "${scoring_window}" --EVE_seeds ${EVE_seeds} --EVE_recalibrate_probas
