#!/bin/bash
# MI355X drop-in for ProteinGym's scripts/scoring_DMS_zero_shot/scoring_EVE_substitutions.sh (same zero_shot_config.sh, same CSVs, same
# checkpoints: <DMS_EVE_model_folder>/<MSA name>_seed_<seed>).  model_parameters_location: the parameter JSON the checkpoints were
# trained with (ProteinGym's proteingym/baselines/EVE/EVE/default_model_params.json).  Scores assay DMS_index (0 .. 216) with the
# reference launcher's settings: 20 000 samples, seeds 0 .. 4, focus-column threshold 1.  EVE_checkpoint_folder and EVE_score_name
# let scoring_DeepSequence_substitutions.sh run the same lines on DeepSequence's checkpoints.
source "$(dirname "${BASH_SOURCE[0]}")/_pgmi_env.sh"
: "${model_parameters_location:=/path/to/ProteinGym/proteingym/baselines/EVE/EVE/default_model_params.json}"
: "${EVE_checkpoint_folder:=${DMS_EVE_model_folder}}"
: "${output_scores_folder:=${DMS_output_score_folder_subs}/${EVE_score_name:-EVE}/}"
: "${num_samples_compute_evol_indices:=20000}"
: "${batch_size:=1024}"
: "${random_seeds:=0 1 2 3 4}"
pgmi_run proteingym_amd.score_eve_proteingym --MSA_data_folder "${DMS_MSA_data_folder}" \
    --DMS_reference_file_path "${DMS_reference_file_path_subs}" --protein_index "${DMS_index:=0}" \
    --VAE_checkpoint_location "${EVE_checkpoint_folder}" --model_parameters_location "${model_parameters_location}" \
    --DMS_data_folder "${DMS_data_folder_subs}" --output_evol_indices_location "${output_scores_folder}" \
    --num_samples_compute_evol_indices "${num_samples_compute_evol_indices}" --batch_size "${batch_size}" --aggregation_method full \
    --threshold_focus_cols_frac_gaps 1 --skip_existing --MSA_weights_location "${DMS_MSA_weights_folder}" --random_seeds ${random_seeds}
