#!/bin/bash
# MI355X drop-in for ProteinGym's scripts/scoring_DMS_zero_shot/scoring_ProteinMPNN_substitutions.sh (same zero_shot_config.sh, same
# CSVs, same structures).  model_checkpoint: a ProteinMPNN checkpoint file (v_48_002.pt and siblings; nothing is downloaded);
# DMS_structure_folder comes from zero_shot_config.sh.  Scores assay DMS_index (0 .. 216) into <output_scores_folder>/<DMS_id>.csv with
# the column pmpnn_ll.  seed: 0 draws a fresh decoding-order seed per run, as the reference does; any other value fixes the orders.
source "$(dirname "${BASH_SOURCE[0]}")/_pgmi_env.sh"
: "${model_checkpoint:=/path/to/ProteinMPNN/vanilla_model_weights/v_48_020.pt}"
: "${output_scores_folder:=${DMS_output_score_folder_subs}/ProteinMPNN}"
pgmi_run proteingym_amd.score_proteinmpnn_proteingym --checkpoint "${model_checkpoint}" --structure_folder "${DMS_structure_folder}" \
    --DMS_index "${DMS_index:=0}" --DMS_reference_file_path "${DMS_reference_file_path_subs}" --DMS_data_folder "${DMS_data_folder_subs}" \
    --output_scores_folder "${output_scores_folder}" --seed "${seed:=0}"
