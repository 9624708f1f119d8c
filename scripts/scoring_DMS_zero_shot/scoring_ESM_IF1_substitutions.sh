#!/bin/bash
# MI355X drop-in for ProteinGym's scripts/scoring_DMS_zero_shot/scoring_ESM_IF1_substitutions.sh (same zero_shot_config.sh, same CSVs,
# same structures).  model_checkpoint: esm_if1_gvp4_t16_142M_UR50.pt (nothing is downloaded); DMS_structure_folder comes from
# zero_shot_config.sh.  Scores assay DMS_index (0 .. 216) into <output_scores_folder>/<DMS_id>.csv with the column esmif1_ll.  The
# backbone is encoded once per assay; only the decoder runs per mutant.
source "$(dirname "${BASH_SOURCE[0]}")/_pgmi_env.sh"
: "${model_checkpoint:=/path/to/esm_if1_gvp4_t16_142M_UR50.pt}"
: "${output_scores_folder:=${DMS_output_score_folder_subs}/ESM-IF1}"
pgmi_run proteingym_amd.score_esmif1_proteingym --model_location "${model_checkpoint}" --structure_folder "${DMS_structure_folder}" \
    --DMS_index "${DMS_index:=0}" --DMS_reference_file_path "${DMS_reference_file_path_subs}" --DMS_data_folder "${DMS_data_folder_subs}" \
    --output_scores_folder "${output_scores_folder}" --chain "${chain:=A}"
