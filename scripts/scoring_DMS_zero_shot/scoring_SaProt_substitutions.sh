#!/bin/bash
# MI355X drop-in for ProteinGym's scripts/scoring_DMS_zero_shot/scoring_SaProt_substitutions.sh (same zero_shot_config.sh, same CSVs).
# SaProt_model_path: a local directory with SaProt's config.json, vocab.txt and model.safetensors (nothing is downloaded);
# foldseek_bin: the Foldseek executable; DMS_structure_folder comes from zero_shot_config.sh.  Scores assay DMS_index (0 .. 216).
source "$(dirname "${BASH_SOURCE[0]}")/_pgmi_env.sh"
: "${SaProt_model_path:=/path/to/SaProt_650M_AF2}"
: "${foldseek_bin:=/path/to/foldseek}"
: "${output_scores_folder:=${DMS_output_score_folder_subs}/SaProt/SaProt_650M_AF2}"
pgmi_run proteingym_amd.score_saprot_proteingym --foldseek_bin "${foldseek_bin}" --SaProt_model_name_or_path "${SaProt_model_path}" \
    --DMS_reference_file_path "${DMS_reference_file_path_subs}" --DMS_data_folder "${DMS_data_folder_subs}" \
    --structure_data_folder "${DMS_structure_folder}" --DMS_index "${DMS_index:=0}" --output_scores_folder "${output_scores_folder}"
