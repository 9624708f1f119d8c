#!/bin/bash
# MI355X drop-in for ProteinGym's scripts/scoring_DMS_zero_shot/scoring_ProtSSN_substitutions.sh (same zero_shot_config.sh, same variables).
# DMS_and_structure_folder: the unzipped ProteinGym_substitutions_pdb-csv_checked folder (it holds DATASET/<name>/<name>.pdb and .tsv);
# model_checkpoint: the folder of protssn_k{k}_h{h}.pt; model_name: the checkpoints to run, all nine for the ensemble; ProtSSN_plm: a
# local ESM2-650M, a fair-esm .pt or an HF EsmModel directory (nothing is downloaded).  DMS_index (optional) scores one assay of the
# sorted folder names instead of all of them.
source "$(dirname "${BASH_SOURCE[0]}")/_pgmi_env.sh"
: "${DMS_and_structure_folder:=/path/to/ProteinGym_substitutions_pdb-csv_checked}"
: "${model_checkpoint:=/path/to/ProtSSN_model}"
: "${model_name:=k10_h512 k20_h512 k30_h512 k10_h768 k20_h768 k30_h768 k10_h1280 k20_h1280 k30_h1280}"
: "${gnn_config:=../../proteingym/baselines/protssn/src/config/egnn.yaml}"
: "${score_info:=../../protssn_scores.csv}"
: "${ProtSSN_plm:=/path/to/esm2_t33_650M_UR50D.pt}"
: "${DMS_output_score_folder:=${DMS_output_score_folder_subs}/ProtSSN}"
pgmi_run proteingym_amd.score_protssn_proteingym --gnn_config "${gnn_config}" --gnn_model_dir "${model_checkpoint}" \
    --gnn_model_name ${model_name} --use_ensemble --mutant_dataset_dir "${DMS_and_structure_folder}" \
    --output_scores_folder "${DMS_output_score_folder}" --score_info "${score_info}" --plm "${ProtSSN_plm}" \
    --repo_path "${PGMI_PROTEINGYM_REPO:-../..}" ${DMS_index:+--DMS_index "${DMS_index}"}
