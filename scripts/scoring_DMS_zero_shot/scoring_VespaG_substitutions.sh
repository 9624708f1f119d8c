#!/bin/bash
# MI355X drop-in for ProteinGym's scripts/scoring_DMS_zero_shot/scoring_VespaG_substitutions.sh (same zero_shot_config.sh, same variables).
# The two paths to set: model_checkpoint_file = VespaG's state_dict_v2.pt, and either precomputed_embedding_file = the pre-computed
# ESM2-3B embeddings (an .npz of id -> [L, 2560]; the reference's .h5 where h5py is installed) or VespaG_plm = a local ESM2-3B, a fair-esm
# .pt or an HF EsmModel directory, to compute them here (nothing is downloaded).  Every assay of the reference file is scored in one call;
# the per-assay CSVs land in ${DMS_output_score_folder_subs}/VespaG, where merge.py looks for config.json's "VespaG" entry.
source "$(dirname "${BASH_SOURCE[0]}")/_pgmi_env.sh"
: "${model_checkpoint_file:=/path/to/state_dict_v2.pt}"
: "${precomputed_embedding_file:=}"
: "${VespaG_plm:=/path/to/esm2_t36_3B_UR50D.pt}"
: "${DMS_output_score_folder:=${DMS_output_score_folder_subs%/}/VespaG}"
if [ -n "${precomputed_embedding_file}" ]; then _pgmi_rows=(-e "${precomputed_embedding_file}"); else _pgmi_rows=(--plm "${VespaG_plm}"); fi
pgmi_run proteingym_amd.score_vespag_proteingym eval-proteingym -o "${DMS_output_score_folder}" --dms-directory "${DMS_data_folder_subs}" \
    --reference-file "${DMS_reference_file_path_subs}" --checkpoint-file "${model_checkpoint_file}" "${_pgmi_rows[@]}"
