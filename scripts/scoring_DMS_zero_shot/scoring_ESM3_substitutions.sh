#!/bin/bash
# MI355X drop-in for ProteinGym's scripts/scoring_DMS_zero_shot/scoring_ESM3_substitutions.sh (same zero_shot_config.sh, same CSVs).
# ESM3_model_path: the esm3-open snapshot directory (data/weights/esm3_sm_open_v1.pth and esm3_structure_encoder_v0.pth) or the model's
# .pth with the encoder's next to it.  As the reference's launcher: every assay of the substitution benchmark (DMS_index -1), with
# structure, the PDB files from ${DMS_structure_folder}, into ESM3/.  ESM3_use_structure=0 scores from the target sequences alone.
source "$(dirname "${BASH_SOURCE[0]}")/_pgmi_env.sh"
: "${ESM3_model_path:=/path/to/esm3-open}"
_structure_flags=(--use_structure --pdb_dir "${DMS_structure_folder}")
if [ "${ESM3_use_structure:-1}" = "0" ]; then _structure_flags=(); fi
pgmi_run proteingym_amd.score_esm3_proteingym --model_type "esm3_open" --model_path "${ESM3_model_path}" \
    --reference_csv "${DMS_reference_file_path_subs}" --dms_dir "${DMS_data_folder_subs}" \
    --output_dir "${DMS_output_score_folder_subs}/ESM3/" --DMS_index "${DMS_index:=-1}" "${_structure_flags[@]}"
