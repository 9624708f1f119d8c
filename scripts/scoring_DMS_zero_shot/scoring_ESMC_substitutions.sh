#!/bin/bash
# MI355X drop-in for ProteinGym's scripts/scoring_DMS_zero_shot/scoring_ESMC_substitutions.sh (same zero_shot_config.sh, same CSVs).
# ESMC_300M_model_path / ESMC_600M_model_path: an ESMC state dict (.pth) or its snapshot directory; both models score every assay of the
# substitution benchmark (DMS_index -1, as the reference's launcher) into ESM_C/300M and ESM_C/600M.
source "$(dirname "${BASH_SOURCE[0]}")/_pgmi_env.sh"
: "${ESMC_300M_model_path:=/path/to/esmc-300}"
: "${ESMC_600M_model_path:=/path/to/esmc-600}"
for _size in 300M 600M; do
    _path_var="ESMC_${_size}_model_path"
    pgmi_run proteingym_amd.score_esmc_proteingym --model_type "esmc_${_size}" --model_path "${!_path_var}" \
        --reference_csv "${DMS_reference_file_path_subs}" --dms_dir "${DMS_data_folder_subs}" \
        --output_dir "${DMS_output_score_folder_subs}/ESM_C/${_size}" --DMS_index "${DMS_index:=-1}" || exit $?
done
