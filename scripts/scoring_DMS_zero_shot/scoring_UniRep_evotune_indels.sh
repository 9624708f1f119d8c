#!/bin/bash
# MI355X launcher for ProteinGym's Unirep_evotune row, indels: the flags of proteingym/baselines/unirep/unirep_inference.py (same
# zero_shot_config.sh, same variables as the reference's launcher of this name; model_path = the folder of per-MSA evotuned weight directories).
source "$(dirname "${BASH_SOURCE[0]}")/_pgmi_env.sh"
pgmi_unirep "${DMS_reference_file_path_indels}" "${DMS_data_folder_indels}" "${DMS_output_score_folder_indels}/UniRep_evotuned" --evotune
