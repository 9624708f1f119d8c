#!/bin/bash
# MI355X launcher for ProteinGym's CARP rows, substitutions: the flags of proteingym/baselines/carp_mif/compute_fitness.py (same
# zero_shot_config.sh, same variables as the reference's launcher of this name: model_name = carp_600k | carp_38M | carp_76M | carp_640M,
# model_path = the folder of <model_name>.pt checkpoints; MIF and MIF-ST are refused).
source "$(dirname "${BASH_SOURCE[0]}")/_pgmi_env.sh"
pgmi_carp "${DMS_reference_file_path_subs}" "${DMS_data_folder_subs}" "${DMS_output_score_folder_subs}/CARP"
