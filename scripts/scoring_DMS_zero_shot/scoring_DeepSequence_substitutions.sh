#!/bin/bash
# DeepSequence on the MI355X: scoring_EVE_substitutions.sh with DeepSequence's parameter file (ProteinGym's
# proteingym/baselines/EVE/EVE/deepseq_model_params.json: sparsity with 4 tiles, decoder 100-2000) and the folder of the checkpoints
# trained with it (DeepSequence_checkpoint_folder; zero_shot_config.sh has no variable for them).
export model_parameters_location="${model_parameters_location:-/path/to/ProteinGym/proteingym/baselines/EVE/EVE/deepseq_model_params.json}"
export EVE_checkpoint_folder="${DeepSequence_checkpoint_folder:-/path/to/DMS_DeepSequence_models}"
export EVE_score_name=DeepSequence
source "$(dirname "${BASH_SOURCE[0]}")/scoring_EVE_substitutions.sh"
