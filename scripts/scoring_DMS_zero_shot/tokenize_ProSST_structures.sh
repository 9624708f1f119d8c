#!/bin/bash
# MI355X launcher for the structure tokens that ProSST's and VenusREM's compute_fitness.py read (proteingym/baselines/venusrem/venusrem/
# data/get_struc_seq.py in the reference; same zero_shot_config.sh as the scoring launchers).  The paths to set: ProSST_structure_folder =
# the folder of PDB files, ProSST_model_path = the structure encoder's AE.pt, ProSST_cluster_dir = the folder of <K>.joblib (or <K>.npy)
# codebooks, ProSST_struc_seq_dir = where <K>/<name>.fasta go (ProSST: <base_dir>/structure_sequence, or one K's folder as --structure_dir;
# VenusREM: this folder itself as --struc_seq_dir, default <base_dir>/struc_seq: its compute_fitness.py appends <K>/).
# ProSST_vocab_sizes: every K to write, all from one encoder pass per structure.  Nothing is downloaded.
source "$(dirname "${BASH_SOURCE[0]}")/_pgmi_env.sh"
: "${ProSST_structure_folder:=${DMS_structure_folder:-/path/to/ProteinGym_AF2_structures}}"
: "${ProSST_model_path:=/path/to/AE.pt}"
: "${ProSST_cluster_dir:=/path/to/static}"
: "${ProSST_struc_seq_dir:=/path/to/structure_sequence}"
: "${ProSST_vocab_sizes:=2048}"
pgmi_run proteingym_amd.prosst_structure_tokens --pdb_dir "${ProSST_structure_folder}" --out_dir "${ProSST_struc_seq_dir}" \
    --vocab_size ${ProSST_vocab_sizes} --model_path "${ProSST_model_path}" --cluster_dir "${ProSST_cluster_dir}"
