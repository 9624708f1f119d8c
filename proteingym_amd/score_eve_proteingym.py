"""Drop-in for ``proteingym/baselines/EVE/compute_evol_indices_DMS.py`` on MI355X (EVE and, with deepseq_model_params.json,
DeepSequence).

Same flags, the same seed loop and the same file: ``<output folder>/<DMS_id>.csv`` with the columns ``mutant`` and
``evol_indices_seed_{seed}``, the ``wt`` row first, invalid mutants dropped by the rules of VAE_model.py:408-450; seeds after the
first are inner-merged on ``mutant`` into the file the first seed wrote; with --skip_existing an existing file ends the run.  The
checkpoint of a seed is ``<VAE_checkpoint_location>/<MSA name without .a2m>_seed_<seed>``.

Divergences, all deliberate: one set of decoder weights is drawn per sample and shared by all mutants (the
reference draws one per batch and sample), the noise comes from a counter-based generator keyed by the seed, and the mean is held in
fp64 -- so --aggregation_method is accepted and its three values give the same estimator, and --batch_size is accepted and only bounds
the rows of a device chunk.  --MSA_weights_location is accepted and unused, as in the reference (use_weights=False).  The reference's
own launcher passes --output_evol_indices_location, which its script does not define: both spellings name the output folder here.
Additive flag: --device.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import pandas as pd

from . import _lib, eve


def parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Evol indices (HIP, MI355X)")
    p.add_argument("--MSA_data_folder", type=str, help="Folder where MSAs are stored")
    p.add_argument("--DMS_reference_file_path", type=str, help="List of proteins and corresponding MSA file name")
    p.add_argument("--protein_index", type=int, help="Row index of protein in input mapping file")
    p.add_argument("--MSA_weights_location", type=str, help="Accepted and unused (the scoring path does not weight sequences)")
    p.add_argument("--theta_reweighting", type=float, help="Parameters for MSA sequence re-weighting (unused without weights)")
    p.add_argument("--random_seeds", type=int, nargs="+", help="Seeds of the VAE checkpoints to score with")
    p.add_argument("--VAE_checkpoint_location", type=str, help="Location where VAE model checkpoints are stored")
    p.add_argument("--model_parameters_location", type=str, help="Location of VAE model parameters")
    p.add_argument("--DMS_data_folder", type=str, help="Location of all mutations to compute the evol indices for")
    p.add_argument("--output_scores_folder", "--output_evol_indices_location", dest="output_scores_folder", type=str,
                   help="Output location of computed evol indices")
    p.add_argument("--num_samples_compute_evol_indices", type=int, help="Num of samples to approximate delta elbo when computing evol indices")
    p.add_argument("--batch_size", default=256, type=int, help="Upper bound on the rows of a device chunk")
    p.add_argument("--skip_existing", action="store_true", help="Skip scoring if output file already exists")
    p.add_argument("--aggregation_method", choices=["full", "batch", "online"], default="full",
                   help="Accepted; all three give the same estimator here")
    p.add_argument("--threshold_focus_cols_frac_gaps", type=float, help="Maximum fraction of gaps allowed in focus columns")
    p.add_argument("--device", type=int, default=0, help="HIP device")
    return p


def score_seed(checkpoint: str, params_path: str, msa: eve.EveAlignment, residues: np.ndarray, num_samples: int, seed: int, device: int,
               max_rows: int):
    """(mean, std) of the ELBO per row for one checkpoint."""
    model = eve.from_checkpoint(checkpoint, params_path, msa.seq_len, device=device)
    try:
        _lib.check(_lib.load().pgmi_set_option(b"eve_max_rows", int(max_rows)))
        return model.evol_indices(residues, num_samples, seed=seed)
    finally:
        _lib.load().pgmi_set_option(b"eve_max_rows", 0)
        model.close()


def main(argv=None):
    args = parser().parse_args(argv)
    print("Arguments:", args)
    assert os.path.isfile(args.DMS_reference_file_path), "MSA list file does not exist: {}".format(args.DMS_reference_file_path)
    mapping = pd.read_csv(args.DMS_reference_file_path)
    DMS_id = mapping["DMS_id"][args.protein_index]
    protein_name = mapping["MSA_filename"][args.protein_index].split(".a2m")[0]
    DMS_filename = mapping["DMS_filename"][args.protein_index]
    msa_location = args.MSA_data_folder + os.sep + mapping["MSA_filename"][args.protein_index]
    out_file = os.path.join(args.output_scores_folder, f"{DMS_id}.csv")
    if os.path.isfile(out_file):
        print("Output file already exists: " + str(out_file))
        if args.skip_existing:
            print("Skipping scoring since args.skip_existing is True")
            return 0
        print("Overwriting existing file: " + str(out_file))
    else:
        assert os.path.isdir(os.path.dirname(out_file)), \
            "Output directory does not exist: {}. Please create directory before running script.".format(os.path.dirname(out_file))
    kw = {}
    if args.threshold_focus_cols_frac_gaps is not None:
        kw["threshold_focus_cols_frac_gaps"] = args.threshold_focus_cols_frac_gaps
    msa = eve.EveAlignment(msa_location, **kw)
    mutants = pd.read_csv(args.DMS_data_folder + os.sep + DMS_filename, header=0)["mutant"]
    names, seqs = eve.valid_mutants(msa, mutants)
    residues = eve.encode_residues(seqs)
    for seed in args.random_seeds:
        model_name = protein_name + f"_seed_{seed}"
        print("Model name: " + str(model_name))
        checkpoint = str(args.VAE_checkpoint_location) + os.sep + model_name
        assert os.path.isfile(checkpoint), "Checkpoint file does not exist: {}".format(checkpoint)
        mean, _std = score_seed(checkpoint, args.model_parameters_location, msa, residues, args.num_samples_compute_evol_indices, seed,
                                args.device, args.batch_size)
        df = pd.DataFrame({"mutant": names, f"evol_indices_seed_{seed}": -(mean - mean[0])})
        if os.path.exists(out_file) and seed != args.random_seeds[0]:
            prev = pd.read_csv(out_file)
            df = pd.merge(prev, df, on="mutant", how="inner")
            assert len(df) == len(prev), "Length of merged dataframe doesn't match previous length, mutants must not match across seeds"
        df.to_csv(out_file, index=False)
    return 0


if __name__ == "__main__":
    sys.exit(main())
