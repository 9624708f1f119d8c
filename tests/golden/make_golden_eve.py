"""Writes the EVE / DeepSequence fixtures and records TOY_EVE_REFERENCE.csv from the UNMODIFIED reference
(proteingym/baselines/EVE/compute_evol_indices_DMS.py, run as a script on the CPU through tests/eve_reference.py's shims):

    EVE_toy/TOY_MSA_seed_0, EVE_toy/model_params.json                      default-style: decoder [32, 72], z 8, conv 40, temperature
    DeepSequence_toy/TOY_MSA_seed_0, DeepSequence_toy/model_params.json    DeepSequence-style: decoder [24, 72], sparsity with 4 tiles
    TOY_EVE_DMS.csv, TOY_EVE_MAPPING.csv                                   the toy assay on TOY_MSA.a2m (50 focus columns, 20 L = 1000)
    TOY_EVE_REFERENCE.csv                                                  mutant, evol_indices_seed_0 (the reference's own output
                                                                           column), elbo_mean, elbo_std, mutated_sequence

    python tests/golden/make_golden_eve.py [num_samples]

The checkpoints are ``torch.save({'model_state_dict': ...})`` files as the reference writes them, with the tensors stored as fp16
(the values are exactly representable; the reference's load_state_dict and our loader both widen them to fp32).  Weights:
proteingym_amd.eve.random_state_dict -- log-variances in [-6, -2], a strong per-position letter profile in the output bias so that
the evolutionary indices are well above their Monte-Carlo error.  The reference's script writes the evol index only; the ELBO mean
and standard deviation per mutant are taken from the values its own all_likelihood_components returns during that run (the method
is wrapped to keep them), and the mutated sequences from the dict it hands to one_hot_3D.  The script checks the condition the
end-to-end test relies on: at least 90 % of the mutants have |evol| above 6 sqrt((s_m^2 + s_wt^2) (2 / N)).
"""
import json
import os
import runpy
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from proteingym_amd import eve  # noqa: E402
import eve_reference as er  # noqa: E402

AA = "ACDEFGHIKLMNPQRSTVWY"
TRAINING = {"num_training_steps": 1, "learning_rate": 1e-4, "batch_size": 256, "annealing_warm_up": 0, "kl_latent_scale": 1.0,
            "kl_global_params_scale": 1.0, "l2_regularization": 0.0, "use_lr_scheduler": False, "use_validation_set": False,
            "validation_set_pct": 0.2, "validation_freq": 1000, "log_training_info": False, "log_training_freq": 1000,
            "save_model_params_freq": 500000}


def params(dec_sizes, sparsity):
    return {"encoder_parameters": {"hidden_layers_sizes": [64, 48], "z_dim": 8, "convolve_input": False, "convolution_input_depth": 40,
                                   "nonlinear_activation": "relu", "dropout_proba": 0.0},
            "decoder_parameters": {"hidden_layers_sizes": dec_sizes, "z_dim": 8, "bayesian_decoder": True,
                                   "first_hidden_nonlinearity": "relu", "last_hidden_nonlinearity": "relu", "dropout_proba": 0.1,
                                   "convolve_output": True, "convolution_output_depth": 40, "include_temperature_scaler": True,
                                   "include_sparsity": bool(sparsity), "num_tiles_sparsity": sparsity,
                                   "logit_sparsity_p": 0.001 if sparsity else 0},
            "training_parameters": TRAINING}


TOYS = {"EVE_toy": (params([32, 72], 0), 101), "DeepSequence_toy": (params([24, 72], 4), 102)}


def write_toys(L, wt):
    import torch
    for name, (p, seed) in TOYS.items():
        os.makedirs(os.path.join(HERE, name), exist_ok=True)
        with open(os.path.join(HERE, name, "model_params.json"), "w") as f:
            json.dump(p, f, indent=1)
        d = eve.dims_from_params(p, L)
        sd = eve.random_state_dict(d, seed, scale=0.5, out_bias_std=1.5)
        # what training does to the output bias: the wild type's letters are the likely ones
        b = sd["decoder.last_hidden_layer_bias_mean"].reshape(L, 20)
        b[np.arange(L), [AA.index(a) for a in wt]] += 5.0
        half = {k: torch.from_numpy(v.astype(np.float16)) for k, v in sd.items()}
        torch.save({"model_state_dict": half}, os.path.join(HERE, name, "TOY_MSA_seed_0"))


def write_assay(msa):
    rng = np.random.default_rng(7)
    wt, start = msa.focus_seq_trimmed, msa.focus_start_loc
    rows = []
    for i in rng.permutation(len(wt))[:34]:
        rows.append(f"{wt[i]}{start + i}{rng.choice([a for a in AA if a != wt[i]])}")
    rows.insert(5, f"{wt[3]}{start + 3}W:{wt[40]}{start + 40}A")                  # a double mutant
    rows.insert(9, f"{wt[7]}{start + 7}{wt[7]}")                                  # same letter: kept, equal to the wild type
    rows.insert(12, f"{wt[2]}{start + 2}{wt[2]}:{wt[20]}{start + 20}C")           # same-letter part skipped, the other applied
    rows.insert(15, f"{'A' if wt[10] != 'A' else 'C'}{start + 10}G")              # wrong wild-type letter: dropped
    rows.insert(20, f"H{start - 4}A")                                             # position before the focus range: dropped
    rows.insert(25, f"{wt[30]}{start + 30}X")                                     # target outside the alphabet: dropped
    rows.insert(30, f"{wt[12]}{start + 12}D:{wt[13]}{start + len(wt) + 3}{wt[13]}")   # same letter at a position past the focus range: skipped before the position is looked at, so the row is kept
    rows.insert(33, f"{wt[14]}{start + 14}D:{wt[15]}{start + len(wt) + 3}{'A' if wt[15] != 'A' else 'C'}")   # double with one bad position: dropped whole
    with open(os.path.join(HERE, "TOY_EVE_DMS.csv"), "w") as f:
        f.write("mutant,DMS_score\n")
        for r in rows:
            f.write(f"{r},{rng.standard_normal():.4f}\n")
    with open(os.path.join(HERE, "TOY_EVE_MAPPING.csv"), "w") as f:
        f.write("DMS_id,DMS_filename,MSA_filename,MSA_theta\nTOY_EVE,TOY_EVE_DMS.csv,TOY_MSA.a2m,0.2\n")


def record(num_samples):
    """Runs the reference script on EVE_toy and returns its CSV plus the kept ELBO samples."""
    vm, _ = er.load_reference()
    kept, seqs = [], {}
    orig_alc, orig_oh = vm.VAE_model.all_likelihood_components, vm.one_hot_3D

    def alc(self, x):
        out = orig_alc(self, x)
        kept.append(out[0].detach().numpy().astype(np.float64).copy())
        return out

    def oh(seq_keys, seq_name_to_sequence, **k):
        if "wt" in seq_name_to_sequence:
            seqs.update(seq_name_to_sequence)
        return orig_oh(seq_keys, seq_name_to_sequence, **k)

    out_dir = tempfile.mkdtemp()
    argv = ["compute_evol_indices_DMS.py", "--MSA_data_folder", HERE, "--DMS_reference_file_path", os.path.join(HERE, "TOY_EVE_MAPPING.csv"),
            "--protein_index", "0", "--VAE_checkpoint_location", os.path.join(HERE, "EVE_toy"),
            "--model_parameters_location", os.path.join(HERE, "EVE_toy", "model_params.json"), "--DMS_data_folder", HERE,
            "--output_scores_folder", out_dir, "--num_samples_compute_evol_indices", str(num_samples), "--batch_size", "1024",
            "--aggregation_method", "full", "--threshold_focus_cols_frac_gaps", "1", "--random_seeds", "0"]
    vm.VAE_model.all_likelihood_components, vm.one_hot_3D = alc, oh
    old_argv = sys.argv
    try:
        with er.eve_imports():
            sys.argv = argv
            runpy.run_path(os.path.join(er.EVE_DIR, "compute_evol_indices_DMS.py"), run_name="__main__")
    finally:
        sys.argv = old_argv
        vm.VAE_model.all_likelihood_components, vm.one_hot_3D = orig_alc, orig_oh
    import pandas as pd
    df = pd.read_csv(os.path.join(out_dir, "TOY_EVE.csv"))
    samples = np.stack(kept, axis=1)                     # [rows, num_samples]: one batch holds the whole toy assay
    assert samples.shape == (len(df), num_samples), samples.shape
    return df, samples, seqs


def main():
    num_samples = int(sys.argv[1]) if len(sys.argv) > 1 else 4000
    msa = eve.EveAlignment(os.path.join(HERE, "TOY_MSA.a2m"), 1.0)
    write_toys(msa.seq_len, msa.focus_seq_trimmed)
    write_assay(msa)
    df, samples, seqs = record(num_samples)
    mean, std = samples.mean(1), samples.std(1, ddof=1)
    evol = df["evol_indices_seed_0"].to_numpy()
    assert np.abs(-(mean - mean[0]) - evol).max() < 1e-2, "kept samples do not reproduce the script's own evol indices"
    df["elbo_mean"], df["elbo_std"] = mean, std
    df["mutated_sequence"] = [seqs[m] for m in df["mutant"]]
    df.to_csv(os.path.join(HERE, "TOY_EVE_REFERENCE.csv"), index=False, float_format="%.6f")
    bound = 6.0 * np.sqrt((std ** 2 + std[0] ** 2) * (2.0 / num_samples))
    moved = list(range(1, len(df)))                       # every mutant, the same-letter row (equal to the wild type) included
    frac = float(np.mean(np.abs(evol[moved]) > bound[moved]))
    print(f"rows {len(df)}; ELBO std {std.min():.2f} .. {std.max():.2f}; bound {bound.min():.3f} .. {bound.max():.3f}; "
          f"|evol| median {np.median(np.abs(evol[moved])):.2f}; above their bound: {frac:.2%}")
    assert frac >= 0.9, "the toy weights do not separate the mutants from the Monte-Carlo error: change the weights, not the bound"


if __name__ == "__main__":
    main()
