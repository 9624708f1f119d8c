"""EVE / DeepSequence host logic -- no GPU needed.

tests/eve_ref.py (the float64 restatement every GPU test compares against) is pinned to the unmodified reference where the
reference tree is present: the reference's all_likelihood_components runs with torch.randn_like and the decoder's dropout layer
wrapped to record their draws, and eve_ref fed the same draws must give its ELBO, BCE and KLD.

tests/golden/TOY_EVE_REFERENCE.csv was recorded by tests/golden/make_golden_eve.py: the reference's own compute_evol_indices_DMS.py
run as a script on the CPU (stub numba / numba_progress / Bio modules, as oracle/ref_harness.py does for ESM) on
EVE_toy/TOY_MSA_seed_0, TOY_MSA.a2m and TOY_EVE_DMS.csv with 4 000 samples, batch size 1 024, aggregation "full" and
threshold_focus_cols_frac_gaps 1; evol_indices_seed_0 is the script's output column, elbo_mean / elbo_std are the mean and the
standard deviation (n - 1) of the values its all_likelihood_components returned during that run, mutated_sequence is what it handed
to one_hot_3D.
"""
import ctypes as C
import json
import os
import shutil

import numpy as np
import pandas as pd
import pytest

import eve_ref
import eve_reference as er
from proteingym_amd import _lib, eve, score_eve_proteingym as cli

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOY = os.path.join(GOLDEN, "EVE_toy")
DEEPSEQ = os.path.join(GOLDEN, "DeepSequence_toy")


def toy_params(conv, sparsity, temperature, dec=(32, 72)):
    return {"encoder_parameters": {"hidden_layers_sizes": [64, 48], "z_dim": 8, "convolve_input": False, "convolution_input_depth": 40,
                                   "nonlinear_activation": "relu", "dropout_proba": 0.0},
            "decoder_parameters": {"hidden_layers_sizes": list(dec), "z_dim": 8, "bayesian_decoder": True,
                                   "first_hidden_nonlinearity": "relu", "last_hidden_nonlinearity": "relu", "dropout_proba": 0.1,
                                   "convolve_output": bool(conv), "convolution_output_depth": 40,
                                   "include_temperature_scaler": bool(temperature), "include_sparsity": bool(sparsity),
                                   "num_tiles_sparsity": 4 if sparsity else 0, "logit_sparsity_p": 0.001 if sparsity else 0}}


# conv, sparsity, temperature: each one on and off
VARIANTS = {"conv_temp": (1, 0, 1), "sparsity_only": (0, 1, 0), "all_on": (1, 1, 1)}


@pytest.mark.skipif(not er.reference_available(), reason="reference tree not present")
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_restatement_matches_the_reference_on_its_own_draws(variant):
    """1e-3 absolute on |ELBO| of a few hundred: 40x the fp32-vs-fp64 gap of the reference's own arithmetic (2.5e-5), and far below any
    indexing mistake, which moves the ELBO by units."""
    import torch
    L, M = 37, 9
    params = toy_params(*VARIANTS[variant])
    d = eve.dims_from_params(params, L)
    state = eve.random_state_dict(d, seed=5, scale=2.0, out_bias_std=1.0)
    model = er.build_model(params, state, L)
    assert list(model.state_dict().keys()) == [k for k, _ in eve.key_shapes(d)]          # the blob's documented order
    assert [tuple(v.shape) for v in model.state_dict().values()] == [s for _, s in eve.key_shapes(d)]
    rng = np.random.default_rng(3)
    residues = rng.integers(0, 20, size=(M, L)).astype(np.uint8)
    residues[2, 5] = residues[4, 0] = eve.NO_LETTER
    x = torch.from_numpy(eve_ref.one_hot(residues)).to(torch.float32)
    names = eve_ref.consumed(d)
    torch.manual_seed(11)
    with torch.no_grad(), er.NoiseRecorder(model, names) as rec:
        ref = [t.numpy().astype(np.float64) for t in model.all_likelihood_components(x)]
    assert list(rec.noise) == names                                                      # every draw named, in order
    got = eve_ref.elbo(state, d, residues, rec.noise)
    for name, g, r in zip(("elbo", "bce", "kld"), got, ref):
        err = np.abs(g - r).max()
        print(f"{variant} {name}: max|err| = {err:.3e} on |value| <= {np.abs(r).max():.1f}")
        assert err <= 1e-3, (name, err)
    # the restatement reads every tensor it is given: a changed draw changes the result
    for k in names:
        n2 = dict(rec.noise)
        n2[k] = 1 - n2[k] if k.startswith("keep") else n2[k] + 0.5
        assert np.abs(eve_ref.elbo(state, d, residues, n2)[0] - got[0]).max() > 1e-6, k


def toy_assay():
    msa = eve.EveAlignment(os.path.join(GOLDEN, "TOY_MSA.a2m"), 1.0)
    dms = pd.read_csv(os.path.join(GOLDEN, "TOY_EVE_DMS.csv"))
    ref = pd.read_csv(os.path.join(GOLDEN, "TOY_EVE_REFERENCE.csv"))
    return msa, dms, ref


def test_mutant_validity_matches_the_recorded_run():
    msa, dms, ref = toy_assay()
    names, seqs = eve.valid_mutants(msa, dms["mutant"])
    assert names == ref["mutant"].tolist()
    assert seqs == ref["mutated_sequence"].tolist()
    dropped = [m for m in dms["mutant"] if m not in set(names)]
    # wrong wild-type letter, position before the focus range, target X, a double with one bad position
    assert len(dropped) == 4 and any(":" in m for m in dropped) and any(m.endswith("X") for m in dropped)
    assert any(":" in m for m in names[1:])
    res = eve.encode_residues(seqs)
    assert res.shape == (len(names), msa.seq_len) and res.dtype == np.uint8 and res.max() < 20
    assert eve.encode_residues(["AXC-"]).tolist() == [[0, 255, 1, 255]]
    # the default threshold (0.3) and the launcher's (1) agree on this alignment; a mutant string that does not parse is dropped
    assert eve.EveAlignment(os.path.join(GOLDEN, "TOY_MSA.a2m")).focus_seq_trimmed == msa.focus_seq_trimmed
    assert eve.valid_mutants(msa, ["H11", "nonsense", "H011A", "H11A"])[0] == ["wt", "H11A"]


@pytest.mark.parametrize("folder", [TOY, DEEPSEQ])
def test_loader_blob_order_and_count(lib, folder):
    import torch
    params = json.load(open(os.path.join(folder, "model_params.json")))
    d, blob = eve.load_checkpoint(os.path.join(folder, "TOY_MSA_seed_0"), params, 50)
    state = torch.load(os.path.join(folder, "TOY_MSA_seed_0"), map_location="cpu")["model_state_dict"]
    assert list(state) == [k for k, _ in eve.key_shapes(d)]
    assert blob.dtype == np.float32
    off = 0
    for k, shape in eve.key_shapes(d):
        n = int(np.prod(shape))
        assert np.array_equal(blob[off:off + n], state[k].numpy().astype(np.float32).reshape(-1)), k
        off += n
    assert off == blob.size
    c = eve.EveConfig(abi_version=_lib.ABI_VERSION, seq_len=50, alphabet=20, z_dim=8, n_enc=2, n_dec=2, conv_depth=d["conv_depth"],
                      temperature=d["temperature"], sparsity_tiles=d["sparsity_tiles"], dropout_p=0.1)
    c.enc_sizes[0], c.enc_sizes[1] = d["enc_sizes"]
    c.dec_sizes[0], c.dec_sizes[1] = d["dec_sizes"]
    assert lib.pgmi_eve_weight_count(C.byref(c)) == blob.size
    c.conv_depth = 30                                                 # not a multiple of 4: refused, with a message
    assert lib.pgmi_eve_weight_count(C.byref(c)) == -1 and b"conv_depth" in lib.pgmi_last_error()
    np_state = {k: v.numpy() for k, v in state.items()}
    with pytest.raises(ValueError, match="lacks"):
        eve.blob_from_state_dict({k: v for k, v in np_state.items() if k != "encoder.fc_mean.bias"}, d)
    with pytest.raises(ValueError, match="does not"):
        eve.blob_from_state_dict(dict(np_state, extra=np.zeros(1)), d)
    with pytest.raises(ValueError, match="shape"):
        eve.blob_from_state_dict(dict(np_state, **{"encoder.fc_mean.bias": np.zeros(9)}), d)


def test_no_cpu_fallback(lib):
    """Without a GPU the model cannot be created: there is no eager fall-back."""
    if lib.pgmi_device_count() > 0:
        pytest.skip("GPU present")
    params = json.load(open(os.path.join(TOY, "model_params.json")))
    d, blob = eve.load_checkpoint(os.path.join(TOY, "TOY_MSA_seed_0"), params, 50)
    with pytest.raises(_lib.PgmiError, match="no HIP device|no CPU fallback"):
        eve.EveModel(d, blob)


def test_cli_flag_surface():
    ref_flags = ["--MSA_data_folder", "--DMS_reference_file_path", "--protein_index", "--MSA_weights_location", "--theta_reweighting",
                 "--random_seeds", "--VAE_checkpoint_location", "--model_parameters_location", "--DMS_data_folder",
                 "--output_scores_folder", "--num_samples_compute_evol_indices", "--batch_size", "--skip_existing",
                 "--aggregation_method", "--threshold_focus_cols_frac_gaps"]
    known = {s for a in cli.parser()._actions for s in a.option_strings}
    assert set(ref_flags) <= known and "--output_evol_indices_location" in known
    p = cli.parser()
    assert p.parse_args(["--output_scores_folder", "a"]).output_scores_folder == "a"
    assert p.parse_args(["--output_evol_indices_location", "b"]).output_scores_folder == "b"
    a = p.parse_args(["--random_seeds", "0", "1", "2", "--aggregation_method", "online", "--skip_existing", "--batch_size", "1024"])
    assert a.random_seeds == [0, 1, 2] and a.aggregation_method == "online" and a.skip_existing and a.batch_size == 1024
    with pytest.raises(SystemExit):
        p.parse_args(["--aggregation_method", "other"])


class FakeModel:
    """EveModel with the library call replaced by the float64 restatement (a few numpy-seeded samples)."""
    calls = []

    def __init__(self, dims, blob, device=0):
        self.dims, self.state = dict(dims), eve.state_from_blob(dims, blob)

    def evol_indices(self, residues, num_samples, seed=0):
        FakeModel.calls.append((num_samples, seed, len(residues)))
        rng = np.random.default_rng(seed)
        s = np.stack([eve_ref.elbo(self.state, self.dims, residues, eve_ref.numpy_noise(self.dims, len(residues), rng))[0]
                      for _ in range(num_samples)], 1)
        return s.mean(1), s.std(1, ddof=1)

    def close(self):
        pass


def test_cli_seed_merge_and_skip_existing(lib, tmp_path, monkeypatch):
    monkeypatch.setattr(eve, "EveModel", FakeModel)
    FakeModel.calls = []
    ck = tmp_path / "ck"
    ck.mkdir()
    for seed in (0, 3):
        shutil.copy(os.path.join(TOY, "TOY_MSA_seed_0"), ck / f"TOY_MSA_seed_{seed}")
    out = tmp_path / "out"
    out.mkdir()
    argv = ["--MSA_data_folder", GOLDEN, "--DMS_reference_file_path", os.path.join(GOLDEN, "TOY_EVE_MAPPING.csv"), "--protein_index", "0",
            "--VAE_checkpoint_location", str(ck), "--model_parameters_location", os.path.join(TOY, "model_params.json"),
            "--DMS_data_folder", GOLDEN, "--num_samples_compute_evol_indices", "3", "--batch_size", "1024", "--aggregation_method", "full",
            "--threshold_focus_cols_frac_gaps", "1", "--MSA_weights_location", "unused", "--random_seeds", "0", "3"]
    assert cli.main(argv + ["--output_evol_indices_location", str(out)]) == 0
    ref = pd.read_csv(os.path.join(GOLDEN, "TOY_EVE_REFERENCE.csv"))
    df = pd.read_csv(out / "TOY_EVE.csv")
    assert list(df.columns) == ["mutant", "evol_indices_seed_0", "evol_indices_seed_3"]
    assert df["mutant"].tolist() == ref["mutant"].tolist() and df["mutant"][0] == "wt"
    assert df["evol_indices_seed_0"][0] == 0 and df["evol_indices_seed_3"][0] == 0
    assert not np.allclose(df["evol_indices_seed_0"], df["evol_indices_seed_3"])          # the seed keys the noise
    assert FakeModel.calls == [(3, 0, len(ref)), (3, 3, len(ref))]
    # the favoured letters of the toy's output bias are the wild type's: most mutants score worse than it
    assert (df["evol_indices_seed_0"][1:] > 0).mean() > 0.8
    # --skip_existing: the file stays as it is and nothing is scored; without it the first seed overwrites
    before = (out / "TOY_EVE.csv").read_bytes()
    assert cli.main(argv + ["--output_scores_folder", str(out), "--skip_existing"]) == 0
    assert (out / "TOY_EVE.csv").read_bytes() == before and len(FakeModel.calls) == 2
    assert cli.main(argv[:-3] + ["--random_seeds", "3", "--output_scores_folder", str(out)]) == 0
    assert list(pd.read_csv(out / "TOY_EVE.csv").columns) == ["mutant", "evol_indices_seed_3"]
    with pytest.raises(AssertionError, match="Checkpoint file does not exist"):
        cli.main(argv[:-3] + ["--random_seeds", "9", "--output_scores_folder", str(out)])


@pytest.mark.parametrize("script,params,folder", [("scoring_EVE_substitutions.sh", "default_model_params.json", "/data/pg/DMS_EVE_models/"),
                                                  ("scoring_DeepSequence_substitutions.sh", "deepseq_model_params.json", "/models/deepseq")])
def test_launchers_build_a_command_line_the_cli_parses(script, params, folder, tmp_path):
    """The launchers source a zero_shot_config.sh written in the reference's variable names and pass the reference launcher's settings."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = tmp_path / "scripts"
    (cfg / "scoring_DMS_zero_shot").mkdir(parents=True)
    (cfg / "zero_shot_config.sh").write_text(
        'export PROTEINGYM_CACHE="/data/pg"\n'
        'export DMS_data_folder_subs="${PROTEINGYM_CACHE}/DMS_ProteinGym_substitutions/"\n'
        'export DMS_MSA_data_folder="${PROTEINGYM_CACHE}/DMS_msa_files/"\n'
        'export DMS_MSA_weights_folder="${PROTEINGYM_CACHE}/DMS_msa_weights/"\n'
        'export DMS_EVE_model_folder="${PROTEINGYM_CACHE}/DMS_EVE_models/"\n'
        'export DMS_reference_file_path_subs=../../reference_files/DMS_substitutions.csv\n'
        'export DMS_output_score_folder_subs="${PROTEINGYM_CACHE}/zero_shot_substitutions_scores/"\n')
    env = dict(os.environ, ZERO_SHOT_CONFIG=str(cfg / "zero_shot_config.sh"), PGMI_LAUNCH_ECHO="1", DMS_index="7",
               DeepSequence_checkpoint_folder="/models/deepseq")
    out = subprocess.run(["bash", os.path.join(root, "scripts", "scoring_DMS_zero_shot", script)], env=env, capture_output=True, text=True,
                         cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr
    module, *argv = out.stdout.strip().split("\n")
    assert module == "proteingym_amd.score_eve_proteingym"
    a = cli.parser().parse_args(argv)
    assert a.protein_index == 7 and a.random_seeds == [0, 1, 2, 3, 4] and a.num_samples_compute_evol_indices == 20000
    assert a.batch_size == 1024 and a.threshold_focus_cols_frac_gaps == 1.0 and a.skip_existing and a.aggregation_method == "full"
    assert a.model_parameters_location.endswith(params) and a.VAE_checkpoint_location == folder
    assert a.output_scores_folder.rstrip("/").endswith("DeepSequence" if "Deep" in script else "EVE")
    assert a.MSA_data_folder == "/data/pg/DMS_msa_files/" and a.DMS_data_folder == "/data/pg/DMS_ProteinGym_substitutions/"
