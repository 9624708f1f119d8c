"""TranceptEVE host logic and the float64 restatement, pinned to the unmodified reference on the CPU
(proteingym/baselines/trancepteve through tests/trancepteve_reference.py; skipped where the reference tree is absent).

1. tests/trancepteve_ref.py's log-prior == get_EVE_log_prior_single on the reference's own recorded randn_like draws, both toy
   parameter files.  Bound 2e-5 per log-probability: tests/test_eve_host.py holds the ELBO, a sum over L = 50 positions, to 1e-3.
2. MSA prior and depth; EVE depth, focus columns and the -inf layout, at focus-column thresholds 1.0 and 0.5.
3. The aggregation weights, by running the reference's own statement block (model_pytorch.py:722-763) at depths on both sides of
   every boundary, with manual weights and for indels.
4. iterative_recalibrations, and both recalibrations end to end at n_ctx = 42, where the 70-residue wild type needs two windows; the
   token log-probabilities come from the reference transformer on the CPU on both sides, so the host logic alone is compared.
5. The CLI's flag surface against the reference's own add_argument calls.  The CLI's columns, file name and log line are checked on
   the GPU (tests/test_gpu_trancepteve.py::test_cli_writes_the_reference_columns_and_log): the CLI loads the Tranception checkpoint onto
   the device before anything else, and libpgmi has no CPU path.
"""
import inspect
import json
import os
import textwrap
import types

import numpy as np
import pytest
import torch

import trancepteve_ref as tref
import trancepteve_reference as tr
from proteingym_amd import eve, tranception as ptr, trancepteve as tte

pytestmark = pytest.mark.skipif(not tr.reference_available(), reason="reference tree not present")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOYS = {"eve": os.path.join(GOLDEN, "EVE_toy"), "deepseq": os.path.join(GOLDEN, "DeepSequence_toy")}
MSA_FILE, WEIGHTS = os.path.join(GOLDEN, "TOY_MSA_TTE.a2m"), os.path.join(GOLDEN, "TOY_MSA_TTE_weights.npy")
AA = "ACDEFGHIKLMNPQRSTVWY"


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "golden_trancepteve.npz"))


@pytest.mark.parametrize("style", sorted(TOYS))
def test_restatement_matches_the_reference_on_its_own_draws(style):
    params = json.load(open(os.path.join(TOYS[style], "model_params.json")))
    d, blob = eve.load_checkpoint(os.path.join(TOYS[style], "TOY_MSA_seed_0"), params, 50)
    state = eve.state_from_blob(d, blob)
    vae = tr.build_vae(params, state, 50)
    seq = "".join(np.random.default_rng(0).choice(list(AA), size=49)) + "X"        # a letter outside the alphabet: an all-zero row
    with tr.DrawRecorder() as rec:
        table = tr.log_prior_single(vae, seq, 3)
    noises = rec.per_sample(tref.noise_names(d))
    assert len(noises) == 3
    mean, _, per_sample = tref.log_prior(state, d, eve.encode_residues([seq])[0], noises)
    err = float(np.abs(table[:, 5:] - mean).max())
    print(f"{style}: max|restatement - reference| {err:.2e}")
    assert err <= 2e-5 and np.isneginf(table[:, :5]).all()
    assert np.abs(per_sample[0] - per_sample[1]).max() > 1e-3                     # the draws matter


def test_msa_prior_depths_and_layout(gold):
    pkg, tok = tr.load_reference()
    ms, me = [int(v) for v in gold["msa_start_end"]]
    want, depth = pkg.utils.msa_utils.get_msa_prior(MSA_data_file=MSA_FILE, MSA_weight_file_name=WEIGHTS, MSA_start=ms, MSA_end=me,
                                                    len_target_seq=70, vocab=tok.get_vocab(), threshold_sequence_frac_gaps=0.5,
                                                    threshold_focus_cols_frac_gaps=0.5)
    got, got_depth = ptr.get_msa_prior(MSA_FILE, WEIGHTS, ms, me, 70, threshold_sequence_frac_gaps=0.5, return_depth=True)
    assert got_depth == depth == int(gold["msa_depth"]) and np.array_equal(got, want)
    assert np.array_equal(ptr.get_msa_prior(MSA_FILE, WEIGHTS, ms, me, 70), got)          # the extension is additive
    for thr, n_cols in ((1.0, 60), (0.5, 56)):
        ref = pkg.utils.msa_utils.MSA_processing(MSA_location=MSA_FILE, use_weights=True, threshold_sequence_frac_gaps=0.5,
                                                 threshold_focus_cols_frac_gaps=thr, weights_location=WEIGHTS)
        ours = tte.EveMSA(MSA_FILE, 0.5, thr)
        assert ours.focus_cols == list(ref.focus_cols) and len(ours.focus_cols) == n_cols
        assert ours.depth == len(ref.seq_name_to_sequence.keys())
        assert ours.focus_seq_trimmed == "".join(ref.focus_seq_trimmed)
    # the table: -inf everywhere except [MSA_start + focus columns, 5:], as get_EVE_log_prior_single lays it out
    params = json.load(open(os.path.join(GOLDEN, "TranceptEVE_toy", "model_params.json")))
    d, blob = eve.load_checkpoint(os.path.join(GOLDEN, "TranceptEVE_toy", "TOY_MSA_TTE_seed_0"), params, 56)
    vae = tr.build_vae(params, eve.state_from_blob(d, blob), 56)
    torch.manual_seed(1)
    table = tr.log_prior_single(vae, ours.focus_seq_trimmed, 2, full_len=70, MSA_start=ms, focus_cols=ours.focus_cols)
    mine = tte.log_prior_table(table[[ms + c for c in ours.focus_cols], 5:], ours.focus_cols, ms, 70)
    assert mine.dtype == table.dtype == np.float32 and np.array_equal(mine, table)
    assert np.isneginf(mine).sum() == 70 * 25 - 56 * 20


def _reference_weights(**fields):
    """Runs the reference's own statements (the block of TrancepteveLMHeadModel.__init__ that sets the two weights) on a namespace."""
    pkg, _ = tr.load_reference()
    src = inspect.getsource(pkg.model_pytorch.TrancepteveLMHeadModel.__init__).split("\n")
    a = next(i for i, l in enumerate(src) if l.strip() == "if self.retrieval_weights_manual:")
    b = next(i for i, l in enumerate(src) if "Aggregation weights of retrieved MSA & EVE model" in l)
    me = types.SimpleNamespace(**fields)
    config = types.SimpleNamespace(retrieval_inference_MSA_weight=fields.get("manual_msa", 0.5), retrieval_inference_EVE_weight=fields.get("manual_eve", 0.5))
    exec(textwrap.dedent("\n".join(src[a:b])), {"self": me, "config": config})
    return me.retrieval_inference_MSA_weight, me.retrieval_inference_EVE_weight


def test_aggregation_weights():
    depths = [0, 9, 10, 99, 100, 999, 1000, 9999, 10000, 99999, 100000, 250000]
    for mode in ("aggregate_substitution", "aggregate_indel"):
        for dm in depths:
            for de in depths if mode == "aggregate_substitution" else (0, 50):
                want = _reference_weights(retrieval_weights_manual=False, inference_time_retrieval_type="TranceptEVE",
                                          retrieval_aggregation_mode=mode, MSA_processed_depth=dm, EVE_processed_depth=de)
                assert tte.aggregation_weights("TranceptEVE", mode, dm, de) == want, (mode, dm, de)
    assert tte.aggregation_weights("TranceptEVE", "aggregate_indel", 10, 0) == (0.5, 0.1)
    assert tte.aggregation_weights("TranceptEVE", "aggregate_indel", 9, 0) == (0.0, 0.0)
    want = _reference_weights(retrieval_weights_manual=False, inference_time_retrieval_type="Tranception", retrieval_aggregation_mode="aggregate_substitution")
    assert tte.aggregation_weights("Tranception", "aggregate_substitution", 5, 5) == want == (0.6, 0.0)
    want = _reference_weights(retrieval_weights_manual=True, manual_msa=0.25, manual_eve=0.75)
    assert tte.aggregation_weights("TranceptEVE", "aggregate_substitution", 5, 5, True, 0.25, 0.75) == want == (0.25, 0.75)


def test_iterative_recalibrations():
    pkg, _ = tr.load_reference()
    ref = pkg.model_pytorch.TrancepteveLMHeadModel.iterative_recalibrations
    rng = np.random.default_rng(3)
    x = torch.log(torch.tensor(rng.dirichlet(np.ones(20) * 0.3, size=30)).float() + 1e-6)
    for target in (-3.2, -4.5, float(x.mean())):
        assert torch.equal(tte.iterative_recalibrations(x.clone(), target), ref(None, x.clone(), target))
    # the stop rule: a target no temperature reaches ends after 1000 steps, on both sides alike
    assert torch.equal(tte.iterative_recalibrations(x.clone(), -2.0), ref(None, x.clone(), -2.0))


class _CpuTransformer:
    """Stands where the device model stands in the recalibrations: token log-probabilities from the reference transformer (CPU)."""

    def __init__(self, ref_model, n_ctx):
        self.ref, self.n_ctx, self.retrieval = ref_model, n_ctx, None
        self.encode_batch = ptr.TranceptionModel.encode_batch.__get__(self)

    def token_logprobs(self, ids):
        ids = torch.from_numpy(np.asarray(ids)).long()
        with torch.no_grad():
            hidden = self.ref.transformer(input_ids=ids, attention_mask=(ids != ptr.PAD).long()).last_hidden_state
            return torch.log_softmax(self.ref.lm_head(hidden), -1).numpy()


@pytest.mark.parametrize("which", ["EVE", "MSA", "MSA_indel"])
def test_recalibrations_end_to_end_two_windows(gold, tmp_path, which):
    """MSA_indel: an indel run with a focus-column threshold below 1 -- the recalibration's forward still runs in substitution mode, with
    the fallback on the non-focus columns."""
    indel, which = which.endswith("_indel"), which.split("_")[0]
    import importlib.util
    import pickle
    import shutil
    from oracle.ref_harness import make_tranception_checkpoint
    spec = importlib.util.spec_from_file_location("make_golden_trancepteve", os.path.join(GOLDEN, "make_golden_trancepteve.py"))
    maker = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(maker)
    seq = str(np.load(os.path.join(GOLDEN, "golden_tranception.npz"))["seq"])
    ms, me = [int(v) for v in gold["msa_start_end"]]
    ckpt = make_tranception_checkpoint(str(tmp_path / "tr"), n_layer=1, n_embd=64, n_head=4, seed=3, n_ctx=42)
    work = tmp_path / "eve"
    work.mkdir()
    shutil.copy(os.path.join(GOLDEN, "TranceptEVE_toy", "TOY_MSA_TTE_seed_0"), work)
    (work / "log_prior").mkdir()
    with open(tte.cache_location(str(work / "TOY_MSA_TTE_seed_0"), 7), "wb") as f:
        pickle.dump(torch.from_numpy(gold["eve_table"]), f)
    model = maker.reference_model(ckpt, seq, dict(
        inference_time_retrieval_type="TranceptEVE", retrieval_aggregation_mode="aggregate_indel" if indel else "aggregate_substitution",
        MSA_filename=MSA_FILE, clustal_omega_location=os.path.join(GOLDEN, "stand_in_clustalo.py"),
        MSA_weight_file_name=WEIGHTS, MSA_start=ms, MSA_end=me, MSA_threshold_sequence_frac_gaps=0.5, MSA_threshold_focus_cols_frac_gaps=0.5,
        retrieval_weights_manual=False, retrieval_inference_MSA_weight=0.5, retrieval_inference_EVE_weight=0.5,
        EVE_model_paths=[str(work / "TOY_MSA_TTE_seed_0")], EVE_num_samples_log_proba=7,
        EVE_model_parameters_location=os.path.join(GOLDEN, "TranceptEVE_toy", "model_params.json"), MSA_recalibrate_probas=False,
        EVE_recalibrate_probas=False))
    assert 1 + int(len(seq) / (model.config.n_ctx - 2)) == 2
    stub = _CpuTransformer(model, 42)
    eve_msa = tte.EveMSA(MSA_FILE, 0.5, 0.5)
    state = tte.build_state(stub, seq, MSA_FILE, WEIGHTS, ms, me, threshold_sequence_frac_gaps=0.5, threshold_focus_cols_frac_gaps=0.5,
                            eve_table=gold["eve_table"], eve_msa=eve_msa, MSA_recalibrate=which == "MSA", EVE_recalibrate=which == "EVE",
                            indel_mode=indel, clustal_omega_location=os.path.join(GOLDEN, "stand_in_clustalo.py"))
    assert state["eve_fallback"] == (not indel) and (state["weight"], state["eve_weight"]) == ((0.5, 0.1) if indel else (0.1, 0.3))
    assert (model.retrieval_inference_MSA_weight, model.retrieval_inference_EVE_weight) == (state["weight"], state["eve_weight"])
    before = model.EVE_log_prior.clone(), model.MSA_log_prior.clone()
    with torch.no_grad():
        (model.recalibrate_EVE_probas if which == "EVE" else model.recalibrate_MSA_probas)()
    want_eve, want_msa = model.EVE_log_prior.numpy(), model.MSA_log_prior.numpy()
    changed = (before[0] if which == "EVE" else before[1]).numpy()
    finite, finite_m = np.isfinite(want_eve), np.isfinite(want_msa)                    # (the MSA table is log 0 outside its range)
    moved = (want_eve[finite] - changed[finite]) if which == "EVE" else (want_msa[finite_m] - changed[finite_m])
    assert np.abs(moved).max() > 1e-2                                                  # the recalibration did something
    assert np.array_equal(np.isfinite(state["eve_log_prior"]), finite) and np.array_equal(np.isfinite(state["log_prior"]), finite_m)
    err_e = np.abs(state["eve_log_prior"][finite] - want_eve[finite]).max()
    err_m = np.abs(state["log_prior"][finite_m] - want_msa[finite_m]).max()
    print(f"recalibrate {which}: max|err| EVE table {err_e:.2e}, MSA table {err_m:.2e}")
    assert err_e <= 1e-5 and err_m <= 1e-5


def test_cli_flag_surface():
    """Every flag of the reference's score_trancepteve.py, with its type, default and action, is a flag of ours (read off the
    reference's own add_argument calls); ours adds --device and --EVE_ignore_log_prior_cache only."""
    import argparse
    import ast
    from proteingym_amd import score_trancepteve_proteingym as cli
    tree = ast.parse(open(os.path.join(tr.TTE_DIR, "score_trancepteve.py")).read())
    want = {}
    for node in ast.walk(tree):
        if isinstance(node, ast.Call) and getattr(node.func, "attr", "") == "add_argument":
            kw = {k.arg: (k.value.id if isinstance(k.value, ast.Name) else ast.literal_eval(k.value)) for k in node.keywords if k.arg != "help"}
            want[ast.literal_eval(node.args[0])] = kw
    assert len(want) == 34
    ours = {a.option_strings[0]: a for a in cli.create_parser()._actions if a.option_strings and a.option_strings[0] != "-h"}
    assert set(ours) - set(want) == {"--device", "--EVE_ignore_log_prior_cache"} and not set(want) - set(ours)
    for flag, kw in want.items():
        a = ours[flag]
        if kw.get("action") == "store_true":
            assert isinstance(a, argparse._StoreTrueAction), flag
            continue
        assert a.default == kw.get("default"), flag
        assert (a.type.__name__ if a.type else None) == kw.get("type"), flag
        assert a.nargs == kw.get("nargs"), flag


@pytest.mark.parametrize("script,indel", [("scoring_TranceptEVE_substitutions.sh", False), ("scoring_TranceptEVE_indels.sh", True)])
def test_launchers_build_a_command_line_the_cli_parses(script, indel, tmp_path):
    import subprocess
    from proteingym_amd import score_trancepteve_proteingym as cli
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = tmp_path / "scripts"
    (cfg / "scoring_DMS_zero_shot").mkdir(parents=True)
    (cfg / "zero_shot_config.sh").write_text("".join(f"export {k}=/data/{k}\n" for k in (
        "DMS_data_folder_subs", "DMS_data_folder_indels", "DMS_MSA_data_folder", "DMS_MSA_weights_folder", "DMS_EVE_model_folder",
        "DMS_reference_file_path_subs", "DMS_reference_file_path_indels", "DMS_output_score_folder_subs", "DMS_output_score_folder_indels")))
    env = dict(os.environ, ZERO_SHOT_CONFIG=str(cfg / "zero_shot_config.sh"), PGMI_LAUNCH_ECHO="1", DMS_index="7")
    out = subprocess.run(["bash", os.path.join(root, "scripts", "scoring_DMS_zero_shot", script)], env=env, capture_output=True, text=True, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr
    argv = out.stdout.strip().split("\n")
    assert argv[0] == "proteingym_amd.score_trancepteve_proteingym"
    a = cli.create_parser().parse_args(argv[1:])
    kind = "indels" if indel else "subs"
    assert a.indel_mode == indel and a.DMS_index == 7 and a.EVE_seeds == ["0", "1", "2", "3", "4"] and a.EVE_num_samples_log_proba == 200000
    assert a.inference_time_retrieval_type == "TranceptEVE" and a.EVE_recalibrate_probas and a.EVE_model_folder == "/data/DMS_EVE_model_folder"
    assert a.DMS_data_folder == f"/data/DMS_data_folder_{kind}" and a.output_scores_folder.startswith(f"/data/DMS_output_score_folder_{kind}/TranceptEVE/")
    assert (a.clustal_omega_location is not None) == indel
