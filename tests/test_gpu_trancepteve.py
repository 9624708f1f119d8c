"""TranceptEVE on the GPU: pgmi_eve_log_prior and the two-prior fusion against tests/trancepteve_ref.py (float64; pinned to the
unmodified reference by tests/test_trancepteve_host.py), and the end-to-end scores against the reference's recorded run
(tests/golden/make_golden_trancepteve.py).

Bounds: 1e-4 per entry of the mean log-prior (the project's flat bound per log-probability, tests/test_gpu_eve.py); T x 1e-4 per
sequence log-likelihood of T tokens (the same bound, summed); the end-to-end scores within TOL = 1e-4 of the recorded ones, the bound
tests/test_gpu_tranception.py::test_retrieval_vs_reference holds its scores to.
"""
import json
import os

import numpy as np
import pandas as pd
import pytest

import trancepteve_ref as tref
from proteingym_amd import _lib, eve, tranception as ptr

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOYS = {"eve": os.path.join(GOLDEN, "EVE_toy"), "deepseq": os.path.join(GOLDEN, "DeepSequence_toy")}
L_TOY = 50
TOL = 1e-4

# the default parameter file's widths (tests/test_gpu_eve.py REAL): H = 2000, so a logit's 2000 terms straddle blocks of 5120
REAL = dict(seq_len=21, z_dim=50, enc_sizes=[2000, 1000, 300], dec_sizes=[300, 1000, 2000], conv_depth=40, temperature=1,
            sparsity_tiles=0, enc_act="relu", dec_first_act="relu", dec_last_act="relu", dropout_p=0.1)
# H % 20 != 0: threads whose 20 values belong to two logits; L H = 504 = 256 + 248: a short last block; sparsity gate on
STRADDLE = dict(seq_len=7, z_dim=5, enc_sizes=[24, 12], dec_sizes=[16, 72], conv_depth=8, temperature=1, sparsity_tiles=4,
                enc_act="relu", dec_first_act="relu", dec_last_act="sigmoid", dropout_p=0.1)
# no convolution (C = 20), no temperature, no gate; L H = 550: three blocks
NOCONV = dict(seq_len=11, z_dim=6, enc_sizes=[20], dec_sizes=[50], conv_depth=0, temperature=0, sparsity_tiles=0,
              enc_act="relu", dec_first_act="relu", dec_last_act="relu", dropout_p=0.0)


def wild_type(L, seed):
    return np.random.default_rng(seed).integers(0, 20, size=L).astype(np.uint8)


@pytest.fixture(scope="module", params=sorted(TOYS))
def toy(request, lib):
    folder = TOYS[request.param]
    params = json.load(open(os.path.join(folder, "model_params.json")))
    d, blob = eve.load_checkpoint(os.path.join(folder, "TOY_MSA_seed_0"), params, L_TOY)
    model = eve.EveModel(d, blob)
    yield request.param, d, eve.state_from_blob(d, blob), model
    model.close()


def synthetic(dims, seed):
    sd = eve.random_state_dict(dims, seed=seed, log_var=(-8.0, -4.0))
    return sd, eve.EveModel(dims, eve.blob_from_state_dict(sd, dims))


@pytest.fixture
def prior_batch(lib):
    def set_(n):
        _lib.check(lib.pgmi_set_option(b"eve_prior_batch", int(n)))
    yield set_
    lib.pgmi_set_option(b"eve_prior_batch", 0)


def check_log_prior(tag, d, state, model, n, seed):
    res = wild_type(d["seq_len"], seed)
    rng = np.random.default_rng(seed + 1)
    noises = [tref.numpy_noise(d, rng) for _ in range(n)]
    want_mean, want_std, _ = tref.log_prior(state, d, res, noises)
    mean, std = model.log_prior(res, n, noise=noises)
    err, err_s = float(np.abs(mean - want_mean).max()), float(np.abs(std - want_std).max())
    print(f"{tag}: max|mean logp - float64| {err:.3e}, std {err_s:.3e} (|logp| <= {np.abs(want_mean).max():.2f}, bound {TOL:.0e})")
    assert err <= TOL and err_s <= TOL
    assert np.exp(mean).sum(-1).max() <= 1.0 + 1e-6            # a mean of log-distributions: Jensen keeps each position's mass <= 1


# ---- 1-5: pgmi_eve_log_prior ----------------------------------------------------------------------------------------------------
def test_injected_noise_vs_float64(toy):
    name, d, state, model = toy
    check_log_prior(f"{name} toy, 3 samples", d, state, model, 3, seed=11)


def test_real_widths(lib):
    sd, model = synthetic(REAL, 17)
    try:
        check_log_prior("real widths, 2 samples", REAL, sd, model, 2, seed=4)
    finally:
        model.close()


@pytest.mark.parametrize("dims", [STRADDLE, NOCONV], ids=["straddle", "noconv"])
def test_straddling_shapes(lib, dims):
    sd, model = synthetic(dims, 23)
    try:
        check_log_prior(f"H = {dims['dec_sizes'][-1]}, L = {dims['seq_len']}, 5 samples", dims, sd, model, 5, seed=6)
    finally:
        model.close()


def test_generator_equals_injection(toy):
    name, d, state, model = toy
    res = wild_type(L_TOY, 3)
    for seed in (0, 12345678901234):
        noises = [model.noise_fill(1, seed, j) for j in range(4)]
        gen = model.log_prior(res, 4, seed=seed)
        inj = model.log_prior(res, 4, noise=noises)
        for g, i in zip(gen, inj):
            assert np.array_equal(g.view(np.uint64), i.view(np.uint64))
        # the float64 restatement on the generator's own noise
        assert np.abs(gen[0] - tref.log_prior(state, d, res, noises)[0]).max() <= TOL
    assert not np.array_equal(model.log_prior(res, 4, seed=0)[0], model.log_prior(res, 4, seed=1)[0])


def test_batch_size_invariance(toy, prior_batch):
    name, d, state, model = toy
    res = wild_type(L_TOY, 5)
    runs = []
    for n in (1, 2, 3, 7):
        prior_batch(n)
        runs.append(model.log_prior(res, 7, seed=9))
    prior_batch(0)
    runs.append(model.log_prior(res, 7, seed=9))
    for mean, std in runs[1:]:
        assert np.array_equal(mean.view(np.uint64), runs[0][0].view(np.uint64))
        assert np.array_equal(std.view(np.uint64), runs[0][1].view(np.uint64))
    # one sample at a time: sample j alone is the generator's noise of j fed back
    singles = np.stack([model.log_prior(res, 1, noise=[model.noise_fill(1, 9, j)])[0] for j in range(7)])
    assert len({s.tobytes() for s in singles}) == 7
    assert np.abs(runs[0][0] - singles.mean(0)).max() <= 1e-9 * np.abs(singles).max()
    assert np.abs(runs[0][1] - singles.std(0, ddof=1)).max() <= 1e-6


# ---- 6-8: the two-prior fusion ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tr_model(lib):
    m = ptr.from_pretrained(os.path.join(GOLDEN, "Tranception_toy"))
    yield m
    m.close()


AA = "ACDEFGHIKLMNPQRSTVWY"


def _sub(s, p, rng):
    return s[:p] + rng.choice([c for c in AA if c != s[p]]) + s[p + 1:]


def _batch(rng, L, n_single=9, n_multi=5):
    wt = "".join(rng.choice(list(AA), size=L))
    seqs = [wt] + [_sub(wt, int(p), rng) for p in rng.choice(L, size=n_single, replace=False)]
    for _ in range(n_multi):
        s = wt
        for p in rng.choice(L, size=int(rng.integers(2, 5)), replace=False):
            s = _sub(s, int(p), rng)
        seqs.append(s)
    return seqs


def _priors(rng, P, holes=()):
    msa = np.log(rng.dirichlet(np.ones(25), size=P)).astype(np.float32)
    eve_t = np.full((P, 25), -np.inf, dtype=np.float32)
    eve_t[:, 5:] = np.log(rng.dirichlet(np.ones(20), size=P)).astype(np.float32)
    for h in holes:
        eve_t[h] = -np.inf
    return msa, eve_t


def _call(model, ids, lens, msa, a0, row0, n, flip, alpha, eve_t=None, beta=0.0, fallback=0, entry="eve", ref=None):
    lib = _lib.load()
    B, T = ids.shape
    lp = _lib.as_f32(msa)
    a0, row0, n, flip = (np.full(B, v, np.int32) for v in (a0, row0, n, flip))
    prior = (_lib.ptr(lp, _lib._f32p), lp.shape[0], _lib.ptr(a0, _lib._i32p), _lib.ptr(row0, _lib._i32p), _lib.ptr(n, _lib._i32p),
             _lib.ptr(flip, _lib._i32p), float(alpha))
    e = _lib.as_f32(eve_t) if eve_t is not None else None
    eve_args = (_lib.ptr(e, _lib._f32p) if e is not None else None, float(beta), int(fallback))
    out = np.empty(B, np.float32)
    ids_p, lens_p, out_p = _lib.ptr(ids, _lib._i32p), _lib.ptr(lens, _lib._i32p), _lib.ptr(out, _lib._f32p)
    rows = np.zeros(1, np.int64)
    if ref is None:
        ref = np.zeros(B, np.int32)
    ref_p = _lib.ptr(ref, _lib._i32p)
    if entry == "eve":
        _lib.check(lib.pgmi_tr_sequence_loglik_eve(model._h, ids_p, lens_p, B, T, *prior, *eve_args, out_p))
    elif entry == "old":
        _lib.check(lib.pgmi_tr_sequence_loglik(model._h, ids_p, lens_p, B, T, *prior, out_p))
    elif entry == "shared_eve":
        _lib.check(lib.pgmi_tr_sequence_loglik_shared_eve(model._h, ids_p, ref_p, B, T, *prior, *eve_args, out_p, None, _lib.ptr(rows, _lib._i64p)))
    else:
        _lib.check(lib.pgmi_tr_sequence_loglik_shared(model._h, ids_p, ref_p, B, T, *prior, out_p, None, _lib.ptr(rows, _lib._i64p)))
    return out


def test_old_entries_same_bits(tr_model):
    rng = np.random.default_rng(31)
    seqs = _batch(rng, 40)
    ids, lens = tr_model.encode_batch(seqs)
    msa, _ = _priors(rng, 50)
    for flip in (0, 1):
        args = (tr_model, ids, lens, msa, 3, 5, 30, flip, 0.6)
        assert np.array_equal(_call(*args, entry="eve").view(np.uint32), _call(*args, entry="old").view(np.uint32))
        assert np.array_equal(_call(*args, entry="shared_eve").view(np.uint32), _call(*args, entry="shared_old").view(np.uint32))
    # padded: the same sequences in a batch with a longer one (right-padded rows, lens < T)
    longer = seqs + ["".join(rng.choice(list(AA), size=47))]
    ids, lens = tr_model.encode_batch(longer)
    assert lens.min() < ids.shape[1]
    args = (tr_model, ids, lens, msa, 3, 5, 30, 0, 0.6)
    assert np.array_equal(_call(*args, entry="eve").view(np.uint32), _call(*args, entry="old").view(np.uint32))


# (a0, row0, n) for L = 40 residues, T = 42 tokens, 40 logit rows with a residue as target: the window cuts the prior's range on the left (the first rows of the
# table are before the window: row0 > 0, a0 = 0), on the right (the table ends inside the window: a0 + n < T - 1) and both
CUTS = {"left": (0, 7, 40), "right": (0, 0, 29), "inside": (6, 0, 27)}


@pytest.mark.parametrize("cut", sorted(CUTS))
@pytest.mark.parametrize("flip", [0, 1])
def test_fusion_vs_float64(tr_model, cut, flip):
    rng = np.random.default_rng(41)
    L = 40
    seqs = _batch(rng, L)
    ids, lens = tr_model.encode_batch(seqs)
    B, T = ids.shape
    a0, row0, n = CUTS[cut]
    hole = row0 + 11                                            # one non-focus column inside the fused rows
    msa, eve_t = _priors(rng, 50, holes=(hole,))
    full = eve_t.copy()                                         # the same table with the hole filled
    full[hole, 5:] = np.log(rng.dirichlet(np.ones(20))).astype(np.float32)
    logp = tr_model.token_logprobs(ids).astype(np.float64)      # the device's own rows: the fusion and the sum are what is under test

    def want(eve_tab, alpha, beta, fallback):
        return np.array([tref.sequence_loglik(logp[b], ids[b], int(lens[b]), msa.astype(np.float64),
                                              None if eve_tab is None else eve_tab.astype(np.float64), a0, row0, n, flip, alpha, beta,
                                              fallback) for b in range(B)])

    alpha, beta = 0.6, 0.35
    got = _call(tr_model, ids, lens, msa, a0, row0, n, flip, alpha, eve_t, beta, 1)
    w = want(eve_t, alpha, beta, 1)
    print(f"{cut} flip {flip}: max|err| {np.abs(got - w).max():.3e} (bound {T * TOL:.1e}, |loglik| ~ {np.abs(w).mean():.1f})")
    assert np.isfinite(w).all() and np.abs(got - w).max() <= T * TOL
    # the fallback matters: the hole's position differs from a finite EVE row
    assert np.abs(w - want(full, alpha, beta, 1)).max() > T * TOL
    # eve_fallback = 0: the -inf goes through, here and in the restatement
    got0 = _call(tr_model, ids, lens, msa, a0, row0, n, flip, alpha, eve_t, beta, 0)
    assert np.isneginf(want(eve_t, alpha, beta, 0)).all() and np.isneginf(got0).all()
    # beta = 0 is the one-prior call
    one = _call(tr_model, ids, lens, msa, a0, row0, n, flip, alpha, entry="old")
    assert np.array_equal(_call(tr_model, ids, lens, msa, a0, row0, n, flip, alpha, full, 0.0, 0), one)
    assert np.array_equal(_call(tr_model, ids, lens, msa, a0, row0, n, flip, alpha, eve_t, 0.0, 1), one)
    # alpha = 0: the network and EVE alone
    got_a = _call(tr_model, ids, lens, msa, a0, row0, n, flip, 0.0, full, beta, 0)
    assert np.abs(got_a - want(full, 0.0, beta, 0)).max() <= T * TOL


def test_prefix_sharing_same_bits(tr_model):
    rng = np.random.default_rng(51)
    for L in (40, 94):
        seqs = _batch(rng, L, n_single=12, n_multi=8)
        ids, lens = tr_model.encode_batch(seqs)
        msa, eve_t = _priors(rng, L + 10, holes=(9, 20))
        for flip, fallback in ((0, 1), (1, 1), (0, 0)):
            args = (tr_model, ids, lens, msa, 2, 4, L - 8, flip, 0.6, eve_t, 0.3, fallback)
            a, b = _call(*args, entry="eve"), _call(*args, entry="shared_eve")
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
            assert np.isfinite(a).all() == bool(fallback)


# ---- 9-10: end to end ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "golden_trancepteve.npz"))


def _state(model, gold, seq, recal, **kw):
    from proteingym_amd import trancepteve as tte
    ms, me = [int(v) for v in gold["msa_start_end"]]
    thr_seq, thr_cols = [float(v) for v in gold["thresholds"]]
    msa_file = os.path.join(GOLDEN, "TOY_MSA_TTE.a2m")
    eve_msa = tte.EveMSA(msa_file, thr_seq, thr_cols)
    assert eve_msa.focus_cols == gold["focus_cols"].tolist() and eve_msa.depth == int(gold["eve_depth"])
    return tte.build_state(model, seq, msa_file, os.path.join(GOLDEN, "TOY_MSA_TTE_weights.npy"), ms, me, threshold_sequence_frac_gaps=thr_seq,
                           threshold_focus_cols_frac_gaps=thr_cols, eve_table=gold["eve_table"], eve_msa=eve_msa, EVE_recalibrate=recal, **kw)


@pytest.mark.parametrize("tag", ["plain", "recal"])
def test_end_to_end_vs_recorded_reference(tr_model, gold, tag):
    """score_mutants with the recorded log-prior table against the reference's recorded scores (four columns outside EVE's focus
    columns: the fallback is on), with and without --EVE_recalibrate_probas; TOL is tests/test_gpu_tranception.py's bound."""
    seq = str(np.load(os.path.join(GOLDEN, "golden_tranception.npz"))["seq"])
    saved = tr_model.retrieval
    try:
        state = _state(tr_model, gold, seq, recal=tag == "recal")
        assert (state["weight"], state["eve_weight"]) == tuple(gold["weights_alpha_beta"]) and state["eve_fallback"]
        assert state["MSA_processed_depth"] == int(gold["msa_depth"])
        if tag == "recal":
            finite = np.isfinite(gold["eve_table_recalibrated"])
            assert np.array_equal(np.isfinite(state["eve_log_prior"]), finite)
            err = np.abs(state["eve_log_prior"][finite] - gold["eve_table_recalibrated"][finite]).max()
            print(f"recalibrated EVE table: max|err| {err:.2e}")
            assert err <= TOL
        tr_model.retrieval = state
        df = pd.read_csv(os.path.join(GOLDEN, "TOY_TRANCEPTION_DMS.csv"))
        r = pd.merge(df[["mutated_sequence"]], tr_model.score_mutants(DMS_data=df, target_seq=seq, scoring_mirror=True), on="mutated_sequence", how="left")
        for c in ("avg_score_L_to_R", "avg_score_R_to_L", "avg_score"):
            err = np.abs(r[c].to_numpy() - gold[f"scores_{tag}/{c}"]).max()
            print(f"{tag} {c}: max|err| {err:.2e}")
            assert err < TOL
    finally:
        tr_model.retrieval = saved


def test_cli_writes_the_reference_columns_and_log(lib, gold, tmp_path, monkeypatch):
    """The CLI from checkpoints to CSV: the reference's file name, columns and log line (seven values under a six-name header); the
    second run reads the log-prior cache the first one wrote (the reference's format) and gives the same file."""
    import shutil
    from proteingym_amd import score_trancepteve_proteingym as cli
    seq = str(np.load(os.path.join(GOLDEN, "golden_tranception.npz"))["seq"])
    ms, me = [int(v) for v in gold["msa_start_end"]]
    folder = tmp_path / "eve"
    shutil.copytree(os.path.join(GOLDEN, "TranceptEVE_toy"), folder)
    monkeypatch.chdir(tmp_path)
    argv = ["--checkpoint", os.path.join(GOLDEN, "Tranception_toy"), "--target_seq", seq, "--DMS_file_name", "TOY_TRANCEPTION_DMS.csv",
            "--DMS_data_folder", GOLDEN, "--output_scores_folder", str(tmp_path / "out"), "--inference_time_retrieval_type", "TranceptEVE",
            "--MSA_folder", GOLDEN, "--MSA_filename", "TOY_MSA_TTE.a2m", "--MSA_weights_folder", GOLDEN, "--MSA_weight_file_name",
            "TOY_MSA_TTE_weights.npy", "--MSA_start", str(ms + 1), "--MSA_end", str(me), "--MSA_threshold_sequence_frac_gaps", "0.5",
            "--MSA_threshold_focus_cols_frac_gaps", "0.5", "--EVE_model_folder", str(folder), "--EVE_seeds", "0",
            "--EVE_num_samples_log_proba", "64", "--EVE_model_parameters_location", str(folder / "model_params.json"), "--EVE_recalibrate_probas"]
    assert cli.main(argv) == 0
    first = pd.read_csv(tmp_path / "out" / "TOY_TRANCEPTION_DMS.csv")
    assert list(first.columns) == gold["columns_recal"].tolist()
    assert np.isfinite(first["avg_score"]).all() and len(first) == 40
    cache = folder / "log_prior" / "TOY_MSA_TTE_seed_0_64_log_space"
    import pickle
    import torch
    table = pickle.load(open(cache, "rb"))
    assert isinstance(table, torch.Tensor) and tuple(table.shape) == (len(seq), 25) and table.dtype == torch.float32
    assert np.isneginf(table.numpy()[:, :5]).all() and np.isfinite(table.numpy()[[ms + c for c in gold["focus_cols"]], 5:]).all()
    assert cli.main(argv) == 0
    assert first.equals(pd.read_csv(tmp_path / "out" / "TOY_TRANCEPTION_DMS.csv"))
    log = open(tmp_path / "TranceptEVE_aggregation_coefficients_log").read().split("\n")
    assert log[0] == cli.LOG_HEADER.strip() and len(log[0].split(",")) == 6
    assert log[1] == log[2] == f"TOY_TRANCEPTION_DMS,40,40,{int(gold['msa_depth'])},{int(gold['eve_depth'])},0.1,0.3"


@pytest.mark.parametrize("style", ["eve", "deepseq"])
def test_statistics_vs_recorded_reference(lib, gold, style):
    """2000 generator samples against the reference's recorded mean over 2000 samples of its own generator: two independent estimates
    of one mean, so every entry lies within 6 sqrt(s_ref^2 / 2000 + s_here^2 / 2000).  Under the null an entry misses a 6-sigma bound
    with probability 2 (1 - Phi(6)) = 2.0e-9; over the 56 x 20 = 1120 entries of a style that is 2.2e-6, over both styles 4.4e-6."""
    from proteingym_amd import trancepteve as tte
    folder = os.path.join(GOLDEN, "TranceptEVE_toy" if style == "eve" else "TranceptEVE_toy_deepseq")
    params = json.load(open(os.path.join(folder, "model_params.json")))
    msa = tte.EveMSA(os.path.join(GOLDEN, "TOY_MSA_TTE.a2m"), *[float(v) for v in gold["thresholds"]])
    d, blob = eve.load_checkpoint(os.path.join(folder, "TOY_MSA_TTE_seed_0"), params, len(msa.focus_cols))
    model = eve.EveModel(d, blob)
    try:
        n = int(gold["n_stat"])
        mean, std = model.log_prior(eve.encode_residues([msa.focus_seq_trimmed])[0], n, seed=0)
    finally:
        model.close()
    want, s_ref = gold[f"{style}/mean"], gold[f"{style}/std"]
    bound = 6.0 * np.sqrt(s_ref ** 2 / n + std ** 2 / n)
    ratio = np.abs(mean - want) / bound
    print(f"{style}: max |mean - recorded| / bound {ratio.max():.3f} (bound {bound.min():.2e} .. {bound.max():.2e}); "
          f"std ratio {np.median(std / s_ref):.3f}")
    assert (ratio <= 1.0).all()
    assert np.abs(np.log(std / s_ref)).max() < 0.5         # the spread itself is the reference's, entry by entry


def test_indels_end_to_end_vs_recorded_reference(lib, gold, tmp_path, monkeypatch):
    """Indel mode through the CLI (--indel_mode --clustal_omega_location, the stand-in aligner of
    tests/test_gpu_tranception.py::test_indels_with_retrieval_vs_reference): every sequence re-aligned, the MSA table AND the EVE table
    re-indexed through the alignment rows, inserted residues left to the network, weights (0.5, 0.1), no fallback.  The EVE table is the
    recorded one (placed in the cache, the reference's format); the scores are the reference's recorded ones, to the same TOL."""
    import pickle
    import shutil
    import stat
    import torch
    from proteingym_amd import score_trancepteve_proteingym as cli, trancepteve as tte
    seq = str(np.load(os.path.join(GOLDEN, "golden_tranception.npz"))["seq"])
    aligner = tmp_path / "clustalo"                                     # an executable of our own: mode bits need not survive a copy of the tree
    aligner.write_text('#!/bin/sh\nexec python3 "%s" "$@"\n' % os.path.join(GOLDEN, "stand_in_clustalo.py"))
    aligner.chmod(aligner.stat().st_mode | stat.S_IXUSR)
    msa = tmp_path / "msa"
    msa.mkdir()
    shutil.copy(os.path.join(GOLDEN, "TOY_MSA_INDEL_FULL.a2m"), msa / "TOY_MSA_INDEL_FULL.a2m")
    folder = tmp_path / "eve"
    shutil.copytree(os.path.join(GOLDEN, "TranceptEVE_toy_indel"), folder)
    (folder / "log_prior").mkdir()
    with open(tte.cache_location(str(folder / "TOY_MSA_INDEL_FULL_seed_0"), 200), "wb") as f:
        pickle.dump(torch.from_numpy(gold["indel/eve_table"]), f)
    monkeypatch.chdir(tmp_path)
    argv = ["--checkpoint", os.path.join(GOLDEN, "Tranception_toy"), "--target_seq", seq, "--DMS_file_name", "TOY_TRANCEPTION_INDEL_RETRIEVAL_DMS.csv",
            "--DMS_data_folder", GOLDEN, "--output_scores_folder", str(tmp_path / "out"), "--inference_time_retrieval_type", "TranceptEVE",
            "--indel_mode", "--clustal_omega_location", str(aligner), "--batch_size_inference", "1",
            "--MSA_folder", str(msa), "--MSA_filename", "TOY_MSA_INDEL_FULL.a2m", "--MSA_weights_folder", GOLDEN, "--MSA_weight_file_name",
            "TOY_MSA_INDEL_FULL_weights.npy", "--MSA_start", "1", "--MSA_end", str(len(seq)), "--MSA_threshold_sequence_frac_gaps", "0.5",
            "--MSA_threshold_focus_cols_frac_gaps", "1.0", "--EVE_model_folder", str(folder), "--EVE_seeds", "0",
            "--EVE_num_samples_log_proba", "200", "--EVE_model_parameters_location", str(folder / "model_params.json")]
    assert cli.main(argv) == 0
    df = pd.read_csv(os.path.join(GOLDEN, "TOY_TRANCEPTION_INDEL_RETRIEVAL_DMS.csv"))
    r = pd.read_csv(tmp_path / "out" / "TOY_TRANCEPTION_INDEL_RETRIEVAL_DMS.csv", float_precision="round_trip")
    assert list(r.columns) == gold["indel/columns"].tolist()
    m = pd.merge(df[["mutated_sequence"]], r, on="mutated_sequence", how="left")
    for c in ("avg_score_L_to_R", "avg_score_R_to_L", "avg_score"):
        err = np.abs(m[c].to_numpy(dtype=np.float64) - gold[f"indel/{c}"]).max()
        print(f"indels, {c}: max|err| {err:.2e}")
        assert err < TOL, c
    # the EVE prior matters in this run: the recorded Tranception-only retrieval scores of the same assay are far away
    other = np.load(os.path.join(GOLDEN, "golden_tranception_indel_retrieval.npz"))["full/avg_score"]
    assert np.abs(other - gold["indel/avg_score"]).max() > 100 * TOL
    log = open(tmp_path / "TranceptEVE_aggregation_coefficients_log").read().split("\n")
    d_msa, d_eve = [int(v) for v in gold["indel/depths"]]
    assert log[1] == f"TOY_TRANCEPTION_INDEL_RETRIEVAL_DMS,{len(r)},{len(r.dropna())},{d_msa},{d_eve},0.5,0.1"
