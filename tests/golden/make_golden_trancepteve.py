"""Records the TranceptEVE fixtures from the unmodified reference on the CPU (where the reference tree exists):

    python tests/golden/make_golden_trancepteve.py

Inputs already under tests/golden: the toy alignment TOY_MSA_GAPPY.a2m, the toy Tranception checkpoint and its assay
(TOY_TRANCEPTION_DMS.csv: single and multiple mutants and the wild type).  Written:

    TOY_MSA_TTE.a2m, TOY_MSA_TTE_weights.npy   TOY_MSA_GAPPY.a2m with four columns gapped in about two thirds of the sequences (so that
                                               a focus-column threshold of 0.5 drops them), and the reference's sequence weights for it
    TranceptEVE_toy/TOY_MSA_TTE_seed_0, model_params.json          an EVE checkpoint (eve.random_state_dict) on the alignment's focus
    TranceptEVE_toy_deepseq/TOY_MSA_TTE_seed_0, model_params.json  columns at threshold 0.5, one per parameter style
    golden_trancepteve.npz   focus columns, depths, per style the reference's mean / std of the log-prior over N_STAT samples (its own
                             decoder in eval(), torch's generator), the [len(target), 25] table of the eve style, and the reference's
                             score columns for that table (through its cache file) with and without --EVE_recalibrate_probas;
                             indel/*: the same in indel mode (below)
    TOY_MSA_INDEL_FULL_weights.npy, TranceptEVE_toy_indel/TOY_MSA_INDEL_FULL_seed_0, model_params.json
                             indel mode: the reference re-aligns every scored sequence, here with tests/golden/stand_in_clustalo.py
                             as tests/golden/make_golden_tranception_indel_retrieval.py does; the alignment (TOY_MSA_INDEL_FULL.a2m,
                             residues 1-70) and the assay (TOY_TRANCEPTION_INDEL_RETRIEVAL_DMS.csv) are that script's

Not recorded: the noise of three samples.  The CPU pin (tests/test_trancepteve_host.py) records the reference's randn_like draws live
and the GPU parity test draws seeded numpy noise for the float64 restatement, so no noise file is kept.
"""
import json
import os
import pickle
import shutil
import sys
import tempfile

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import torch  # noqa: E402

import trancepteve_reference as tr  # noqa: E402
from proteingym_amd import eve, trancepteve as tte  # noqa: E402

N_STAT = 2000
THR_SEQ, THR_COLS = 0.5, 0.5
STYLES = {"eve": ("EVE_toy", "TranceptEVE_toy"), "deepseq": ("DeepSequence_toy", "TranceptEVE_toy_deepseq")}


def small_params(folder):
    p = json.load(open(os.path.join(HERE, folder, "model_params.json")))
    p["encoder_parameters"].update(hidden_layers_sizes=[32, 24], z_dim=4)
    p["decoder_parameters"].update(hidden_layers_sizes=[16, 40], z_dim=4)
    if p["decoder_parameters"]["convolve_output"]:
        p["decoder_parameters"]["convolution_output_depth"] = 8
    if p["decoder_parameters"]["include_sparsity"]:
        p["decoder_parameters"]["num_tiles_sparsity"] = 4
    return p


def make_alignment(msa_file, weights):
    lines = open(os.path.join(HERE, "TOY_MSA_GAPPY.a2m")).read().split("\n")
    # the reference reads ONE weights file for both of its alignments (focus-column thresholds 1.0 and THR_COLS): the first seed
    # whose gaps leave both with the same sequences
    for seed in range(77, 177):
        rng = np.random.default_rng(seed)
        out, first = [], True
        for line in lines:
            if line and not line.startswith(">"):
                if not first:
                    line = "".join("-" if (i in (7, 8, 23, 41) and rng.random() < 0.65) else ch for i, ch in enumerate(line))
                first = False
            out.append(line)
        open(msa_file, "w").write("\n".join(out))
        a, b = tte.EveMSA(msa_file, THR_SEQ, 1.0), tte.EveMSA(msa_file, THR_SEQ, THR_COLS)
        if a.depth == b.depth and len(b.focus_cols) == len(a.focus_cols) - 4:
            break
    else:
        raise RuntimeError("no seed gives both alignments the same sequences")
    if os.path.exists(weights):
        os.remove(weights)
    # TranceptEVE's MSA_processing only reads weights; Tranception's (tranception/utils/msa_utils.py:341-352) computes and saves them
    from oracle.ref_harness import load_reference_tranception
    tranception, _ = load_reference_tranception()
    tranception.utils.msa_utils.MSA_processing(MSA_location=msa_file, theta=0.2, use_weights=True, weights_location=weights,
                                               threshold_sequence_frac_gaps=THR_SEQ, threshold_focus_cols_frac_gaps=1.0)
    assert os.path.exists(weights)


def reference_model(checkpoint_dir, target_seq, fields):
    """The reference's TrancepteveLMHeadModel as score_trancepteve.py:106-160 builds it, weights through load_state_dict."""
    pkg, tok = tr.load_reference()
    c = json.load(open(os.path.join(checkpoint_dir, "config.json")))
    c.pop("model_type", None)
    c.pop("architectures", None)
    cfg = pkg.config.TranceptEVEConfig(**c)
    cfg.attention_mode, cfg.position_embedding, cfg.tokenizer = "tranception", "grouped_alibi", tok
    cfg.full_target_seq, cfg.scoring_window = target_seq, "optimal"
    for k, v in fields.items():
        setattr(cfg, k, v)
    model = pkg.model_pytorch.TrancepteveLMHeadModel(cfg)
    sd = torch.load(os.path.join(checkpoint_dir, "pytorch_model.bin"), map_location="cpu")
    missing, unexpected = model.load_state_dict(sd, strict=False)
    bad = [k for k in missing if not (k.endswith(".attn.bias") or k.endswith("masked_bias") or k.endswith("alibi"))]
    assert not bad and not unexpected, (bad, unexpected)
    model.eval()
    return model


def record_indel(out, seq):
    """The reference in indel mode for a GIVEN log-prior table: both tables go through update_retrieved_MSA_log_prior_indel."""
    msa_src, weights = os.path.join(HERE, "TOY_MSA_INDEL_FULL.a2m"), os.path.join(HERE, "TOY_MSA_INDEL_FULL_weights.npy")
    aligner = os.path.join(HERE, "stand_in_clustalo.py")
    if os.path.exists(weights):
        os.remove(weights)
    from oracle.ref_harness import load_reference_tranception
    tranception, _ = load_reference_tranception()
    tranception.utils.msa_utils.MSA_processing(MSA_location=msa_src, theta=0.2, use_weights=True, weights_location=weights,
                                               threshold_sequence_frac_gaps=THR_SEQ, threshold_focus_cols_frac_gaps=1.0)
    msa = tte.EveMSA(msa_src, THR_SEQ, 1.0)
    L = len(msa.focus_cols)
    assert L == len(seq)
    params = small_params("EVE_toy")
    d = eve.dims_from_params(params, L)
    state = eve.random_state_dict(d, seed=8, log_var=(-6.0, -3.0))
    dst = os.path.join(HERE, "TranceptEVE_toy_indel")
    os.makedirs(dst, exist_ok=True)
    json.dump(params, open(os.path.join(dst, "model_params.json"), "w"), indent=1)
    torch.save({"model_state_dict": {k: torch.from_numpy(v) for k, v in state.items()}}, os.path.join(dst, "TOY_MSA_INDEL_FULL_seed_0"))
    vae = tr.build_vae(params, state, L)
    torch.manual_seed(99)
    table = tr.log_prior_single(vae, msa.focus_seq_trimmed, 200, full_len=len(seq), MSA_start=0, focus_cols=msa.focus_cols)
    out["indel/eve_table"] = table
    dms = pd.read_csv(os.path.join(HERE, "TOY_TRANCEPTION_INDEL_RETRIEVAL_DMS.csv"))
    work = tempfile.mkdtemp()                            # the reference writes <MSA folder>/Sampled/*: keep the golden folder clean
    try:
        local = shutil.copy(msa_src, os.path.join(work, os.path.basename(msa_src)))
        shutil.copy(os.path.join(dst, "TOY_MSA_INDEL_FULL_seed_0"), work)
        os.makedirs(os.path.join(work, "log_prior"))
        with open(tte.cache_location(os.path.join(work, "TOY_MSA_INDEL_FULL_seed_0"), 200), "wb") as f:
            pickle.dump(torch.from_numpy(table), f)
        model = reference_model(os.path.join(HERE, "Tranception_toy"), seq, dict(
            inference_time_retrieval_type="TranceptEVE", retrieval_aggregation_mode="aggregate_indel", MSA_filename=local,
            MSA_weight_file_name=weights, MSA_start=0, MSA_end=len(seq), MSA_threshold_sequence_frac_gaps=THR_SEQ,
            MSA_threshold_focus_cols_frac_gaps=1.0, retrieval_weights_manual=False, retrieval_inference_MSA_weight=0.5,
            retrieval_inference_EVE_weight=0.5, EVE_model_paths=[os.path.join(work, "TOY_MSA_INDEL_FULL_seed_0")],
            EVE_num_samples_log_proba=200, EVE_model_parameters_location=os.path.join(dst, "model_params.json"),
            MSA_recalibrate_probas=False, EVE_recalibrate_probas=False, clustal_omega_location=aligner))
        with torch.no_grad():
            r = model.score_mutants(DMS_data=dms, target_seq=seq, scoring_mirror=True, batch_size_inference=1, num_workers=0, indel_mode=True)
        key = r["mutated_sequence"].fillna(r["mutant"]) if "mutant" in r else r["mutated_sequence"]
        m = pd.merge(dms[["mutated_sequence"]], r.assign(key=key), left_on="mutated_sequence", right_on="key", how="left")
        for c in ("avg_score_L_to_R", "avg_score_R_to_L", "avg_score"):
            out[f"indel/{c}"] = m[c].to_numpy(dtype=np.float64)
        out["indel/columns"] = np.array(list(r.columns))
        out["indel/depths"] = np.array([model.MSA_processed_depth, model.EVE_processed_depth])
        out["indel/weights_alpha_beta"] = np.array([model.retrieval_inference_MSA_weight, model.retrieval_inference_EVE_weight])
    finally:
        shutil.rmtree(work)


def main():
    gold = np.load(os.path.join(HERE, "golden_tranception.npz"))
    seq = str(gold["seq"])
    ms, me = [int(v) for v in np.load(os.path.join(HERE, "golden_msa_weights.npz"))["msa_start_end"]]
    msa_file, weights = os.path.join(HERE, "TOY_MSA_TTE.a2m"), os.path.join(HERE, "TOY_MSA_TTE_weights.npy")
    make_alignment(msa_file, weights)
    msa = tte.EveMSA(msa_file, THR_SEQ, THR_COLS)
    L = len(msa.focus_cols)
    assert 0 < L < me - ms, "the fixture needs columns outside EVE's focus columns"
    out = dict(focus_cols=np.array(msa.focus_cols), eve_depth=msa.depth, thresholds=np.array([THR_SEQ, THR_COLS]), n_stat=N_STAT,
               msa_start_end=np.array([ms, me]))
    residues = eve.encode_residues([msa.focus_seq_trimmed])
    torch.manual_seed(20240607)
    for style, (src, dst) in STYLES.items():
        params = small_params(src)
        d = eve.dims_from_params(params, L)
        state = eve.random_state_dict(d, seed=5 if style == "eve" else 6, log_var=(-6.0, -3.0))
        os.makedirs(os.path.join(HERE, dst), exist_ok=True)
        json.dump(params, open(os.path.join(HERE, dst, "model_params.json"), "w"), indent=1)
        torch.save({"model_state_dict": {k: torch.from_numpy(v) for k, v in state.items()}}, os.path.join(HERE, dst, "TOY_MSA_TTE_seed_0"))
        vae = tr.build_vae(params, state, L)
        vae.eval()
        x = torch.tensor(np.eye(20)[np.minimum(residues, 19)] * (residues < 20)[..., None], dtype=torch.float32)
        with torch.no_grad():
            mu, log_var = vae.encoder(x)
            lp = np.stack([vae.decoder(vae.sample_latent(mu, log_var)).view(L, 20).double().numpy() for _ in range(N_STAT)])
        out[f"{style}/mean"], out[f"{style}/std"] = lp.mean(0), lp.std(0, ddof=1)
    # the reference's scores for a GIVEN table: the eve style's recorded mean goes into its cache file
    table = tte.log_prior_table(out["eve/mean"], msa.focus_cols, ms, len(seq))
    out["eve_table"] = table
    dms = pd.read_csv(os.path.join(HERE, "TOY_TRANCEPTION_DMS.csv"))
    work = tempfile.mkdtemp()
    try:
        shutil.copy(os.path.join(HERE, "TranceptEVE_toy", "TOY_MSA_TTE_seed_0"), work)
        os.makedirs(os.path.join(work, "log_prior"))
        with open(tte.cache_location(os.path.join(work, "TOY_MSA_TTE_seed_0"), N_STAT), "wb") as f:
            pickle.dump(torch.from_numpy(table), f)
        for tag, recal in (("plain", False), ("recal", True)):
            model = reference_model(os.path.join(HERE, "Tranception_toy"), seq, dict(
                inference_time_retrieval_type="TranceptEVE", retrieval_aggregation_mode="aggregate_substitution", MSA_filename=msa_file,
                MSA_weight_file_name=weights, MSA_start=ms, MSA_end=me, MSA_threshold_sequence_frac_gaps=THR_SEQ,
                MSA_threshold_focus_cols_frac_gaps=THR_COLS, retrieval_weights_manual=False, retrieval_inference_MSA_weight=0.5,
                retrieval_inference_EVE_weight=0.5, EVE_model_paths=[os.path.join(work, "TOY_MSA_TTE_seed_0")],
                EVE_num_samples_log_proba=N_STAT, EVE_model_parameters_location=os.path.join(HERE, "TranceptEVE_toy", "model_params.json"),
                MSA_recalibrate_probas=False, EVE_recalibrate_probas=recal))
            assert np.array_equal(model.EVE_log_prior.numpy(), table, equal_nan=True)
            with torch.no_grad():
                scores = model.score_mutants(DMS_data=dms, target_seq=seq, scoring_mirror=True, batch_size_inference=20, num_workers=0)
            scores = pd.merge(dms[["mutated_sequence"]], scores, on="mutated_sequence", how="left")
            for c in ("avg_score_L_to_R", "avg_score_R_to_L", "avg_score"):
                out[f"scores_{tag}/{c}"] = scores[c].to_numpy()
            out[f"columns_{tag}"] = np.array(list(scores.columns))
            out["msa_depth"], out["weights_alpha_beta"] = model.MSA_processed_depth, np.array(
                [model.retrieval_inference_MSA_weight, model.retrieval_inference_EVE_weight])
            assert model.EVE_processed_depth == msa.depth, (model.EVE_processed_depth, msa.depth)
            if recal:
                out["eve_table_recalibrated"] = model.EVE_log_prior.numpy()
    finally:
        shutil.rmtree(work)
    record_indel(out, seq)
    np.savez_compressed(os.path.join(HERE, "golden_trancepteve.npz"), **out)
    print({k: np.shape(v) for k, v in out.items()})


if __name__ == "__main__":
    main()
