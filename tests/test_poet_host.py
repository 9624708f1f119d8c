"""PoET's host side without a GPU: the encoder, the a3m reader, the filter and the sampling against the recorded reference results,
the blob order, the CLI flags; and, where the reference tree exists, the float64 / fp32 restatement of tests/poet_ref.py (what the GPU
tests compare against) pinned to the LIVE reference, the sampling pinned to the reference's own MSASampler, and the goldens regenerated."""
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest
import torch

import poet_ref
import poet_reference as pr
from proteingym_amd import poet, score_poet_proteingym as cli

HERE = os.path.dirname(os.path.abspath(__file__))
TOY = os.path.join(HERE, "golden", "PoET_toy")
CONTEXT_LENGTHS = (60, 150, 400)
needs_reference = pytest.mark.skipif(not pr.reference_available(), reason="the reference tree is not on this machine")


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(TOY, "golden_poet.npz"))


@pytest.fixture(scope="module")
def sd():
    ckpt = torch.load(os.path.join(TOY, "poet_toy.ckpt"), map_location="cpu", weights_only=True)
    return {k.split(".", 1)[1]: v.float().numpy() for k, v in ckpt["state_dict"].items()}


@pytest.fixture(scope="module")
def msa_sequences():
    return poet.read_msa(TOY, "TOY_POET.csv")


def test_encoding_framing_and_reversal():
    assert poet.encode(b"ARNDCQEGHILKMFPSTWYV-*$X").tolist() == list(range(24))
    assert poet.encode(b"OUBZ").tolist() == [11, 4, 23, 23]
    assert poet.encode(b"aJ?").tolist() == [23, 23, 23]                      # anything else is the mask token
    f = poet.frame("ACD")
    assert f.tolist() == [21, 0, 4, 3, 22] and f.dtype == np.uint8
    assert (poet.GAP, poet.START, poet.STOP, poet.MASK) == (20, 21, 22, 23)
    assert np.ascontiguousarray(f[::-1]).tolist() == [22, 3, 4, 0, 21]        # the backward pass reverses start and stop too


def test_a3m_reader_keeps_lower_case(msa_sequences, g):
    text = open(os.path.join(TOY, "TOY_POET.a3m"), "rb").read()
    assert text.startswith(b"#")                                             # a comment line, skipped
    assert len(msa_sequences) == text.count(b">") == g["msa"].shape[0]
    assert any(any(chr(c).islower() for c in s) for s in msa_sequences) and any(b"-" in s for s in msa_sequences)
    assert poet.parse_a3m(b">a\nAC\nde\n>b\n\nFG-\n") == [b"ACde", b"FG-"]
    msa = poet.encoded_msa(msa_sequences)
    assert msa.dtype == np.uint8 and np.array_equal(msa, g["msa"])
    with pytest.raises(ValueError, match="differ in length"):
        poet.encoded_msa([b"ACD", b"AC"])


def test_msa_file_lookup(tmp_path):
    (tmp_path / "X.a3m").write_bytes(b">w\nACD\n")
    assert poet.read_msa(str(tmp_path), "X.csv") == [b"ACD"]
    (tmp_path / "Y.a3m.zst").write_bytes(b"not zstd")
    try:
        import pyzstd  # noqa: F401
    except ImportError:
        try:
            import zstandard  # noqa: F401
        except ImportError:
            with pytest.raises(FileNotFoundError, match=r"Y\.a3m\.zst: no zstd module"):
                poet.read_msa(str(tmp_path), "Y.csv")
    with pytest.raises(FileNotFoundError, match=r"neither .*Z\.a3m\.zst nor .*Z\.a3m exists"):
        poet.read_msa(str(tmp_path), "Z.csv")


def test_similarity_filter_has_rows_on_both_sides_of_every_cutoff(g):
    msa = g["msa"]
    sim = (msa == msa[[0]]).sum(axis=1) / msa.shape[1]
    for c in poet.SIMILARITY_CUTOFFS:
        keep = poet.sim_filtered_idxs(msa, c)
        assert np.array_equal(keep, np.where(sim <= c)[0]) and keep.size > 0
        if c < 1.0:
            assert keep.size < len(msa)


def test_sampled_indices_and_prompts_of_all_15_members(msa_sequences, g):
    msa = poet.encoded_msa(msa_sequences)
    w = poet.homology_weights(g["neighbors"])
    prompts = poet.member_prompts(msa_sequences, msa, w, CONTEXT_LENGTHS, poet.SEED)
    assert len(prompts) == 15
    overshoot = set()
    for k, ((idxs, prompt), (budget, _)) in enumerate(zip(prompts, poet.ensemble_members(CONTEXT_LENGTHS))):
        assert np.array_equal(idxs, g[f"idxs_{k}"]), k
        assert [len(s) for s in prompt] == g[f"prompt_lens_{k}"].tolist(), k
        assert np.array_equal(np.concatenate(prompt), g[f"prompt_tokens_{k}"]), k
        assert all(s[0] == poet.START and s[-1] == poet.STOP and (s != poet.GAP).all() for s in prompt)
        overshoot.add(sum(len(s) for s in prompt) > budget)
    assert overshoot == {True, False}                                        # both: the budget passed by one sequence, and never reached
    assert poet.max_prompt_tokens(prompts) == max(int(g[f"prompt_lens_{k}"].sum()) for k in range(15))


def test_homology_weights_are_the_reference_statements():
    n = np.array([8, 1, 5, 5])
    p = poet.homology_weights(n)
    assert p.dtype == np.float64 and np.array_equal(p, (1 / n) / np.sum(1 / n))


def test_blob_order_and_config(sd):
    init = dict(n_vocab=24, hidden_dim=128, ff_dim=256, num_layers=2, nhead=2, norm=True)
    cfg = poet.config_from_init_args(init)
    assert cfg == dict(layers=2, embed_dim=128, heads=2, ffn_dim=256, vocab=24, final_norm=True)
    assert poet.config_from_init_args(dict(n_vocab=24))["ffn_dim"] == 4 * 768
    with pytest.raises(ValueError, match="unknown model init args \\['rotary_scale'\\]"):
        poet.config_from_init_args(dict(init, rotary_scale=5))
    keys = poet.expected_keys(cfg)
    assert keys[:9] == ["token_embed.weight", "decoder.layers.0.norm1.weight", "decoder.layers.0.norm1.bias",
                        "decoder.layers.0.self_attn.q_proj.weight", "decoder.layers.0.self_attn.k_proj.weight",
                        "decoder.layers.0.self_attn.v_proj.weight", "decoder.layers.0.self_attn.out_proj.weight",
                        "decoder.layers.0.self_attn.out_proj.bias", "decoder.layers.0.norm2.weight"]
    assert keys[-4:] == ["norm.weight", "norm.bias", "linear.weight", "linear.bias"]
    blob = poet.pack(cfg, sd)
    assert blob.size == poet.weight_count(cfg) == sum(sd[k].size for k in keys)
    o = 24 * 128 + 2 * 128
    assert np.array_equal(blob[:24 * 128], sd["token_embed.weight"].ravel())
    assert np.array_equal(blob[o:o + 128 * 128], sd["decoder.layers.0.self_attn.q_proj.weight"].ravel())
    assert np.array_equal(blob[-24:], sd["linear.bias"])
    cfg2, blob2 = poet.load_checkpoint(os.path.join(TOY, "poet_toy.ckpt"))
    assert cfg2 == cfg and np.array_equal(blob2, blob)
    with pytest.raises(RuntimeError, match="Missing key"):
        poet.pack(cfg, {k: v for k, v in sd.items() if k != "linear.bias"})
    assert not any(k.endswith("linear2.weight") and not np.any(sd[k]) for k in sd)      # the toy's MLP is alive


def test_cli_flags_and_refusals(tmp_path):
    a = cli.parser().parse_args([])
    assert a.context_lengths == [6144, 12288, 24576] and a.seed == 188257 and a.batch_size == 8 and not a.relative_to_wt and a.DMS_index == 1
    pd.DataFrame({"mutant": ["A1G"], "DMS_score": [0.1]}).to_csv(tmp_path / "M.csv", index=False)
    pd.DataFrame([{"DMS_id": "M", "DMS_filename": "M.csv", "target_seq": "ACDE", "MSA_start": 1, "MSA_end": 4}]).to_csv(tmp_path / "ref.csv", index=False)
    base = ["--DMS_reference_file_path", str(tmp_path / "ref.csv"), "--DMS_data_folder", str(tmp_path), "--DMS_index", "0",
            "--output_scores_folder", str(tmp_path / "out"), "--MSA_folder", str(tmp_path)]
    with pytest.raises(SystemExit, match="no mutated_sequence column"):
        cli.main(base)
    pd.DataFrame({"mutated_sequence": ["ACDF"]}).to_csv(tmp_path / "M.csv", index=False)
    with pytest.raises(SystemExit, match=r"neither .*M\.a3m\.zst nor .*M\.a3m exists"):
        cli.main(base)
    (tmp_path / "M.a3m").write_bytes(b">x\nACDF\n")
    with pytest.raises(SystemExit, match="first MSA row"):
        cli.main(base)


@pytest.mark.parametrize("script,indels", [("scoring_PoET_substitutions.sh", False), ("scoring_PoET_indels.sh", True)])
def test_launchers_build_a_valid_command_line(script, indels, tmp_path):
    cfg_dir = tmp_path / "scripts"
    (cfg_dir / "scoring_DMS_zero_shot").mkdir(parents=True)
    (cfg_dir / "zero_shot_config.sh").write_text(
        'export DMS_data_folder_subs="/data/pg/subs/"\nexport DMS_data_folder_indels="/data/pg/indels/"\n'
        'export DMS_MSA_data_folder="/data/pg/msa/"\nexport DMS_reference_file_path_subs=../../reference_files/DMS_substitutions.csv\n'
        'export DMS_reference_file_path_indels=../../reference_files/DMS_indels.csv\n'
        'export DMS_output_score_folder_subs="/data/pg/out_subs/"\nexport DMS_output_score_folder_indels="/data/pg/out_indels/"\n')
    env = dict(os.environ, ZERO_SHOT_CONFIG=str(cfg_dir / "zero_shot_config.sh"), PGMI_LAUNCH_ECHO="1", DMS_index="7", checkpoint="/w/poet.ckpt")
    out = subprocess.run(["bash", os.path.join(os.path.dirname(HERE), "scripts", "scoring_DMS_zero_shot", script)], env=env,
                         capture_output=True, text=True, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr
    argv = out.stdout.strip().split("\n")
    assert argv[0] == "proteingym_amd.score_poet_proteingym"
    a = cli.parser().parse_args(argv[1:])
    assert a.DMS_index == 7 and a.checkpoint == "/w/poet.ckpt" and a.MSA_folder == "/data/pg/msa/" and a.context_lengths == [6144, 12288, 24576]
    assert a.DMS_reference_file_path.endswith("DMS_indels.csv" if indels else "DMS_substitutions.csv")
    assert os.path.normpath(a.output_scores_folder) == ("/data/pg/out_indels/PoET" if indels else "/data/pg/out_subs/PoET")
    if pr.reference_available():                                             # the reference's own parser takes the same line
        saved = sys.argv
        try:
            sys.argv = ["score.py"] + [x if x != a.output_scores_folder else str(tmp_path / "o") for x in argv[1:]]
            b = pr.score_module().parse_args()
        finally:
            sys.argv = saved
        assert b.DMS_index == 7 and b.context_lengths == a.context_lengths and b.batch_size == a.batch_size and b.seed == a.seed


# ---- pins to the live reference ------------------------------------------------------------------------------------------------
INIT_ARGS = dict(n_vocab=24, hidden_dim=128, ff_dim=256, num_layers=2, nhead=2, norm=True)


@needs_reference
@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-12), (torch.float32, 2e-5)])
def test_restatement_equals_the_live_reference(sd, g, dtype, tol):
    """Token log-probabilities of a prompt and of variants given it, and scores: tests/poet_ref.py against the reference's own layers.
    float64: rounding of two orders of the same sums; fp32: two fp32 evaluations, each ~1e-6 from float64 on these shapes."""
    model = pr.build_model(INIT_ARGS, sd, dtype)
    ref = poet_ref.PoetRef(poet.config_from_init_args(INIT_ARGS), sd, dtype)
    prompt = np.split(g["prompt_tokens_7"], np.cumsum(g["prompt_lens_7"])[:-1])
    lp, mem = ref.prompt(prompt)
    assert float(np.abs(lp - pr.tiered_forward(model, prompt)).max()) <= tol
    for s in ("ACDEFGHIKLMNPQRSTVWY", "MKV", "AXC"):
        v = poet.frame(s).astype(np.int64)
        assert float(np.abs(ref.variant_logprobs(v[:-1], mem) - pr.variant_logprobs(model, prompt, v[:-1])).max()) <= tol
        assert abs(ref.score(v, mem) - pr.score(model, prompt, v)) <= tol * len(v)
        assert abs(ref.score(v, None) - pr.score(model, [], v)) <= tol * len(v)       # memory=None: the variant alone


@needs_reference
def test_restatement_reproduces_the_recorded_member_scores(sd, g):
    ref = poet_ref.PoetRef(poet.config_from_init_args(INIT_ARGS), sd, torch.float64)
    variants = [poet.frame(s).astype(np.int64) for s in pd.read_csv(os.path.join(TOY, "TOY_POET.csv"))["mutated_sequence"]]
    prompt = np.split(g["prompt_tokens_3"], np.cumsum(g["prompt_lens_3"])[:-1])
    _, members = poet_ref.ensemble(ref, [prompt], variants)
    assert np.abs(members[0][0] - g["fwd_3"][:-1]).max() <= 1e-10 and np.abs(members[0][1] - g["bwd_3"][:-1]).max() <= 1e-10


@needs_reference
def test_encoder_reader_weights_and_sampling_equal_the_reference(msa_sequences, g):
    import pathlib
    sc, sampling, alphabet = pr.score_module(), pr.sampling(), pr.alphabet()
    every = bytes(range(256))
    assert np.array_equal(poet.encode(every), alphabet.encode(every))
    assert (alphabet.gap_token, alphabet.start_token, alphabet.stop_token, alphabet.mask_token) == (poet.GAP, poet.START, poet.STOP, poet.MASK)
    assert sc.get_seqs_from_fastalike(pathlib.Path(os.path.join(TOY, "TOY_POET.a3m"))) == msa_sequences
    msa = sc.get_encoded_msa_from_a3m_seqs(msa_sequences=msa_sequences, alphabet=alphabet)
    assert np.array_equal(msa, poet.encoded_msa(msa_sequences))
    n_eff, p = sampling.compute_homology_weights(ungapped_msa=msa, gap_token=alphabet.gap_token, hamming_csim_func=sampling.compute_hamming_csim_np,
                                                 can_use_torch=False)
    assert np.array_equal(p, poet.homology_weights(g["neighbors"]))
    for max_similarity in poet.SIMILARITY_CUTOFFS:
        sampler = sampling.MSASampler(method=sampling.NeighborsSampler(can_use_torch=False), max_similarity=max_similarity)
        idxs = sampler.get_sample_idxs(msa=msa, gap_token=alphabet.gap_token, seed=poet.SEED)
        assert np.array_equal(idxs, poet.sample_idxs(msa, p, max_similarity, poet.SEED))
        for budget in CONTEXT_LENGTHS:
            want = sc.sample_msa_sequences(get_sequence_fn=lambda ii: msa_sequences[ii].upper().translate(None, delete=b"-"), sample_idxs=idxs,
                                           max_tokens=budget, alphabet=alphabet, shuffle_seed=poet.SEED, truncate=False)
            got = poet.prompt_sequences(msa_sequences, idxs, budget, poet.SEED)
            assert len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want))


@needs_reference
def test_goldens_regenerate(tmp_path, g):
    sys.path.insert(0, os.path.join(HERE, "golden"))
    try:
        import make_golden_poet
    finally:
        sys.path.remove(os.path.join(HERE, "golden"))
    rec = make_golden_poet.generate(str(tmp_path))
    for name in ("TOY_POET.a3m", "TOY_POET.csv", "TOY_POET_REFERENCE.csv", "TOY_POET_scores.csv", "TOY_POET_scores_relative.csv"):
        assert open(tmp_path / name, "rb").read() == open(os.path.join(TOY, name), "rb").read(), name
    assert sorted(rec) == sorted(g.files)
    for k in g.files:
        assert np.array_equal(rec[k], g[k]) if rec[k].dtype.kind in "iu" else np.allclose(rec[k], g[k], rtol=0, atol=1e-10), k
    a = torch.load(tmp_path / "poet_toy.ckpt", weights_only=True)
    b = torch.load(os.path.join(TOY, "poet_toy.ckpt"), weights_only=True)
    assert a["hyper_parameters"] == b["hyper_parameters"] and a["state_dict"].keys() == b["state_dict"].keys()
    assert all(torch.equal(a["state_dict"][k], b["state_dict"][k]) for k in a["state_dict"])
