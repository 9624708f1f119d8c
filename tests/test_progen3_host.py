"""ProGen3's host side without a GPU: the token table and both directions' ids against the recording, the float64 restatement of
tests/progen3_ref.py (what the GPU tests compare against) against the recorded reference, the scoring plan and the combine against the
recorded scores, both checkpoint layouts, the refusals, the CLI's file read by the reference's merge.py; and, where the reference tree
exists, the restatement's attention and expert block pinned to the LIVE reference's own layers in float64 (1e-12) and the recorded
scores regenerated."""
import ctypes as C
import json
import os

import numpy as np
import pandas as pd
import pytest

import progen3_ref as R
import progen3_reference as pr
from proteingym_amd import _lib, progen3 as pg3, score_progen3_proteingym as cli
from proteingym_amd.causal_lm import get_mutated_sequence

HERE = os.path.dirname(os.path.abspath(__file__))
TOY = os.path.join(HERE, "golden", "ProGen3_toy")
needs_reference = pytest.mark.skipif(not pr.reference_available(), reason="the reference tree is not on this machine")


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(TOY, "golden_progen3.npz"))


@pytest.fixture(scope="module")
def toys():
    """name -> (cfg, fp32 state dict) of the two eager toy checkpoints."""
    out = {}
    for name in "AB":
        c, sd = pg3.load_directory(os.path.join(TOY, name))
        out[name] = (pg3.config_from_json(c), {k: np.asarray(v, np.float32) for k, v in sd.items()})
    return out


@pytest.fixture(scope="module")
def restated(g, toys):
    """(name, direction) -> per fixture sequence (ids, float64 log-probs, routers)."""
    return {(name, tag): [(ids,) + R.forward(toys[name][1], toys[name][0], ids) for ids in (pg3.encode(s, rev) for s in g["sequences"])]
            for name in "AB" for tag, rev in (("fwd", False), ("rev", True))}


def assay_sequences(kind):
    dms = pd.read_csv(os.path.join(TOY, f"TOY_PG3_{kind.upper()}.csv"))
    target = pd.read_csv(os.path.join(TOY, "TOY_PG3_REFERENCE.csv"))["target_seq"][0]
    return list(dms["mutated_sequence"]) if kind == "indel" else [get_mutated_sequence(target, m) for m in dms["mutant"]]


# ---- tokenisation ----------------------------------------------------------------------------------------------------------
def test_token_table_is_the_tokenizers(g):
    t = json.load(open(os.path.join(TOY, "tokenizer.json")))
    assert t["model"]["vocab"] == pg3.TOKENS and max(pg3.TOKENS.values()) == 33
    added = {a["content"]: a["id"] for a in t["added_tokens"]}
    assert all(added[k] == v for k, v in pg3.SPECIALS.items())
    assert max(added.values()) + 1 == pg3.TOKENIZER_VOCAB == 134 and t["padding"]["pad_id"] == pg3.PAD_ID
    assert pg3.encode("ACY").tolist() == [1, 6, 8, 10, 32, 7, 2] and pg3.encode("ACY", reverse=True).tolist() == [1, 7, 32, 10, 8, 6, 2]
    for bad in ("", "acd", "AC-D", "AC[GLM]0-1-1"):
        with pytest.raises(ValueError, match="amino-acid sequence"):
            pg3.encode(bad)


def test_ids_of_both_directions_match_the_recording(g):
    for tag, rev in (("fwd", False), ("rev", True)):
        rec = g[f"ids_{tag}"]
        for b, s in enumerate(g["sequences"]):
            ids = pg3.encode(str(s), rev)
            assert np.array_equal(ids, rec[b, :len(ids)]) and (rec[b, len(ids):] == pg3.PAD_ID).all()


def test_ids_match_the_tokenizers_library(g):
    tokenizers = pytest.importorskip("tokenizers")
    tok = tokenizers.Tokenizer.from_file(os.path.join(TOY, "tokenizer.json"))
    for s in list(g["sequences"]) + ["ABCDEFGHIJKLMNOPQRSTUVWXYZ"]:
        for rev in (False, True):
            body = "1" + str(s) + "2"
            assert tok.encode("<bos>" + (body[::-1] if rev else body) + "<eos>").ids == pg3.encode(str(s), rev).tolist()


# ---- the restatement against the recording ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B"])
def test_restatement_matches_the_recorded_reference(g, restated, name):
    """Log-probs within 2e-5 (the recording is fp32: its own rounding through two layers and a 134-column log-softmax of |values| < 10),
    router probabilities within 2e-6, chosen experts equal, and the router-gap condition the fixtures were made under."""
    for tag in ("fwd", "rev"):
        T = g[f"ids_{tag}"].shape[1]
        for b, (ids, lp, routers) in enumerate(restated[name, tag]):
            assert np.abs(lp - g[f"{name}_logprobs_{tag}"][b, :len(ids)]).max() <= 2e-5
            for layer, (p, chosen) in enumerate(routers):
                rows = slice(b * T, b * T + len(ids))
                assert np.abs(p - g[f"{name}_router_{tag}"][layer, rows]).max() <= 2e-6
                assert np.array_equal(chosen, g[f"{name}_experts_{tag}"][layer, rows])
                assert R.router_gap(p, chosen.shape[1]) >= R.GAP - 2e-6


# ---- scoring plan and combine ----------------------------------------------------------------------------------------------
def test_group_by_length_is_the_reference_scorers():
    seqs = ["A" * n for n in (5, 3, 9, 3, 7, 9)]
    assert pg3.group_by_length(seqs, 65536) == [[1, 3, 0, 4, 2, 5]]
    assert pg3.group_by_length(seqs, 12) == [[1, 3], [0], [4], [2], [5]]          # 3 * 2 <= 12 < 5 * 3: the batch closes before the length-5 one
    assert pg3.group_by_length(seqs, 1) == [[1], [3], [0], [4], [2], [5]]       # a batch always takes one sequence
    plan = pg3.scoring_plan(["AC", "D"])
    assert [(i, rev) for i, rev, _ in plan] == [(0, False), (0, True), (1, False), (1, True)]
    assert plan[1][2].tolist() == [1, 7, 10, 8, 6, 2]


@pytest.mark.parametrize("name", ["A", "B"])
def test_plan_and_combine_reproduce_the_recorded_scores(toys, name):
    """The host arithmetic on the restatement's log-probs: per pass the sum of the fp32 target terms, then combine()."""
    cfg, sd = toys[name]
    for kind in ("sub", "indel"):
        seqs = assay_sequences(kind)
        plan = pg3.scoring_plan(seqs)
        sums = [float(np.sum(R.forward(sd, cfg, ids)[0][np.arange(len(ids) - 1), ids[1:]].astype(np.float32).astype(np.float64))) for _, _, ids in plan]
        ll, ppl = pg3.combine(len(seqs), plan, sums, [len(ids) - 1 for _, _, ids in plan])
        rec = pd.read_csv(os.path.join(TOY, f"scores_{name}_{kind}.csv"))
        assert np.abs(ll - rec["log_likelihood"]).max() <= 2e-5 and np.allclose(ppl, rec["perplexity"], rtol=5e-5)
        assert ll.dtype == np.float64 and np.array_equal(ll, ll.astype(np.float32))      # fp32 values, as .item() returns them
    ll, ppl = pg3.combine(1, [(0, False, None), (0, True, None)], [-6.0, -9.0], [3, 3])
    assert ll.tolist() == [-2.5] and ppl[0] == float(np.exp(np.float32(2.5)))


# ---- checkpoints -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B"])
def test_both_expert_layouts_load_to_the_same_blob(name):
    cfg_e, blob_e = pg3.load_checkpoint(os.path.join(TOY, name))
    cfg_m, blob_m = pg3.load_checkpoint(os.path.join(TOY, name + "_megablocks"))
    assert cfg_e == cfg_m and blob_e.dtype == np.float32 and np.array_equal(blob_e, blob_m)
    assert blob_e.size == pg3.weight_count(cfg_e)
    c, sd = pg3.load_directory(os.path.join(TOY, name))
    assert pg3.expert_layout(sd) == "eager" and pg3.expert_layout(pg3.load_directory(os.path.join(TOY, name + "_megablocks"))[1]) == "megablocks"
    # the blob's documented order: the folded embedding inputs first, the head last
    V, D = cfg_e["vocab"], cfg_e["embed_dim"]
    assert np.array_equal(blob_e[:V * D].reshape(V, D), np.asarray(sd["model.embed_tokens.weight"], np.float32))
    assert np.array_equal(blob_e[V * D:V * D + D], np.asarray(sd["model.embed_seq_id.weight"], np.float32)[0])
    assert np.array_equal(blob_e[-V * D:].reshape(V, D), np.asarray(sd["lm_head.weight"], np.float32))


def test_library_counts_the_same_blob(lib):
    for name in "AB":
        cfg, blob = pg3.load_checkpoint(os.path.join(TOY, name))
        c = _lib.Config(abi_version=_lib.ABI_VERSION, arch=_lib.ARCH_PROGEN3, layers=cfg["layers"], embed_dim=cfg["embed_dim"], heads=cfg["heads"],
                        ffn_dim=cfg["ffn_dim"], vocab=cfg["vocab"], max_positions=cfg["max_positions"], precision=_lib.PREC_F16X3)
        p = _lib.Pg3Params(kv_heads=cfg["kv_heads"], n_experts=cfg["n_experts"], top_k=cfg["top_k"], gated=int(cfg["gated"]), rope_theta=cfg["rope_theta"])
        assert lib.pgmi_pg3_weight_count(C.byref(c), C.byref(p)) == blob.size
        assert lib.pgmi_weight_count(C.byref(c)) == -1


def test_refusals(lib, toys):
    base = json.load(open(os.path.join(TOY, "A", "config.json")))
    with pytest.raises(ValueError, match="head_dim 32"):
        pg3.config_from_json(dict(base, num_attention_heads=4))
    with pytest.raises(ValueError, match="hidden_act 'gelu'"):
        pg3.config_from_json(dict(base, hidden_act="gelu"))
    with pytest.raises(ValueError, match="clip_qkv"):
        pg3.config_from_json(dict(base, clip_qkv=8.0))
    cfg, sd = toys["A"]
    odd = {k.replace("experts.0.", "experts.expert_0.").replace("experts.mlp.", "experts.glu."): v for k, v in sd.items()}
    with pytest.raises(ValueError, match="unrecognised ProGen3 expert layout.*accept_real_weights"):
        pg3.pack(dict(cfg), odd)
    # the library's own refusals, with the number in the message (no device is touched before them)
    def create(cfg_over=None, **params):
        c = dict(abi_version=_lib.ABI_VERSION, arch=_lib.ARCH_PROGEN3, layers=1, embed_dim=128, heads=2, ffn_dim=192, vocab=134, max_positions=64,
                 precision=_lib.PREC_F16X3)
        c.update(cfg_over or {})
        p = dict(kv_heads=1, n_experts=4, top_k=2, gated=1, rope_theta=1e5)
        p.update(params)
        h = C.c_void_p()
        rc = lib.pgmi_pg3_model_create(C.byref(_lib.Config(**c)), C.byref(_lib.Pg3Params(**p)), None, 0, 0, C.byref(h))
        return rc, lib.pgmi_last_error().decode()
    rc, msg = create(dict(heads=4))
    assert rc == _lib.EINVAL and "head_dim 32" in msg
    rc, msg = create(clip_qkv=8.0)
    assert rc == _lib.EINVAL and "clip_qkv = 8" in msg
    rc, msg = create(kv_heads=3)
    assert rc == _lib.EINVAL and "num_key_value_heads 3" in msg
    rc, msg = create(n_experts=65)
    assert rc == _lib.EINVAL and "65 experts" in msg
    rc, msg = create(dict(vocab=33))
    assert rc == _lib.EINVAL and "vocab" in msg
    rc, msg = create()
    assert rc == _lib.EINVAL and "weight blob has 0 elements" in msg


# ---- the CLI ---------------------------------------------------------------------------------------------------------------
class _RestatedModel:
    """Stands in for the device model behind the CLI: ProGen3Model.score's host arithmetic on the float64 restatement."""

    def __init__(self, d):
        c, sd = pg3.load_directory(d)
        self.cfg, self.sd = pg3.config_from_json(c), {k: np.asarray(v, np.float32) for k, v in sd.items()}

    def sequence_loglik(self, rows):
        out = [R.forward(self.sd, self.cfg, ids)[0][np.arange(len(ids) - 1), ids[1:]].astype(np.float32).astype(np.float64).sum() for ids in rows]
        return np.array(out), np.array([len(r) - 1 for r in rows], np.int32)

    score = pg3.ProGen3Model.score

    def close(self):
        pass


@pytest.mark.parametrize("kind", ["sub", "indel"])
def test_cli_writes_the_columns_merge_reads(tmp_path, monkeypatch, kind):
    monkeypatch.setattr(pg3, "from_pretrained", lambda d, device=0, max_rows=0: _RestatedModel(d))
    argv = ["--Progen3_model_name_or_path", os.path.join(TOY, "A"), "--DMS_reference_file_path", os.path.join(TOY, "TOY_PG3_REFERENCE.csv"),
            "--DMS_data_folder", TOY, "--DMS_index", "0" if kind == "sub" else "1", "--output_scores_folder", str(tmp_path / "Progen3" / "339m")]
    out = cli.main(argv + (["--indel_mode", "--max_batch_tokens", "64"] if kind == "indel" else []))
    got, rec = pd.read_csv(out), pd.read_csv(os.path.join(TOY, f"scores_A_{kind}.csv"))
    assert os.path.basename(out) == f"TOY_PG3_{kind.upper()}.csv"
    assert list(got.columns) == ["mutant", "log_likelihood", "perplexity", "DMS_score"] and list(got["mutant"]) == list(rec["mutant"])
    assert np.abs(got["log_likelihood"] - rec["log_likelihood"]).max() <= 2e-5
    if kind == "indel" or not pr.reference_available():
        return
    # the reference's own merge.py with its own registry row for this family
    import importlib.util
    import sys
    from oracle.ref_harness import REF_ROOT
    registry = json.load(open(os.path.join(REF_ROOT, "config.json")))["model_list_zero_shot_substitutions_DMS"]
    assert registry["Progen3_339m"]["input_score_name"] == "log_likelihood" and registry["Progen3_339m"]["key"] == "mutant"
    json.dump({"model_list_zero_shot_substitutions_DMS": {"Progen3_339m": registry["Progen3_339m"]}}, open(tmp_path / "config.json", "w"))
    assert registry["Progen3_339m"]["location"] == "Progen3/339m"
    spec = importlib.util.spec_from_file_location("pg_reference_merge_pg3", os.path.join(REF_ROOT, "proteingym", "merge.py"))
    merge = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(merge)
    ref_one = tmp_path / "ref.csv"
    pd.read_csv(os.path.join(TOY, "TOY_PG3_REFERENCE.csv")).iloc[:1].assign(DMS_total_number_mutants=len(got)).to_csv(ref_one, index=False)
    monkeypatch.setattr(sys, "argv", ["merge.py", "--DMS_assays_location", TOY, "--model_scores_location", str(tmp_path),
                                      "--DMS_reference_file", str(ref_one), "--config_file", str(tmp_path / "config.json")])
    merge.main()
    merged = pd.read_csv(tmp_path / "merged_scores" / "TOY_PG3_SUB.csv")
    assert list(merged["mutant"]) == list(got["mutant"]) and np.allclose(merged["Progen3_339m"], got["log_likelihood"])


# ---- pins to the live reference --------------------------------------------------------------------------------------------
@needs_reference
@pytest.mark.parametrize("name", ["A", "B"])
def test_restatement_is_pinned_to_the_live_reference_layers(toys, name):
    """The reference's own Attention and SparseMoeBlock modules in float64 against the restatement's functions (1e-12), on rows of the
    scale the layers see; the rotary tables are the module's own (the restatement's numpy tables against them: 1e-6)."""
    import torch
    cfg, sd = toys[name]
    config = pr.make_config(**{k: v for k, v in json.load(open(os.path.join(TOY, name, "config.json"))).items()
                               if k not in ("model_type", "moe_implementation", "torch_dtype")})
    mods = pr._load()
    rng = np.random.default_rng(3)
    T, D = 19, cfg["embed_dim"]
    h = rng.standard_normal((T, D))
    p = "model.layers.1."
    att = mods["attention"].Attention(config, 1).double()
    att.load_state_dict({k[len(p + "self_attn."):]: torch.from_numpy(v).double() for k, v in sd.items() if k.startswith(p + "self_attn.")})
    with torch.no_grad():
        want = att(torch.from_numpy(h)[None], torch.arange(T)[None])[0][0].numpy()
    cos, sin = att.rotary_emb.cos_cached[:T].numpy(), att.rotary_emb.sin_cached[:T].numpy()
    mine = R.rotary_tables(T, D // cfg["heads"], cfg["rope_theta"])
    assert np.abs(mine[0] - cos).max() <= 1e-6 and np.abs(mine[1] - sin).max() <= 1e-6
    w = [sd[p + f"self_attn.{n}_proj.weight"].astype(np.float64) for n in "qkvo"]
    got = R.attention(h, *w, cfg["heads"], cfg["kv_heads"], cos.astype(np.float64), sin.astype(np.float64))
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    moe = mods["moe"].SparseMoeBlock(config).double()
    m = p + "block_sparse_moe."
    moe.load_state_dict({k[len(m):]: torch.from_numpy(v).double() for k, v in sd.items() if k.startswith(m)})
    with torch.no_grad():
        want, probs = moe(torch.from_numpy(h)[None])
    E = cfg["n_experts"]
    w1 = np.stack([sd[m + f"experts.{e}.w1.weight"] for e in range(E)])
    w3 = np.stack([sd[m + f"experts.{e}.w3.weight"] for e in range(E)]) if cfg["gated"] else None
    w2 = np.stack([sd[m + f"experts.{e}.w2.weight"] for e in range(E)])
    got, pmine, _, _ = R.moe_block(h, sd[m + "gate.weight"], w1, w3, w2, cfg["top_k"], cfg["gated"])
    # the reference's router softmax is fp32 by construction (logits_to_probs(dtype=float32)) even in a float64 module, so the block as a
    # whole agrees to fp32 rounding of the weights only; its experts, which carry all the other arithmetic, agree to 1e-12
    assert np.abs(pmine - probs.numpy()).max() <= 1e-6
    assert np.abs(got - want[0].numpy()).max() <= 1e-6 * max(1.0, np.abs(got).max())
    for e in range(E):
        with torch.no_grad():
            want_e = moe.experts[e](torch.from_numpy(h)).numpy()
        got_e = R.expert(h, w1[e].astype(np.float64), w3[e].astype(np.float64) if cfg["gated"] else None, w2[e].astype(np.float64), cfg["gated"])
        assert np.abs(got_e - want_e).max() <= 1e-12 * max(1.0, np.abs(want_e).max())
    x = rng.standard_normal((5, D)).astype(np.float32)
    nw = sd[p + "input_layernorm.weight"]
    with torch.no_grad():
        want = mods["modeling"].RMSNorm(D, eps=cfg["ln_eps"])
        want.weight.copy_(torch.from_numpy(nw))
        want = want(torch.from_numpy(x)).numpy()
    assert np.abs(R.rmsnorm(x.astype(np.float64), nw.astype(np.float64), cfg["ln_eps"]) - want).max() <= 2e-6


@needs_reference
def test_recorded_scores_come_from_the_live_reference(toys):
    import torch
    cfg, sd = toys["A"]
    config = pr.make_config(**{k: v for k, v in json.load(open(os.path.join(TOY, "A", "config.json"))).items()
                               if k not in ("model_type", "moe_implementation", "torch_dtype")})
    model = pr.build_model(config, 0)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    ll, ppl = pr.score(model, assay_sequences("indel"))
    rec = pd.read_csv(os.path.join(TOY, "scores_A_indel.csv"))
    assert np.abs(ll - rec["log_likelihood"]).max() <= 1e-6 and np.allclose(ppl, rec["perplexity"], rtol=1e-6)
    assert pg3.group_by_length(assay_sequences("indel"), 30) == [[i for i, _ in b] for b in
                                                                 pr._load()["scorer"].ProGen3Scorer(model, max_batch_tokens=30).group_by_length(list(enumerate(assay_sequences("indel"))))]


# ---- the launchers ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("script", ["scoring_Progen3_substitutions.sh", "scoring_Progen3_indels.sh"])
def test_launchers_build_a_command_line_the_cli_parses(script, tmp_path):
    """The launchers source a zero_shot_config.sh written in ProteinGym's variable names; what they pass parses with the CLI's parser."""
    import subprocess
    root = os.path.dirname(HERE)
    cfg_dir = tmp_path / "scripts"
    (cfg_dir / "scoring_DMS_zero_shot").mkdir(parents=True)
    (tmp_path / "reference_files").mkdir()
    (cfg_dir / "zero_shot_config.sh").write_text(
        'export PROTEINGYM_CACHE="/data/pg"\n'
        'export DMS_data_folder_subs="${PROTEINGYM_CACHE}/DMS_ProteinGym_substitutions/"\n'
        'export DMS_data_folder_indels="${PROTEINGYM_CACHE}/DMS_ProteinGym_indels/"\n'
        'export DMS_reference_file_path_subs=../../reference_files/DMS_substitutions.csv\n'
        'export DMS_reference_file_path_indels=../../reference_files/DMS_indels.csv\n'
        'export DMS_output_score_folder_subs="${PROTEINGYM_CACHE}/zero_shot_substitutions_scores/"\n'
        'export DMS_output_score_folder_indels="${PROTEINGYM_CACHE}/zero_shot_indels_scores/"\n')
    env = dict(os.environ, ZERO_SHOT_CONFIG=str(cfg_dir / "zero_shot_config.sh"), PGMI_LAUNCH_ECHO="1", DMS_index="7",
               Progen3_model_name_or_path="/ckpt/progen3-762m", Progen3_size="762m")
    out = subprocess.run(["bash", os.path.join(root, "scripts", "scoring_DMS_zero_shot", script)], env=env, capture_output=True, text=True, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr
    argv = out.stdout.strip().split("\n")
    assert argv[0] == "proteingym_amd.score_progen3_proteingym"
    a = cli.parser().parse_args(argv[1:])
    indels = "indels" in script
    assert a.DMS_index == 7 and bool(a.indel_mode) == indels and a.max_batch_tokens == 65536 and a.Progen3_model_name_or_path == "/ckpt/progen3-762m"
    assert os.path.isabs(a.DMS_reference_file_path) and a.DMS_reference_file_path.endswith("DMS_indels.csv" if indels else "DMS_substitutions.csv")
    assert a.output_scores_folder == f"/data/pg/zero_shot_{'indels' if indels else 'substitutions'}_scores//Progen3/762m"   # merge.py: location Progen3/<size>
