"""CARP host code (proteingym_amd/carp.py, score_carp_proteingym.py) on the CPU: the checkpoint's key map and shapes, the parameter
count, the refusals, the token-table fold and the convolution weight permutation against the float64 restatement (tests/carp_ref.py --
sequence_models is not installed here, so the live reference produced no value in this file), the dilation schedule, the scoring rules
and the CLI's files on the toy assay of tests/golden/CARP_toy (recipe: tests/golden/make_golden_carp.py)."""
import os

import numpy as np
import pandas as pd
import pytest
import torch

import carp_ref as R
from proteingym_amd import _lib, carp, score_carp_proteingym as cli

TOY = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "CARP_toy")
TARGET = "MKVLAAGIVRHDESTNQCGPAVIFYWLMKRHDESTNQ"


@pytest.fixture(scope="module")
def toy():
    return torch.load(os.path.join(TOY, "carp_toy.pt"), map_location="cpu", weights_only=False)


@pytest.fixture(scope="module")
def expected():
    return np.load(os.path.join(TOY, "expected.npz"))


def test_alphabet_and_tokens():
    assert carp.PROTEIN_ALPHABET == R.ALPHABET and len(carp.PROTEIN_ALPHABET) == 30
    assert carp.PROTEIN_ALPHABET[:20] == "ACDEFGHIKLMNPQRSTVWY" and carp.MASK_ID == R.MASK_ID == carp.PROTEIN_ALPHABET.index("#")
    t = carp.tokenize("ACY")
    assert t.tolist() == [0, 1, 19] and t.dtype == np.int32                   # L letters are L tokens: no start, no stop
    with pytest.raises(ValueError, match="alphabet"):
        carp.tokenize("A1C")


# the four published shapes; tiny layer counts at the two wide ones
@pytest.mark.parametrize("name,layers", [("carp_600k", 16), ("carp_38M", 2), ("carp_76M", 2), ("carp_640M", 1)])
def test_key_map_and_shapes(name, layers):
    D, _, slim = carp.CHECKPOINT_SHAPES[name]
    ck = carp.random_checkpoint(3, D, layers, slim, name=name)
    spec = carp.check_checkpoint(ck)
    H = D // 2 if slim else D
    assert (spec.d_model, spec.d_hidden, spec.n_layers, spec.kernel_size, spec.r, spec.vocab, spec.slim) == (D, H, layers, 5, 128, 30, slim)
    assert H in (64, 512, 1280)
    sd = ck["model_state_dict"]
    b = carp.block_keys(layers - 1)
    assert b["conv"] == f"embedder.layers.{layers - 1}.conv" and b["ln2"].endswith("sequence1.3") and b["pff2"].endswith("sequence2.2.conv")
    assert sd[b["pff1"] + ".weight"].shape == (H, D, 1) and sd[b["conv"] + ".weight"].shape == (H, H, 5)
    assert sum(v.size for v in sd.values()) == carp.param_count(D, layers, slim)
    blob = carp.blob_from_state(sd, spec)
    assert blob.dtype == np.float32
    # the blob replaces the 8-wide embedding and its up-projection by the folded [V][D] table
    assert blob.size == carp.param_count(D, layers, slim) - (30 * 8 + 8 * D + D) + 30 * D
    assert R.n_blocks(sd) == layers


def test_parameter_counts_match_the_checkpoint_names():
    assert carp.param_count(128, 16, True) == 607630
    assert round(carp.param_count(1024, 16, True) / 1e5) == 379 and round(carp.param_count(1024, 32, True) / 1e5) == 757
    assert carp.param_count(1280, 56, False) // 100000 == 6429 and round(carp.param_count(1280, 56, True) / 1e6) == 207


def test_dilation_schedule():
    assert carp.dilation_schedule(10) == [1, 2, 4, 8, 16, 32, 64, 128, 1, 2] == R.dilations(10)
    assert carp.dilation_schedule(3, r=2) == [1, 2, 1]


def _ck(**over):
    ck = carp.random_checkpoint(5, 64, 2, True, name="carp_x")
    ck.update(over)
    return ck


@pytest.mark.parametrize("over,match", [
    ({"model": "mif"}, "MIF"), ({"model": "mif-st"}, "MIF"), ({"model": "carp_big"}, "big"), ({"big": True}, "big"),
    ({"causal": True}, "causal"), ({"rank": 16}, "rank"), ({"activation": "relu"}, "relu"), ({"model": "bytenet"}, "not a CARP"),
    ({"d_model": 128}, "d_model"), ({"n_layers": 3}, "n_layers"), ({"slim": False}, "slim"), ({"kernel_size": 3}, "kernel_size"),
    ({"r": 96}, "power of two")])
def test_refusals(over, match):
    with pytest.raises(_lib.PgmiError, match=match):
        carp.check_checkpoint(_ck(**over))


def test_refuses_wrong_alphabet_length_missing_and_extra_tensors():
    ck = _ck()
    ck["model_state_dict"][carp.K_EMBED] = np.zeros((31, 8), np.float32)
    with pytest.raises(_lib.PgmiError, match="31 rows, the alphabet has 30"):
        carp.check_checkpoint(ck)
    ck = _ck()
    del ck["model_state_dict"]["embedder.layers.1.sequence1.3.bias"]
    with pytest.raises(_lib.PgmiError, match="sequence1.3.bias"):
        carp.check_checkpoint(ck)
    ck = _ck()
    ck["model_state_dict"]["embedder.layers.0.sequence1.2.conv.weight"] = np.zeros((32, 16, 1), np.float32)      # a factorised PFF
    with pytest.raises(_lib.PgmiError, match="shape"):
        carp.check_checkpoint(ck)
    ck = _ck()
    ck["model_state_dict"]["embedder.layers.0.gnn.weight"] = np.zeros(3, np.float32)
    with pytest.raises(_lib.PgmiError, match="does not have"):
        carp.check_checkpoint(ck)


def test_checkpoint_resolution(tmp_path):
    with pytest.raises(_lib.PgmiError, match="carp_640M.pt"):
        carp.resolve_checkpoint("CARP_640M", str(tmp_path))                    # no download: the missing file is named
    with pytest.raises(_lib.PgmiError, match="MIF"):
        carp.resolve_checkpoint("mif", str(tmp_path))
    with pytest.raises(_lib.PgmiError, match="not found"):
        carp.resolve_checkpoint(str(tmp_path / "x.pt"), None)
    assert carp.resolve_checkpoint("carp_toy", TOY) == os.path.join(TOY, "carp_toy.pt")
    assert carp.resolve_checkpoint(os.path.join(TOY, "carp_toy.pt"), None) == os.path.join(TOY, "carp_toy.pt")
    ck = carp.read_checkpoint(os.path.join(TOY, "carp_toy.pt"))
    assert carp.check_checkpoint(ck).d_hidden == 32
    torch.save({"x": 1}, tmp_path / "bad.pt")
    with pytest.raises(_lib.PgmiError, match="model_state_dict"):
        carp.read_checkpoint(str(tmp_path / "bad.pt"))


def test_token_table_fold_and_conv_permutation(toy):
    sd = toy["model_state_dict"]
    table = carp.fold_token_table(sd)
    tok = np.arange(30)
    x = torch.nn.functional.conv1d(torch.nn.functional.embedding(torch.as_tensor(tok)[None], sd[carp.K_EMBED].double()).transpose(1, 2),
                                   sd[carp.K_UP_W].double(), sd[carp.K_UP_B].double())[0].transpose(0, 1).numpy()
    assert table.dtype == np.float64 and np.abs(table - x).max() <= 1e-14
    assert np.abs(table[carp.MASK_ID] - sd[carp.K_UP_B].double().numpy()).max() == 0      # the zero padding row leaves the bias
    # the permuted weight [out][tap][in] as the implicit GEMM reads it: per segment, zero beyond both ends, no neighbour's rows
    rng = np.random.default_rng(0)
    Cc, seg = 32, np.array([0, 5, 42, 43, 173, 176])
    w = rng.normal(0, 1, (Cc, Cc, 5))
    wp = carp.permute_conv_weight(w)
    assert wp.shape == (Cc, 5, Cc) and wp.flags["C_CONTIGUOUS"] and wp[3, 4, 7] == w[3, 7, 4]
    x, bias = rng.normal(0, 1, (176, Cc)), rng.normal(0, 1, Cc)
    for dil in (1, 2, 16, 128):
        got = np.tile(bias, (176, 1))
        for s in range(5):
            for m in range(seg[s], seg[s + 1]):
                for j in range(5):
                    src = m + (j - 2) * dil
                    if seg[s] <= src < seg[s + 1]:
                        got[m] += wp[:, j, :] @ x[src]
        assert np.abs(got - R.conv_segments(x, w, bias, seg, dil)).max() <= 1e-12
        leak = np.tile(bias, (176, 1))
        for m in range(176):
            for j in range(5):
                if 0 <= m + (j - 2) * dil < 176:
                    leak[m] += wp[:, j, :] @ x[m + (j - 2) * dil]
        assert np.abs(leak - got).max() > 5                                     # a version that ignores the bounds is far off
    blob = carp.blob_from_state(sd, carp.check_checkpoint(toy))
    assert np.array_equal(blob[:30 * 64], table.astype(np.float32).ravel())
    o = 30 * 64 + 2 * 64 + 32 * 64 + 32 + 2 * 32
    assert np.array_equal(blob[o:o + 32 * 5 * 32], carp.permute_conv_weight(sd["embedder.layers.0.conv.weight"]).ravel())


def test_mean_rule_offset_and_wildtype_check(toy, expected):
    lp = expected["masked_lp"]
    row_of = dict(enumerate(lp))
    subs = carp.parse_mutant("M1A:A5C", TARGET)
    assert subs == [(0, "M", "A"), (4, "A", "C")]
    a = lp[0][carp.PROTEIN_ALPHABET.index("A")] - lp[0][carp.PROTEIN_ALPHABET.index("M")]
    b = lp[4][carp.PROTEIN_ALPHABET.index("C")] - lp[4][carp.PROTEIN_ALPHABET.index("A")]
    assert carp.mean_substitution_score(subs, row_of) == pytest.approx((a + b) / 2, abs=1e-15)         # the mean, not the sum
    assert carp.mean_substitution_score(subs, row_of) == pytest.approx(R.label_row("M1A:A5C", TARGET, lp), abs=1e-15)
    assert carp.parse_mutant("M11A", TARGET, offset_idx=11) == [(0, "M", "A")]
    with pytest.raises(ValueError, match="wildtype"):
        carp.parse_mutant("K1A", TARGET)
    with pytest.raises(ValueError, match="wildtype"):
        carp.parse_mutant("Q38A", TARGET)
    assert carp.get_mutated_sequence(TARGET, "M1A:A5C") == "A" + TARGET[1:4] + "C" + TARGET[5:]
    model = R.RestatedModel(toy)
    mutants = list(pd.read_csv(os.path.join(TOY, "TOY_CARP.csv"))["mutant"])
    got = carp.masked_marginal_scores(model, TARGET, mutants)                  # touched positions only: the same scores
    assert np.abs(got - expected["mm_scores"]).max() <= 1e-12
    got = carp.pseudo_likelihood_scores(model, [carp.get_mutated_sequence(TARGET, m) for m in mutants])
    assert np.abs(got - expected["pl_scores"]).max() <= 1e-12


def cli_argv(out, perf, index, *extra):
    return ["--model_name", "carp_toy", "--model_path", TOY, "--DMS_reference_file_path", os.path.join(TOY, "reference.csv"),
            "--DMS_data_folder", TOY, "--DMS_index", str(index), "--output_scores_folder", out, "--performance_file", perf,
            "--structure_data_folder", "ignored", *extra]


def test_cli_writes_the_reference_files(tmp_path, monkeypatch):
    seen = []

    def fake(path, device=0, precision="f16x3", max_rows=0):
        seen.append(path)
        return R.RestatedModel(torch.load(path, map_location="cpu", weights_only=False))

    monkeypatch.setattr(carp, "from_pretrained", fake)
    exp = np.load(os.path.join(TOY, "expected.npz"))
    out, perf = str(tmp_path / "scores"), str(tmp_path / "perf.csv")
    runs = [((0,), "TOY_CARP", "mm_scores"), ((0, "--fitness_computation_mode", "pseudo_likelihood"), "TOY_CARP", "pl_scores"),
            ((1, "--fitness_computation_mode", "pseudo_likelihood", "--indel_mode"), "TOY_CARP_INDELS", "indel_scores")]
    for argv, dms, key in runs:
        fn = cli.main(cli_argv(out, perf, *argv))
        assert fn == out + os.sep + "carp_toy" + os.sep + dms + ".csv" and seen[-1] == os.path.join(TOY, "carp_toy.pt")
        got, src = pd.read_csv(fn), pd.read_csv(os.path.join(TOY, dms + ".csv"))
        assert list(got.columns) == ["mutant", "carp_toy_score", "DMS_score"]
        assert list(got["mutant"]) == list(src["mutant"]) and np.array_equal(got["DMS_score"], src["DMS_score"])
        assert np.abs(got["carp_toy_score"] - exp[key]).max() <= 1e-12
    lines = open(perf).read().splitlines()
    assert lines[0] == "DMS_id,spearman" and [ln.split(",")[0] for ln in lines[1:]] == ["TOY_CARP", "TOY_CARP", "TOY_CARP_INDELS"]
    rho = pd.Series(exp["mm_scores"]).corr(pd.read_csv(os.path.join(TOY, "TOY_CARP.csv"))["DMS_score"], method="spearman")
    assert float(lines[1].split(",")[1]) == pytest.approx(rho, abs=1e-12)
    with pytest.raises(_lib.PgmiError, match="MIF"):
        cli.main(cli_argv(out, perf, 0)[2:] + ["--model_name", "mif"])
    with pytest.raises(_lib.PgmiError, match="indel_mode"):
        cli.main(cli_argv(out, perf, 1, "--indel_mode"))


def test_launcher_builds_a_command_line_the_cli_parses(tmp_path):
    """The launcher of the reference's name reads zero_shot_config.sh and passes the reference's flags."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg_dir = tmp_path / "scripts"
    (cfg_dir / "scoring_DMS_zero_shot").mkdir(parents=True)
    (cfg_dir / "zero_shot_config.sh").write_text(
        'export DMS_data_folder_subs="/data/pg/subs/"\nexport DMS_reference_file_path_subs=../../reference_files/DMS_substitutions.csv\n'
        'export DMS_output_score_folder_subs="/data/pg/out_subs"\n')
    env = dict(os.environ, ZERO_SHOT_CONFIG=str(cfg_dir / "zero_shot_config.sh"), PGMI_LAUNCH_ECHO="1", DMS_index="7", model_path="/w/carp",
               model_name="carp_76M")
    out = subprocess.run(["bash", os.path.join(root, "scripts", "scoring_DMS_zero_shot", "scoring_CARP_substitutions.sh")], env=env,
                         capture_output=True, text=True, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr
    argv = out.stdout.strip().split("\n")
    assert argv[0] == "proteingym_amd.score_carp_proteingym"
    a = cli.parser().parse_args(argv[1:])
    assert a.DMS_index == 7 and a.model_path == "/w/carp" and a.model_name == "carp_76M" and a.DMS_data_folder == "/data/pg/subs/"
    assert a.DMS_reference_file_path.endswith("DMS_substitutions.csv") and os.path.isabs(a.DMS_reference_file_path)
    assert a.output_scores_folder == "/data/pg/out_subs/CARP" and a.fitness_computation_mode == "masked_marginals" and not a.indel_mode
