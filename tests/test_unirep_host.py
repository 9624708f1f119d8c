"""UniRep host code (proteingym_amd/unirep.py, score_unirep_proteingym.py) on the CPU: tokens and the sequence filter, the loader, the
folding against the float64 restatement (tests/unirep_ref.py, which follows the reference's unirep.py line by line -- TensorFlow is not
available here, so the live reference produced no value in this file), the prefix planner, and the CLI's file."""
import json
import os

import numpy as np
import pandas as pd
import pytest

import unirep_ref as R
from proteingym_amd import _lib, unirep as ur, score_unirep_proteingym as cli

from oracle.ref_harness import REF_ROOT

TARGET = "MKVLAAGIVRHDESTNQCGPAVIFYWLMKRHDESTNQ"          # 37 residues


def test_tokens_match_the_reference_table():
    assert {k: v for k, v in R.AA_TO_INT.items() if k not in ("start", "stop", "-")} == ur.AA_TO_INT
    assert (ur.TOK_PAD, ur.TOK_START, ur.TOK_STOP) == (0, R.AA_TO_INT["start"], R.AA_TO_INT["stop"])
    assert ur.AA_TO_INT["M"] == 1 and ur.AA_TO_INT["L"] == 21 and ur.AA_TO_INT["O"] == 22
    assert {ur.AA_TO_INT[a] for a in "XZBJ"} == {23}
    t = ur.format_seq("MRL")
    assert t.tolist() == [24, 1, 2, 21] == R.format_seq("MRL") and t.dtype == np.int32       # start first, no stop
    assert ur.format_seq("M-L").tolist() == [24, 1, 23, 21]                                   # '-' -> 'X'
    with pytest.raises(ValueError):
        ur.format_seq("M1L")


def test_sequences_are_unique_sorted_stripped_and_filtered():
    vals = ["MKV*", "MKA", "MKV", "MXA", "MK-A", "*AKV", "MKA"]
    df = pd.DataFrame({"mutant": ["a"] * len(vals), "mutated_sequence": vals})
    got = ur.load_and_filter_seqs(df)
    assert got == R.load_and_filter_seqs(vals) == ["AKV", "MKA", "MKV", "MKV"]                # 'MKV' and 'MKV*' both survive np.unique
    assert ur.load_and_filter_seqs(pd.DataFrame({"mutant": ["MKV", "AKV"]})) == ["AKV", "MKV"]  # the mutant column as a fallback
    assert not ur.is_valid_seq("MXA") and not ur.is_valid_seq("M" * 4001) and ur.is_valid_seq("M" * 4000)
    assert ur.evotune_path("w", "TOY_MSA.a2m") == "w" + os.sep + "TOY_MSA"


@pytest.mark.parametrize("dense", ["dense", "fully_connected"])
def test_loader_reads_both_dense_names_and_checks_shapes(tmp_path, dense):
    files = R.toy_checkpoint(3, 12, 1.5)
    if dense == "fully_connected":
        files["fully_connected_weights:0.npy"] = files.pop("dense_kernel:0.npy")
        files["fully_connected_biases:0.npy"] = files.pop("dense_bias:0.npy")
    R.save_checkpoint(str(tmp_path / "ck"), files)
    a = ur.load_arrays(str(tmp_path / "ck"))
    ref = R.load_arrays(str(tmp_path / "ck"))
    assert np.array_equal(a["dense_w"], R.dense_of(ref)[0]) and np.array_equal(a["dense_b"], R.dense_of(ref)[1])
    assert a["wmh"].shape == (12, 12) and a["embed"].shape == (26, 10)
    b = ur.arrays_from_files(files)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    # both names present: the reference takes fully_connected_* (unirep.py:386)
    if dense == "fully_connected":
        np.save(tmp_path / "ck" / "dense_kernel:0.npy", np.zeros((12, 25), np.float32))
        assert np.array_equal(ur.load_arrays(str(tmp_path / "ck"))["dense_w"], a["dense_w"])
    os.remove(tmp_path / "ck" / "rnn_mlstm_mlstm_gmh:0.npy")
    with pytest.raises(_lib.PgmiError, match="gmh"):
        ur.load_arrays(str(tmp_path / "ck"))
    with pytest.raises(_lib.PgmiError, match="not a directory"):
        ur.load_arrays(str(tmp_path / "nope"))


def test_strict_shape_errors():
    files = R.toy_checkpoint(3, 12, 1.5)
    for name, bad in (("rnn_mlstm_mlstm_wh:0.npy", (12, 47)), ("rnn_mlstm_mlstm_gx:0.npy", (12,)), ("dense_bias:0.npy", (26,)),
                      ("embed_matrix:0.npy", (25, 10)), ("rnn_mlstm_mlstm_wmh:0.npy", (12, 13))):
        f = dict(files)
        f[name] = np.zeros(bad, np.float32)
        with pytest.raises(_lib.PgmiError, match="shape|rows"):
            ur.arrays_from_files(f)
    f = dict(files)
    f["rnn_mlstm_mlstm_b:0.npy"] = np.full(48, np.nan, np.float32)
    with pytest.raises(_lib.PgmiError, match="non-finite"):
        ur.arrays_from_files(f)
    del f["embed_matrix:0.npy"]
    with pytest.raises(_lib.PgmiError, match="embed_matrix"):
        ur.arrays_from_files(f)


@pytest.mark.parametrize("H", [12, 76])
def test_folding_reproduces_the_restatement(H):
    files = R.toy_checkpoint(5, H, 1.5)
    f = ur.fold(ur.arrays_from_files(files))
    wx, wh, wmx, wmh, b = R.effective_weights(files)
    E = files["embed_matrix:0.npy"].astype(np.float64)
    for got, ref in ((f["Tmx"], E @ wmx), (f["Tx"], E @ wx + b), (f["wmh"], wmh), (f["wh"], wh)):
        assert got.dtype == np.float64 and np.abs(got - ref).max() <= 1e-14 * max(1.0, np.abs(ref).max())
    assert f["Tmx"].shape == (26, H) and f["Tx"].shape == (26, 4 * H)
    # a step from the folded quantities equals the restatement's step
    rng = np.random.default_rng(0)
    h, c, tok = rng.normal(0, 0.5, (4, H)), rng.normal(0, 1, (4, H)), np.array([0, 24, 23, 7])
    h1, c1, z1 = R.cell_step((wx, wh, wmx, wmh, b), E[tok], c, h)
    z = f["Tx"][tok] + (f["Tmx"][tok] * (h @ f["wmh"])) @ f["wh"]
    assert np.abs(z - z1).max() <= 1e-12
    blob = ur.blob_from_arrays(ur.arrays_from_files(files))
    assert blob.dtype == np.float32 and blob.size == 26 * H + 26 * 4 * H + H * H + 4 * H * H + 25 * H + 25
    # a zero column: the epsilon of l2_normalize keeps it zero instead of NaN
    files["rnn_mlstm_mlstm_wmh:0.npy"][:, 3] = 0.0
    assert np.array_equal(ur.fold(ur.arrays_from_files(files))["wmh"][:, 3], np.zeros(H))


def _variants():
    t = TARGET
    sub = lambda s, i, a: s[:i] + a + s[i + 1:]
    return {
        "single_first": (sub(t, 0, "A"), 0),
        "single_mid": (sub(t, 17, "W"), 17),
        "single_last": (sub(t, 36, "A"), 36),
        "multiple": (sub(sub(sub(t, 30, "W"), 9, "W"), 21, "W"), 9),
        "target": (t, 37),
        "insertion": (t[:12] + "W" + t[12:], 12),
        "deletion": (t[:20] + t[21:], 20),
        "prefix": (t[:15], 15),
        "longer": (t + "MK", 37),
    }


def test_planner_join_steps():
    tgt = ur.format_seq(TARGET)
    for name, (seq, join) in _variants().items():
        assert ur.join_step(ur.format_seq(seq), tgt) == join, name
        assert ur.join_step(ur.format_seq(seq), None) == 0
    v = _variants()
    assert v["target"][1] == len(TARGET) and v["prefix"][1] == len(v["prefix"][0])          # no cell step runs for either
    # X, Z, B and J are one token: the planner compares what the model reads
    assert ur.join_step(ur.format_seq("MKZA"), ur.format_seq("MKXL")) == 3


def test_planner_order_chunks_and_row_steps():
    v = _variants()
    seqs = [s for s, _ in v.values()]
    rows = [ur.format_seq(s) for s in seqs]
    p = ur.plan(rows, ur.format_seq(TARGET), max_rows=3)
    assert p.join.tolist() == [j for _, j in v.values()] and p.lens.tolist() == [len(s) for s in seqs]
    assert p.row_steps == sum(len(s) - j for s, j in v.values())
    assert sorted(p.order.tolist()) == list(range(len(seqs)))
    for i0, i1 in p.chunks:
        idx = p.order[i0:i1]
        assert 1 <= len(idx) <= 3 and len(set(p.lens[idx])) == 1 and list(p.join[idx]) == sorted(p.join[idx])
    assert [c[0] for c in p.chunks[1:]] == [c[1] for c in p.chunks[:-1]] and p.chunks[0][0] == 0 and p.chunks[-1][1] == len(seqs)
    s = ur.plan(rows, None)
    assert s.join.tolist() == [0] * len(seqs) and s.row_steps == sum(len(x) for x in seqs) and s.row_steps > p.row_steps


class _RestatedModel:
    """UniRepModel's scoring surface on the float64 restatement (no GPU)."""

    def __init__(self, path):
        self.files = R.load_arrays(path)
        self.last_row_steps = 0

    def set_target(self, seq):
        self.target = seq

    def nll(self, seqs, from_scratch=False):
        return R.scores(self.files, seqs)

    def close(self):
        pass


def make_toy_assay(root, H=12, evotuned_H=None):
    """A mapping row, its assay CSV and the checkpoint directories under root; returns (argv, expected sequences)."""
    os.makedirs(root, exist_ok=True)
    seqs = [s for s, _ in _variants().values()] + [TARGET[:10] + "X" + TARGET[11:], TARGET + "*"]
    pd.DataFrame({"mutant": [f"m{i}" for i in range(len(seqs))], "mutated_sequence": seqs,
                  "DMS_score": np.linspace(0, 1, len(seqs))}).to_csv(os.path.join(root, "TOY_UR.csv"), index=False)
    pd.DataFrame({"DMS_id": ["TOY_UR"], "DMS_filename": ["TOY_UR.csv"], "MSA_filename": ["TOY_UR_MSA.a2m"], "target_seq": [TARGET],
                  "DMS_total_number_mutants": [len(seqs)]}).to_csv(os.path.join(root, "mapping.csv"), index=False)
    R.save_checkpoint(os.path.join(root, "base"), R.toy_checkpoint(21, H, 1.5))
    R.save_checkpoint(os.path.join(root, "evo", "TOY_UR_MSA"), R.toy_checkpoint(22, evotuned_H or H, 1.5))
    return seqs


def cli_argv(root, model, out, *extra):
    return ["--model_path", os.path.join(root, model), "--data_path", root, "--mapping_path", os.path.join(root, "mapping.csv"),
            "--output_dir", out, "--DMS_index", "0", "--batch_size", "8", *extra]


@pytest.mark.parametrize("evotune", [False, True])
def test_cli_writes_the_reference_file(tmp_path, monkeypatch, evotune):
    root = str(tmp_path / "toy")
    make_toy_assay(root)
    seen = {}

    def fake(path, device=0, precision="f16x3", max_rows=0):
        seen["path"] = path
        return _RestatedModel(path)

    monkeypatch.setattr(ur, "from_pretrained", fake)
    out = cli.main(cli_argv(root, "evo" if evotune else "base", str(tmp_path / "UniRep"), *(["--evotune", "--save_hidden"] if evotune else [])))
    assert seen["path"] == os.path.join(root, "evo", "TOY_UR_MSA") if evotune else os.path.join(root, "base")
    assert out == str(tmp_path / "UniRep") + os.sep + "TOY_UR.csv"
    got = pd.read_csv(out)
    assert list(got.columns) == ["mutated_sequence", "Unirep_score"]
    want = R.load_and_filter_seqs(pd.read_csv(os.path.join(root, "TOY_UR.csv"))["mutated_sequence"].values)
    assert list(got["mutated_sequence"]) == want and "X" not in "".join(want) and want == sorted(want)
    assert np.abs(got["Unirep_score"] - R.scores(R.load_arrays(seen["path"]), want)).max() <= 1e-12
    assert os.listdir(tmp_path / "UniRep") == ["TOY_UR.csv"]                    # --save_hidden saves nothing
    if evotune or not os.path.isfile(os.path.join(REF_ROOT, "proteingym", "merge.py")):
        return
    # the reference's own merge.py with its own registry row for this family
    import importlib.util
    import sys
    registry = json.load(open(os.path.join(REF_ROOT, "config.json")))["model_list_zero_shot_substitutions_DMS"]
    row = registry["Unirep"]
    assert (row["input_score_name"], row["key"], row["directionality"], row["location"]) == ("Unirep_score", "mutated_sequence", -1, "UniRep")
    json.dump({"model_list_zero_shot_substitutions_DMS": {"Unirep": row}}, open(tmp_path / "config.json", "w"))
    spec = importlib.util.spec_from_file_location("pg_reference_merge_unirep", os.path.join(REF_ROOT, "proteingym", "merge.py"))
    merge = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(merge)
    # merge.py joins on the key and expects every assay row: an assay of the sequences the scorer keeps
    dms = pd.read_csv(os.path.join(root, "TOY_UR.csv"))
    dms = dms[dms["mutated_sequence"].isin(want)].drop_duplicates("mutated_sequence")
    dms.to_csv(os.path.join(root, "TOY_UR.csv"), index=False)
    ref_one = tmp_path / "ref.csv"
    pd.read_csv(os.path.join(root, "mapping.csv")).assign(DMS_total_number_mutants=len(dms)).to_csv(ref_one, index=False)
    monkeypatch.setattr(sys, "argv", ["merge.py", "--DMS_assays_location", root, "--model_scores_location", str(tmp_path),
                                      "--DMS_reference_file", str(ref_one), "--config_file", str(tmp_path / "config.json")])
    merge.main()
    merged = pd.read_csv(tmp_path / "merged_scores" / "TOY_UR.csv").set_index("mutated_sequence")
    # directionality -1: merge.py flips the sign, so that higher is fitter in the merged file
    assert np.allclose(merged.loc[got["mutated_sequence"], "Unirep"].values, -got["Unirep_score"].values)


def test_toy_gain_keeps_fp32_within_3e_5_of_float64():
    """The seeded gain (1.5) is the largest of the grid 1, 1.25, 1.5, 2, 4 at which the CPU fp32 restatement stays within 3e-5 of the
    float64 one at every shape the GPU tests use (at 2 the recurrence amplifies rounding to 1e-4 .. 1e-3, at 4 to 0.1); the distances
    are printed."""
    rng = np.random.default_rng(5)
    for H, L, n in ((76, 37, 4), (128, 37, 4), (1900, 24, 2)):
        files = R.toy_checkpoint(11 + H, H, 1.5)
        seqs = ["".join(rng.choice(list(R.VALID_AAS), L)) for _ in range(n)]
        d = float(np.abs(R.scores(files, seqs) - R.scores(files, seqs, np.float32)).max())
        print(f"unirep toy gain 1.5 H={H} L={L}: fp32-vs-fp64 score distance {d:.3e}")
        assert d <= 3e-5


def test_library_refuses_bad_configs(lib):
    import ctypes as C
    ok = dict(abi_version=_lib.ABI_VERSION, hidden=76, vocab=26, precision=_lib.PREC_F16X3, max_rows=0)
    assert lib.pgmi_unirep_weight_count(C.byref(ur.UniRepConfig(**ok))) == 26 * 76 * 5 + 5 * 76 * 76 + 25 * 76 + 25
    for bad, msg in ((dict(precision=_lib.PREC_BF16), "bf16"), (dict(vocab=25), "vocabulary"), (dict(hidden=0), "hidden"),
                     (dict(abi_version=_lib.ABI_VERSION - 1), "ABI")):
        assert lib.pgmi_unirep_weight_count(C.byref(ur.UniRepConfig(**dict(ok, **bad)))) == -1
        assert msg in lib.pgmi_last_error().decode()
    assert lib.pgmi_set_option(b"unirep_max_rows", 0) == 0


@pytest.mark.parametrize("script", ["scoring_UniRep_substitutions.sh", "scoring_UniRep_indels.sh", "scoring_UniRep_evotune_substitutions.sh",
                                    "scoring_UniRep_evotune_indels.sh"])
def test_launchers_build_a_command_line_the_cli_parses(script, tmp_path):
    """The launchers of the reference's names read zero_shot_config.sh and pass the reference's flags."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg_dir = tmp_path / "scripts"
    (cfg_dir / "scoring_DMS_zero_shot").mkdir(parents=True)
    (cfg_dir / "zero_shot_config.sh").write_text(
        'export DMS_data_folder_subs="/data/pg/subs/"\nexport DMS_data_folder_indels="/data/pg/indels/"\n'
        'export DMS_reference_file_path_subs=../../reference_files/DMS_substitutions.csv\n'
        'export DMS_reference_file_path_indels=../../reference_files/DMS_indels.csv\n'
        'export DMS_output_score_folder_subs="/data/pg/out_subs"\nexport DMS_output_score_folder_indels="/data/pg/out_indels"\n')
    env = dict(os.environ, ZERO_SHOT_CONFIG=str(cfg_dir / "zero_shot_config.sh"), PGMI_LAUNCH_ECHO="1", DMS_index="7", model_path="/w/unirep")
    out = subprocess.run(["bash", os.path.join(root, "scripts", "scoring_DMS_zero_shot", script)], env=env, capture_output=True, text=True,
                         cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr
    argv = out.stdout.strip().split("\n")
    assert argv[0] == "proteingym_amd.score_unirep_proteingym"
    a = cli.parser().parse_args(argv[1:])
    kind, evo = ("indels" if "indels" in script else "subs"), "evotune" in script
    assert a.DMS_index == 7 and a.model_path == "/w/unirep" and a.evotune == evo and a.data_path == f"/data/pg/{kind}/"
    assert a.mapping_path.endswith("DMS_indels.csv" if kind == "indels" else "DMS_substitutions.csv") and os.path.isabs(a.mapping_path)
    assert a.output_dir == f"/data/pg/out_{kind}/" + ("UniRep_evotuned" if evo else "UniRep")
