"""VespaG's host side (proteingym_amd/vespag.py, score_vespag_proteingym.py) and the library's host-only chunk plan: no GPU needed.
The restatement they are checked against is tests/vespag_ref.py."""
import math
import os

import numpy as np
import pandas as pd
import pytest
import torch

import vespag_ref as R
from proteingym_amd import _lib, vespag
from proteingym_amd import esm as pesm
from proteingym_amd import score_vespag_proteingym as cli

ALL20 = "ACDEFGHIKLMNPQRSTVWY"


def small_sd(seed=4, input_dim=64, hidden=32):
    return vespag.random_state_dict(seed, input_dim, hidden, gain=1.0, bias_std=0.1)


def landscape_for(seq, seed=9):
    """A float32 landscape with the wild type masked, as the device hands it over."""
    y = np.random.default_rng(seed).standard_normal((len(seq), 20)).astype(np.float32)
    y[np.arange(len(seq)), [ALL20.index(a) for a in seq]] = 0.0
    return y


def test_restatement_equals_the_module_construct_fnn_builds():
    """Linear, Dropout(0.2), LeakyReLU, Linear in eval, from the same seeded state dict: pins the layer order and the key names."""
    sd = small_sd()
    net = torch.nn.Sequential(torch.nn.Linear(64, 32), torch.nn.Dropout(0.2), torch.nn.LeakyReLU(), torch.nn.Linear(32, 20)).double().eval()
    net.load_state_dict({k[len("net."):]: torch.from_numpy(v).double() for k, v in sd.items()})           # strict: the keys are net.0 / net.3
    x = np.random.default_rng(1).standard_normal((11, 64))
    x[3] -= 4.0                                                                # a row with mostly negative pre-activations
    with torch.no_grad():
        want = net(torch.from_numpy(x))
    got = R.fnn(sd, x)
    assert got.dtype == torch.float64 and (want < 0).any()
    assert torch.allclose(got, want, rtol=0, atol=1e-13)


def test_checkpoint_reader_round_trips_a_seeded_state_dict(tmp_path):
    sd = small_sd()
    path = str(tmp_path / "state_dict_v2.pt")
    torch.save({k: torch.from_numpy(v) for k, v in sd.items()}, path)
    back = vespag.load_checkpoint(path)
    assert list(back) == list(vespag.KEYS) and all(np.array_equal(back[k], sd[k]) for k in sd)
    assert vespag.check_state_dict(back) == (64, 32)
    blob = vespag.pack(back)
    assert blob.dtype == np.float32 and blob.size == 32 * 64 + 32 + 20 * 32 + 20
    assert np.array_equal(blob[:32 * 64].reshape(32, 64), sd["net.0.weight"]) and np.array_equal(blob[-20:], sd["net.3.bias"])
    with pytest.raises(FileNotFoundError, match="never downloads"):
        vespag.load_checkpoint(str(tmp_path / "missing.pt"))


def test_checkpoint_refusals_name_their_cause():
    sd = small_sd()
    for key in ("conv.0.weight", "fnn.0.weight", "combined.0.bias"):
        with pytest.raises(ValueError, match="CNN or combined"):
            vespag.check_state_dict({**sd, key: np.zeros((2, 2), np.float32)})
    two = {"net.0.weight": np.zeros((32, 64)), "net.0.bias": np.zeros(32), "net.3.weight": np.zeros((16, 32)), "net.3.bias": np.zeros(16),
           "net.6.weight": np.zeros((20, 16)), "net.6.bias": np.zeros(20)}
    with pytest.raises(ValueError, match="2 hidden layers"):
        vespag.check_state_dict(two)
    with pytest.raises(ValueError, match="ProtT5"):
        vespag.check_state_dict(vespag.random_state_dict(1, 1024, 32))
    with pytest.raises(ValueError, match=r"net.3.weight \(19, 32\)"):
        vespag.check_state_dict({**sd, "net.3.weight": np.zeros((19, 32), np.float32)})
    with pytest.raises(ValueError, match="net.0.bias"):
        vespag.check_state_dict({**sd, "net.0.bias": np.zeros(31, np.float32)})
    with pytest.raises(ValueError, match="unexpected key"):
        vespag.check_state_dict({**sd, "head.weight": np.zeros(3, np.float32)})


def test_tokenisation_maps_uzob_to_x_and_refuses_other_letters():
    assert tuple(R.ESM_IDS) == pesm.VOCABULARY                                 # the restatement's table is the alphabet
    x = pesm.VOCABULARY.index("X")
    tok = vespag.tokenize("AUZOBX")
    assert tok.dtype == np.uint8 and tok.tolist() == [0, pesm.VOCABULARY.index("A"), x, x, x, x, x, 2]
    assert vespag.tokenize(ALL20).tolist() == [0] + [pesm.VOCABULARY.index(a) for a in ALL20] + [2]
    for bad in ("AJC", "AC*", "Ac", "A-C"):
        with pytest.raises(ValueError, match="position"):
            vespag.tokenize(bad)
    with pytest.raises(ValueError, match="empty"):
        vespag.tokenize("")
    toks, off = vespag.pack_library(["AC", "G"])
    assert off.tolist() == [0, 4, 7] and toks.size == 7
    assert vespag.wt_columns("AXY").tolist() == [0, -1, 19]                    # the stated deviation: X stays unmasked


def test_landscape_order_for_a_sequence_that_holds_every_letter():
    seq = "MKV" + ALL20 + "WA"
    for one in (True, False):
        got = [str(s) for s in vespag.landscape(seq, one)]
        assert len(got) == 19 * len(seq) and got == R.full_landscape(seq, one)
    first = [str(s) for s in vespag.landscape(seq)[:19]]
    assert first[0] == "M1A" and first[-1] == "M1Y" and "M1M" not in first
    assert len(vespag.landscape("AX")) == 19 + 20                              # a wild type outside the 20 lists all 20 targets


def test_scoring_rules():
    seq = "MKVLAAGIWY"
    y = landscape_for(seq)
    y64 = y.astype(np.float64)
    mut = vespag.Mutation.from_mutation_string
    # a multi-mutant sums its SAVs before the logistic, in float64, exactly as the restatement
    m = "M1A:K2C:Y10W"
    s = float(y[0, 0]) + float(y[1, 1]) + float(y[9, 18])
    assert vespag.mutation_score(y, mut(m, True)) == 1 / (1 + math.exp(-s)) == R.score(y, m)
    assert vespag.mutation_score(y, mut(m, True), normalize=False) == s == R.score(y64, m, normalize=False)
    # --zero-idx shifts positions by one
    assert vespag.mutation_score(y, mut("M0A", False)) == vespag.mutation_score(y, mut("M1A", True))
    assert str(mut("M0A:K1C", False)) == "M0A:K1C" and str(mut("M1A", True)) == "M1A"
    assert vespag.mutation_score(y, mut("K1C", False)) == R.score(y, "K1C", one_indexed=False)
    # to_aa == wild type: the masked entry, exactly 0.5
    assert vespag.mutation_score(y, mut("M1M", True)) == 0.5 and vespag.mutation_score(y, mut("M1M", True), normalize=False) == 0.0
    # a wrong from_aa changes nothing (the reference never reads it)
    assert vespag.mutation_score(y, mut("Q1A", True)) == vespag.mutation_score(y, mut("M1A", True))
    # a SAV scores as a one-SAV mutation
    assert vespag.mutation_score(y, vespag.SAV(0, "M", "A", True)) == vespag.mutation_score(y, mut("M1A", True))
    for bad, what in (("M11A", "outside the sequence"), ("M0A", "outside the sequence"), ("M1A:K2B", "target 'B'"), ("M1A:KxC", "expected")):
        with pytest.raises(ValueError, match=what) as e:
            vespag.mutation_score(y, mut(bad, True))
        assert bad.split(":")[-1] in str(e.value) or bad in str(e.value)          # the mutant is named
    full = vespag.score_mutations(y, vespag.landscape(seq))
    assert list(full) == R.full_landscape(seq) and np.array_equal(list(full.values()), R.scores(y, R.full_landscape(seq)))


def test_mutation_file_and_fasta_readers(tmp_path):
    f = tmp_path / "muts.csv"
    f.write_text("protein,mutation\nP1,M1A\nP1,M1A:K2C\nP2,G1A\n")              # a header line, as polars' read_csv expects
    got = vespag.read_mutation_file(str(f))
    assert {k: [str(m) for m in v] for k, v in got.items()} == {"P1": ["M1A", "M1A:K2C"], "P2": ["G1A"]}
    assert got["P1"][0].savs[0].position == 0
    assert vespag.read_mutation_file(str(f), one_indexed=False)["P1"][0].savs[0].position == 1
    fa = tmp_path / "p.fasta"
    fa.write_text(">P1 some description\nMKV\nLA\n\n>P2\nGG\n")
    assert vespag.read_fasta(str(fa)) == {"P1": "MKVLA", "P2": "GG"}


def test_chunk_plan_covers_every_sequence_once(lib):
    lengths = [70, 1, 300, 7, 37, 70]                                          # the caller's order, not sorted
    cap = 320
    order, chunks, packed = vespag.plan_chunks(lengths, cap)
    assert sorted(order) == list(range(6)) and [i for c in chunks for i in c] == order
    assert order == [2, 0, 5, 4, 3, 1]                                         # descending length, stable: 70 (index 0) before 70 (index 5)
    assert len(chunks) >= 3
    for c in chunks:
        T = lengths[c[0]] + 2
        assert all(lengths[i] + 2 <= T for i in c)                             # T is the chunk's first sequence
        assert len(c) * T <= cap and (len(c) == 1 or len(c) * ((T + 31) // 32 * 32) <= cap)
    assert packed == [0, 70, 71, 371, 378, 415, 485]                           # the caller's order
    # a cap below one padded sequence still runs it alone
    _, chunks1, _ = vespag.plan_chunks(lengths, 64)
    assert [len(c) for c in chunks1[:3]] == [1, 1, 1] and sum(len(c) for c in chunks1) == 6
    # one chunk when everything fits
    assert len(vespag.plan_chunks([1, 7, 37, 70, 70], 2048)[1]) == 1
    off = np.array([0, 2], np.int64)
    z32, z64 = np.zeros(1, np.int32), np.zeros(2, np.int64)
    rc = lib.pgmi_op_packed_rows_plan(_lib.ptr(off, _lib._i64p), 1, 64, _lib.ptr(z32, _lib._i32p), _lib.ptr(z32.copy(), _lib._i32p),
                                      _lib.ptr(z32.copy(), _lib._i32p), _lib.ptr(z64, _lib._i64p))
    assert rc == _lib.EINVAL and "2 tokens" in lib.pgmi_last_error().decode()


def test_embeddings_npz_h5_and_id_map(tmp_path):
    rows = {"e1": np.ones((5, 64), np.float32), "e2": np.zeros((2, 64), np.float32)}
    npz = str(tmp_path / "emb.npz")
    np.savez(npz, **rows)
    got = vespag.load_embeddings(npz)
    assert set(got) == {"e1", "e2"} and got["e1"].dtype == np.float32 and got["e1"].shape == (5, 64)
    (tmp_path / "map.csv").write_text("e1,P1\n")
    mapped = vespag.apply_id_map(got, str(tmp_path / "map.csv"))
    assert set(mapped) == {"P1", "e2"}
    vespag.check_embedding("P1", "MKVLA", mapped["P1"], 64)
    with pytest.raises(ValueError, match="5 residues"):
        vespag.check_embedding("e2", "MKVLA", mapped["e2"], 64)
    with pytest.raises(KeyError, match="e9"):
        (tmp_path / "bad.csv").write_text("e9,P9\n")
        vespag.apply_id_map(mapped, str(tmp_path / "bad.csv"))
    try:
        import h5py  # noqa: F401
    except ImportError:
        with pytest.raises(RuntimeError, match="h5py"):
            vespag.load_embeddings(str(tmp_path / "emb.h5"))
        args = cli.parser().parse_args(["predict", "-i", "x.fasta", "--h5-output", "-e", npz])
        with pytest.raises(RuntimeError, match="--h5-output needs h5py"):
            cli.check_outputs(args)
    with pytest.raises(ValueError, match=".npz or .h5"):
        vespag.load_embeddings(str(tmp_path / "emb.csv"))


def test_cli_flags_and_csv_layouts(tmp_path):
    p = cli.parser()
    a = p.parse_args(["predict", "-i", "in.fasta", "-o", "out", "-e", "e.npz", "--checkpoint-file", "c.pt", "--mutation-file", "m.csv",
                      "--id-map", "i.csv", "--single-csv", "--zero-idx", "--dont-normalize"])
    assert (a.fasta_file, a.output_path, a.embedding_file, a.checkpoint_file, a.mutation_file, a.id_map_file) == \
        ("in.fasta", "out", "e.npz", "c.pt", "m.csv", "i.csv")
    assert a.single_csv and a.zero_based_mutations and not a.normalize_scores and not a.no_csv and not a.h5_output
    d = p.parse_args(["predict", "--input", "in.fasta", "--multi-csv", "--csv", "--one-idx", "--normalize"])
    assert not d.single_csv and not d.no_csv and not d.zero_based_mutations and d.normalize_scores and d.precision == "f16x3"
    with pytest.raises(ValueError, match="--plm is required"):
        cli.check_outputs(d)
    with pytest.raises(ValueError, match="--save-embeddings writes the rows computed here"):
        cli.check_outputs(p.parse_args(["predict", "-i", "in.fasta", "-e", "e.npz", "--save-embeddings", "rows.npz"]))
    e = p.parse_args(["eval-proteingym", "--reference-file", "r.csv", "--dms-directory", "dms", "-o", "o", "-e", "e.npz", "--checkpoint-file",
                      "c.pt", "--id-map", "i.csv", "--dont-normalize", "--plm", "esm.pt", "--precision", "fp32", "--max_rows", "4096",
                      "--save-embeddings", "rows.npz", "--device", "1"])                       # (parsed only: -e with --save-embeddings is refused later)
    assert (e.dms_reference_file, e.dms_directory, e.plm, e.precision, e.max_rows, e.save_embeddings, e.device) == \
        ("r.csv", "dms", "esm.pt", "fp32", 4096, "rows.npz", 1)
    # the frames of runner/predict.py:206-232 from a given landscape
    seq = "MKVLA"
    y = landscape_for(seq)
    scores = {"P1": vespag.score_mutations(y, vespag.landscape(seq)), "P2": vespag.score_mutations(y, [vespag.Mutation.from_mutation_string("M1A:K2C", True)])}
    cli.write_csvs(str(tmp_path), scores, single_csv=False)
    assert open(tmp_path / "P1.csv").readline() == "mutant,VespaG\n"
    one = pd.read_csv(tmp_path / "P1.csv", float_precision="round_trip")          # repr(float) round-trips
    assert list(one.columns) == ["mutant", "VespaG"]                           # merge.py's key column and config.json's input_score_name
    assert list(one["mutant"]) == R.full_landscape(seq) and np.array_equal(one["VespaG"], R.scores(y, R.full_landscape(seq)))
    assert open(tmp_path / "P2.csv").read() == f"mutant,VespaG\nM1A:K2C,{R.score(y, 'M1A:K2C')}\n"
    cli.write_csvs(str(tmp_path), scores, single_csv=True)
    both = pd.read_csv(tmp_path / "vespag_scores_all.csv")
    assert list(both.columns) == ["DMS_id", "mutant", "VespaG"] and list(both["DMS_id"]) == ["P1"] * 95 + ["P2"]


def test_launcher_builds_a_valid_command_line(tmp_path):
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg_dir = tmp_path / "scripts"
    (cfg_dir / "scoring_DMS_zero_shot").mkdir(parents=True)
    (cfg_dir / "zero_shot_config.sh").write_text(
        'export DMS_data_folder_subs="/data/pg/DMS_ProteinGym_substitutions/"\n'
        'export DMS_reference_file_path_subs=/data/pg/reference_files/DMS_substitutions.csv\n'
        'export DMS_output_score_folder_subs="/data/pg/zero_shot_substitutions_scores/"\n')
    env = dict(os.environ, ZERO_SHOT_CONFIG=str(cfg_dir / "zero_shot_config.sh"), PGMI_LAUNCH_ECHO="1",
               model_checkpoint_file="/w/state_dict_v2.pt", precomputed_embedding_file="/w/emb.npz")
    out = subprocess.run(["bash", os.path.join(root, "scripts", "scoring_DMS_zero_shot", "scoring_VespaG_substitutions.sh")], env=env,
                         capture_output=True, text=True, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr
    module, *argv = out.stdout.strip().split("\n")
    assert module == "proteingym_amd.score_vespag_proteingym"
    a = cli.parser().parse_args(argv)
    assert a.command == "eval-proteingym" and a.checkpoint_file == "/w/state_dict_v2.pt" and a.embedding_file == "/w/emb.npz"
    assert a.output_path.rstrip("/").endswith("zero_shot_substitutions_scores/VespaG") and a.dms_reference_file.endswith("DMS_substitutions.csv")
