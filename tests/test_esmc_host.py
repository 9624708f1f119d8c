"""ESM C host logic without a GPU: the reference's mutant parsing and skips, its window rule, the state-dict loader against the
reference's own key list, the packed blob and its SwiGLU interleave (a float64 numpy forward against the reference's golden
output), and the CLI's flags, output contract and refusals (the device model replaced by that numpy forward)."""
import json
import os

import numpy as np
import pandas as pd
import pytest

from esmc_ref import numpy_forward
from proteingym_amd import esm as pesm, esmc, synthetic as S
from proteingym_amd import score_esmc_proteingym as cli

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REDUCED = ["d128", "d192", "d960", "d1152"]


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLDEN, "golden_esmc.npz"))


@pytest.fixture(scope="module")
def ref_keys():
    with open(os.path.join(GOLDEN, "esmc_state_dict_keys.json")) as f:
        return json.load(f)


def model_of(g, name):
    D, layers, seed = (int(v) for v in g[f"{name}_cfg"])
    cfg = S.esmc_config(D, layers)
    return cfg, esmc.pack(cfg, S.esmc_state_dict(cfg, seed))


def test_tokens_match_reference_tokenizer(g):
    assert [esmc.tokenize(str(c))[1] for c in g["tok_chars"]] == g["tok_ids"].tolist()
    assert g["d128_ids"][0] == esmc.CLS and g["d128_ids"][-1] == esmc.EOS


def test_parse_skips_like_reference():
    seq = "MKTAYIAKQR"
    parsed = esmc.parse_mutations(seq, ["M1A", "K2C:T3D", "A1C", "M11A", "M0A", "m1A", "M1A:", "K2C:X3D", "M1AX", "Q9Q", "K2C:K2D"])
    names = [p[4] for p in parsed]
    # "M1AX" re.match-es its prefix (the reference does not anchor the end); "K2C:K2D" keeps both parts at one position
    assert names == ["M1A", "K2C:T3D", "M1AX", "Q9Q", "K2C:K2D"]
    assert parsed[1][:4] == ("KT", [2, 3], "CD", [1, 2])
    with pytest.raises(KeyError):
        esmc.check_letters(esmc.parse_mutations(seq, ["M1B"]))


def test_parse_matches_reference_nan_pattern():
    ref = pd.read_csv(os.path.join(GOLDEN, "TOY_ESMC_REFERENCE.csv")).set_index("DMS_id")["target_seq"]
    df = pd.read_csv(os.path.join(GOLDEN, "TOY_ESMC_SHORT.csv"))
    scorable = {p[4] for p in esmc.parse_mutations(ref["TOY_ESMC_SHORT"], df["mutant"])}
    assert [m in scorable for m in df["mutant"]] == df["esmc_300M_score"].notna().tolist()


@pytest.mark.parametrize("L", [1022, 1023, 1100, 3000])
def test_window_rule(L):
    for p in sorted({0, 1, 510, 511, 512, L // 2, L - 512, L - 511, L - 2, L - 1}):
        s, e = esmc.window(p, L)
        if L <= 1022:
            assert (s, e) == (0, L)
            continue
        start = max(0, p - 511)
        end = min(L, start + 1022)
        if end == L:
            start = max(0, L - 1022)
        assert (s, e) == (start, end) and e - s == 1022 and s <= p < e, (L, p)
    assert esmc.window(1022, 1023) == (1, 1023) and esmc.window(0, 1023) == (0, 1022)
    assert esmc.window(1500, 3000) == (989, 2011) and esmc.window(2999, 3000) == (1978, 3000)


def test_window_rule_differs_from_esm(lib):
    """ESM (compute_fitness.py masked-marginals) cuts a 1024-TOKEN window out of <cls> + residues + <eos> around token p + 1; ESM C
    cuts 1022 residues, 511 before the position, and wraps each window in its own <cls> ... <eos>."""
    def esm_residues(p, L):
        s, e = pesm.get_optimal_window(p + 1, L + 2, 1024)
        return max(0, s - 1), min(L, e - 1)
    for L in (1023, 1100, 3000):
        diff = [p for p in range(L) if esmc.window(p, L) != esm_residues(p, L)]
        assert diff, L
    assert esm_residues(1500, 3000) == (988, 2012) and esmc.window(1500, 3000) == (989, 2011)
    assert esm_residues(0, 1100) == (0, 1023) and esmc.window(0, 1100) == (0, 1022)


def test_masked_rows():
    seq = "ACDEFGHIKL" * 110                         # 1100 residues: every row is <cls> + 1022 residues + <eos>
    tokens, mask = esmc.masked_rows(seq, [0, 600, 1099])
    assert tokens.shape == (3, 1024) and mask.tolist() == [1, 600 - 78 + 1, 1099 - 78 + 1]
    tok = esmc.tokenize(seq)
    assert tokens[1, 1:-1].tolist() == tok[1 + 78:1 + 78 + 1022].tolist() and tokens[2, -1] == esmc.EOS
    tokens, mask = esmc.masked_rows(seq[:50], [3])
    assert tokens.shape == (1, 52) and mask.tolist() == [4]


def test_expected_keys_are_the_reference_state_dict(ref_keys):
    for model_type, want in ref_keys.items():
        L = esmc.RELEASED[model_type]["layers"]
        assert sorted(esmc.expected_keys(L)) == sorted(k for k, _ in want)        # the blob's order is include/pgmi.h's
        shapes = {k: np.broadcast_to(np.float32(0), tuple(s)) for k, s in want}
        cfg = esmc.config_from_state_dict(shapes, model_type)
        assert cfg == dict(layers=L, embed_dim=esmc.RELEASED[model_type]["embed_dim"], heads=esmc.RELEASED[model_type]["heads"],
                           ffn_dim=esmc.swiglu_hidden(esmc.RELEASED[model_type]["embed_dim"]), vocab=64)
        other = "esmc_600M" if model_type == "esmc_300M" else "esmc_300M"
        with pytest.raises(ValueError, match="configuration"):
            esmc.config_from_state_dict(shapes, other)


def test_synthetic_state_dict_has_reference_shapes(ref_keys):
    import torch  # noqa: F401
    cfg = S.esmc_config(128, 2)
    sd = S.esmc_state_dict(cfg, 1)
    assert sorted(sd) == sorted(esmc.expected_keys(2))
    assert np.any(sd["sequence_head.3.weight"][33:] != 0) and np.any(sd["transformer.blocks.0.attn.q_ln.weight"] != 1)
    assert np.array_equal(sd["embed.weight"], S.esmc_state_dict(cfg, 1)["embed.weight"])


@pytest.mark.parametrize("form", ["file", "dir"])
def test_loader_file_and_snapshot_dir(tmp_path, form):
    torch = pytest.importorskip("torch")
    cfg = S.esmc_config(128, 2)
    sd = S.esmc_state_dict(cfg, 5)
    tsd = {k: torch.from_numpy(v).to(torch.bfloat16 if "ffn" in k else torch.float32) for k, v in sd.items()}
    if form == "file":
        path = tmp_path / "w.pth"
    else:
        (tmp_path / "data" / "weights").mkdir(parents=True)
        path = tmp_path / "data" / "weights" / "esmc_300m_2024_12_v0.pth"
    torch.save(tsd, path)
    got = esmc.load_state_dict(str(path if form == "file" else tmp_path), "esmc_300M")
    assert sorted(got) == sorted(sd) and all(v.dtype == np.float32 for v in got.values())
    assert np.array_equal(got["embed.weight"], sd["embed.weight"])
    tsd["transformer.extra"] = torch.zeros(1)
    torch.save(tsd, path)
    with pytest.raises(ValueError, match="unexpected"):
        esmc.load_state_dict(str(path if form == "file" else tmp_path))
    with pytest.raises(FileNotFoundError):
        esmc.load_state_dict(str(tmp_path / "nothing_here" if form == "file" else tmp_path / "data"), "esmc_600M")


def test_blob_round_trip_and_w1_interleave():
    cfg = S.esmc_config(192, 2)
    sd = S.esmc_state_dict(cfg, 3)
    blob = esmc.pack(cfg, sd)
    assert blob.size == esmc.weight_count(cfg)
    back = esmc.unpack(cfg, blob)
    assert all(np.array_equal(back[k], sd[k]) for k in sd)
    F = cfg["ffn_dim"]
    w1 = sd["transformer.blocks.1.ffn.1.weight"]
    wi = esmc.interleave_w1(w1)
    for b in range(F // 32):
        assert np.array_equal(wi[64 * b:64 * b + 32], w1[32 * b:32 * b + 32])
        assert np.array_equal(wi[64 * b + 32:64 * b + 64], w1[F + 32 * b:F + 32 * b + 32])


def test_weight_count_matches_library(lib):
    import ctypes as C
    from proteingym_amd import _lib
    for D, L in ((128, 2), (960, 30), (1152, 36)):
        cfg = S.esmc_config(D, L)
        c = _lib.Config(abi_version=_lib.ABI_VERSION, arch=_lib.ARCH_ESMC, layers=L, embed_dim=D, heads=D // 64, ffn_dim=cfg["ffn_dim"],
                        vocab=64, precision=_lib.PREC_F16X3)
        assert lib.pgmi_weight_count(C.byref(c)) == esmc.weight_count(cfg)


@pytest.mark.parametrize("name", REDUCED)
def test_numpy_forward_over_blob_matches_reference(g, name):
    cfg, blob = model_of(g, name)
    ids = g[f"{name}_ids"]
    lp = numpy_forward(cfg, blob, ids)
    assert np.abs(lp - g[f"{name}_lp"]).max() < 2e-4
    for p, ref in zip(g[f"{name}_mask_pos"], g[f"{name}_mask_lp"]):
        t = ids.copy()
        t[p] = esmc.MASK
        assert np.abs(numpy_forward(cfg, blob, t)[p] - ref).max() < 2e-4


def test_combine_sums_fp32_differences_as_python_floats():
    lp = np.array(np.random.default_rng(0).standard_normal(64), dtype=np.float32)
    parsed = esmc.parse_mutations("ACD", ["A1C", "A1C:C2D:D3A"])
    s = esmc.combine(parsed, {0: lp, 1: lp, 2: lp})
    t = esmc.AA_TO_TOKEN
    assert s["A1C"] == float(lp[t["C"]] - lp[t["A"]])
    want = 0.0
    for w, m in (("A", "C"), ("C", "D"), ("D", "A")):
        want += float(lp[t[m]] - lp[t[w]])
    assert s["A1C:C2D:D3A"] == want


# -- CLI -------------------------------------------------------------------------------------------------------------------
class NumpyESMC:
    """The device model's scoring on the float64 numpy forward (fp32 log-probabilities)."""

    def __init__(self, cfg, blob):
        self.cfg, self.blob, self.calls = cfg, blob, 0

    def masked_logprobs(self, tokens, mask):
        self.calls += 1
        out = []
        for row, p in zip(tokens, mask):
            t = row.copy()
            t[p] = esmc.MASK
            out.append(numpy_forward(self.cfg, self.blob, t)[p])
        return np.array(out, dtype=np.float32)

    score_mutations = esmc.ESMC.score_mutations

    def close(self):
        pass


@pytest.fixture
def assays(tmp_path):
    dms = tmp_path / "dms"
    dms.mkdir()
    for n in ("TOY_ESMC_SHORT", "TOY_ESMC_BADLETTER"):
        df = pd.read_csv(os.path.join(GOLDEN, n + ".csv"))
        df[["mutant", "DMS_score"]].to_csv(dms / f"{n}.csv", index=False)
    ref = pd.read_csv(os.path.join(GOLDEN, "TOY_ESMC_REFERENCE.csv"))
    ref = ref[ref["DMS_id"] != "TOY_ESMC_LONG"]
    ref.to_csv(tmp_path / "ref.csv", index=False)
    return tmp_path


@pytest.fixture
def fake_model(monkeypatch):
    cfg = S.esmc_config(128, 2)
    blob = esmc.pack(cfg, S.esmc_state_dict(cfg, 31))
    made = []

    def from_pretrained(path, model_type=None, device=0, max_rows=0):
        made.append((path, model_type))
        return NumpyESMC(cfg, blob)
    monkeypatch.setattr(esmc, "from_pretrained", from_pretrained)
    return made


def run_cli(assays, *extra):
    return cli.main(["--reference_csv", str(assays / "ref.csv"), "--dms_dir", str(assays / "dms"), "--output_dir", str(assays / "out"),
                     "--model_path", "/nonexistent.pth", *extra])


def test_cli_outputs_and_summary(assays, fake_model):
    assert run_cli(assays) == 0
    assert fake_model == [("/nonexistent.pth", "esmc_300M")]
    out = pd.read_csv(assays / "out" / "TOY_ESMC_SHORT.csv")
    ref = pd.read_csv(os.path.join(GOLDEN, "TOY_ESMC_SHORT.csv"))
    assert list(out.columns) == ["mutant", "DMS_score", "esmc_300M_score"]
    assert out["esmc_300M_score"].isna().tolist() == ref["esmc_300M_score"].isna().tolist()
    ok = ref["esmc_300M_score"].notna()
    assert np.abs(out["esmc_300M_score"][ok] - ref["esmc_300M_score"][ok]).max() < 2e-4
    assert not (assays / "out" / "TOY_ESMC_BADLETTER.csv").exists()
    summary = pd.read_csv(assays / "out" / "correlation_summary_esmc_300M.csv")
    assert summary["assay"].tolist() == ["TOY_ESMC_SHORT", "TOY_ESMC_BADLETTER"] and np.isnan(summary["correlation"][1])
    assert run_cli(assays, "--DMS_index", "0") == 0                     # appended, no second header
    summary = pd.read_csv(assays / "out" / "correlation_summary_esmc_300M.csv")
    assert summary["assay"].tolist() == ["TOY_ESMC_SHORT", "TOY_ESMC_BADLETTER", "TOY_ESMC_SHORT"]


def test_cli_dms_index_rules(assays, fake_model, capsys):
    ref = pd.read_csv(assays / "ref.csv")
    assert cli.select_assays(ref, -1)["DMS_id"].tolist() == ref["DMS_id"].tolist()
    assert cli.select_assays(ref, "1")["DMS_id"].tolist() == ["TOY_ESMC_BADLETTER"]
    assert cli.select_assays(ref, "7")["DMS_id"].tolist() == ref["DMS_id"].tolist()
    assert "out of range" in capsys.readouterr().out
    assert cli.select_assays(ref, "-1")["DMS_id"].tolist() == ref["DMS_id"].tolist()
    assert cli.select_assays(ref, "x")["DMS_id"].tolist() == ref["DMS_id"].tolist()
    assert run_cli(assays, "--DMS_index", "1", "--model_type", "esmc_600M") == 0
    assert fake_model[-1][1] == "esmc_600M"
    assert pd.read_csv(assays / "out" / "correlation_summary_esmc_600M.csv")["assay"].tolist() == ["TOY_ESMC_BADLETTER"]


def test_cli_flags_and_refusals(assays, fake_model, capsys):
    a = cli.parser().parse_args(["--reference_csv", "r", "--dms_dir", "d", "--output_dir", "o"])
    assert (a.model_type, a.model_path, a.pdb_dir, a.use_structure, a.DMS_index) == ("esmc_300M", None, None, False, -1)
    with pytest.raises(SystemExit):
        cli.parser().parse_args(["--reference_csv", "r", "--dms_dir", "d", "--output_dir", "o", "--model_type", "esmc_6B"])
    assert run_cli(assays, "--model_type", "esm3_open") == 2
    assert run_cli(assays, "--use_structure", "--pdb_dir", "p") == 2
    assert "not supported on this path" in capsys.readouterr().err
    assert cli.main(["--reference_csv", str(assays / "ref.csv"), "--dms_dir", "d", "--output_dir", str(assays / "o2")]) == 2
    assert "--model_path is required" in capsys.readouterr().err
    assert fake_model == []
