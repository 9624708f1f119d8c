"""VespaG on the device against tests/vespag_ref.py (float64): the head's op entry, the packed residue rows of a library through a small
seeded ESM2 (against a float64 HF EsmModel that runs each sequence alone), the device hand-off, the refusals that need a handle, and the
CLI on tests/golden/VespaG_toy.  The bound is DESIGN.md section 3's flat 1e-4 on the pre-logistic landscape y and on the scores, in f16x3
and in fp32.  The seeded head's gain is 1 (kaiming_normal_ as FNN draws it): at the released width the fp32 torch restatement of that head
is within 4e-6 of float64 (profiles/vespag/README.md), inside the 1e-5 the bound's reading asks for.
"""
import functools
import os

import numpy as np
import pandas as pd
import pytest
import torch

import vespag_ref as R
from proteingym_amd import _lib, vespag, synthetic as S
from proteingym_amd import esm as pesm
from proteingym_amd import score_vespag_proteingym as cli

pytestmark = pytest.mark.gpu
TOL = 1e-4
PRECISIONS = ["f16x3", "fp32"]
TOY = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "VespaG_toy")
LENGTHS = (37, 70, 1, 70, 7)                  # the library {1, 7, 37, 70, 70} in an order that is not sorted


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def head_sd(D, H):
    sd = vespag.random_state_dict(**dict(R.TOY_HEAD, input_dim=D, hidden=H))
    return {k: _frozen(v) for k, v in sd.items()}


@functools.lru_cache(maxsize=None)
def head_case(Rn, D, H):
    """Unit-variance rows, as emb_layer_norm_after leaves them; row 0 is fitted so that its pre-activations are large and negative;
    wt columns that walk 0 .. 19 and -1.  (rows, wt, float64 y with the wild type masked)."""
    sd = head_sd(D, H)
    x = np.random.default_rng(5).standard_normal((Rn, D))
    w, b = sd["net.0.weight"].astype(np.float64), sd["net.0.bias"].astype(np.float64)
    x[0] = np.linalg.lstsq(w, -6.0 - b, rcond=None)[0]
    x = x.astype(np.float32)
    wt = (((np.arange(Rn) * 5 + 3) % 21) - 1).astype(np.int32)
    y = R.fnn(sd, x).numpy()
    for r in range(Rn):
        if wt[r] >= 0:
            y[r, wt[r]] = 0.0
    return _frozen(x), _frozen(wt), _frozen(y)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("Rn,D,H", [(1, 128, 256), (63, 128, 256), (64, 128, 256), (65, 128, 256), (130, 128, 256), (9, 2560, 256)])
def test_op_head_against_float64(lib, Rn, D, H, precision):
    sd = head_sd(D, H)
    x, wt, want = head_case(Rn, D, H)
    got = vespag.op_vespag_head(sd, x, wt, precision=precision)
    err = np.abs(got - want).max()
    print(f"\nhead op {precision} R={Rn} {D}->{H}->20: max |y - float64| = {err:.3e}, max |y| = {np.abs(want).max():.2f}")
    assert np.isfinite(got).all() and err <= TOL
    masked = wt >= 0
    assert (got[masked, wt[masked]] == 0.0).all() and not np.signbit(got[masked, wt[masked]]).any()       # exact +0.0
    assert (got == 0.0).sum() == masked.sum()                                  # and no zero written anywhere else
    if Rn >= 21:
        assert set(wt.tolist()) == set(range(-1, 20))
    # row 0: the slope decides the result -- with slope 0 or 1 in its place the float64 row moves by far more than the bound
    for other in (0.0, 1.0):
        moved = np.abs(R.fnn(sd, x[:1], slope=other).numpy()[0] - R.fnn(sd, x[:1]).numpy()[0]).max()
        assert moved > 100 * TOL, (other, moved)
    h0 = x[:1].astype(np.float64) @ sd["net.0.weight"].astype(np.float64).T + sd["net.0.bias"]
    assert (h0 < -1).mean() > 0.5


def test_op_head_refusals(lib):
    sd = head_sd(128, 256)
    x, wt, _ = head_case(9, 128, 256)
    bad = wt.copy()
    bad[4] = 20
    with pytest.raises(_lib.PgmiError, match=r"wt_cols\[4\] = 20") as e:
        vespag.op_vespag_head(sd, x, bad)
    assert e.value.code == _lib.EINVAL
    with pytest.raises(_lib.PgmiError, match="hidden 800"):
        vespag.op_vespag_head(vespag.random_state_dict(1, 128, 800), x, wt)


# -- packed rows ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def esm_case():
    """The seeded small ESM2 (2 layers, D = 128, 4 heads), the library, and each sequence's float64 HF rows, run alone."""
    cfg, blob = R.toy_esm()
    hf = R.hf_model(cfg, blob)
    rng = np.random.default_rng(17)
    seqs = [S.random_sequence(rng, L) for L in LENGTHS]
    seqs[1] = seqs[1][:5] + "U" + seqs[1][6:]                                   # tokenised as X
    rows = [_frozen(R.hf_rows(hf, s)) for s in seqs]
    return cfg, blob, hf, tuple(seqs), tuple(rows)


@pytest.fixture(scope="module")
def models():
    """The small ESM2 on the device, one per precision, made on demand and closed with the module."""
    cfg, blob = R.toy_esm()
    live = {}

    def get(precision):
        if precision not in live:
            live[precision] = pesm.EsmModel(cfg, blob, precision=precision)
        return live[precision]
    yield get
    for m in live.values():
        m.close()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_packed_rows_against_the_float64_forward_of_each_sequence_alone(lib, models, precision):
    _, _, _, seqs, want = esm_case()
    esm = models(precision)
    one, st1 = vespag.packed_rows(esm, seqs, want_stats=True)
    assert st1["chunks"] == 1 and st1["tokens"] == sum(LENGTHS) + 2 * len(LENGTHS) and st1["padded_tokens"] == 72 * len(LENGTHS)
    for i, (got, ref) in enumerate(zip(one, want)):
        err = np.abs(got - ref).max()
        print(f"\npacked rows {precision} L={len(seqs[i])}: max |row - HF float64| = {err:.3e}")
        assert got.shape == ref.shape and np.isfinite(got).all() and err <= TOL
    # a row cap that forces more chunks: 70 | 70 | 37, 7 | 1
    many, st = vespag.packed_rows(esm, seqs, row_cap=128, want_stats=True)
    assert st["chunks"] >= 3 and st["padded_tokens"] < st1["padded_tokens"]
    equal = all(np.array_equal(a, b) for a, b in zip(one, many))
    print(f"\npacked rows {precision}: {st['chunks']} chunks vs one: max |diff| = {max(np.abs(a - b).max() for a, b in zip(one, many)):.3e}, "
          f"bit-equal: {equal}")
    # at this shape a row's bits depend neither on the chunk it ran in nor on that chunk's pad length (csrc/api_vespag.hip)
    assert equal
    again = vespag.packed_rows(esm, seqs)
    assert all(np.array_equal(a, b) for a, b in zip(one, again))               # a repeated call returns the same bits


@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_sequence_past_1024_residues(lib, models, precision):
    """L = 1100: the rotary table grows past 1 026 positions and the keys run past 1 024."""
    cfg, blob, hf, _, _ = esm_case()
    seq = S.random_sequence(np.random.default_rng(23), 1100)
    want = R.hf_rows(hf, seq)
    got = vespag.packed_rows(models(precision), [seq, "MKV"])
    err = np.abs(got[0] - want).max()
    print(f"\nL = 1100 {precision}: max |row - HF float64| = {err:.3e}")
    assert got[0].shape == (1100, cfg["embed_dim"]) and err <= TOL
    assert np.abs(got[1] - R.hf_rows(hf, "MKV")).max() <= TOL                   # a 3-residue neighbour padded to 1 102 tokens


@pytest.mark.parametrize("precision", PRECISIONS)
def test_landscapes_equal_the_packed_rows_through_the_head_to_the_bit(lib, models, precision):
    _, _, _, seqs, rows64 = esm_case()
    sd = head_sd(128, 256)
    esm = models(precision)
    with_esm = vespag.from_state_dict(sd, esm=esm, precision=precision)
    alone = vespag.from_state_dict(sd, precision=precision)
    try:
        ys, rows = with_esm.landscapes(seqs, want_rows=True)
        assert all(np.array_equal(a, b) for a, b in zip(rows, vespag.packed_rows(esm, seqs)))
        for s, y, x, x64 in zip(seqs, ys, rows, rows64):
            wt = vespag.wt_columns(s)
            assert np.array_equal(alone.head(x, wt), y) and np.array_equal(with_esm.head(x, wt), y)       # the hand-off adds nothing
            want = R.landscape_y(sd, x64, s)
            muts = R.full_landscape(s)
            got_scores = np.array(list(vespag.score_mutations(y, vespag.landscape(s)).values()))
            e_y, e_s = np.abs(y - want).max(), np.abs(got_scores - R.scores(want, muts)).max()
            print(f"\nlandscape {precision} L={len(s)}: max |y - float64| = {e_y:.3e}, max |score - float64| = {e_s:.3e}, max |y| = {np.abs(want).max():.2f}")
            assert e_y <= TOL and e_s <= TOL
            assert (y[wt >= 0, wt[wt >= 0]] == 0.0).all() and (y[wt < 0] != 0.0).all()
        # calls cut at a residue budget give the same bits as one call
        assert all(np.array_equal(a, b) for a, b in zip(with_esm.landscapes(seqs, max_residues=80), ys))
    finally:
        with_esm.close()
        alone.close()


def test_refusals_that_need_a_handle(lib, models):
    sd = head_sd(128, 256)
    esm = models("f16x3")
    x, wt, _ = head_case(9, 128, 256)
    old = dict(S.ESM1V_650M, layers=1, embed_dim=128, heads=2, ffn_dim=256)
    esm1 = pesm.EsmModel(old, S.random_weights(old, seed=2), max_rows=2048)
    alone = vespag.from_state_dict(sd)
    try:
        with pytest.raises(_lib.PgmiError, match="must be an ESM2 model") as e:
            vespag.from_state_dict(sd, esm=esm1)
        assert e.value.code == _lib.EINVAL
        with pytest.raises(_lib.PgmiError, match="must be an ESM2 model"):
            vespag.packed_rows(esm1, ["MKV"])
        with pytest.raises(_lib.PgmiError, match="no ESM2 model"):
            alone.landscapes(["MKV"])
        with pytest.raises(_lib.PgmiError, match="input_dim 64 differs from the ESM2 model's width 128"):
            vespag.from_state_dict(head_sd(64, 256), esm=esm)
        with pytest.raises(_lib.PgmiError, match="precision"):
            vespag.from_state_dict(sd, esm=esm, precision="fp32")
        with pytest.raises(_lib.PgmiError, match=r"wt_cols\[2\] = -2"):
            alone.head(x, np.where(np.arange(9) == 2, -2, wt))
        bad = x.copy()
        bad[3, 7] = np.inf
        with pytest.raises(_lib.PgmiError, match="element 7 of row 3 is not finite"):
            alone.head(bad, wt)
        # finite rows beyond the fp16 range of the first Linear's split operand: the landscape is read on the host and the call says so
        with pytest.raises(_lib.PgmiError, match="fp16 range") as e:
            alone.head(x * np.float32(1e6), wt)
        assert e.value.code == _lib.EOVERFLOW
        wide = vespag.from_state_dict(sd, precision="fp32")
        try:
            assert np.isfinite(wide.head(x * np.float32(1e6), wt)).all()
        finally:
            wide.close()
    finally:
        alone.close()
        esm1.close()
    cfg, blob = R.toy_esm()
    small = pesm.EsmModel(cfg, blob, max_rows=2048)
    try:
        with pytest.raises(_lib.PgmiError, match="T=2022 exceeds the ESM2 model's workspace rows 2048") as e:
            vespag.packed_rows(small, ["MKV", "A" * 2020])
        assert e.value.code == _lib.EINVAL
        assert vespag.packed_rows(small, ["MKV"])[0].shape == (3, 128)          # the handle is usable after a refusal
    finally:
        small.close()


# -- the CLI on tests/golden/VespaG_toy -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    """The toy's ESM2 as the fair-esm .pt the CLI reads, and the float64 landscape of each protein of the FASTA."""
    cfg, blob, hf, _, _ = esm_case()
    d = tmp_path_factory.mktemp("vespag_toy")
    plm = S.save_fair_esm_checkpoint(str(d / "esm2_toy.pt"), cfg, blob)
    sd = {k: v.numpy() for k, v in torch.load(os.path.join(TOY, "state_dict_v2.pt"), weights_only=True).items()}
    want = vespag.random_state_dict(**R.TOY_HEAD)
    assert all(np.array_equal(sd[k], want[k]) for k in want)                   # the committed head is the generator's seeded one
    seqs = vespag.read_fasta(os.path.join(TOY, "proteins.fasta"))
    ys = {k: R.landscape_y(sd, R.hf_rows(hf, s), s) for k, s in seqs.items()}
    return dict(plm=plm, seqs=seqs, ys=ys)


def _read(path):
    return pd.read_csv(path, float_precision="round_trip")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_cli_predict_on_the_toy_fasta(lib, toy, tmp_path, precision):
    base = ["predict", "-i", os.path.join(TOY, "proteins.fasta"), "--checkpoint-file", os.path.join(TOY, "state_dict_v2.pt"), "--plm", toy["plm"],
            "--precision", precision]
    out1, out2 = str(tmp_path / "multi"), str(tmp_path / "single")
    npz = str(tmp_path / "rows.npz")
    assert cli.main(base + ["-o", out1, "--save-embeddings", npz]) == 0        # the full landscape, one CSV per protein
    for pid, seq in toy["seqs"].items():
        got = _read(os.path.join(out1, pid + ".csv"))
        muts = R.full_landscape(seq)
        assert list(got.columns) == ["mutant", "VespaG"] and list(got["mutant"]) == muts
        assert len(muts) == 19 * len(seq) + ("U" in seq)
        err = np.abs(got["VespaG"].to_numpy() - R.scores(toy["ys"][pid], muts)).max()
        print(f"\nCLI predict {precision} {pid}: max |score - float64| = {err:.3e}")
        assert err <= TOL
    # the mutation file, one CSV for all, from the saved rows and without the logistic
    argv = ["predict", "-i", os.path.join(TOY, "proteins.fasta"), "--checkpoint-file", os.path.join(TOY, "state_dict_v2.pt"), "-e", npz,
            "--precision", precision, "-o", out2, "--single-csv", "--mutation-file", os.path.join(TOY, "mutations.csv"), "--dont-normalize"]
    assert cli.main(argv) == 0
    got = _read(os.path.join(out2, "vespag_scores_all.csv"))
    ref = pd.read_csv(os.path.join(TOY, "mutations.csv"))
    assert list(got.columns) == ["DMS_id", "mutant", "VespaG"]
    ref = pd.concat([ref[ref.iloc[:, 0] == pid] for pid in toy["seqs"]])      # the file's rows, protein by protein in FASTA order
    assert list(got["DMS_id"]) == list(ref.iloc[:, 0]) and list(got["mutant"]) == list(ref.iloc[:, 1])
    want = np.array([R.score(toy["ys"][p], m, normalize=False) for p, m in zip(ref.iloc[:, 0], ref.iloc[:, 1])])
    assert np.abs(got["VespaG"].to_numpy() - want).max() <= TOL
    same = [m[0] == m[-1] and ":" not in m for m in got["mutant"]]
    assert sum(same) == 1 and (got["VespaG"][same] == 0.0).all()               # to_aa == wild type: the masked entry
    assert not os.path.exists(os.path.join(out2, "TOY_A.csv"))


def test_cli_eval_proteingym_on_two_assays(lib, toy, tmp_path):
    out = str(tmp_path / "VespaG")
    argv = ["eval-proteingym", "--reference-file", os.path.join(TOY, "reference.csv"), "--dms-directory", os.path.join(TOY, "DMS"), "-o", out,
            "--checkpoint-file", os.path.join(TOY, "state_dict_v2.pt"), "--plm", toy["plm"]]
    assert cli.main(argv) == 0
    from scipy.stats import spearmanr
    rho = {}
    for pid in ("TOY_A", "TOY_B"):
        dms = pd.read_csv(os.path.join(TOY, "DMS", pid + ".csv"))
        got = _read(os.path.join(out, pid + ".csv"))
        assert list(got.columns) == ["mutant", "VespaG"] and list(got["mutant"]) == list(dms["mutant"])
        want = R.scores(toy["ys"][pid], list(dms["mutant"]))
        assert np.abs(got["VespaG"].to_numpy() - want).max() <= TOL
        rho[pid] = spearmanr(dms["DMS_score"], want).correlation
    assert any(":" in m for m in pd.read_csv(os.path.join(TOY, "DMS", "TOY_B.csv"))["mutant"])
    sp = pd.read_csv(os.path.join(out, "VespaG_Spearman_per_DMS.csv"))
    assert list(sp.columns) == ["DMS_id", "spearman"] and list(sp["DMS_id"]) == ["TOY_A", "TOY_B"]
    assert np.abs(sp["spearman"].to_numpy() - np.array([rho["TOY_A"], rho["TOY_B"]])) .max() < 0.05     # ranks of 30 mutants, scores within 1e-4
    assert sorted(os.listdir(out)) == ["TOY_A.csv", "TOY_B.csv", "VespaG_Spearman_per_DMS.csv"]
