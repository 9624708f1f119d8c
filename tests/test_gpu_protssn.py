"""ProtSSN on the MI355X against the float64 torch restatement (tests/protssn_ref.py): one layer's message and aggregation alone
(pgmi_op_egnn_message), one layer plus the head at the released width, six layers at three sizes, the whole path over a small seeded
ESM2 (pgmi_esm_residue_rows into the GNN, against a float64 HF EsmModel on the CPU), the CLI on the toy folder of
tests/golden/ProtSSN_toy, the bits of a checkpoint across runs / calls / edge chunks, and the refusals that need a handle.

Bounds: log-probabilities, scores and message sums within the flat 1e-4 of DESIGN.md section 3, in both precisions.  Weights are
Xavier-normal times 0.5 (protssn.random_state_dict): at that gain the fp32 restatement is within 1.1e-6 of float64, at the reference's
own gain 1.0 the softmax saturates at the 1e-9 floor and fp32 itself misses the bound.  Shapes: D = 128 gives a first edge Linear of
700 columns (704 padded), D = 1280 the released 5308 (5312); L = 9 has 8 neighbours per node (fewer than k), 37 is odd, 70 is past two
64-row tiles; the op's coordinates hold an in-degree of 44 (above 32), an in-degree of 0 and a residue beyond 30 A of everything."""
import ctypes as C
import functools
import os

import numpy as np
import pandas as pd
import pytest
import torch

import protssn_ref as R
from proteingym_amd import _lib, protssn, synthetic as S
from proteingym_amd import esm as pesm
from proteingym_amd import score_protssn_proteingym as cli

pytestmark = pytest.mark.gpu
TOL = 1e-4
PRECISIONS = ["f16x3", "fp32"]
TOY = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ProtSSN_toy")


def _frozen(d):
    for v in d.values():
        v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def state_dict(D, h, layers, seed=5):
    return _frozen(protssn.random_state_dict(seed, D, h, gain=0.5, layers=layers, bias_std=0.02))


@functools.lru_cache(maxsize=None)
def norm(k):
    return protssn.load_norm(k, norm_dir=TOY)


def _sph(colat, az):
    c, a = np.radians(colat), np.radians(az)
    return np.array([np.sin(c) * np.cos(a), np.sin(c) * np.sin(a), -np.cos(c)])


@functools.lru_cache(maxsize=None)
def hub_case():
    """45 residues around a hub at the origin: four clusters of ten 8 A from it in directions at least 66 degrees apart (a member's ten
    nearest are its nine mates and the hub), two lone residues W at 8 A, a residue Z at 8.3 A that nobody has among its ten nearest,
    and a residue X 31 A away on the far side, beyond 30 A of everything, whose nearest is the hub.  Indices are shuffled."""
    rng = np.random.default_rng(8)
    ring = [_sph(94, az) for az in (36, 108, 180, 252, 324)]
    pts = [np.zeros(3)]
    for u in (ring[1], ring[4], _sph(35, 0), _sph(35, 144)):
        pts += list(8.0 * u + 0.05 * rng.standard_normal((10, 3)))
    pts += [8.0 * ring[2], 8.0 * ring[3], 8.3 * ring[0], np.array([0.0, 0.0, 31.0])]
    perm = rng.permutation(45)
    ca = np.array(pts)[perm]
    where = {name: int(np.where(perm == i)[0][0]) for name, i in (("hub", 0), ("Z", 43), ("X", 44))}
    n, ca, c = R.toy_backbone(ca, seed=3)
    graph = protssn.build_graph(n, ca, c, 10, norm(10))
    return ca, where, _frozen(dict(zip(("pos", "centre", "nb", "ea"), graph)))


@functools.lru_cache(maxsize=None)
def serpentine_case(L, k=10):
    n, ca, c = R.toy_backbone(R.serpentine(L, seed=1), seed=2)
    return _frozen(dict(zip(("pos", "centre", "nb", "ea"), protssn.build_graph(n, ca, c, k, norm(k)))))


@functools.lru_cache(maxsize=None)
def rows(L, D, seed=13):
    """Stand-ins for ESM2's residue rows: unit-variance rows, as emb_layer_norm_after leaves them."""
    x = np.random.default_rng(seed).standard_normal((L, D)).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def reference(D, h, layers, L):
    """float64 (lp, hidden) of the serpentine case, computed once."""
    g = serpentine_case(L)
    lp, hid = R.forward(state_dict(D, h, layers), rows(L, D), g["pos"], g["centre"], g["nb"], g["ea"], layers=layers)
    return lp.numpy(), hid.numpy()


def run(D, h, layers, g, x, precision, edge_chunk=0, want_hidden=False):
    m = protssn.from_state_dict(state_dict(D, h, layers), D, h, layers, precision=precision, edge_chunk=edge_chunk)
    try:
        m.set_graph(g["pos"], g["centre"], g["nb"], g["ea"])
        return m.forward(x, want_hidden=want_hidden)
    finally:
        m.close()


def test_hub_case_has_the_degrees_the_op_test_needs():
    ca, where, g = hub_case()
    indeg = np.bincount(g["nb"], minlength=45)
    assert len(ca) == 45 and indeg[where["hub"]] == 44 > 32 and indeg[where["Z"]] == 0
    d = np.sqrt(((ca - ca[where["X"]]) ** 2).sum(1))
    assert np.sort(d)[1] > 30 and g["nb"][g["centre"] == where["X"]].tolist() == [where["hub"]]     # beyond 30 A: its one edge goes to the nearest
    assert len(g["centre"]) == 44 * 10 + 1 and protssn.dims(128, 64)["Hp"] == 704 != protssn.dims(128, 64)["Hh"]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("edge_chunk", [0, 100])
def test_op_egnn_message_against_float64(lib, precision, edge_chunk):
    D, h = 128, 64
    _, where, g = hub_case()
    sd, x = state_dict(D, h, 1), rows(45, D)
    want = R.message_sums(sd, x, g["pos"], g["centre"], g["nb"], g["ea"])
    got = protssn.op_egnn_message(sd, D, h, g["pos"], g["centre"], g["nb"], g["ea"], x, precision=precision, edge_chunk=edge_chunk)
    err = np.abs(got - want)
    print(f"\nop {precision} chunk {edge_chunk}: max |m_i - float64| = {err.max():.3e} (hub row {err[where['hub']].max():.3e}), max |m_i| = {np.abs(want).max():.3f}")
    assert got.shape == (45, h) and np.isfinite(got).all()
    assert not got[where["Z"]].any() and not got[where["X"]].any()          # in-degree 0: exactly zero
    assert not want[where["Z"]].any()
    assert np.abs(want[where["hub"]]).max() > 0.1                            # 44 messages arrive at the hub
    assert err.max() <= TOL


@pytest.mark.parametrize("precision", PRECISIONS)
def test_real_width_one_layer_and_head(lib, precision):
    D, h, L = 1280, 512, 19
    assert protssn.dims(D, h)["Hh"] == 5308 and protssn.dims(D, h)["Hp"] == 5312
    want, want_hid = reference(D, h, 1, L)
    got, hid = run(D, h, 1, serpentine_case(L), rows(L, D), precision, want_hidden=True)
    err = np.abs(got - want).max()
    print(f"\nreal width {precision}: max |lp - float64| = {err:.3e}, max |hidden - float64| = {np.abs(hid - want_hid).max():.3e}, min lp {want.min():.2f}")
    assert np.isfinite(got).all() and err <= TOL
    assert np.abs(np.exp(got).sum(1) - 1).max() < 1e-5


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("h", [64, 96])
@pytest.mark.parametrize("L", [9, 37, 70])
def test_six_layers_against_float64(lib, precision, h, L):
    D = 128
    g = serpentine_case(L)
    if L == 9:
        assert np.bincount(g["centre"]).tolist() == [8] * 9                  # fewer than k within 30 A: every other residue
    want, _ = reference(D, h, 6, L)
    got = run(D, h, 6, g, rows(L, D), precision)
    err = np.abs(got - want).max()
    print(f"\nsix layers {precision} h={h} L={L}: max |lp - float64| = {err:.3e}, lp range [{want.min():.2f}, {want.max():.3f}]")
    assert np.isfinite(got).all() and err <= TOL
    assert want.min() > -18                                                  # off the 1e-9 floor: the comparison reads real digits


@functools.lru_cache(maxsize=None)
def esm_case():
    """The toy's seeded two-layer ESM2 as a float64 HF EsmModel, its state dict through the HF key map, and a 37-residue sequence."""
    cfg, blob = R.toy_esm()
    hf = R.fair_to_hf(S.blob_to_arrays(cfg, blob), cfg)
    seq = S.random_sequence(np.random.default_rng(17), 37)
    return hf, seq, R.hf_residue_rows(hf, protssn.tokenize(seq))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_end_to_end_esm_rows_into_the_gnn(lib, precision):
    hf, seq, rows64 = esm_case()
    cfg, fair = protssn.hf_to_fair({k: v.float() for k, v in hf.state_dict().items()}, hf.config.to_dict())
    D, h, L = cfg["embed_dim"], 64, len(seq)
    g = serpentine_case(L)
    want, _ = R.forward(state_dict(D, h, 6), rows64, g["pos"], g["centre"], g["nb"], g["ea"])
    esm = pesm.EsmModel(cfg, pesm.pack_state_dict(cfg, fair), precision=precision)
    try:
        got_rows = protssn.residue_rows(esm, seq)
        with pytest.raises(_lib.PgmiError, match="T = 2"):
            _lib.check(lib.pgmi_esm_residue_rows(esm._h, _lib.ptr(protssn.tokenize(""), _lib._i32p), 2, _lib.ptr(got_rows, _lib._f32p)))
    finally:
        esm.close()
    got = run(D, h, 6, g, got_rows, precision)
    err = np.abs(got - want.numpy()).max()
    print(f"\nend to end {precision}: max |rows - HF float64| = {np.abs(got_rows - rows64).max():.3e}, max |lp - float64| = {err:.3e}")
    assert got_rows.shape == (L, D) and err <= TOL


@pytest.fixture(scope="module")
def toy_files(tmp_path_factory):
    """The toy's seeded models as the files the CLI reads: a fair-esm ESM2 .pt, two ProtSSN checkpoints, the yaml."""
    d = tmp_path_factory.mktemp("protssn_toy")
    cfg, blob = R.toy_esm()
    plm = S.save_fair_esm_checkpoint(str(d / "esm2_toy.pt"), cfg, blob)
    for name, k, h, seed in R.TOY_MODELS:
        torch.save({key: torch.from_numpy(v) for key, v in R.toy_state_dict(h, seed).items()}, str(d / f"protssn_{name}.pt"))
    yml = d / "egnn.yaml"
    yml.write_text("egnn:\n  edge_attr_dim: 93\n  output_dim: 20\n  dropout: 0\n  n_layers: 6\n  residual: False\n  embedding: False\n"
                   "  embedding_dim: 64\n  mlp_num: 2\n")
    return dict(dir=str(d), plm=plm, yml=str(yml))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_cli_on_the_toy_folder(lib, toy_files, tmp_path, precision):
    out = str(tmp_path / "scores")
    argv = ["--gnn_config", toy_files["yml"], "--gnn_model_dir", toy_files["dir"], "--gnn_model_name", "k10_h64", "k20_h96", "--use_ensemble",
            "--mutant_dataset_dir", TOY, "--output_scores_folder", out, "--plm", toy_files["plm"], "--norm_dir", TOY, "--test_widths",
            "--precision", precision, "--score_info", str(tmp_path / "info.csv")]
    assert cli.main(argv) == 0
    ref = pd.read_csv(os.path.join(TOY, "reference.csv"))
    got = pd.read_csv(os.path.join(out, R.TOY_NAME + ".csv"))
    assert list(got.columns) == ["mutant", "DMS_score", "ProtSSN_k10_h64", "ProtSSN_k20_h96", "ProtSSN_ensemble"]
    assert list(got["mutant"]) == list(ref["mutant"]) and np.array_equal(got["DMS_score"], ref["DMS_score"])
    for col in got.columns[2:]:
        err = np.abs(got[col] - ref[col]).max()
        print(f"\nCLI {precision} {col}: max |score - float64| = {err:.3e}")
        assert err <= TOL
    assert (got.iloc[-2:, 2:] == 0).all().all()                              # the wt rows
    info = pd.read_csv(tmp_path / "info.csv")
    assert list(info["name"]) == [R.TOY_NAME] and info["count"][0] == len(ref) and "ProtSSN_k10_h64" in info.columns
    first = got["ProtSSN_ensemble"].to_numpy().copy()
    assert cli.main(argv + ["--DMS_index", "0"]) == 0                        # a second run leaves the ensemble unchanged
    again = pd.read_csv(os.path.join(out, R.TOY_NAME + ".csv"))
    assert np.array_equal(again["ProtSSN_ensemble"].to_numpy(), first) and list(again.columns) == list(got.columns)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_bits_do_not_depend_on_run_call_or_chunk(lib, precision):
    D, L = 128, 37
    x, g10 = rows(L, D), serpentine_case(L, 10)
    base = run(D, 64, 6, g10, x, precision)
    assert np.array_equal(run(D, 64, 6, g10, x, precision), base)           # two runs
    for chunk in (1, 7, 64, 369, 100000):                                    # 370 edges: one per chunk, ragged tails, one short of all, all
        assert np.array_equal(run(D, 64, 6, g10, x, precision, edge_chunk=chunk), base), chunk
    # a checkpoint alone and as one of two in a call, on the same structure
    n, ca, c = R.toy_backbone(R.serpentine(L, seed=1), seed=2)
    norms = {10: norm(10), 20: norm(20)}
    a = protssn.from_state_dict(state_dict(D, 64, 6), D, 64, 6, precision=precision)
    b = protssn.from_state_dict(state_dict(D, 96, 6, seed=6), D, 96, 6, precision=precision)
    try:
        alone = protssn.score_structure({"a": (10, a)}, x, n, ca, c, norms)["a"]
        both = protssn.score_structure({"b": (20, b), "a": (10, a)}, x, n, ca, c, norms)
        assert np.array_equal(alone, base) and np.array_equal(both["a"], base)
        assert np.array_equal(protssn.score_structure({"b": (20, b)}, x, n, ca, c, norms)["b"], both["b"])
    finally:
        a.close()
        b.close()


def test_refusals_that_need_a_handle(lib):
    D, h, L = 128, 64, 9
    g = serpentine_case(L)
    m = protssn.from_state_dict(state_dict(D, h, 1), D, h, 1)
    try:
        with pytest.raises(_lib.PgmiError, match="no graph set"):
            _lib.check(lib.pgmi_protssn_forward(m._h, _lib.ptr(rows(L, D), _lib._f32p), _lib.ptr(np.empty((L, 20), np.float32), _lib._f32p), None))
        with pytest.raises(_lib.PgmiError, match="L = 1") as e:
            m.set_graph(g["pos"][:1], g["centre"][:1], g["nb"][:1], g["ea"][:1])
        assert e.value.code == _lib.EINVAL
        bad = g["nb"].copy()
        bad[5] = L
        with pytest.raises(_lib.PgmiError, match="edge 5"):
            m.set_graph(g["pos"], g["centre"], bad, g["ea"])
        bad[5] = g["centre"][5]
        with pytest.raises(_lib.PgmiError, match="self edge"):
            m.set_graph(g["pos"], g["centre"], bad, g["ea"])
        ea = g["ea"].copy()
        ea[3, 70] = np.nan
        with pytest.raises(_lib.PgmiError, match="edge attribute 70 of edge 3"):
            m.set_graph(g["pos"], g["centre"], g["nb"], ea)
        m.set_graph(g["pos"], g["centre"], g["nb"], g["ea"])
        with pytest.raises(ValueError, match="esm_rep"):
            m.forward(rows(L + 1, D))
        x = rows(L, D).copy()
        x[2, 2] = np.inf
        with pytest.raises(_lib.PgmiError, match="not finite"):
            m.forward(x)
        assert np.isfinite(m.forward(rows(L, D))).all()                      # the handle still works after the refusals
    finally:
        m.close()
    with pytest.raises(_lib.PgmiError, match="weight blob"):
        protssn.ProtSSN(np.zeros(10, np.float32), D, h, 1)
    two = protssn.ProtssnConfig(abi_version=_lib.ABI_VERSION, node_in=D, hidden=h, layers=2, edge_attr_dim=93, precision=_lib.PREC_FP32)
    out = np.empty((L, h), np.float32)
    with pytest.raises(_lib.PgmiError, match="one-layer"):
        _lib.check(lib.pgmi_op_egnn_message(0, C.byref(two), None, 0, None, L, 1, None, None, None, _lib.ptr(rows(L, D), _lib._f32p),
                                            _lib.ptr(out, _lib._f32p)))
