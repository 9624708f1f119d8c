"""ESM C on the MI355X: token and masked-row log-probabilities against the unmodified reference (fp32, CPU) at every frozen shape,
the CLI end to end on the TOY_ESMC_* assays, batch invariance across device chunks, the SwiGLU epilogue and the QK-LayerNorm prep
pass against float64, and the fp16 range guard through the SwiGLU epilogue."""
import ctypes as C
import os

import numpy as np
import pandas as pd
import pytest

from proteingym_amd import _lib, esmc, synthetic as S
from proteingym_amd import score_esmc_proteingym as cli

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHAPES = ["d128", "d192", "d960", "d1152", "d960_full"]
TOL = 1e-4


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLDEN, "golden_esmc.npz"))


def build(g, name, max_rows=0, scale_w1=None):
    D, layers, seed = (int(v) for v in g[f"{name}_cfg"])
    cfg = S.esmc_config(D, layers)
    sd = S.esmc_state_dict(cfg, seed)
    if scale_w1 is not None:
        sd["transformer.blocks.0.ffn.1.weight"] = sd["transformer.blocks.0.ffn.1.weight"] * np.float32(scale_w1)
    blob = esmc.pack(cfg, sd)
    del sd
    return esmc.ESMC(cfg, blob, max_rows=max_rows)


@pytest.mark.parametrize("name", SHAPES)
def test_logprobs_match_reference(lib, g, name, monkeypatch):
    """... and the masked rows, whose last layer runs its row-local stages on those rows only, have the bits of the full
    evaluation (PGMI_KEEP_ROWS=0, read at model creation)."""
    model = build(g, name)
    ids = g[f"{name}_ids"]
    lp = model.token_logprobs(ids[None])[0]
    assert np.abs(lp - g[f"{name}_lp"]).max() <= TOL
    pos = g[f"{name}_mask_pos"]
    mlp = model.masked_logprobs(np.repeat(ids[None], len(pos), 0), pos)
    assert np.abs(mlp - g[f"{name}_mask_lp"]).max() <= TOL
    model.close()
    monkeypatch.setenv("PGMI_KEEP_ROWS", "0")
    full = build(g, name)
    assert np.array_equal(full.masked_logprobs(np.repeat(ids[None], len(pos), 0), pos), mlp)
    full.close()


def run_cli(tmp_path, model_path, *extra):
    dms = tmp_path / "dms"
    dms.mkdir(exist_ok=True)
    for n in ("TOY_ESMC_SHORT", "TOY_ESMC_LONG", "TOY_ESMC_BADLETTER"):
        pd.read_csv(os.path.join(GOLDEN, n + ".csv"))[["mutant", "DMS_score"]].to_csv(dms / f"{n}.csv", index=False)
    out = tmp_path / "out"
    rc = cli.main(["--model_type", "esmc_300M", "--model_path", str(model_path), "--reference_csv", os.path.join(GOLDEN, "TOY_ESMC_REFERENCE.csv"),
                   "--dms_dir", str(dms), "--output_dir", str(out), *extra])
    assert rc == 0
    return out


@pytest.fixture(scope="module")
def toy_pth(tmp_path_factory):
    torch = pytest.importorskip("torch")
    cfg = S.esmc_config(128, 2)
    path = tmp_path_factory.mktemp("esmc") / "toy.pth"
    torch.save({k: torch.from_numpy(v) for k, v in S.esmc_state_dict(cfg, 31).items()}, path)
    return path


def test_cli_matches_reference_csvs(lib, tmp_path, toy_pth):
    out = run_cli(tmp_path, toy_pth)
    for n in ("TOY_ESMC_SHORT", "TOY_ESMC_LONG"):
        got, ref = pd.read_csv(out / f"{n}.csv"), pd.read_csv(os.path.join(GOLDEN, n + ".csv"))
        assert list(got.columns) == list(ref.columns)
        assert got["mutant"].tolist() == ref["mutant"].tolist()
        assert got["esmc_300M_score"].isna().tolist() == ref["esmc_300M_score"].isna().tolist()
        ok = ref["esmc_300M_score"].notna()
        assert np.abs(got["esmc_300M_score"][ok] - ref["esmc_300M_score"][ok]).max() <= TOL, n
    assert not (out / "TOY_ESMC_BADLETTER.csv").exists()
    summary = pd.read_csv(out / "correlation_summary_esmc_300M.csv")
    assert summary["assay"].tolist() == ["TOY_ESMC_SHORT", "TOY_ESMC_LONG", "TOY_ESMC_BADLETTER"]
    assert summary["correlation"][:2].notna().all() and np.isnan(summary["correlation"][2])


def test_batch_invariance(lib, tmp_path, toy_pth):
    """2048 workspace rows: two of the long assay's 1024-token rows per device chunk (seven chunks), the same scores bit for bit."""
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    a, b = run_cli(tmp_path / "a", toy_pth), run_cli(tmp_path / "b", toy_pth, "--max_rows", "2048")
    for n in ("TOY_ESMC_SHORT", "TOY_ESMC_LONG"):
        assert pd.read_csv(a / f"{n}.csv")["esmc_300M_score"].equals(pd.read_csv(b / f"{n}.csv")["esmc_300M_score"]), n


def test_swiglu_epilogue_against_float64(lib):
    rng = np.random.default_rng(5)
    for M, N, K in ((77, 128, 64), (300, 1024, 192), (513, 5120, 960)):
        A = rng.standard_normal((M, K), dtype=np.float32)
        W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
        b = (0.1 * rng.standard_normal(N)).astype(np.float32)
        out = np.empty((M, N // 2), dtype=np.float32)
        _lib.check(lib.pgmi_op_gemm(0, _lib.PREC_F16X3, _lib.ptr(A, _lib._f32p), _lib.ptr(W, _lib._f32p), _lib.ptr(b, _lib._f32p), None,
                                    M, N, K, 4 + 256, _lib.ptr(out, _lib._f32p)))
        y = A.astype(np.float64) @ W.astype(np.float64).T + b
        blk = y.reshape(M, N // 64, 64)
        gate, up = blk[:, :, :32].reshape(M, N // 2), blk[:, :, 32:].reshape(M, N // 2)
        want = gate / (1.0 + np.exp(-gate)) * up
        assert np.abs(out - want).max() <= 2e-5 * max(1.0, np.abs(want).max()), (M, N, K)
    bad = np.empty(64, dtype=np.float32)
    rc = lib.pgmi_op_gemm(0, _lib.PREC_F16X3, _lib.ptr(A, _lib._f32p), _lib.ptr(W, _lib._f32p), None, None, M, N, K, 4,
                          _lib.ptr(bad, _lib._f32p))
    assert rc == _lib.EINVAL                                        # the SwiGLU epilogue writes split planes only


def test_qkln_prep_against_float64(lib):
    rng = np.random.default_rng(6)
    for B, T, H in ((2, 45, 2), (1, 100, 15), (3, 70, 18)):
        D = 64 * H
        qkv = (3.0 * rng.standard_normal((B * T, 3 * D)) + 0.5).astype(np.float32)
        qw, kw = (1.0 + 0.1 * rng.standard_normal(D)).astype(np.float32), (1.0 + 0.1 * rng.standard_normal(D)).astype(np.float32)
        qk = np.empty((B * T, 2 * D), dtype=np.float32)
        v = np.empty((B * T, D), dtype=np.float32)
        _lib.check(lib.pgmi_op_qkln_prep(0, _lib.ptr(qkv, _lib._f32p), _lib.ptr(qw, _lib._f32p), _lib.ptr(kw, _lib._f32p), B, T, H, 0,
                                         _lib.ptr(qk, _lib._f32p), _lib.ptr(v, _lib._f32p), None))
        x = qkv.astype(np.float64)
        inv = (1.0 / (10000 ** (np.arange(0, 64, 2, dtype=np.float32) / np.float32(64)))).astype(np.float32)
        ang = (np.arange(T, dtype=np.float32)[:, None] * inv[None, :]).astype(np.float64)
        cos, sin = np.tile(np.concatenate([np.cos(ang)] * 2, -1), (B, 1))[:, None], np.tile(np.concatenate([np.sin(ang)] * 2, -1), (B, 1))[:, None]

        def ln_rot(a, w):
            a = (a - a.mean(-1, keepdims=True)) / np.sqrt(a.var(-1, keepdims=True) + 1e-5) * w
            a = a.reshape(B * T, H, 64)
            return (a * cos + np.concatenate([-a[..., 32:], a[..., :32]], -1) * sin).reshape(B * T, D)
        assert np.abs(qk[:, :D] - ln_rot(x[:, :D], qw) * np.log2(np.e)).max() <= 1e-5 * 8
        assert np.abs(qk[:, D:] - ln_rot(x[:, D:2 * D], kw)).max() <= 1e-5 * 8
        assert np.abs(v - x[:, 2 * D:]).max() <= 1e-6 * np.abs(x).max()


def test_overflow_through_swiglu_trips_the_range_guard(lib, g):
    """FC1 weights of the first block times 1e4: silu(gate) * up leaves fp16's range inside the SwiGLU epilogue; the NaN / Inf it
    carries reaches the log-softmax and the call returns PGMI_EOVERFLOW (no wrong finite number)."""
    model = build(g, "d128", scale_w1=1e4)
    ids = g["d128_ids"]
    with pytest.raises(_lib.PgmiError) as e:
        model.masked_logprobs(ids[None], np.array([5], dtype=np.int32))
    assert e.value.code == _lib.EOVERFLOW
    model.close()
    ok = build(g, "d128")
    assert np.isfinite(ok.masked_logprobs(ids[None], np.array([5], dtype=np.int32))).all()
    ok.close()


def test_config_refusals(lib):
    for kw, msg in ((dict(precision=_lib.PREC_BF16), b"f16x3"), (dict(heads=4), b"head_dim 64"), (dict(vocab=33), b"vocab")):
        c = dict(abi_version=_lib.ABI_VERSION, arch=_lib.ARCH_ESMC, layers=1, embed_dim=128, heads=2, ffn_dim=512, vocab=64,
                 precision=_lib.PREC_F16X3)
        c.update(kw)
        cfg = _lib.Config(**c)
        w = np.zeros(1, dtype=np.float32)
        h = C.c_void_p()
        assert lib.pgmi_model_create(C.byref(cfg), _lib.ptr(w, _lib._f32p), 1, 0, C.byref(h)) == _lib.EINVAL
        assert msg in lib.pgmi_last_error()
