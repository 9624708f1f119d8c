"""ProGen2 on the GPU against the reference's own outputs (tests/golden/make_golden_progen2.py): token log-probabilities at every
toy head dim and at real width, calc_fitness scores through the CLI, batch invariance, and the tanh-GELU GEMM epilogue."""
import os

import numpy as np
import pandas as pd
import pytest

from proteingym_amd import _lib, progen2 as pg, synthetic as S

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOY = {"h32": (256, 8, 16, 11), "h64": (512, 8, 32, 12), "h64_full_rotary": (512, 8, 64, 13), "h80": (640, 8, 32, 14),
       "h96": (768, 8, 48, 15), "h128": (1024, 8, 64, 16),
       "h256": (2048, 8, 64, 17), "h256_full_rotary": (2048, 8, 256, 18)}


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "golden_progen2.npz"))


def toy_model(name, max_rows=4096):
    D, H, rd, seed = TOY[name]
    cfg = S.progen2_config(2, D, H, rd, n_positions=96)
    return pg.ProGen2Model(cfg, pg.pack(cfg, S.progen2_state_dict(cfg, seed)), max_rows=max_rows)


@pytest.mark.parametrize("name", list(TOY))
def test_token_logprobs_toy(golden, name):
    m = toy_model(name)
    try:
        for T in (20, 77, 96):
            ids, ref = golden[f"{name}_T{T}_ids"], golden[f"{name}_T{T}_lp"]
            lp = m.token_logprobs(ids)
            err = float(np.abs(lp - ref).max())
            assert err <= 1e-4, (name, T, err)
    finally:
        m.close()


@pytest.mark.parametrize("width", list(S.PROGEN2_WIDTHS))
def test_token_logprobs_real_width(width):
    g = np.load(os.path.join(GOLDEN, "golden_progen2_real_width.npz"))
    w = S.PROGEN2_WIDTHS[width]
    cfg = S.progen2_config(2, w["embed_dim"], w["heads"], w["rotary_dim"])
    m = pg.ProGen2Model(cfg, pg.pack(cfg, S.progen2_state_dict(cfg, int(g[f"{width}_seed"]))), max_rows=4096)
    try:
        lp = m.token_logprobs(g[f"{width}_ids"])
        err = float(np.abs(lp - g[f"{width}_lp64"]).max())
        tol = max(1e-4, 3 * float(g[f"{width}_noise32"]))        # the house rule of test_gpu_parity_real_width.py
        assert err <= tol, (width, err, tol)
    finally:
        m.close()


def _toy_checkpoint(tmp_path):
    cfg = S.progen2_config(2, 512, 8, 32, n_positions=96)
    path = str(tmp_path / "progen2-toy")
    S.save_progen2_checkpoint(path, cfg, S.progen2_state_dict(cfg, 12))
    return path


@pytest.mark.parametrize("index,dms_id", [(0, "TOY_PROGEN2_SUB"), (1, "TOY_PROGEN2_SUB_SEQ"), (2, "TOY_PROGEN2_INDEL"),
                                          (3, "TOY_PROGEN2_LONG")])
def test_cli_scores_match_reference(golden, tmp_path, index, dms_id):
    from proteingym_amd import score_progen2_proteingym as cli
    ckpt = _toy_checkpoint(tmp_path)
    argv = ["--Progen2_model_name_or_path", ckpt, "--DMS_reference_file_path", os.path.join(GOLDEN, "TOY_PROGEN2_REFERENCE.csv"),
            "--DMS_data_folder", GOLDEN, "--DMS_index", str(index), "--output_scores_folder", str(tmp_path / "out"), "--fp16"]
    if dms_id == "TOY_PROGEN2_INDEL":
        argv.append("--indel_mode")
    out = cli.main(argv)
    assert out.endswith(dms_id + ".csv")
    df = pd.read_csv(out)
    assert list(df.columns) == ["mutant", "Progen2_score", "DMS_score"]
    ref = golden[f"score_{dms_id}"]
    err = float(np.abs(df["Progen2_score"].to_numpy() - ref).max())
    assert err <= 1e-4, (dms_id, err)


def test_batch_invariance():
    m = toy_model("h80")
    try:
        rng = np.random.default_rng(3)
        rows = rng.integers(5, 30, size=(9, 57)).astype(np.int32)
        rows[:, 0] = 3
        rows[4, -1] = 4
        alone, k_alone = m.sequence_loglik(rows[4:5])
        full, k_full = m.sequence_loglik(rows)
        part, _ = m.sequence_loglik(rows[2:7])
        assert np.array_equal(alone, full[4:5]) and np.array_equal(alone, part[2:3])
        assert k_alone[0] == 55 and k_full[0] == 56
        lp_a = m.token_logprobs(rows[4:5, :-1])
        lp_b = m.token_logprobs(rows[:, :-1])
        assert np.array_equal(lp_a[0], lp_b[4])
    finally:
        m.close()


def test_tanh_gelu_epilogue():
    lib = _lib.load()
    rng = np.random.default_rng(5)
    M, N, K = 200, 256, 128
    A = (rng.standard_normal((M, K)) * 0.5).astype(np.float32)
    W = (rng.standard_normal((N, K)) / np.sqrt(K) * 4).astype(np.float32)
    b = (rng.standard_normal(N) * 0.5).astype(np.float32)
    u = A.astype(np.float64) @ W.T.astype(np.float64) + b
    ref = 0.5 * u * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) * (u + 0.044715 * u ** 3)))
    for prec, epi, tol in ((_lib.PREC_F16X3, 3, 2e-5), (_lib.PREC_F16X3, 3 + 256, 2e-3), (_lib.PREC_FP32, 3, 2e-5)):
        out = np.empty((M, N), dtype=np.float32)
        _lib.check(lib.pgmi_op_gemm(0, prec, _lib.ptr(A, _lib._f32p), _lib.ptr(W, _lib._f32p), _lib.ptr(b, _lib._f32p), None,
                                    M, N, K, epi, _lib.ptr(out, _lib._f32p)))
        err = float(np.abs(out - ref).max())
        assert err <= tol, (prec, epi, err)
        assert out.min() < -0.1                                  # the negative lobe is exercised
