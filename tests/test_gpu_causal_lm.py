"""RITA / ProtGPT2 on the GPU against the reference's own outputs (tests/golden/make_golden_rita.py, make_golden_protgpt2.py): token
log-probabilities at head dims 32 / 64 / 128 (RITA, narrow head) and on a toy BPE vocabulary (GPT-2, wide head), the wide head at
ProtGPT2's vocabulary against a float64 forward, CLI scores, batch invariance and the degenerate-chunk error."""
import os

import numpy as np
import pandas as pd
import pytest

from causal_lm_ref import numpy_forward
from proteingym_amd import causal_lm as clm, synthetic as S

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RITA_TOK = os.path.join(GOLDEN, "rita_toy_tokenizer")
GPT2_TOK = os.path.join(GOLDEN, "protgpt2_toy_tokenizer")
RITA_TOY = {"h32": (128, 4, 21), "h64": (256, 4, 22), "h128": (256, 2, 23)}
GPT2_TOY = {"h32": (128, 4, 31), "h64": (128, 2, 32)}


@pytest.fixture(scope="module")
def g_rita():
    return np.load(os.path.join(GOLDEN, "golden_rita.npz"))


@pytest.fixture(scope="module")
def g_gpt2():
    return np.load(os.path.join(GOLDEN, "golden_protgpt2.npz"))


def rita_model(name, max_rows=4096):
    D, H, seed = RITA_TOY[name]
    cfg = S.rita_config(2, D, H)
    return clm.CausalLM(cfg, clm.pack(cfg, S.rita_state_dict(cfg, seed)), max_rows=max_rows)


def gpt2_model(name, V, max_rows=4096):
    D, H, seed = GPT2_TOY[name]
    cfg = S.gpt2_config(2, D, H, V)
    return clm.CausalLM(cfg, clm.pack(cfg, S.gpt2_state_dict(cfg, seed)), max_rows=max_rows)


@pytest.mark.parametrize("family,name", [("rita", n) for n in RITA_TOY] + [("gpt2", n) for n in GPT2_TOY])
def test_token_logprobs_toy(g_rita, g_gpt2, family, name):
    g = g_rita if family == "rita" else g_gpt2
    m = rita_model(name) if family == "rita" else gpt2_model(name, int(g["vocab_size"]))
    try:
        for T in (20, 77):
            ids, ref = g[f"{name}_T{T}_ids"], g[f"{name}_T{T}_lp"]
            err = float(np.abs(m.token_logprobs(ids) - ref).max())
            assert err <= 1e-4, (family, name, T, err)
    finally:
        m.close()


@pytest.mark.parametrize("T", [97, 129, 1024])
@pytest.mark.parametrize("family,name", [("rita", "h64"), ("rita", "h128"), ("gpt2", "h64")])
def test_token_logprobs_longer_contexts(g_gpt2, family, name, T):
    """The toy models beyond T = 77, up to the families' real context: four and more key tiles, several query blocks per sequence, the
    LDS ring wrapping.  Against the float64 forward over the packed blob; the bound is max(1e-4, 3 noise32), noise32 = the same forward
    in plain fp32 against the float64 one (the rule of test_gpu_progen2.py::test_token_logprobs_real_width)."""
    m = rita_model(name) if family == "rita" else gpt2_model(name, int(g_gpt2["vocab_size"]))
    try:
        cfg = m.cfg
        D, H, seed = (RITA_TOY if family == "rita" else GPT2_TOY)[name]
        blob = clm.pack(cfg, (S.rita_state_dict if family == "rita" else S.gpt2_state_dict)(cfg, seed))
        ids = np.random.default_rng(T + D + H).integers(0, cfg["vocab"], (1 if T == 1024 else 2, T)).astype(np.int32)
        lp = m.token_logprobs(ids)
        for b, row in enumerate(ids):
            ref = numpy_forward(cfg, blob, row)
            noise32 = float(np.abs(numpy_forward(cfg, blob, row, np.float32) - ref).max())
            err, tol = float(np.abs(lp[b] - ref).max()), max(1e-4, 3 * noise32)
            print(f"causal_lm long {family} {name} T={T} row={b} err={err:.3e} noise32={noise32:.3e} tol={tol:.3e}")
            assert err <= tol, (family, name, T, b, err, tol)
    finally:
        m.close()


def test_wide_head_at_protgpt2_vocabulary():
    """V = 50 257 (pad columns up to 50 304), D = 1280, 2 layers, T = 45: full rows and scored targets against float64."""
    sh = S.PROTGPT2_SHAPE
    cfg = S.gpt2_config(2, sh["embed_dim"], sh["heads"], sh["vocab"], max_positions=sh["max_positions"])
    blob = clm.pack(cfg, S.gpt2_state_dict(cfg, 77))
    m = clm.CausalLM(cfg, blob, max_rows=4096)
    try:
        rng = np.random.default_rng(6)
        ids = rng.integers(0, sh["vocab"], 46).astype(np.int32)
        ids[:3] = [sh["vocab"] - 1, sh["vocab"] - 2, 0]             # the last real columns, next to the pad columns
        ref = numpy_forward(cfg, blob, ids[:-1])
        lp = m.token_logprobs(ids[None, :-1])[0]
        err = float(np.abs(lp - ref).max())
        assert err <= 1e-4, err
        s, n = m.sequence_loglik([ids, ids[:30]])
        want = [ref[np.arange(45), ids[1:]].sum(), ref[np.arange(29), ids[1:30]].sum()]
        assert n.tolist() == [45, 29]
        assert np.abs(s - want).max() <= 45e-4, (s, want)
    finally:
        m.close()


def _checkpoint(tmp_path, family, V=None):
    if family == "rita":
        cfg = S.rita_config(2, 256, 4)
        sd = S.rita_state_dict(cfg, 22)
    else:
        cfg = S.gpt2_config(2, 128, 2, V)
        sd = S.gpt2_state_dict(cfg, 32)
    path = str(tmp_path / f"{family}-toy")
    S.save_causal_lm_checkpoint(path, cfg, sd)
    return path


@pytest.mark.parametrize("family", ["rita", "protgpt2"])
@pytest.mark.parametrize("index,kind", [(0, "SUB"), (1, "SUB_SEQ"), (2, "INDEL"), (3, "LONG")])
def test_cli_scores_match_reference(g_rita, g_gpt2, tmp_path, family, index, kind):
    from proteingym_amd import score_protgpt2_proteingym as gcli, score_rita_proteingym as rcli
    rita = family == "rita"
    prefix = "TOY_RITA" if rita else "TOY_PROTGPT2"
    ckpt = _checkpoint(tmp_path, "rita" if rita else "gpt2", None if rita else int(g_gpt2["vocab_size"]))
    argv = ["--RITA_model_name_or_path" if rita else "--ProtGPT2_model_name_or_path", ckpt,
            "--DMS_reference_file_path", os.path.join(GOLDEN, prefix + "_REFERENCE.csv"), "--DMS_data_folder", GOLDEN,
            "--DMS_index", str(index), "--output_scores_folder", str(tmp_path / "out"),
            "--tokenizer_path", RITA_TOK if rita else GPT2_TOK]
    if kind == "INDEL":
        argv.append("--indel_mode")
    out = (rcli if rita else gcli).main(argv)
    dms_id = f"{prefix}_{kind}"
    assert out.endswith(dms_id + ".csv")
    df = pd.read_csv(out)
    col = "RITA_score" if rita else "ProtGPT2_score"
    assert list(df.columns) == (["mutant", col, "DMS_score"] if rita else ["mutated_sequence", col, "DMS_score"])
    ref = (g_rita if rita else g_gpt2)[f"score_{dms_id}"]
    err = float(np.abs(df[col].to_numpy() - ref).max())
    assert err <= 1e-4, (dms_id, err)


@pytest.mark.parametrize("family", ["rita", "gpt2"])
def test_batch_invariance(g_gpt2, family):
    m = rita_model("h64") if family == "rita" else gpt2_model("h64", int(g_gpt2["vocab_size"]))
    try:
        rng = np.random.default_rng(3)
        V = m.cfg["vocab"]
        rows = [rng.integers(0, V, int(n)).astype(np.int32) for n in (57, 5, 130, 33, 57, 2, 90)]
        rows[4] = rows[0].copy()                                        # the same row twice in one batch
        alone, n_alone = m.sequence_loglik([rows[0]])
        mixed, n_mixed = m.sequence_loglik(rows)
        part, _ = m.sequence_loglik(rows[:4][::-1])
        assert alone[0] == mixed[0] == part[3], (alone[0], mixed[0], part[3])
        assert n_alone[0] == 56 and n_mixed.tolist() == [56, 4, 129, 32, 56, 1, 89]
        assert mixed[0] == mixed[4]
    finally:
        m.close()


def test_exact_multiple_of_context_raises_naming_the_sequence():
    m = rita_model("h64")
    try:
        encode = clm.load_tokenizer(RITA_TOK)
        with pytest.raises(ValueError, match=r"sequence 1 \(length 2046\)"):
            m.calc_fitness(["MKTAYIAKQ", "A" * 2046], encode)
    finally:
        m.close()
