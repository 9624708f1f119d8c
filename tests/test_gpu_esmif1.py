"""ESM-IF1 on the GPU (the seeded toy model of tests/esmif1_cases.py only): the cross-attention op against float64, its independence
from the rest of the launch and its refusals; the decoder's log-probabilities and scores against the reference's float64 goldens
(tests/golden/golden_esmif1.npz) and against the float64 NumPy decoder (tests/esmif1_ref.py, pinned to those goldens by
tests/test_esmif1_host.py); bit-identity of a sequence's score across batch composition and chunking; the encoder restatement on the
device against its own float64 CPU run; and the CLI's CSV against the CSV the reference script wrote.

Bounds.  Context values of the attention op: max(2e-5 max(1, |ref|max), 3 noise32) with noise32 from the fp32 evaluation of the same
attention (the rule of tests/test_gpu_poet.py).  Log-probability rows against float64: the project's flat 1e-4.  Scores:
max(1e-4, 3 noise32) with noise32 = |the reference's float32 score - its float64 score| from the goldens.  Encoder output on the device:
max(2e-5 max(1, |ref|max), 3 noise32) with noise32 = |the reference's float32 encoder_out - its float64 one|.  Every test prints its
figures before it asserts."""
import argparse
import os

import numpy as np
import pandas as pd
import pytest
import torch

import esmif1_cases as K
import esmif1_ref
from proteingym_amd import _lib, esmif1, score_esmif1_proteingym

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SEG_LENS = (1, 31, 33, 65)


def _p(a):
    return None if a is None else a.ctypes.data_as(_lib._f32p if a.dtype == np.float32 else _lib._i32p)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(GOLDEN, "golden_esmif1.npz")))


@pytest.fixture(scope="module")
def toy():
    cfg = esmif1.config_from_args(K.toy_args())
    return cfg, K.state_dict(cfg)


@pytest.fixture(scope="module")
def decoder(toy):
    cfg, sd = toy
    m = esmif1.EsmIf1Decoder(cfg, esmif1.pack_decoder(cfg, sd), device=0, max_memory=128)
    yield m
    m.close()


# ---- the attention op ------------------------------------------------------------------------------------------------------
def cross_rows(rng, lens, S, heads):
    """Queries as test_gpu_poet.py's att_rows builds them (one spiky row per segment); the memory with V offsets 0 / 1e-3 / 5 and one
    spiky key with V = 5 as the LAST memory key, so that a dropped or doubly counted tail key moves rows by O(1)."""
    Da = heads * 64
    q = []
    for n in lens:
        x = (0.4 * rng.standard_normal((n, Da))).astype(np.float32)
        if n > 2:
            x[(2 * n) // 3] *= 6.0
        q.append(x)
    mem = rng.standard_normal((S, 2 * Da)).astype(np.float32)
    mem[:, Da:] += rng.choice([0.0, 1e-3, 5.0], size=(S, 1)).astype(np.float32)
    mem[S - 1, :Da] *= 6.0
    mem[S - 1, Da:] = 5.0
    return np.concatenate(q), mem


def run_cross(lib, q, seg_off, mem, heads, split):
    ctx = np.full((q.shape[0], heads * 64), np.nan, np.float32)
    so = np.ascontiguousarray(seg_off, dtype=np.int32)
    _lib.check(lib.pgmi_op_cross_attention(0, _p(q), _p(so), len(so) - 1, _p(mem), mem.shape[0], heads, int(split), _p(ctx)))
    return ctx


def cross_reference(q, mem, heads, dtype):
    Da = heads * 64
    q, mem = q.astype(dtype), mem.astype(dtype)
    out = np.empty_like(q)
    for h in range(heads):
        c = slice(h * 64, h * 64 + 64)
        sc = q[:, c] @ mem[:, :Da][:, c].T
        p = np.exp(sc - sc.max(axis=1, keepdims=True))
        out[:, c] = (p / p.sum(axis=1, keepdims=True)) @ mem[:, Da:][:, c]
    return out


@pytest.mark.parametrize("heads", [2, 9])
@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("S", [1, 31, 32, 33, 97])
def test_cross_attention_against_float64(lib, S, split, heads):
    """Segments of 1, 31, 33 and 65 rows in one launch (one, one, two and three query tiles; five workgroups of four waves with the
    last one partly idle); 9 heads: two head groups of the XCD-local order, the second padded."""
    rng = np.random.default_rng(100 * S + 10 * heads + split)
    q, mem = cross_rows(rng, SEG_LENS, S, heads)
    ctx = run_cross(lib, q, np.concatenate([[0], np.cumsum(SEG_LENS)]), mem, heads, split)
    ref = cross_reference(q, mem, heads, np.float64)
    assert np.abs(esmif1_ref.cross_attention(q, mem, heads) - ref).max() < 1e-12
    noise32 = float(np.abs(cross_reference(q, mem, heads, np.float32) - ref).max())
    err, tol = float(np.abs(ctx - ref).max()), max(2e-5 * max(1.0, float(np.abs(ref).max())), 3.0 * noise32)
    print(f"cross_att S={S} heads={heads} split={split} err={err:.3e} noise32={noise32:.3e} tol={tol:.3e}")
    assert np.isfinite(ctx).all()
    assert err < tol, (S, heads, split, err, tol)


def test_cross_attention_row_does_not_depend_on_its_neighbours(lib):
    """A segment alone, first, last and in the middle of a launch: the same bits."""
    rng = np.random.default_rng(9)
    heads, S = 2, 97
    _, mem = cross_rows(rng, (1,), S, heads)
    segs = [cross_rows(rng, (n,), S, heads)[0] for n in (33, 70, 5, 64)]
    for split in (0, 1):
        alone = [run_cross(lib, s, [0, len(s)], mem, heads, split) for s in segs]
        for order in ([0, 1, 2, 3], [3, 2, 1, 0], [1, 0, 3]):
            off = np.concatenate([[0], np.cumsum([len(segs[i]) for i in order])])
            ctx = run_cross(lib, np.concatenate([segs[i] for i in order]), off, mem, heads, split)
            for j, i in enumerate(order):
                assert np.array_equal(ctx[off[j]:off[j + 1]], alone[i]), (split, order, i)


def test_cross_attention_refuses_bad_arguments(lib):
    q, mem, ctx = np.zeros((4, 64), np.float32), np.zeros((3, 128), np.float32), np.zeros((4, 64), np.float32)
    ok = np.array([0, 4], np.int32)
    assert lib.pgmi_op_cross_attention(0, _p(q), _p(ok), 1, _p(mem), 0, 1, 0, _p(ctx)) == _lib.EINVAL            # S = 0
    assert lib.pgmi_op_cross_attention(0, _p(q), _p(ok), 1, None, 3, 1, 0, _p(ctx)) == _lib.EINVAL               # NULL memory
    assert lib.pgmi_op_cross_attention(0, _p(q), _p(np.array([0, 2, 2, 4], np.int32)), 3, _p(mem), 3, 1, 0, _p(ctx)) == _lib.EINVAL
    assert b"empty" in lib.pgmi_last_error()


# ---- the ReLU epilogue -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(300, 96, 64), (33, 256, 128), (600, 2048, 512)])
def test_relu_epilogue_is_the_plain_gemm_clamped_at_zero(lib, shape):
    """EPI_RELU against the same GEMM without an activation: ReLU is exact on the fp32 value, so both output kinds (fp32 rows, and the
    split planes FC2 reads, rebuilt as fp32) must equal max(plain, 0) bit for bit; the plain GEMM has its own tests against float64.
    Shapes: a partial row tile, a partial row tile with two column panels, and FC1's N and K at the released widths."""
    M, N, K = shape
    rng = np.random.default_rng(M)
    A, W, b = (rng.standard_normal(s).astype(np.float32) for s in ((M, K), (N, K), (N,)))

    def gemm(epi, precision=_lib.PREC_F16X3):
        C_ = np.full((M, N), np.nan, np.float32)
        rc = lib.pgmi_op_gemm(0, precision, _p(A), _p(W), _p(b), None, M, N, K, epi, _p(C_))
        return rc, C_
    for planes in (0, 256):
        (rc0, plain), (rc1, relu) = gemm(0 + planes), gemm(5 + planes)
        assert rc0 == 0 and rc1 == 0, lib.pgmi_last_error()
        neg = float((plain < 0).mean())
        print(f"relu epilogue M={M} N={N} K={K} split_planes={planes != 0} share of negative outputs={neg:.3f}")
        assert 0.3 < neg < 0.7 and np.isfinite(relu).all()
        assert np.array_equal(relu, np.maximum(plain, 0.0))
    assert gemm(5, _lib.PREC_FP32)[0] == _lib.EINVAL and gemm(5, _lib.PREC_BF16)[0] == _lib.EINVAL


# ---- the model -------------------------------------------------------------------------------------------------------------
def _pos_table(cfg, n):
    return esmif1._sinusoid(torch.arange(n) + esmif1.PAD + 1, cfg["embed_dim"], esmif1.PAD).numpy()


@pytest.mark.parametrize("name", ["L30", "L31", "L70"])
def test_decoder_logprobs_and_scores(decoder, toy, golden, name):
    """Memory = the reference's float64 encoder_out.  L31's second sequence has 17 residues against a memory of 33 rows: T != S - 2."""
    cfg, sd = toy
    _, seqs = K.case(name)
    mem = golden[f"{name}_enc64"].astype(np.float32)
    decoder.set_memory(mem)
    toks = [esmif1.tokenize(s) for s in seqs]
    lp = decoder.token_logprobs(toks)
    ll = decoder.sequence_loglik(toks)
    for i, t in enumerate(toks):
        n = len(t) - 1
        want = golden[f"{name}_lp64_{i}"]
        mine = esmif1_ref.decoder_logprobs(cfg, sd, mem, t[:-1], _pos_table(cfg, n))
        err, err_ref = float(np.abs(lp[i, :n] - want).max()), float(np.abs(lp[i, :n] - mine).max())
        noise32 = abs(float(golden[f"{name}_ll32"][i] - golden[f"{name}_ll64"][i]))
        serr, tol = abs(ll[i] - golden[f"{name}_ll64"][i]), max(1e-4, 3 * noise32)
        print(f"esmif1 {name} seq {i} T={n} S={mem.shape[0]} lp_err={err:.3e} (numpy float64: {err_ref:.3e}) score_err={serr:.3e} "
              f"noise32={noise32:.3e} tol={tol:.3e}")
        assert np.isnan(lp[i, len(t):]).all() and np.isfinite(lp[i, :len(t)]).all()
        assert err < 1e-4 and err_ref < 1e-4, (name, i, err, err_ref)
        assert serr < tol, (name, i, serr, tol)
        assert abs(ll[i] - esmif1_ref.score(lp[i, :n].astype(np.float64), t)) < 1e-6          # the device's fp64 mean of its own rows
    # one and two residues: a single query row, and a key tile with one and two keys
    tiny = [esmif1.tokenize("M"), esmif1.tokenize("MK")]
    lp, ll = decoder.token_logprobs(tiny), decoder.sequence_loglik(tiny)
    for i, t in enumerate(tiny):
        n = len(t) - 1
        mine = esmif1_ref.decoder_logprobs(cfg, sd, mem, t[:-1], _pos_table(cfg, n))
        err, serr = float(np.abs(lp[i, :n] - mine).max()), abs(ll[i] - esmif1_ref.score(mine, t))
        print(f"esmif1 {name} tiny T={n} lp_err={err:.3e} score_err={serr:.3e}")
        assert err < 1e-4 and serr < 1e-4


def test_score_bits_alone_batched_and_chunked(decoder, toy, golden):
    """A sequence's fp64 score: the same bits alone, in any batch, and under a workspace that forces chunking (2048 rows: the 44
    sequences of 44 mixed lengths below take 2 175)."""
    cfg, sd = toy
    decoder.set_memory(golden["L70_enc64"].astype(np.float32))
    rng = np.random.default_rng(3)
    toks = [esmif1.tokenize(K.sequence_of(900 + i, int(n))) for i, n in enumerate(rng.choice([17, 31, 32, 33, 64, 70, 97], 44))]
    toks += [esmif1.tokenize("M"), esmif1.tokenize("MK")]
    batched = decoder.sequence_loglik(toks)
    by_length = np.argsort([len(t) for t in toks], kind="stable")              # runs of equal length share a launch: the same bits again
    assert np.array_equal(decoder.sequence_loglik([toks[i] for i in by_length]), batched[by_length])
    for i in (0, 7, 43, 44, 45):
        assert decoder.sequence_loglik([toks[i]])[0] == batched[i], i
    assert np.array_equal(decoder.sequence_loglik(toks[::-1])[::-1], batched)
    small = esmif1.EsmIf1Decoder(cfg, esmif1.pack_decoder(cfg, sd), device=0, max_rows=2048, max_memory=72)
    try:
        assert sum(len(t) - 1 for t in toks) > 2048
        small.set_memory(golden["L70_enc64"].astype(np.float32))
        assert np.array_equal(small.sequence_loglik(toks), batched)
    finally:
        small.close()


def test_decoder_refusals(decoder, toy, golden):
    cfg, sd = toy
    with pytest.raises(_lib.PgmiError) as e:
        decoder.set_memory(np.zeros((129, cfg["enc_dim"]), np.float32))             # above max_memory = 128
    assert e.value.code == _lib.EINVAL
    with pytest.raises(_lib.PgmiError):                                             # the failed call left no memory behind
        decoder.sequence_loglik([esmif1.tokenize("ACD")])
    bad = dict(cfg, heads=4)                                                        # head_dim 32
    with pytest.raises(_lib.PgmiError) as e:
        esmif1.EsmIf1Decoder(bad, esmif1.pack_decoder(cfg, sd), device=0)
    assert e.value.code == _lib.EINVAL and "head_dim" in str(e.value)


@pytest.mark.parametrize("name", ["L31", "nanca"])
def test_encoder_on_the_device(toy, golden, name):
    cfg, sd = toy
    coords, _ = K.case(name)
    ref = esmif1.Encoder(cfg, sd, "cpu", torch.float64).encode(coords)
    got = esmif1.Encoder(cfg, sd, "cuda:0", torch.float32).encode(coords)
    noise32 = float(np.abs(golden[f"{name}_enc32"] - golden[f"{name}_enc64"]).max())
    err, tol = float(np.abs(got - ref).max()), max(2e-5 * max(1.0, float(np.abs(ref).max())), 3.0 * noise32)
    print(f"esmif1 encoder {name} rows={ref.shape[0]} err={err:.3e} noise32={noise32:.3e} tol={tol:.3e}")
    assert got.shape == ref.shape and err < tol, (name, err, tol)


def test_cli_end_to_end(toy, tmp_path):
    """The toy assay through the CLI, checkpoint file included, against the CSV compute_fitness_esm_if1.py wrote for it."""
    cfg, sd = toy
    ckpt = {k: torch.from_numpy(v) for k, v in sd.items()}
    ckpt["encoder.embed_positions._float_tensor"] = torch.zeros(1)
    ckpt["decoder.embed_positions._float_tensor"] = torch.zeros(1)
    path = str(tmp_path / "toy_esmif1.pt")
    torch.save({"args": argparse.Namespace(**K.TOY_ARGS), "model": ckpt}, path)
    out = score_esmif1_proteingym.main(["--DMS_reference_file_path", os.path.join(GOLDEN, "TOY_ESMIF1_REFERENCE.csv"), "--DMS_data_folder", GOLDEN,
                                        "--structure_folder", os.path.join(GOLDEN, "ESMIF1_structures"), "--DMS_index", "0",
                                        "--model_location", path, "--output_scores_folder", str(tmp_path / "out"), "--chain", "A",
                                        "--multichain-backbone", "--batch_size", "3"])
    assert open(out).readline() == "mutant,esmif1_ll\n"
    got, want = pd.read_csv(out), pd.read_csv(os.path.join(GOLDEN, "TOY_ESMIF1_reference_scores.csv"))
    assert got["mutant"].tolist() == want["mutant"].tolist()
    err = float(np.abs(got["esmif1_ll"].values - want["esmif1_ll"].values).max())
    print(f"esmif1 cli rows={len(got)} err={err:.3e}")
    assert err < 1e-4
    with pytest.raises(SystemExit):
        score_esmif1_proteingym.main(["--nogpu"])
