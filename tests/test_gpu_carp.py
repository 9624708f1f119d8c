"""CARP on the MI355X against the float64 torch restatement (tests/carp_ref.py): the dilated convolution alone in both precisions
(pgmi_op_dilated_conv), a second run over stale operands, the LayerNorm + GELU row kernel, the whole model on seeded checkpoints, the
bits of a sequence alone / in a batch / under a row cap, the CLI on the toy assay of tests/golden/CARP_toy, and the refusals.

Bounds: an intermediate tensor (the convolution's output, the row kernel's) within 10 x the deviation of fp32 torch from float64 on
the same input, computed here and printed; log-probabilities and scores within the flat 1e-4 of DESIGN.md section 3.
Convolution shapes: segments of (5, 37, 1, 130, 3) rows, M = 176 -- taps fall off both ends at every dilation, a 1-row and a 3-row
segment sit between longer ones, and a shift of 128 rows lands inside the 130-row segment for two rows only; a version that ignored
the segment bounds would be off by tens.  (300,) and (257, 256) put tile edges (128 rows) inside a segment and next to a boundary.
C = 64 is narrower than a column tile, 512 is four, 1280 ten."""
import functools
import os

import numpy as np
import pandas as pd
import pytest
import torch

import carp_ref as R
from proteingym_amd import _lib, carp, score_carp_proteingym as cli

pytestmark = pytest.mark.gpu
TOL = 1e-4
TOY = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "CARP_toy")
PACKED = (5, 37, 1, 130, 3)
CONV_CASES = [(C, d, PACKED) for C in (64, 512, 1280) for d in (1, 2, 16, 128)] + \
             [(C, d, lens) for C in (64, 512) for d, lens in ((16, (300,)), (2, (257, 256)))]
CONV_IDS = [f"C{C}-d{d}-M{sum(lens)}" for C, d, lens in CONV_CASES]


@functools.lru_cache(maxsize=None)
def conv_case(C, dilation, lens):
    """Inputs, the float64 reference and fp32 torch's deviation from it, computed once."""
    rng = np.random.default_rng(1000 * C + dilation + len(lens))
    M = sum(lens)
    x = rng.normal(0, 1, (M, C)).astype(np.float32)
    w = (rng.normal(0, 1, (C, C, 5)) / np.sqrt(5 * C)).astype(np.float32)
    bias = rng.normal(0, 0.1, C).astype(np.float32)
    seg = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ref = R.conv_segments(x, w, bias, seg, dilation, torch.float64)
    dev = float(np.abs(R.conv_segments(x, w, bias, seg, dilation, torch.float32) - ref).max())
    for a in (x, w, bias, seg, ref):
        a.setflags(write=False)
    return x, w, bias, seg, ref, dev


@functools.lru_cache(maxsize=None)
def conv_out(C, dilation, lens, precision):
    x, w, bias, seg, _, _ = conv_case(C, dilation, lens)
    out = carp.op_dilated_conv(x, carp.permute_conv_weight(w), bias, seg, dilation, precision=precision)
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("C,dilation,lens", CONV_CASES, ids=CONV_IDS)
def test_dilated_conv_op(lib, C, dilation, lens):
    _, _, _, _, ref, dev = conv_case(C, dilation, lens)
    got = {p: conv_out(C, dilation, lens, p) for p in ("f16x3", "fp32")}
    errs = {p: float(np.abs(got[p] - ref).max()) for p in got}
    cross = float(np.abs(got["f16x3"].astype(np.float64) - got["fp32"]).max())
    print(f"C {C} dilation {dilation} M {sum(lens)}: max|err| f16x3 {errs['f16x3']:.3e}, fp32 {errs['fp32']:.3e}, f16x3 vs fp32 {cross:.3e}; "
          f"fp32 torch vs float64 {dev:.3e} (bound {10 * dev:.1e})")
    assert np.isfinite(got["f16x3"]).all() and np.isfinite(got["fp32"]).all()
    assert errs["f16x3"] <= 10 * dev and errs["fp32"] <= 10 * dev and cross <= 10 * dev


@pytest.mark.parametrize("C,dilation", [(64, 128), (512, 16), (1280, 1), (1280, 128)])
def test_dilated_conv_after_stale_operands(lib, C, dilation):
    """A boundary lane that left old LDS or register contents in place would pick up the 1e4 of the run before."""
    x, w, bias, seg, _, _ = conv_case(C, dilation, PACKED)
    first = conv_out(C, dilation, PACKED, "f16x3")
    wp = carp.permute_conv_weight(w)
    carp.op_dilated_conv(np.full_like(x, 1e4), wp, bias, seg, dilation)
    again = carp.op_dilated_conv(x, wp, bias, seg, dilation)
    assert np.array_equal(first.view(np.uint32), again.view(np.uint32))


@pytest.mark.parametrize("rows", [1, 63, 130])
@pytest.mark.parametrize("D", [64, 128, 512, 1024, 1280])
def test_ln_gelu_op(lib, D, rows):
    rng = np.random.default_rng(D + rows)
    x = (rng.normal(0, 1, (rows, D)) * rng.uniform(0.1, 4.0, (rows, 1)) + rng.normal(0, 1, (rows, 1))).astype(np.float32)
    w, b = (1 + 0.1 * rng.normal(0, 1, D)).astype(np.float32), rng.normal(0, 0.1, D).astype(np.float32)
    ref = R.ln_gelu(x, w, b, torch.float64)
    dev = float(np.abs(R.ln_gelu(x, w, b, torch.float32) - ref).max())
    for p in ("f16x3", "fp32"):
        got = carp.op_ln_gelu(x, w, b, precision=p)
        err = float(np.abs(got - ref).max())
        print(f"D {D} rows {rows} {p}: max|err| {err:.3e}; fp32 torch vs float64 {dev:.3e} (bound {10 * dev:.1e})")
        assert np.isfinite(got).all() and err <= 10 * dev, p


# ---- the model -----------------------------------------------------------------------------------------------------------------
MODELS = {"600k": (128, 16, True), "nonslim": (64, 3, False), "640M-width": (1280, 2, False)}
LENS = (37, 5, 130)


@functools.lru_cache(maxsize=None)
def checkpoint(name):
    D, layers, slim = MODELS[name]
    ck = carp.random_checkpoint(11 + D, D, layers, slim)
    for v in ck["model_state_dict"].values():
        v.setflags(write=False)
    return ck


@functools.lru_cache(maxsize=None)
def sequences(lens=LENS):
    rng = np.random.default_rng(17)
    toks = [rng.integers(0, 20, n).astype(np.int32) for n in lens]
    toks[0][3], toks[-1][-2] = 22, 25                                        # an ambiguous and a rare letter
    return tuple(toks)


@functools.lru_cache(maxsize=None)
def ref_token_lp(name, lens=LENS):
    return tuple(R.logprobs(checkpoint(name), t) for t in sequences(lens))


@pytest.fixture(scope="module")
def models(lib):
    live = {}

    def get(name, **kw):
        key = (name, tuple(sorted(kw.items())))
        if key not in live:
            live[key] = carp.CarpModel(checkpoint(name), **kw)
        return live[key]

    yield get
    for m in live.values():
        m.close()


@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
@pytest.mark.parametrize("name", ["600k", "nonslim"])
def test_model_parity(models, name, precision):
    m, ck, toks = models(name, precision=precision), checkpoint(name), sequences()
    got = m.token_logprobs(toks)
    for g, r in zip(got, ref_token_lp(name)):
        err = float(np.abs(g - r).max())
        print(f"{name} {precision} token_logprobs L {len(r)}: max|err| {err:.3e}")
        assert g.shape == r.shape and err <= TOL
    ll = m.sequence_loglik(toks)
    want = np.array([r[np.arange(len(t)), t].sum() for r, t in zip(ref_token_lp(name), toks)])
    print(f"{name} {precision} sequence_loglik: max|err| {np.abs(ll - want).max():.3e}")
    assert np.abs(ll - want).max() <= TOL                                     # the sum itself, and so the mean the host makes of it
    positions = np.arange(37)
    mlp = m.masked_logprobs(toks[0], positions)
    ref = R.masked_logprobs(ck, toks[0], positions)
    print(f"{name} {precision} masked_logprobs: max|err| {np.abs(mlp - ref).max():.3e}")
    assert mlp.shape == (37, 30) and np.abs(mlp - ref).max() <= TOL
    sub = m.masked_logprobs(toks[0], [36, 0, 7])                              # any order, any subset: the same rows
    assert np.array_equal(sub, mlp[[36, 0, 7]])


def test_model_parity_at_the_640m_width(models):
    m, toks = models("640M-width"), sequences((37,))
    got = m.token_logprobs(toks)[0]
    err = float(np.abs(got - ref_token_lp("640M-width", (37,))[0]).max())
    print(f"640M width token_logprobs: max|err| {err:.3e}")
    assert err <= TOL


def test_bits_alone_in_a_batch_and_under_a_row_cap(models):
    toks = sequences()
    batch = models("600k").token_logprobs(toks)
    capped = models("600k", max_rows=64).token_logprobs(toks)                 # 37 + 5 rows, then the 130-row sequence alone
    ll, ll_capped = models("600k").sequence_loglik(toks), models("600k", max_rows=64).sequence_loglik(toks)
    for i, t in enumerate(toks):
        alone = models("600k").token_logprobs([t])[0]
        assert np.array_equal(alone.view(np.uint32), batch[i].view(np.uint32)), i
        assert np.array_equal(alone.view(np.uint32), capped[i].view(np.uint32)), i
    assert np.array_equal(ll, ll_capped)
    m37 = models("600k").masked_logprobs(toks[0], np.arange(37))
    assert np.array_equal(m37, models("600k", max_rows=64).masked_logprobs(toks[0], np.arange(37)))      # one copy per chunk


@pytest.mark.parametrize("mode,index,extra,key", [("masked_marginals", 0, (), "mm_scores"), ("pseudo_likelihood", 0, (), "pl_scores"),
                                                  ("pseudo_likelihood", 1, ("--indel_mode",), "indel_scores")])
def test_cli_reproduces_the_golden_scores(lib, tmp_path, mode, index, extra, key):
    out, perf = str(tmp_path / "scores"), str(tmp_path / "perf.csv")
    fn = cli.main(["--model_name", "carp_toy", "--model_path", TOY, "--DMS_reference_file_path", os.path.join(TOY, "reference.csv"),
                   "--DMS_data_folder", TOY, "--DMS_index", str(index), "--output_scores_folder", out, "--performance_file", perf,
                   "--fitness_computation_mode", mode, *extra])
    got, exp = pd.read_csv(fn), np.load(os.path.join(TOY, "expected.npz"))[key]
    assert list(got.columns) == ["mutant", "carp_toy_score", "DMS_score"]
    print(f"{mode} {extra}: max|err| {np.abs(got['carp_toy_score'] - exp).max():.3e}")
    assert np.abs(got["carp_toy_score"] - exp).max() <= TOL
    assert open(perf).read().splitlines()[0] == "DMS_id,spearman" and len(open(perf).read().splitlines()) == 2


def test_bad_inputs_are_refused(models):
    m, t = models("nonslim"), sequences()[1]
    for call in (lambda: m.token_logprobs([t, np.zeros(0, np.int32)]),       # L = 0
                 lambda: m.sequence_loglik([np.zeros(0, np.int32)]),
                 lambda: m.masked_logprobs(np.zeros(0, np.int32), [0]),
                 lambda: m.token_logprobs([np.array([1, 30, 2], np.int32)]),     # a token >= V
                 lambda: m.masked_logprobs(np.array([1, -1, 2], np.int32), [0]),
                 lambda: m.masked_logprobs(t, []),                               # an empty position list
                 lambda: m.masked_logprobs(t, [len(t)]),                         # a position >= L
                 lambda: m.masked_logprobs(t, [-1])):
        with pytest.raises(_lib.PgmiError) as e:
            call()
        assert e.value.code == _lib.EINVAL
    assert np.isfinite(m.token_logprobs([t])[0]).all()                          # the handle still works
