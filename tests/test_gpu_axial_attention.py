"""The MSA Transformer's two axial attentions, op by op (pgmi_op_tied_row_attention / pgmi_op_column_attention: the launchers and the
argument pattern of run_msa) against the float64 reference of axial_ref.py, on every row.

Inputs in the manner of test_gpu_ops.py::test_attention (axial_ref.tied_inputs / column_inputs): q times 0.4, so that the tied scores
after / sqrt(R) spread by about 3; one spiky query column (q times 6 in every row: one key dominates its softmax row); one spiky key column
near the end whose V rows are 5; V rows offset by 0 / 1e-3 / 5 per token.  The column op multiplies its rows by the near-identity weight of
test_gpu_causal_attention.make_fused; the reference always forms X W^T + b itself.

The ops start every buffer the kernels write or must ignore -- partial scores, P, V^T, context -- as 0xFF bytes (NaN): the scores GEMM
writes roundup(C, 4) columns of rows of Kp = roundup(C, 64), and whatever lies between is the stale workspace of a wider alignment.

Bound: the suite's rule, max(2e-5 max(1, |ref|max), 3 noise32), noise32 = the same reference in plain fp32 NumPy against its float64 value,
for the context and for the probabilities (|ref|max <= 1).  Both are computed from the reference alone and rehearsed on the CPU in
test_axial_ref.py.  Every case prints its shape, the S in force, the error, noise32 and the bound before it asserts.

Bit-identity of a column alone against the column inside a launch rests on this reading of the code: the fused QKV GEMM computes every
output row from its own operand row with one K order whatever tile holds it (test_gemm16x_row_chunks_are_bit_identical), V^T is stored
per (sequence, head), and an attention workgroup serves one (sequence, head, query block) with the instantiation T alone selects."""
import functools

import numpy as np
import pytest

import axial_ref as ax
from proteingym_amd import _lib

pytestmark = pytest.mark.gpu


def _p(a):
    return a.ctypes.data_as(_lib._f32p) if a is not None else None


def _frozen(*arrays):
    for a in arrays:
        a.flags.writeable = False


@functools.lru_cache(maxsize=None)
def tied_case(R, C, H):
    """(qkv, (ctx, P) float64, (noise32, bound) of ctx, (noise32, bound) of P): computed once, shared, read-only."""
    qkv = ax.tied_inputs(R, C, H)
    ref = ax.tied_reference(qkv, R, C, H)
    _frozen(qkv, *ref[0])
    return (qkv,) + ref


@functools.lru_cache(maxsize=None)
def column_case(R, C, H):
    X, W, bias = ax.column_inputs(R, C, H)
    ref = ax.column_reference(X, W, bias, R, C, H)
    _frozen(X, W, bias, ref[0])
    return (X, W, bias) + ref


def run_tied(lib, qkv, R, C, H, splits=0):
    ctx = np.full((R * C, H * 64), np.nan, np.float32)
    probs = np.full((H, C, ax.tied_kp(C)), np.nan, np.float32)
    _lib.check(lib.pgmi_op_tied_row_attention(0, _p(qkv), R, C, H, splits, _p(ctx), _p(probs)))
    return ctx, probs


def run_column(lib, X, W, bias, R, C, H):
    ctx = np.full((C * R, H * 64), np.nan, np.float32)
    _lib.check(lib.pgmi_op_column_attention(0, _p(X), _p(W), _p(bias), X.shape[1], R, C, H, _p(ctx)))
    return ctx


def check_tied(lib, tag, R, C, H, splits=0):
    qkv, (ref, pref), (nc, bc), (npr, bp) = tied_case(R, C, H)
    S = splits or lib.pgmi_op_tied_row_splits(R, C, H)
    ctx, probs = run_tied(lib, qkv, R, C, H, splits)
    err, perr = float(np.abs(ctx - ref).max()), float(np.abs(probs[:, :, :C] - pref).max())
    rows = float(np.abs(probs.astype(np.float64).sum(-1) - 1.0).max())
    print(f"tied_row {tag} R={R} C={C} H={H} S={S}{' (forced)' if splits else ''} ctx err={err:.3e} noise32={nc:.3e} tol={bc:.3e} | "
          f"probs err={perr:.3e} noise32={npr:.3e} tol={bp:.3e} |rowsum-1|={rows:.2e}")
    # the poison never leaks (probabilities, and through them scores and V^T; a context row left unwritten would hold q: the bound finds it)
    assert np.isfinite(ctx).all() and np.isfinite(probs).all()
    assert err < bc, (tag, R, C, H, S, err, bc)
    assert perr < bp, (tag, R, C, H, S, perr, bp)
    assert np.all(probs[:, :, C:] == 0.0)                                    # padding columns: excluded by index, written as exact zeros
    assert rows < 1e-5, (tag, R, C, H, S, rows)
    return S, ctx, probs


@pytest.mark.parametrize("R,C,H", ax.TIED_COLUMN_EDGES)
def test_tied_column_edges_vs_fp64(lib, R, C, H):
    """N = roundup(C, 4) against C, Kp against C, launch_gemm16_ex's all-half-height rule (C % 256 in 1 .. 128), the softmax's 16-column
    lanes up to the limit of 1024."""
    check_tied(lib, "columns", R, C, H)


@pytest.mark.parametrize("case,want", list(zip(ax.TIED_ROW_EDGES, ax.TIED_ROW_EDGE_SPLITS)))
def test_tied_row_and_split_edges_vs_fp64(lib, case, want):
    S, _, _ = check_tied(lib, "rows", *case)
    assert S == want == ax.tied_splits(*case)                                # the library's choice, the issue's list, the mirrored rule


def test_tied_where_the_tile_cap_decides_vs_fp64(lib):
    (case,) = ax.TIED_TILE_CAP
    S, _, _ = check_tied(lib, "cap", *case)
    assert S == 6 == ax.tied_splits(*case)


@pytest.mark.parametrize("R,C,H", ax.TIED_WIDTH)
def test_tied_width_vs_fp64(lib, R, C, H):
    S, _, _ = check_tied(lib, "width", R, C, H)
    assert S == ax.tied_splits(R, C, H)


@pytest.mark.parametrize("splits", ax.TIED_FORCED_SPLITS)
def test_tied_forced_splits_vs_fp64(lib, splits):
    """Every S against float64: the summation order differs, no bit-identity is claimed."""
    check_tied(lib, "forced", *ax.TIED_FORCED, splits=splits)


def test_tied_forced_splits_take_effect(lib):
    """`splits` reaches the launch: the rule's own S forced (12 here) gives the bits of `splits` = 0, and S = 1 -- one summation chain
    per score instead of twelve partial sums added by the softmax -- does not."""
    R, C, H = ax.TIED_FORCED
    qkv = tied_case(R, C, H)[0]
    assert lib.pgmi_op_tied_row_splits(R, C, H) == 12
    (c0, p0), (c12, p12), (c1, p1) = (run_tied(lib, qkv, R, C, H, s) for s in (0, 12, 1))
    assert np.array_equal(c0, c12) and np.array_equal(p0, p12)
    assert not np.array_equal(p1, p12)


def test_tied_refusals_come_back_as_einval(lib):
    R, C, H = ax.TIED_FORCED
    qkv = tied_case(R, C, H)[0]
    tiny = np.zeros(16, np.float32)                                          # refused before anything is read or allocated
    for args, data, msg in (((R, C, H, 5), qkv, "K splits"), ((R, C, H, 24), qkv, "K splits"), ((2, 1025, 1, 0), tiny, "at most 1024 columns"),
                            ((1024, 1024, 20, 0), tiny, "32-bit offset range")):
        with pytest.raises(_lib.PgmiError, match=msg) as e:
            run = np.zeros(1, np.float32)
            _lib.check(lib.pgmi_op_tied_row_attention(0, _p(data), *args, _p(run), None))
        assert e.value.code == _lib.EINVAL, args


@pytest.mark.parametrize("which", ["k", "v"])
def test_tied_operand_beyond_fp16_range_is_non_finite_never_wrong(lib, which):
    """kTiedWScale's promise (msa_transformer.hip): |k| or |v| above 1023 ends non-finite, never in a wrong number.  One element set to
    2000: every output is non-finite or within the bound of the float64 reference of the same input; heads the element does not belong
    to stay finite.  The bound is the clean input's (the outputs that stay finite are the clean ones: the element reaches no other)."""
    R, C, H = 3, 20, 2
    D = H * 64
    clean, _, (_, bc), (_, bp) = tied_case(R, C, H)
    qkv = clean.copy()
    r, j, h, d = 1, 7, 1, 13
    qkv[r * C + j, (1 if which == "k" else 2) * D + h * 64 + d] = 2000.0
    ref, pref = ax.tied_row_attention(qkv, R, C, H)
    ctx, probs = run_tied(lib, qkv, R, C, H)
    ctx, probs = ctx.reshape(R, C, H, 64), probs[:, :, :C]
    ref = ref.reshape(R, C, H, 64)
    bad, pbad = ~np.isfinite(ctx), ~np.isfinite(probs)
    err = float(np.abs(np.where(bad, 0.0, ctx - ref)).max())
    perr = float(np.abs(np.where(pbad, 0.0, probs - pref)).max())
    print(f"tied_row range {which}=2000 R={R} C={C} H={H} non-finite ctx={int(bad.sum())} of {bad.size} probs={int(pbad.sum())} of {pbad.size} "
          f"finite ctx err={err:.3e} tol={bc:.3e} probs err={perr:.3e} tol={bp:.3e}")
    assert bad.any()
    assert err < bc and perr < bp
    assert not bad[:, :, 1 - h].any() and not pbad[1 - h].any()


def check_column(lib, R, C, H, tag="grid"):
    X, W, bias, ref, noise32, tol = column_case(R, C, H)
    ctx = run_column(lib, X, W, bias, R, C, H)
    err = float(np.abs(ctx - ref).max())
    print(f"column {tag} R={R} C={C} H={H} err={err:.3e} noise32={noise32:.3e} tol={tol:.3e}")
    assert np.isfinite(ctx).all()
    assert err < tol, (tag, R, C, H, err, tol)
    return ctx


@pytest.mark.parametrize("R,C,H", ax.COLUMN_CASES)
def test_column_attention_vs_fp64(lib, R, C, H):
    """One / two / four waves per workgroup, R on and off multiples of 32 (zeroed pad keys), a single key tile, the model's 70 x 45 x 12."""
    check_column(lib, R, C, H)


@pytest.mark.parametrize("R", [224, 257])
def test_column_attention_v3_bits_equal_v2(lib, R):
    """Both dense kernels through the split-plane store: within the bound each, and equal bits."""
    try:
        _lib.check(lib.pgmi_set_option(b"att_v3", 0))
        base = check_column(lib, R, 3, 2, "att_v3=0")
        _lib.check(lib.pgmi_set_option(b"att_v3", 1))
        got = check_column(lib, R, 3, 2, "att_v3=1")
        assert np.array_equal(got, base), float(np.abs(got - base).max())
    finally:
        lib.pgmi_set_option(b"att_v3", -1)


@pytest.mark.parametrize("R", [2, 33, 70, 257])
def test_a_column_does_not_depend_on_the_others(lib, R):
    """The middle column of a launch of three against a launch of that column alone: equal bits (module docstring)."""
    C, H = 3, 2
    X, W, bias, _, _, _ = column_case(R, C, H)
    full = run_column(lib, X, W, bias, R, C, H)
    alone = run_column(lib, np.ascontiguousarray(X[R:2 * R]), W, bias, R, 1, H)
    assert np.isfinite(alone).all()
    assert np.array_equal(full[R:2 * R], alone), float(np.abs(full[R:2 * R] - alone).max())
