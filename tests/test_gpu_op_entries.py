"""What the single-op and timing entries (pgmi_op_* / pgmi_bench_*) do around their kernels: a refused call holds nothing and breaks
nothing, a device ordinal past the last one is an error return and no crash, and the timing entries report a time.  The values the
kernels compute are the business of the op-by-op files (test_gpu_ops.py, test_gpu_scoring_ops.py, test_gpu_dense_attention.py,
test_gpu_causal_attention.py, test_gpu_axial_attention.py and the per-model files); their input builders and runners are used here as
they are, at the smallest shapes at which an entry still runs every branch it has.

Every runner of those files passes device 0 and valid arguments.  `Rerouted` stands between a runner and the library: it replaces the
device ordinal (argument 0 of every such entry) and, when asked, passes every pointer argument as NULL, which every entry refuses as
PGMI_EINVAL ("bad argument", its first check) before it looks for a device.  The runners that call _lib.load() themselves (carp.op_dilated_conv,
esm3.geom_attention) are reached by putting it in the place of the loaded library for the length of the call.

Shapes that are not the plain smallest ones: the bf16 GEMM has K = 64 (its K step), the conv form of the causal attention four heads
(its four head groups), the sequence sums V = 25 and six ragged sequences (scoring_ref's builders), the column attention K = 32 on
inputs drawn here (axial_ref's builder has K = 3 D)."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import axial_ref as ax
import esm3_cases
import progen3_ref
import scoring_ref as sr
import test_gpu_axial_attention as t_axial
import test_gpu_causal_attention as t_causal
import test_gpu_dense_attention as t_dense
import test_gpu_esmif1 as t_if1
import test_gpu_poet as t_poet
import test_gpu_progen3 as t_pg3
import test_gpu_scoring_ops as t_score
from proteingym_amd import _lib, carp, esm3

pytestmark = pytest.mark.gpu

F32P, I32P = _lib._f32p, _lib._i32p


def _p(a, ty=F32P):
    return a.ctypes.data_as(ty) if a is not None else None


class Rerouted:
    """The library with argument 0 of every pgmi_op_* / pgmi_bench_* call replaced by `device` and, with null_pointers, every
    pointer argument of the call by NULL."""

    def __init__(self, lib, device, null_pointers):
        self._lib, self._device, self._null = lib, device, null_pointers

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith(("pgmi_op_", "pgmi_bench_")):
            return fn

        def call(*args):
            args = [None if self._null and issubclass(t, C._Pointer) else a for a, t in zip(args, fn.argtypes)]
            args[0] = self._device
            return fn(*args)
        return call


@contextlib.contextmanager
def rerouted(lib, device=0, null_pointers=False):
    r = Rerouted(lib, device, null_pointers)
    loaded, _lib._lib = _lib._lib, r
    try:
        yield r
    finally:
        _lib._lib = loaded


# ---- one valid call per case: fn(lib, ...) -> the output arrays, each of the shape the entry documents ---------------------------------
def layernorm(lib, rows=3, D=32):
    rng = np.random.default_rng(0)
    x, w, b = (rng.standard_normal(s).astype(np.float32) for s in ((rows, D), D, D))
    y = np.full((rows, D), np.nan, np.float32)
    _lib.check(lib.pgmi_op_layernorm(0, _p(x), _p(w), _p(b), rows, D, 1e-5, _p(y)))
    return [y]


def rmsnorm(lib, rows=3, D=32):
    rng = np.random.default_rng(1)
    x, w = (rng.standard_normal(s).astype(np.float32) for s in ((rows, D), D))
    y = np.full((rows, D), np.nan, np.float32)
    _lib.check(lib.pgmi_op_rmsnorm(0, _p(x), _p(w), rows, D, 1e-5, _p(y)))
    return [y]


def gemm(lib, precision, epilogue=0, residual=False, M=33, N=64, K=32):
    rng = np.random.default_rng(2)
    A, W, bias = (rng.standard_normal(s).astype(np.float32) for s in ((M, K), (N, K), N))
    R = rng.standard_normal((M, N)).astype(np.float32) if residual else None
    Cc = np.full((M, N), np.nan, np.float32)
    _lib.check(lib.pgmi_op_gemm(0, precision, _p(A), _p(W), _p(bias), _p(R), M, N, K, epilogue, _p(Cc)))
    return [Cc]


def moe(lib, E, k, gated, M=5, D=32, F=32):
    h, gate, w1, w3, w2 = progen3_ref.moe_inputs(M, E, k, gated, None, D=D, F=F)
    out, ids, wts = t_pg3.run_moe(lib, h, gate, w1, w3, w2, E, k, gated)
    return [out] + ([ids, wts] if E > 1 else [])


def qkln_prep(lib, iters=0, B=2, T=33, H=1):
    rng = np.random.default_rng(3)
    D = 64 * H
    qkv, qw, kw = (rng.standard_normal(s).astype(np.float32) for s in ((B * T, 3 * D), D, D))
    qk, v = np.full((B * T, 2 * D), np.nan, np.float32), np.full((B * T, D), np.nan, np.float32)
    ms = C.c_double(-1.0)
    _lib.check(lib.pgmi_op_qkln_prep(0, _p(qkv), _p(qw), _p(kw), B, T, H, iters, _p(qk), _p(v), C.byref(ms) if iters else None))
    return [qk, v] + ([np.array([ms.value])] if iters else [])


def attention(lib, precision, rotary, B=2, T=33, H=1):
    rng = np.random.default_rng(4)
    qkv = rng.standard_normal((B, T, 3 * 64 * H)).astype(np.float32)
    ctx = np.full((B, T, 64 * H), np.nan, np.float32)
    _lib.check(lib.pgmi_op_attention(0, precision, _p(qkv), None, B, T, H, rotary, _p(ctx)))
    return [ctx]


def causal_fused(lib, lanes, rot, B=2, T=33, heads=1):
    rng = np.random.default_rng(5)
    X, W, bias = t_causal.make_fused(rng, t_causal.make_rows(rng, B, T, heads, lanes))
    cos, sin = t_causal.rotary_tables(rot, T, lanes)
    return [t_causal.run_fused(lib, X, W, bias, B, T, heads, lanes, np.zeros(heads, np.float32), cos, sin)]


def causal_conv(lib, B=2, T=33, heads=4):
    rng = np.random.default_rng(6)
    qkv = np.ascontiguousarray(t_causal.make_rows(rng, B, T, heads, 64).reshape(B * T, -1))
    return [t_causal.run_conv(lib, qkv, t_causal.make_conv(rng), B, T, heads, t_causal.tranception_slopes(heads))]


def dense(lib, lanes, out, B=2, T=33, heads=1):
    kv = (T, (T + 1) // 2)[:B] if B == 2 else t_dense.ragged(B, T)
    case = t_dense.make_case(7, B, T, heads, lanes, "esm2", kv)
    ctx, qk, v = t_dense.run(lib, case, B, T, heads, lanes, out, operands=True)
    return [ctx[t_dense.valid_rows(kv, T)], qk, v]                 # query rows from kv_len[b] on are nobody's to read


def prefix(lib, P, split, lens=(5, 33), heads=1):
    rng = np.random.default_rng(8)
    qkv = np.concatenate([t_poet.att_rows(rng, n, heads) for n in lens])
    pre = np.ascontiguousarray(t_poet.att_rows(rng, P, heads)[:, heads * 64:]) if P else None
    return [t_poet.run_att(lib, qkv, np.concatenate([[0], np.cumsum(lens)]), pre, heads, split)]


def cross(lib, split, S=33, lens=(5, 33), heads=1):
    q, mem = t_if1.cross_rows(np.random.default_rng(9), lens, S, heads)
    return [t_if1.run_cross(lib, q, np.concatenate([[0], np.cumsum(lens)]), mem, heads, split)]


def tied_row(lib, probs, R=2, C=33, H=1):
    qkv = ax.tied_inputs(R, C, H)
    if probs:
        return list(t_axial.run_tied(lib, qkv, R, C, H))
    ctx = np.full((R * C, H * 64), np.nan, np.float32)
    _lib.check(lib.pgmi_op_tied_row_attention(0, _p(qkv), R, C, H, 0, _p(ctx), None))
    return [ctx]


def column(lib, R=3, C=2, H=1, K=32):
    rng = np.random.default_rng(10)
    X = rng.standard_normal((C * R, K)).astype(np.float32)
    W, bias = (rng.standard_normal((3 * 64 * H, K)) / np.sqrt(K)).astype(np.float32), (0.05 * rng.standard_normal(3 * 64 * H)).astype(np.float32)
    return [t_axial.run_column(lib, X, W, bias, R, C, H)]


def geom(lib, name="s17_h24"):
    proj, rot, trans, mask, w_rot, w_dist = esm3_cases.op_case(name)
    return [esm3.geom_attention(proj, rot, trans, mask, w_rot, w_dist, per_row_frames=rot.shape[0] > 1)]


def dilated_conv(lib, precision, C_=32, dilation=2, lens=(5, 33)):
    rng = np.random.default_rng(11)
    M = sum(lens)
    x, w, bias = rng.standard_normal((M, C_)).astype(np.float32), (rng.standard_normal((C_, C_, 5)) / np.sqrt(5 * C_)).astype(np.float32), \
        rng.standard_normal(C_).astype(np.float32)
    return [carp.op_dilated_conv(x, carp.permute_conv_weight(w), bias, np.concatenate([[0], np.cumsum(lens)]), dilation, precision=precision)]


def ln_gelu(lib, precision, rows=38, D=32):
    rng = np.random.default_rng(12)
    x, w, b = (rng.standard_normal(s).astype(np.float32) for s in ((rows, D), D, D))
    return [carp.op_ln_gelu(x, w, b, precision=precision)]


def narrow(lib, V=33, D=32, rows=3):
    h, E, bias, _ = sr.head_inputs(V, D, rows)
    out, flag = t_score.run_narrow(lib, h, E, bias)
    assert flag == 0
    return [out]


def wide(lib, targets, V=33, ldl=36, rows=3):
    x, _, tgt = sr.wide_inputs(V, ldl, rows, 1)                    # kinds normal8, ascending, descending: every logit finite
    out, flag = t_score.run_wide(lib, x, V, tgt if targets else None)
    assert flag == 0
    return [out]


def group(lib, mode, V=33, first=3, groups=3, width=10, D=32, rows=3):
    h, E, bias, _ = sr.head_inputs(V, D, rows, seed=1)
    full, grp, flag = t_score.run_group(lib, h, E, bias, first, groups, width, mode)
    assert flag == 0
    return [a for a in (full, grp) if a is not None]


def seq_sum(lib, ragged, B=3, T=33):
    c = sr.seq_ragged_case(T, 0)[1] if ragged else sr.seq_dense_case(B, T, 0)
    return [t_score.run_seq(lib, c, alpha=0.5)]


PREC = {"fp32": _lib.PREC_FP32, "f16x3": _lib.PREC_F16X3, "bf16": _lib.PREC_BF16}
SPLIT_PLANES = 256                                                 # pgmi_op_gemm: the 16-bit-plane output, rebuilt as fp32
CASES = {
    "layernorm": (layernorm, (), [(3, 32)]),
    "rmsnorm": (rmsnorm, (), [(3, 32)]),
    "gemm-fp32-residual": (gemm, (PREC["fp32"], 1, True), [(33, 64)]),
    "gemm-f16x3-residual": (gemm, (PREC["f16x3"], 1, True), [(33, 64)]),
    "gemm-f16x3-planes": (gemm, (PREC["f16x3"], 1 + SPLIT_PLANES), [(33, 64)]),
    "gemm-bf16": (gemm, (PREC["bf16"], 0, True, 33, 64, 64), [(33, 64)]),
    "gemm-bf16-plane": (gemm, (PREC["bf16"], SPLIT_PLANES, False, 33, 64, 64), [(33, 64)]),
    "moe-E1-gated": (moe, (1, 1, 1), [(5, 32)]),
    "moe-E1-plain": (moe, (1, 1, 0), [(5, 32)]),
    "moe-E4k2-gated": (moe, (4, 2, 1), [(5, 32), (5, 2), (5, 2)]),
    "moe-E4k2-plain": (moe, (4, 2, 0), [(5, 32), (5, 2), (5, 2)]),
    "qkln_prep": (qkln_prep, (), [(66, 128), (66, 64)]),
    "attention-fp32-rotary": (attention, (PREC["fp32"], 1), [(2, 33, 64)]),
    "attention-f16x3": (attention, (PREC["f16x3"], 0), [(2, 33, 64)]),
    "attention-f16x3-rotary": (attention, (PREC["f16x3"], 1), [(2, 33, 64)]),
    "causal-fused-64": (causal_fused, (64, "none"), [(2, 33, 64)]),
    "causal-fused-128-rotary": (causal_fused, (128, "group"), [(2, 33, 128)]),
    "causal-conv": (causal_conv, (), [(2, 33, 256)]),
    "dense-64-split": (dense, (64, t_dense.SPLIT), [(33 + 17, 64), (66, 128), (66, 64)]),
    "dense-128-f32": (dense, (128, t_dense.F32), [(33 + 17, 128), (66, 256), (66, 128)]),
    "dense-128-bf16": (dense, (128, t_dense.BF16), [(33 + 17, 128), (66, 256), (66, 128)]),
    "prefix-P0": (prefix, (0, 0), [(38, 64)]),
    "prefix-P33-split": (prefix, (33, 1), [(38, 64)]),
    "cross-S33": (cross, (0,), [(38, 64)]),
    "cross-S33-split": (cross, (1,), [(38, 64)]),
    "tied_row-probs": (tied_row, (True,), [(66, 64), (1, 33, ax.tied_kp(33))]),
    "tied_row": (tied_row, (False,), [(66, 64)]),
    "column": (column, (), [(6, 64)]),
    "geom": (geom, (), [(2, 17, 72)]),
    "dilated_conv-f16x3": (dilated_conv, ("f16x3",), [(38, 32)]),
    "dilated_conv-fp32": (dilated_conv, ("fp32",), [(38, 32)]),
    "ln_gelu-f16x3": (ln_gelu, ("f16x3",), [(38, 32)]),
    "ln_gelu-fp32": (ln_gelu, ("fp32",), [(38, 32)]),
    "narrow": (narrow, (), [(3, 33)]),
    "wide": (wide, (False,), [(3, 33)]),
    "wide-targets": (wide, (True,), [(3,)]),
    "group-both": (group, ("both",), [(3, 33), (3, 3)]),
    "group-only": (group, ("group",), [(3, 3)]),
    "seq_sum-dense": (seq_sum, (False,), [(3,)]),
    "seq_sum-ragged": (seq_sum, (True,), [(6,)]),
}


def run_valid(lib, name):
    fn, args, shapes = CASES[name]
    outs = fn(lib, *args)
    assert [o.shape for o in outs] == shapes, (name, [o.shape for o in outs])
    for o in outs:
        assert np.isfinite(o).all(), name


def run_after_bad_ordinal(run):
    """hipSetDevice leaves its error behind as the thread's last HIP error, which stays until somebody reads it.  An entry that does not
    read it when it reports the refusal leaves it to the next call whose launcher asks hipGetLastError(): that call then fails, once,
    with the ordinal's error, and reading it clears it.  Either way the call after that works."""
    try:
        return run()
    except _lib.PgmiError as stale:
        assert stale.code == _lib.EHIP and "invalid device ordinal" in str(stale), stale
    return run()


@pytest.mark.parametrize("name", CASES)
def test_a_refused_call_leaves_the_entry_usable(lib, name):
    fn, args, _ = CASES[name]
    with rerouted(lib, null_pointers=True) as r, pytest.raises(_lib.PgmiError) as e:
        fn(r, *args)
    assert e.value.code == _lib.EINVAL and "bad argument" in str(e.value), e.value
    run_valid(lib, name)


@pytest.mark.parametrize("name", CASES)
def test_a_device_ordinal_past_the_last_is_an_error_return(lib, name):
    fn, args, _ = CASES[name]
    with rerouted(lib, device=lib.pgmi_device_count()) as r, pytest.raises(_lib.PgmiError) as e:
        fn(r, *args)
    assert e.value.code == _lib.EHIP and "hipSetDevice" in str(e.value), e.value
    run_after_bad_ordinal(lambda: run_valid(lib, name))


# ---- the timing entries ----------------------------------------------------------------------------------------------------------------
def bench_gemm(lib, precision=_lib.PREC_F16X3, split_out=0):
    ms = C.c_double(-1.0)
    _lib.check(lib.pgmi_bench_gemm(0, precision, 33, 64, 64, 0, split_out, 0, 2, C.byref(ms)))
    return [ms.value]


def bench_gemm_ab(lib, split_out=0, N=64):
    variants, ms = np.array([0, 1002], np.int32), np.full(2, -1.0)
    _lib.check(lib.pgmi_bench_gemm_ab(0, _lib.PREC_F16X3, 33, N, 32, 0, split_out, _p(variants, I32P), 2, 2, 2, _p(ms, _lib._f64p)))
    return list(ms)


def bench_dilated_conv(lib):
    ms = C.c_double(-1.0)
    _lib.check(lib.pgmi_bench_dilated_conv(0, 38, 2, 32, 5, 2, 2, C.byref(ms)))
    return [ms.value]


def bench_qkln_prep(lib):
    return list(qkln_prep(lib, iters=2)[2])


BENCHES = {
    "gemm-f16x3": (bench_gemm, ()), "gemm-fp32": (bench_gemm, (_lib.PREC_FP32,)), "gemm-bf16-planes": (bench_gemm, (_lib.PREC_BF16, 1)),
    "gemm_ab": (bench_gemm_ab, ()), "gemm_ab-in-place-residual": (bench_gemm_ab, (2,)), "gemm_ab-fused-qkv": (bench_gemm_ab, (3, 192)),
    "dilated_conv": (bench_dilated_conv, ()), "qkln_prep": (bench_qkln_prep, ()),
}


@pytest.mark.parametrize("name", BENCHES)
def test_a_timing_entry_reports_a_time(lib, name):
    fn, args = BENCHES[name]
    for _ in range(2):                                             # the second call finds what the first released
        ms = fn(lib, *args)
        assert all(np.isfinite(t) and t > 0 for t in ms), (name, ms)


@pytest.mark.parametrize("name", ["gemm_ab", "dilated_conv"])
def test_a_timing_entry_refuses_like_an_op_entry(lib, name):
    fn, args = BENCHES[name]
    with rerouted(lib, null_pointers=True) as r, pytest.raises(_lib.PgmiError) as e:
        fn(r, *args)
    assert e.value.code == _lib.EINVAL, e.value
    with rerouted(lib, device=lib.pgmi_device_count()) as r, pytest.raises(_lib.PgmiError) as e:
        fn(r, *args)
    assert e.value.code == _lib.EHIP, e.value
    assert all(t > 0 for t in run_after_bad_ordinal(lambda: fn(lib, *args)))
