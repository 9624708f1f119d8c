"""The GEMM epilogues (gemm16x_kernel.h) output kind by output kind: values against float64, and the bit-equalities the kernel promises --
a row's bits do not depend on the item kind (full / half height), on the rows computed beside it (interior / guarded epilogue path) or on
the row chunking -- including for outputs below fp16's normal range, where the split planes carry everything in lo.

Through pgmi_op_gemm.  That entry uploads the residual into a buffer of its own, so it reaches the residual epilogue out of place only; the
in-place form (residual == output, both residual GEMMs of the encoder) runs in every model test and in smoke().  Split planes come back
rebuilt as fp32 (hi + lo 2^-11); f16x3 offers them for N % 32 == 0, SwiGLU for N % 64 == 0, bf16 planes for N % 4 == 0.

Tolerances.  fp32 outputs: the bounds of tests/test_gpu_ops.py (f16x3: 2e-5 sqrt(K / 128) relative to max(1, the row's largest |a|);
bf16: 1e-4 max(1, sqrt(K / 256)) against the bf16-rounded operands, here times the same row factor because the rows are scaled), which
bound the error e of the pre-activation value.  Behind an activation f the same error passes through f's slope: |f'| <= 1.13 for both
GELUs, 1 for ReLU, 2 |x| for the squared ReLU; for SwiGLU silu(g) u the two errors weigh 1.1 |u| and |silu(g)|; where two errors multiply
(squared ReLU, SwiGLU) e^2 is added, and 3e-7 (1 + |value|) for the kernels' own activation forms (the polynomial erf-GELU is within
2.8e-7 of the exact one, gemm16x_kernel.h).  On top comes the rounding of the result itself: 2^-22 |value| for fp32 and for the split
planes alike (hi holds 11 bits, lo the next 11).  Split planes against the fp32 run of the same GEMM, elementwise: for |F| >= 2^-14
hi = F to 11 bits and lo = the rest to 11 bits, error <= 2^-22 |F|, the fp32 rebuild another 2^-24 |F|: 2^-21 |F| covers both; below 2^-14
hi is 0 and lo = 2^11 F in fp16: 11 bits while it is normal, 2^-24 absolute as an fp16 subnormal, i.e. 2^-11 |F| + 2^-35."""
import numpy as np
import pytest
import torch

from proteingym_amd import _lib

pytestmark = pytest.mark.gpu

ACTS = {0: "none", 1: "gelu", 2: "sqrelu", 3: "gelu_tanh", 5: "relu"}
SHAPES = [(1, 128, 256),
          (300, 384, 128),          # rows past M inside a tile
          (513, 1284, 192),         # N % 64 != 0 (and N % 32 != 0: fp32 outputs only)
          (600, 1312, 128),         # N % 64 != 0 with split planes: the unstaged path of the last wave
          (200, 1344, 384),         # narrow last column tile
          (4200, 5120, 128),        # 340 tiles on 256 CUs: a second item per workgroup
          (2300, 1280, 128),        # 45 tiles, each as two half-height items
          (2100, 640, 256)]         # cut into row chunks below


def _p(a, ty=_lib._f32p):
    return a.ctypes.data_as(ty) if a is not None else None


def _gemm(lib, prec, A, W, bias, R, epi):
    M, K = A.shape
    N = W.shape[0]
    C = np.full((M, N // 2 if (epi & 255) == 4 else N), np.nan, np.float32)
    _lib.check(lib.pgmi_op_gemm(0, prec, _p(A), _p(W), _p(bias), _p(R), M, N, K, epi, _p(C)))
    return C


def _act64(epi, x):
    """(f(x), bound on |f'| at x) in float64."""
    if epi == 0:
        return x, np.ones_like(x)
    if epi == 1:
        return x * 0.5 * (1.0 + torch.erf(torch.from_numpy(x) / np.sqrt(2.0)).numpy()), np.full_like(x, 1.13)
    if epi == 2:
        t = np.maximum(x, 0.0)
        return t * t, 2.0 * np.abs(x)
    if epi == 3:
        return 0.5 * x * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) * (x + 0.044715 * x ** 3))), np.full_like(x, 1.13)
    assert epi == 5
    return np.maximum(x, 0.0), np.ones_like(x)


def _operands(M, N, K, seed, row_scales=(0.01, 1.0, 30.0)):
    rng = np.random.default_rng(seed)
    A = (rng.standard_normal((M, K)) * rng.choice(row_scales, size=(M, 1))).astype(np.float32)
    W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    R = rng.standard_normal((M, N)).astype(np.float32)
    return A, W, bias, R


def _check(C, ref, e_pre, slope, what, second_order=False, act=True):
    bound = e_pre * slope + np.abs(ref) * 2.0 ** -22
    if second_order:                    # squared ReLU, SwiGLU: the product of two errors
        bound = bound + e_pre * e_pre
    if act:                             # the kernels' own activation forms (polynomial erf-GELU: 2.8e-7 abs, gemm16x_kernel.h; exp2, rcp)
        bound = bound + 3e-7 * (1.0 + np.abs(ref))
    worst = (np.abs(C - ref) / bound).max()
    print(f"{what}: max err / bound = {worst:.3f}")
    assert np.isfinite(C).all(), what
    assert worst < 1.0, (what, worst)


def _swiglu64(pre):
    """pre [M, N] in the SwiGLU block order (blocks of 64 columns = 32 gate | 32 up) -> (value, weight of the gate error, of the up error)."""
    M, N = pre.shape
    b = pre.reshape(M, N // 64, 2, 32)
    g, u = b[:, :, 0], b[:, :, 1]
    s = g / (1.0 + np.exp(-g))
    return (s * u).reshape(M, N // 2), (1.1 * np.abs(u)).reshape(M, N // 2), np.abs(s).reshape(M, N // 2)


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_every_output_kind_against_float64(lib, gemm_option, M, N, K):
    if (M, N, K) == (2100, 640, 256):
        gemm_option("gemm_max_rows", 500)
    A, W, bias, R = _operands(M, N, K, seed=11)
    scale = np.maximum(np.abs(A).max(1, keepdims=True).astype(np.float64), 1.0)
    # ---- f16x3 ----
    pre = A.astype(np.float64) @ W.astype(np.float64).T + bias.astype(np.float64)
    e_pre = 2e-5 * np.sqrt(K / 128) * scale
    _check(_gemm(lib, _lib.PREC_F16X3, A, W, bias, None, 0), pre, e_pre, 1.0, "f16x3 bias")
    _check(_gemm(lib, _lib.PREC_F16X3, A, W, bias, R, 0), pre + R, e_pre, 1.0, "f16x3 bias + residual")
    _check(_gemm(lib, _lib.PREC_F16X3, A, W, bias, R, 1), _act64(1, pre)[0] + R, e_pre, 1.13, "f16x3 gelu + residual")
    for epi in ACTS:
        ref, slope = _act64(epi, pre)
        if epi:
            _check(_gemm(lib, _lib.PREC_F16X3, A, W, bias, None, epi), ref, e_pre, slope, f"f16x3 {ACTS[epi]} fp32", epi == 2)
        if N % 32 == 0:
            _check(_gemm(lib, _lib.PREC_F16X3, A, W, bias, None, epi + 256), ref, e_pre, slope, f"f16x3 {ACTS[epi]} split planes", epi == 2)
    if N % 64 == 0:
        ref, wg, wu = _swiglu64(pre)
        _check(_gemm(lib, _lib.PREC_F16X3, A, W, bias, None, 4 + 256), ref, e_pre * (wg + wu), 1.0, "f16x3 swiglu split planes", True)
    # ---- bf16 (no ReLU kernel; its plane output is the fp32 output rounded to bf16) ----
    b16 = lambda a: torch.from_numpy(a).bfloat16().double().numpy()  # noqa: E731
    pre = b16(A) @ b16(W).T + bias.astype(np.float64)
    e_pre = 1e-4 * max(1.0, np.sqrt(K / 256)) * scale        # test_gpu_ops.py's bound is for unit rows; fp32 accumulation errs relative to the row
    _check(_gemm(lib, _lib.PREC_BF16, A, W, bias, R, 0), pre + R, e_pre, 1.0, "bf16 bias + residual")
    for epi in (0, 1, 2, 3):
        ref, slope = _act64(epi, pre)
        F = _gemm(lib, _lib.PREC_BF16, A, W, bias, None, epi)
        _check(F, ref, e_pre, slope, f"bf16 {ACTS[epi]} fp32", epi == 2)
        P = _gemm(lib, _lib.PREC_BF16, A, W, bias, None, epi + 256)
        assert np.array_equal(P, torch.from_numpy(F).bfloat16().float().numpy()), f"bf16 {ACTS[epi]} plane"


def _kinds(N):
    """(epilogue, with residual) of every f16x3 output kind the shape allows."""
    kinds = [(0, False), (0, True), (1, True)] + [(e, False) for e in ACTS if e]
    if N % 32 == 0:
        kinds += [(e + 256, False) for e in ACTS]
    if N % 64 == 0:
        kinds.append((4 + 256, False))
    return kinds


SMALL = (0.0, 1e-6, 6e-5, 1.0)          # row scales: exact zeros, outputs far below 2^-14, around it, and ordinary rows


def _small_operands(M, N, K, seed):
    """No bias, rows of A scaled so that more than a third of the outputs lie below fp16's normal range and some are exactly 0."""
    rng = np.random.default_rng(seed)
    sc = rng.choice(SMALL, size=(M, 1), p=(0.1, 0.3, 0.3, 0.3))
    sc[0] = 1e-6                        # the row the row-alone test looks at
    A = (rng.standard_normal((M, K)) * sc).astype(np.float32)
    W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    return A, W


def _split_against_fp32(P, F, what):
    a = np.abs(F.astype(np.float64))
    bound = np.where(a >= 2.0 ** -14, a * 2.0 ** -21, a * 2.0 ** -11 + 2.0 ** -35)
    assert (np.abs(P.astype(np.float64) - F) <= bound).all(), what


@pytest.mark.parametrize("small", [False, True])
def test_half_height_items_same_bits(lib, gemm_option, small):
    M, N, K = 2300, 1280, 128
    A, W, bias, R = _operands(M, N, K, seed=12)
    if small:
        (A, W), bias = _small_operands(M, N, K, seed=13), None
    out = {}
    for half in (1, 0):
        gemm_option("gemm_half_tail", half)
        out[half] = {k: _gemm(lib, _lib.PREC_F16X3, A, W, bias, R if k[1] else None, k[0]) for k in _kinds(N)}
    for k in _kinds(N):
        assert np.array_equal(out[1][k], out[0][k]), k
    if small:
        F = out[1][(0, False)]
        tiny = (np.abs(F) < 2.0 ** -14) & (F != 0)
        assert tiny.mean() > 1 / 3 and (F == 0).any()
        for e in ACTS:
            _split_against_fp32(out[1][(e + 256, False)], out[1][(e, False)], ACTS[e])


@pytest.mark.parametrize("small", [False, True])
def test_a_row_alone_and_among_2300_same_bits(lib, small):
    """Row 0 as a launch of its own runs the guarded epilogue of an edge tile; among 2300 rows it sits in an interior tile."""
    M, N, K = 2300, 1280, 128
    A, W, bias, R = _operands(M, N, K, seed=14)
    if small:
        (A, W), bias = _small_operands(M, N, K, seed=15), None
    for epi, res in _kinds(N):
        many = _gemm(lib, _lib.PREC_F16X3, A, W, bias, R if res else None, epi)
        one = _gemm(lib, _lib.PREC_F16X3, A[:1].copy(), W, bias, R[:1].copy() if res else None, epi)
        assert np.array_equal(one[0], many[0]), (epi, res)
    if small:
        assert (np.abs(many[0]) < 2.0 ** -14).all()


@pytest.mark.parametrize("split", [0, 256])
@pytest.mark.parametrize("epi", [0, 1])
def test_non_finite_inputs_come_out_non_finite(lib, epi, split):
    """NaN and +-inf in A reach every output of their rows as non-finite values, through the fp32 and the split-plane epilogue (interior
    tiles and the edge tile alike); the other rows keep their bits."""
    M, N, K = 600, 1280, 128
    A, W, bias, _ = _operands(M, N, K, seed=16, row_scales=(1.0,))
    clean = _gemm(lib, _lib.PREC_F16X3, A, W, bias, None, epi + split)
    assert np.isfinite(clean).all()
    bad = A.copy()
    rows = [3, 100, 300, 599]
    bad[3, 7], bad[100, 0], bad[300, 127], bad[599, 64] = np.nan, np.inf, -np.inf, np.nan
    out = _gemm(lib, _lib.PREC_F16X3, bad, W, bias, None, epi + split)
    assert not np.isfinite(out[rows]).any()
    keep = np.ones(M, bool)
    keep[rows] = False
    assert np.array_equal(out[keep], clean[keep])
