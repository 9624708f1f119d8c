"""The f16x3 / bf16 GEMM on 16x16x32 MFMAs (gemm16x_kernel.h): every output form at the 16-row and 16-column boundaries of the
accumulator tiles, where a lane -> (row, column) mapping error of the 16-row layout would show and the 32-row layout's could not."""
import numpy as np
import pytest
import torch

from proteingym_amd import _lib

pytestmark = pytest.mark.gpu

ROWS = [1, 15, 17, 241, 272, 2300]        # one row, either side of a 16-row tile, inside the last M16 tile of a half item, a half-tail launch
N_RAGGED, K = 1284, 256                   # the last column tile holds one N16 tile of a wave (N % 256 = 4, N % 16 = 4)
N_PLANES = 1312                           # the split-plane form needs N % 32 == 0: the last tile holds two N16 tiles of one wave


def _p(a, ty=_lib._f32p):
    return a.ctypes.data_as(ty) if a is not None else None


def _operands(M, seed, N=N_RAGGED):
    rng = np.random.default_rng(seed)
    A = (rng.standard_normal((M, K)) * rng.choice([0.01, 1.0, 30.0], size=(M, 1))).astype(np.float32)
    W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    R = rng.standard_normal((M, N)).astype(np.float32)
    return A, W, bias, R


def _ref(A, W, bias, R, gelu):
    pre = torch.from_numpy(A).double() @ torch.from_numpy(W).double().T + torch.from_numpy(bias).double()
    out = pre * 0.5 * (1.0 + torch.erf(pre / np.sqrt(2.0))) if gelu else pre
    if R is not None:
        out = out + torch.from_numpy(R).double()
    return out.numpy()


@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("res", [False, True])
def test_fp32_out_at_tile_boundaries(lib, M, res):
    """OUT 0 (fp32, + residual): every element against fp64, tolerance as test_gemm_f16x3."""
    A, W, bias, R = _operands(M, 11)
    R = R if res else None
    C = np.full((M, N_RAGGED), np.nan, np.float32)
    _lib.check(lib.pgmi_op_gemm(0, _lib.PREC_F16X3, _p(A), _p(W), _p(bias), _p(R), M, N_RAGGED, K, 0, _p(C)))
    scale = np.maximum(np.abs(A).max(1, keepdims=True), 1.0)
    assert (np.abs(C - _ref(A, W, bias, R, False)) / scale).max() < 2e-5 * np.sqrt(K / 128)


@pytest.mark.parametrize("M", ROWS)
def test_split_plane_out_with_gelu_at_tile_boundaries(lib, M):
    """OUT 1 (K-interleaved split planes, GELU): against fp64, and to the operand's 22 bits of the fp32 form."""
    A, W, bias, _ = _operands(M, 12, N_PLANES)
    P = np.full((M, N_PLANES), np.nan, np.float32)
    _lib.check(lib.pgmi_op_gemm(0, _lib.PREC_F16X3, _p(A), _p(W), _p(bias), None, M, N_PLANES, K, 1 + 256, _p(P)))
    F = np.full((M, N_PLANES), np.nan, np.float32)
    _lib.check(lib.pgmi_op_gemm(0, _lib.PREC_F16X3, _p(A), _p(W), _p(bias), None, M, N_PLANES, K, 1, _p(F)))
    assert np.isfinite(P).all()
    scale = np.maximum(np.abs(A).max(1, keepdims=True), 1.0)
    assert (np.abs(F - _ref(A, W, bias, None, True)) / scale).max() < 2e-5 * np.sqrt(K / 128)
    assert np.abs(P - F).max() <= np.abs(F).max() * 2.0 ** -21


@pytest.mark.parametrize("M", ROWS)
def test_bf16_forms_at_tile_boundaries(lib, M):
    """The one-plane bf16 form: fp32 out against fp64 on the bf16-rounded operands, the bf16-plane out = that rounded to bf16."""
    A, W, bias, _ = _operands(M, 13)
    C = np.full((M, N_RAGGED), np.nan, np.float32)
    _lib.check(lib.pgmi_op_gemm(0, _lib.PREC_BF16, _p(A), _p(W), _p(bias), None, M, N_RAGGED, K, 0, _p(C)))
    ref = (torch.from_numpy(A).bfloat16().double() @ torch.from_numpy(W).bfloat16().double().T + torch.from_numpy(bias).double())
    scale = np.maximum(np.abs(A).max(1, keepdims=True), 1.0)
    assert (np.abs(C - ref.numpy()) / scale).max() < 1e-4
    Cp = np.full((M, N_RAGGED), np.nan, np.float32)
    _lib.check(lib.pgmi_op_gemm(0, _lib.PREC_BF16, _p(A), _p(W), _p(bias), None, M, N_RAGGED, K, 256, _p(Cp)))
    assert np.array_equal(Cp, torch.from_numpy(C).bfloat16().float().numpy())


@pytest.mark.parametrize("T", [17, 45])
def test_esm2_fused_qkv_rotary_vs_fp64(lib, T):
    """An ESM2 forward at T = 17 / 45 tokens: the fused QKV epilogue (q . log2e | k planes with rotary, the transposed,
    key-permuted V^T planes) feeds attention; token log-probs against the fp64 oracle."""
    from oracle import esm_oracle as eo
    from proteingym_amd import esm as pesm, synthetic
    cfg = dict(synthetic.ESM2_650M, layers=2, embed_dim=256, heads=4, ffn_dim=512)
    blob = synthetic.random_weights(cfg, seed=21)
    seq = synthetic.random_sequence(np.random.default_rng(T), T - 2)
    _, _, toks = pesm.Alphabet().get_batch_converter()([("p", seq)])
    m = pesm.EsmModel(cfg, blob, device=0)
    try:
        lp = np.asarray(m(toks)["logits"][0])
    finally:
        m.close()
    ocfg, W = eo.from_arrays(arrays=synthetic.blob_to_arrays(cfg, blob), dtype=torch.float64, **cfg)
    ref = torch.log_softmax(eo.forward_logits(ocfg, W, np.asarray(toks))[0].double(), -1).numpy()
    assert lp.shape == ref.shape
    assert np.abs(lp - ref).max() < 1e-4
