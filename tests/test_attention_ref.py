"""Pins tests/attention_ref.py (the float64 reference of test_gpu_causal_attention.py) against torch's own operators, on the CPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import attention_ref as ar


def _qkv(rng, B, T, heads, lanes):
    Da = heads * lanes
    return [(rng.standard_normal((B, T, Da)) * s).astype(np.float32) for s in (0.4 * np.sqrt(64 / lanes), 1.0, 1.0)]


def _heads(t, heads, lanes):
    B, T, _ = t.shape
    return torch.from_numpy(t).double().reshape(B, T, heads, lanes).transpose(1, 2)


@pytest.mark.parametrize("B,T,heads,lanes", [(2, 1, 1, 64), (1, 33, 3, 64), (2, 70, 2, 128), (1, 129, 1, 256)])
def test_causal_attention_matches_torch_sdpa(B, T, heads, lanes):
    q, k, v = _qkv(np.random.default_rng(0), B, T, heads, lanes)
    got = ar.causal_attention(q, k, v, heads, lanes, np.zeros(heads, np.float32))
    want = F.scaled_dot_product_attention(*(_heads(t, heads, lanes) for t in (q, k, v)), is_causal=True, scale=1.0)
    want = want.transpose(1, 2).reshape(B, T, heads * lanes).numpy()
    assert got.dtype == np.float64 and np.abs(got - want).max() < 1e-12


@pytest.mark.parametrize("T,heads,lanes", [(40, 4, 64), (97, 2, 128)])
def test_alibi_matches_an_explicit_bias_matrix(T, heads, lanes):
    rng = np.random.default_rng(1)
    q, k, v = _qkv(rng, 2, T, heads, lanes)
    slopes = rng.uniform(0.0, 0.3, heads).astype(np.float32)
    got = ar.causal_attention(q, k, v, heads, lanes, slopes)
    bias = torch.zeros(heads, T, T, dtype=torch.float64)
    for h in range(heads):
        for i in range(T):
            for j in range(T):
                bias[h, i, j] = float(slopes[h]) * j if j <= i else float("-inf")
    want = F.scaled_dot_product_attention(*(_heads(t, heads, lanes) for t in (q, k, v)), attn_mask=bias[None], scale=1.0)
    want = want.transpose(1, 2).reshape(2, T, heads * lanes).numpy()
    assert np.abs(got - want).max() < 1e-12


def test_rotation_is_rotate_half_per_slot_group_and_restarts_per_sequence():
    rng = np.random.default_rng(2)
    B, T, heads, lanes = 2, 19, 2, 128
    x = rng.standard_normal((B, T, heads * lanes)).astype(np.float32)
    ang = rng.uniform(-3, 3, (T, lanes // 64, 32)).astype(np.float32)
    cos, sin = (np.concatenate([f(ang)] * 2, -1).astype(np.float32) for f in (np.cos, np.sin))
    got = ar.rotate_pairs(x, cos, sin, lanes).reshape(B, T, heads, lanes // 64, 64)
    xg = torch.from_numpy(x).double().reshape(B, T, heads, lanes // 64, 64)
    c, s = (torch.from_numpy(t).double()[None, :, None] for t in (cos, sin))
    want = xg * c + torch.cat((-xg[..., 32:], xg[..., :32]), -1) * s            # rotate_half inside every 64-lane group
    assert np.abs(got - want.numpy()).max() < 1e-13
    assert np.array_equal(got[0], ar.rotate_pairs(x[:1], cos, sin, lanes).reshape(1, T, heads, lanes // 64, 64)[0])
    one = ar.rotate_pairs(x[1:], cos, sin, lanes).reshape(1, T, heads, lanes // 64, 64)
    assert np.array_equal(got[1], one[0])                                      # sequence 1 starts at position 0 again


@pytest.mark.parametrize("heads", [4, 8])
def test_depthwise_filter_matches_torch_conv1d(heads):
    rng = np.random.default_rng(3)
    B, T = 3, 41
    qkv = rng.standard_normal((B, T, 3 * heads * 64)).astype(np.float32)
    conv = rng.standard_normal((3, 4, 64, 8)).astype(np.float32)
    got = ar.depthwise_filter(qkv, conv, heads).reshape(B, T, 3, heads, 64)
    x = torch.from_numpy(qkv).double().reshape(B, T, 3, heads, 64)
    for which in range(3):
        for h in range(heads):
            cw = torch.from_numpy(conv[which, h // (heads // 4)]).double()     # [64, 8]
            inp = F.pad(x[:, :, which, h].transpose(1, 2), (6, 0))             # [B, 64, 6 + T]: zero history before token 0
            want = F.conv1d(inp, cw[:, None, :7], cw[:, 7], groups=64).transpose(1, 2)
            assert np.abs(got[:, :, which, h] - want.numpy()).max() < 1e-12


def test_fp32_evaluation_stays_fp32():
    q, k, v = _qkv(np.random.default_rng(4), 1, 50, 2, 64)
    lo = ar.causal_attention(q, k, v, 2, 64, np.zeros(2, np.float32), dtype=np.float32)
    hi = ar.causal_attention(q, k, v, 2, 64, np.zeros(2, np.float32))
    assert lo.dtype == np.float32 and 0 < np.abs(lo - hi).max() < 1e-5
