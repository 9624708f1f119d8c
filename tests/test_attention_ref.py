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


def esm_slots(dh):
    """Slot (inside a head's 64 G lanes) of model dim j = 0 .. dh - 1 in the rotate-half layout (model.h rotate_half_slot): dh <= 64: j or
    32 + (j - dh / 2); dh 128: group (j >> 5) & 1, slot 32 (j >> 6) + (j & 31)."""
    j = np.arange(dh)
    if dh > 64:
        return ((j >> 5) & 1) * 64 + ((j >> 6) << 5) + (j & 31)
    return np.where(j < dh // 2, j, 32 + j - dh // 2)


def esm2_tables(T, dh):
    """upload_rotate_half (api_esm.hip) restated: cos / sin fp32 [T, G, 64], G = 2 for dh 128 else 1.  fp32 inv[j] = 1 / powf(10000,
    2 j / dh), fp32 angle t * inv[j]; slots i and 32 + i of group g hold the pair j = i (dh <= 64) or 32 g + i (dh 128); j >= dh / 2: angle 0."""
    G = 2 if dh == 128 else 1
    g, i = np.meshgrid(np.arange(G), np.arange(32), indexing="ij")
    j = i if G == 1 else 32 * g + i
    inv = np.float32(1.0) / np.power(np.float32(10000.0), (2 * j).astype(np.float32) / np.float32(dh), dtype=np.float32)
    inv = np.where(j < dh // 2, inv, np.float32(0.0)).astype(np.float32)
    ang = np.arange(T, dtype=np.float32)[:, None, None] * inv[None]
    assert ang.dtype == np.float32
    return tuple(np.ascontiguousarray(np.concatenate([f(ang)] * 2, -1), dtype=np.float32) for f in (np.cos, np.sin))


RAGGED = [(2, 1, 1, 64, None), (3, 33, 3, 64, [33, 17, 1]), (2, 70, 2, 128, [32, 70]), (3, 97, 2, 64, [32, 33, 64])]


@pytest.mark.parametrize("B,T,heads,lanes,kv_len", RAGGED)
def test_dense_attention_matches_torch_softmax_with_a_key_padding_mask(B, T, heads, lanes, kv_len):
    q, k, v = _qkv(np.random.default_rng(5), B, T, heads, lanes)
    got = ar.dense_attention(q, k, v, heads, lanes, kv_len)
    tq, tk, tv = (_heads(t, heads, lanes) for t in (q, k, v))
    scores = tq @ tk.transpose(-1, -2)                                          # [B, heads, T, T]
    if kv_len is not None:
        pad = torch.arange(T)[None, :] >= torch.tensor(kv_len)[:, None]         # [B, T]: True at a padded key
        scores = scores.masked_fill(pad[:, None, None, :], float("-inf"))
    want = (torch.softmax(scores, -1) @ tv).transpose(1, 2).reshape(B, T, heads * lanes).numpy()
    assert got.dtype == np.float64 and np.isfinite(got).all() and np.abs(got - want).max() < 1e-12
    if kv_len is not None:                                                      # what a masked key holds does not matter
        k2, v2 = k.copy(), v.copy()
        for b, n in enumerate(kv_len):
            k2[b, n:], v2[b, n:] = 50.0, -7.0
        assert np.array_equal(ar.dense_attention(q, k2, v2, heads, lanes, kv_len), got)


@pytest.mark.parametrize("dh", [16, 24, 32, 64, 128])
def test_esm2_tables_and_slots_are_esm_rotate_half(dh):
    """A head of dh model dims laid into its slots and rotated by rotate_pairs with the tables of esm2_tables equals ESM's
    x cos + rotate_half(x) sin (rotary_embedding.py) in model space with the same fp32 cos / sin; the padded slots stay zero."""
    rng = np.random.default_rng(dh)
    B, T, heads = 2, 41, 3
    lanes = 128 if dh == 128 else 64
    slots = esm_slots(dh)
    assert len(set(slots.tolist())) == dh and slots.max() < lanes
    cos, sin = esm2_tables(T, dh)
    assert cos.shape == (T, lanes // 64, 64) and cos.dtype == np.float32
    assert np.array_equal(cos[..., :32], cos[..., 32:]) and np.array_equal(sin[..., :32], sin[..., 32:])
    # the frequencies are ESM's: inv_freq = 1 / 10000^(arange(0, dh, 2) / dh) in fp32, angle t * inv_freq in fp32
    inv = 1.0 / (10000 ** (torch.arange(0, dh, 2).float() / dh))
    ang = torch.outer(torch.arange(T).float(), inv).numpy()                      # [T, dh / 2]
    first = slots[:dh // 2]                                                     # slot of dim j < dh / 2 = its pair's table entry
    tab = cos.reshape(T, lanes)[:, first], sin.reshape(T, lanes)[:, first]
    assert np.abs(tab[0] - np.cos(ang)).max() < 1e-4 and np.abs(tab[1] - np.sin(ang)).max() < 1e-4   # fp32 angles up to 40 rad: ulp(40) = 4e-6
    assert np.abs(tab[1][:2] - np.sin(ang)[:2]).max() < 5e-7                    # t = 0, 1: the angle is inv_freq itself (an ulp of pow, an ulp of sin)
    x = rng.standard_normal((B, T, heads, dh)).astype(np.float32)
    xs = np.zeros((B, T, heads, lanes), np.float32)
    xs[..., slots] = x
    got = ar.rotate_pairs(xs.reshape(B, T, heads * lanes), cos, sin, lanes).reshape(B, T, heads, lanes)
    c, s = (torch.from_numpy(np.concatenate([t, t], -1)).double()[None, :, None] for t in tab)    # emb = cat(freqs, freqs)
    xt = torch.from_numpy(x).double()
    want = xt * c + torch.cat((-xt[..., dh // 2:], xt[..., :dh // 2]), -1) * s
    assert np.abs(got[..., slots] - want.numpy()).max() < 1e-13
    holes = np.setdiff1d(np.arange(lanes), slots)
    assert np.all(got[..., holes] == 0.0)


@pytest.mark.parametrize("dh", [32, 64, 128])
def test_dense_fused_reference_matches_torch(dh):
    rng = np.random.default_rng(6)
    B, T, heads, K = 3, 37, 2, 96
    lanes = 128 if dh == 128 else 64
    Da, kv_len = heads * lanes, [37, 19, 1]
    X = rng.standard_normal((B * T, K)).astype(np.float32)
    W = (rng.standard_normal((3 * Da, K)) / np.sqrt(K)).astype(np.float32)
    bias = rng.standard_normal(3 * Da).astype(np.float32)
    cos, sin = esm2_tables(T, dh)
    ctx, qk, v = ar.dense_fused_reference(X, W, bias, B, T, heads, lanes, kv_len, cos, sin)
    qkv = F.linear(torch.from_numpy(X).double(), torch.from_numpy(W).double(), torch.from_numpy(bias).double()).numpy().reshape(B, T, 3 * Da)
    q, k = (ar.rotate_pairs(qkv[..., i * Da:(i + 1) * Da], cos, sin, lanes) for i in (0, 1))
    assert np.abs(qk - np.concatenate([q, k], -1).reshape(B * T, 2 * Da)).max() < 1e-12
    assert np.abs(v - qkv[..., 2 * Da:].reshape(B * T, Da)).max() < 1e-12
    tq, tk, tv = (torch.from_numpy(np.ascontiguousarray(t)).reshape(B, T, heads, lanes).transpose(1, 2) for t in (q, k, qkv[..., 2 * Da:]))
    pad = torch.arange(T)[None, :] >= torch.tensor(kv_len)[:, None]
    p = torch.softmax((tq @ tk.transpose(-1, -2)).masked_fill(pad[:, None, None, :], float("-inf")), -1)
    want = (p @ tv).transpose(1, 2).reshape(B, T, Da).numpy()
    assert ctx.shape == (B, T, Da) and np.abs(ctx - want).max() < 1e-12
    lo = ar.dense_fused_reference(X, W, bias, B, T, heads, lanes, kv_len, cos, sin, dtype=np.float32)
    assert all(t.dtype == np.float32 for t in lo) and 0 < np.abs(lo[0] - ctx).max() < 1e-4


def test_fp32_evaluation_stays_fp32():
    q, k, v = _qkv(np.random.default_rng(4), 1, 50, 2, 64)
    lo = ar.causal_attention(q, k, v, 2, 64, np.zeros(2, np.float32), dtype=np.float32)
    hi = ar.causal_attention(q, k, v, 2, 64, np.zeros(2, np.float32))
    assert lo.dtype == np.float32 and 0 < np.abs(lo - hi).max() < 1e-5
