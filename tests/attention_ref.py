"""Plain NumPy reference of the causal decoder attention in SLOT SPACE (heads of `lanes` = 64 G lanes, each G slot groups of 64), as
pgmi_op_causal_attention computes it: optional rotation of the slot pairs (i, i + 32) of every group, scores over all lanes of a head,
+ slope[h] * key, mask key <= query, softmax, P V; Tranception's right-aligned 7-tap causal depth-wise filter; and the encoder's dense
attention as pgmi_op_dense_attention computes it: the same rotation, every key below kv_len[b] visible to every query.  Every function
computes in `dtype`: float64 is the reference, float32 the "same reference in plain fp32" that sizes a tolerance (noise32).  Pinned
against torch's own operators in test_attention_ref.py; shared with test_gpu_causal_attention.py and test_gpu_dense_attention.py."""
import numpy as np


def rotate_pairs(x, cos, sin, lanes, dtype=np.float64):
    """x [B, T, heads * lanes]; cos / sin fp32 [T, lanes / 64, 64] (entry i of a group is the angle's; 32 + i repeats it): the pair
    (i, i + 32) of group g at position t becomes (a c - b s, b c + a s).  Positions restart at 0 for every sequence."""
    B, T, Da = x.shape
    G = lanes // 64
    xg = x.astype(dtype).reshape(B, T, Da // lanes, G, 2, 32)
    c = np.asarray(cos)[:T, None, :, :32].astype(dtype)
    s = np.asarray(sin)[:T, None, :, :32].astype(dtype)
    a, b = xg[..., 0, :], xg[..., 1, :]
    return np.stack([a * c - b * s, b * c + a * s], axis=-2).reshape(B, T, Da)


def causal_attention(q, k, v, heads, lanes, slopes, cos=None, sin=None, dtype=np.float64):
    """q, k, v [B, T, heads * lanes] (q pre-scaled) -> context [B, T, heads * lanes]."""
    B, T, Da = q.shape
    assert Da == heads * lanes
    if cos is not None:
        q, k = rotate_pairs(q, cos, sin, lanes, dtype), rotate_pairs(k, cos, sin, lanes, dtype)
    q, k, v = (t.astype(dtype).reshape(B, T, heads, lanes).transpose(0, 2, 1, 3) for t in (q, k, v))
    key = np.arange(T, dtype=dtype)
    bias = np.asarray(slopes).astype(dtype)[:, None, None] * key[None, None, :]
    visible = np.arange(T)[None, :] <= np.arange(T)[:, None]
    out = np.empty((B, heads, T, lanes), dtype)
    for b in range(B):
        s = np.matmul(q[b], k[b].transpose(0, 2, 1)) + bias
        s = np.where(visible[None], s, dtype(-np.inf))
        p = np.exp(s - s.max(-1, keepdims=True))
        p /= p.sum(-1, keepdims=True)
        out[b] = np.matmul(p, v[b])
    return out.transpose(0, 2, 1, 3).reshape(B, T, Da)


def depthwise_filter(qkv, conv, heads, dtype=np.float64):
    """qkv [B, T, 3 * heads * 64]; conv [3, 4, 64, 8]: per (q | k | v, head group h // (heads / 4), lane) seven taps, tap j on token
    t - 6 + j of the same sequence (zero before its start), entry 7 the bias.  Returns the filtered rows, same shape."""
    B, T, W = qkv.shape
    assert W == 3 * heads * 64 and heads % 4 == 0
    x = qkv.astype(dtype).reshape(B, T, 3, heads, 64)
    cw = np.asarray(conv).astype(dtype).reshape(3, 4, 64, 8)[:, np.arange(heads) // (heads // 4)]      # [3, heads, 64, 8]
    pad = np.concatenate([np.zeros((B, 6, 3, heads, 64), dtype), x], axis=1)
    y = np.broadcast_to(cw[None, None, ..., 7], x.shape).copy()
    for j in range(7):
        y += cw[None, None, ..., j] * pad[:, j:j + T]
    return y.reshape(B, T, W)


def fused_reference(X, W, bias, B, T, heads, lanes, slopes, cos=None, sin=None, dtype=np.float64):
    """The fused form: q | k | v = X W^T + bias in `dtype`, then causal_attention."""
    Da = heads * lanes
    qkv = (X.astype(dtype) @ W.astype(dtype).T + bias.astype(dtype)).reshape(B, T, 3 * Da)
    return causal_attention(qkv[..., :Da], qkv[..., Da:2 * Da], qkv[..., 2 * Da:], heads, lanes, slopes, cos, sin, dtype)


def conv_reference(qkv, conv, B, T, heads, slopes, dtype=np.float64):
    """The conv form (64 lanes): depthwise_filter, then causal_attention."""
    Da = heads * 64
    f = depthwise_filter(qkv.reshape(B, T, 3 * Da), conv, heads, dtype)
    return causal_attention(f[..., :Da], f[..., Da:2 * Da], f[..., 2 * Da:], heads, 64, slopes, dtype=dtype)


def dense_attention(q, k, v, heads, lanes, kv_len=None, cos=None, sin=None, dtype=np.float64):
    """q, k, v [B, T, heads * lanes] (q pre-scaled) -> context [B, T, heads * lanes]: every query of sequence b sees the keys below
    kv_len[b] (None: T), keys from kv_len[b] on are at -inf.  Rows t >= kv_len[b] are computed like any other query."""
    B, T, Da = q.shape
    assert Da == heads * lanes
    if cos is not None:
        q, k = rotate_pairs(q, cos, sin, lanes, dtype), rotate_pairs(k, cos, sin, lanes, dtype)
    q, k, v = (t.astype(dtype).reshape(B, T, heads, lanes).transpose(0, 2, 1, 3) for t in (q, k, v))
    kv_len = np.full(B, T) if kv_len is None else np.asarray(kv_len)
    out = np.empty((B, heads, T, lanes), dtype)
    for b in range(B):
        s = np.matmul(q[b], k[b].transpose(0, 2, 1))
        s = np.where(np.arange(T)[None, None, :] < kv_len[b], s, dtype(-np.inf))
        p = np.exp(s - s.max(-1, keepdims=True))
        p /= p.sum(-1, keepdims=True)
        out[b] = np.matmul(p, v[b])
    return out.transpose(0, 2, 1, 3).reshape(B, T, Da)


def dense_fused_reference(X, W, bias, B, T, heads, lanes, kv_len=None, cos=None, sin=None, dtype=np.float64):
    """The encoder's fused form: q | k | v = X W^T + bias in `dtype`, then dense_attention.  Returns (context [B, T, Da], the rotated
    q | k rows [B * T, 2 Da] without the kernels' log2(e) on q, the v rows [B * T, Da]) as it formed them."""
    Da = heads * lanes
    qkv = (X.astype(dtype) @ W.astype(dtype).T + bias.astype(dtype)).reshape(B, T, 3 * Da)
    q, k, v = qkv[..., :Da], qkv[..., Da:2 * Da], qkv[..., 2 * Da:]
    ctx = dense_attention(q, k, v, heads, lanes, kv_len, cos, sin, dtype)
    if cos is not None:
        q, k = rotate_pairs(q, cos, sin, lanes, dtype), rotate_pairs(k, cos, sin, lanes, dtype)
    return ctx, np.concatenate([q, k], -1).reshape(B * T, 2 * Da), np.ascontiguousarray(v).reshape(B * T, Da)
