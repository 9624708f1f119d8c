"""Plain NumPy reference of the MSA Transformer's two axial attentions as pgmi_op_tied_row_attention / pgmi_op_column_attention compute
them, the inputs and the case lists of test_gpu_axial_attention.py.  Every function computes in `dtype`: float64 is the reference,
float32 the "same reference in plain fp32" that sizes a tolerance (noise32).  Pinned against the oracle's einsum blocks in
test_axial_ref.py, where every GPU case's noise32 and bound are rehearsed on the CPU."""
import numpy as np

DH = 64


def _softmax(s):
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    return p


def tied_row_attention(qkv, R, C, H, dtype=np.float64):
    """qkv [R*C, 3*H*64], token order (r, c), q as given (pre-scaled by 1/8) -> (ctx [R*C, H*64], P [H, C, C]):
    s[h, i, j] = sum_{r, d} q[r, i, h, d] k[r, j, h, d] / sqrt(R), P = softmax_j, ctx[r, i, h, :] = sum_j P[h, i, j] v[r, j, h, :]."""
    D = H * DH
    x = np.asarray(qkv).astype(dtype).reshape(R, C, 3, H, DH)
    q, k, v = (x[:, :, w].transpose(2, 1, 0, 3) for w in range(3))                     # [H, C, R, 64]
    s = np.matmul(q.reshape(H, C, R * DH), k.reshape(H, C, R * DH).transpose(0, 2, 1)) / np.sqrt(dtype(R))
    p = _softmax(s)
    ctx = np.matmul(p, v.reshape(H, C, R * DH)).reshape(H, C, R, DH)                   # [h, i, r, d]
    return np.ascontiguousarray(ctx.transpose(2, 1, 0, 3)).reshape(R * C, D), p


def column_attention(X, W, bias, R, C, H, dtype=np.float64):
    """X [C*R, K], token order (c, r); W [3 D, K] (rows q | k | v), bias [3 D]: q | k | v = X W^T + bias in `dtype`, then for every
    column an ordinary softmax attention over its R rows, q as given.  Returns ctx [C*R, D], order (c, r)."""
    D = H * DH
    qkv = (np.asarray(X).astype(dtype) @ np.asarray(W).astype(dtype).T + np.asarray(bias).astype(dtype)).reshape(C, R, 3, H, DH)
    q, k, v = (qkv[:, :, w].transpose(0, 2, 1, 3) for w in range(3))                   # [C, H, R, 64]
    p = _softmax(np.matmul(q, k.transpose(0, 1, 3, 2)))
    return np.ascontiguousarray(np.matmul(p, v).transpose(0, 2, 1, 3)).reshape(C * R, D)


# ---- the product's rules, mirrored (msa_transformer.hip tied_row_kp / tied_row_splits) ------------------------------------------------
def tied_kp(C):
    return (C + 63) // 64 * 64


def tied_splits(R, C, H):
    """The largest S <= 16 that divides R and keeps S x (score tiles of one split) <= 640."""
    last = C % 256
    tm = (C + 127) // 128 if 0 < last <= 128 else (C + 255) // 256
    tiles = tm * ((C + 255) // 256) * H
    return max([1] + [s for s in range(1, 17) if R % s == 0 and tiles * s <= 640])


# ---- inputs (test_gpu_ops.py::test_attention / test_gpu_causal_attention.py::make_rows) ------------------------------------------------
def make_grid(rng, A, B, H, spiky_q, spiky_k):
    """q | k | v rows [A, B, 3 D] of standard normals, q times 0.4, V rows offset by a draw of 0 / 1e-3 / 5 per token; spiky_q / spiky_k:
    index tuples (into the [A, B] token grid) of the queries times 6 and of the keys times 6 whose V rows are 5."""
    D = H * DH
    x = rng.standard_normal((A, B, 3 * D)).astype(np.float32)
    x[..., :D] *= 0.4
    x[..., 2 * D:] += rng.choice([0.0, 1e-3, 5.0], size=(A, B, 1)).astype(np.float32)
    x[spiky_q + (slice(0, D),)] *= 6.0
    x[spiky_k + (slice(D, 2 * D),)] *= 6.0
    x[spiky_k + (slice(2 * D, 3 * D),)] = 5.0
    return x


def tied_inputs(R, C, H, seed=0):
    """qkv [R*C, 3 D], order (r, c): scores after / sqrt(R) spread by about 3; query column (2 C) // 3 spiky in every row (a near one-hot
    softmax row), key column max(C - 2, 0) spiky with V rows of 5."""
    rng = np.random.default_rng(100003 * R + 101 * C + H + seed)
    i0, je = (2 * C) // 3, max(C - 2, 0)
    x = make_grid(rng, R, C, H, (slice(None), i0), (slice(None), je))
    return np.ascontiguousarray(x.reshape(R * C, -1))


def column_inputs(R, C, H, seed=0):
    """(X [C*R, 3 D] order (c, r), W [3 D, 3 D], bias): rows as above (query row (2 R) // 3 of column 0 spiky, key row max(R - 2, 0) of
    every column spiky) and the near-identity weight of test_gpu_causal_attention.make_fused."""
    rng = np.random.default_rng(100003 * R + 101 * C + H + 7 + seed)
    x = make_grid(rng, C, R, H, (0, (2 * R) // 3), (slice(None), max(R - 2, 0)))
    K = x.shape[-1]
    W = (2e-4 * rng.standard_normal((K, K))).astype(np.float32)
    W[np.arange(K), np.arange(K)] += rng.uniform(0.8, 1.2, K).astype(np.float32)
    bias = (0.05 * rng.standard_normal(K)).astype(np.float32)
    bias[:K // 3] *= 0.1
    return np.ascontiguousarray(x.reshape(C * R, K)), W, bias


def bound(ref, noise32):
    """The suite's rule (test_gpu_causal_attention.py): max(2e-5 max(1, |ref|max), 3 noise32)."""
    return max(2e-5 * max(1.0, float(np.abs(ref).max())), 3.0 * noise32)


def tied_reference(qkv, R, C, H):
    """((ctx, P) in float64, (noise32, bound) of ctx, (noise32, bound) of P)."""
    ctx, p = tied_row_attention(qkv, R, C, H)
    c32, p32 = tied_row_attention(qkv, R, C, H, np.float32)
    nc, npr = float(np.abs(c32 - ctx).max()), float(np.abs(p32 - p).max())
    return (ctx, p), (nc, bound(ctx, nc)), (npr, bound(p, npr))


def column_reference(X, W, bias, R, C, H):
    """(ctx in float64, noise32, bound)."""
    ctx = column_attention(X, W, bias, R, C, H)
    n = float(np.abs(column_attention(X, W, bias, R, C, H, np.float32) - ctx).max())
    return ctx, n, bound(ctx, n)


# ---- the cases of test_gpu_axial_attention.py: (R, C, H) ------------------------------------------------------------------------------
TIED_COLUMN_EDGES = [(6, C, 2) for C in (1, 3, 4, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257, 385)] + [(4, 1024, 1)]
TIED_ROW_EDGES = [(R, 45, 2) for R in (1, 2, 7, 13, 16, 17, 34, 48)]
TIED_ROW_EDGE_SPLITS = [1, 2, 7, 13, 16, 1, 2, 16]
TIED_TILE_CAP = [(18, 300, 12)]                                                        # S = 6: the 640-tile cap decides
TIED_WIDTH = [(5, 70, H) for H in (1, 12, 20)]
TIED_FORCED = (12, 70, 2)
TIED_FORCED_SPLITS = [1, 2, 3, 4, 6, 12]
TIED_CASES = TIED_COLUMN_EDGES + TIED_ROW_EDGES + TIED_TILE_CAP + TIED_WIDTH
COLUMN_CASES = [(R, 3, 2) for R in (1, 2, 31, 32, 33, 64, 70, 97, 129, 224, 257)] + [(70, 45, 12), (33, 1, 1)]
