"""Float64 NumPy forward of ESM3 over the packed blob of proteingym_amd.esm3.pack, written independently of the device code as
esmc_ref.py is: the fold of the constant tracks into the input embedding (esm/models/esm3.py EncodeInputs), the backbone frames
(esm/utils/structure/affine3d.py build_affine3d_from_coordinates), the geometric attention of block 0
(esm/layers/geom_attention.py) and ESM C's blocks and head.  Shared by test_esm3_host.py and test_gpu_esm3.py."""
from math import erf, sqrt

import numpy as np

_erf = np.vectorize(erf)
STRUCTURE_MASK, STRUCTURE_EOS, STRUCTURE_BOS = 4096, 4097, 4098


def _layernorm(x, w, b=None, eps=1e-5):
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    y = (x - mu) / np.sqrt(var + eps) * w
    return y if b is None else y + b


def rbf16(v):
    """misc.py rbf(v, 0, 1, 16)."""
    centres = np.linspace(0.0, 1.0, 16)
    return np.exp(-(((v - centres) * 16.0) ** 2))


def frames(coords):
    """coords [T, >=3, 3] (N, CA, C) -> rot [T,3,3] (columns x, e1, e2), trans [T,3], mask [T]: Gram-Schmidt on (C, CA, N), origin CA;
    frameless tokens get the frame of the mean N / CA / C of the framed ones (the identity when there is none)."""
    c = np.array(coords[:, :3, :], dtype=np.float64)
    with np.errstate(invalid="ignore"):
        mask = (np.isfinite(c) & (c < 1e6)).all(-1).all(-1)
    c[~mask] = 0

    def gs(n, ca, cc):
        x = ca - cc
        x = x / np.sqrt((x ** 2).sum(-1, keepdims=True) + 1e-10)
        e1 = n - ca
        e1 = e1 - x * (x * e1).sum(-1, keepdims=True)
        e1 = e1 / np.sqrt((e1 ** 2).sum(-1, keepdims=True) + 1e-10)
        return np.stack([x, e1, np.cross(x, e1)], -1)
    rot, trans = gs(c[:, 0], c[:, 1], c[:, 2]), c[:, 1].copy()
    if mask.any():
        avg = c[mask].mean(0)
        hole_rot, hole_trans = gs(avg[0], avg[1], avg[2]), avg[1]
    else:
        hole_rot, hole_trans = np.eye(3), np.zeros(3)
    rot[~mask], trans[~mask] = hole_rot, hole_trans
    return rot, trans, mask


def geom_attention(proj, rot, trans, mask, w_rot, w_dist):
    """geom_attention.py:74-146 between proj and out_proj for one row: proj [S, 15H], rot [S,3,3], trans [S,3], mask [S], the
    softplus-ed per-head weights [H] -> [S, 3H].  Frameless keys get no weight; frameless queries give zero rows."""
    proj = np.asarray(proj, dtype=np.float64)
    rot, trans, mask = np.asarray(rot, dtype=np.float64).reshape(-1, 3, 3), np.asarray(trans, dtype=np.float64), np.asarray(mask, dtype=bool)
    S, H = proj.shape[0], proj.shape[1] // 15
    vr = np.einsum("sij,shj->shi", rot, proj[:, :9 * H].reshape(S, 3 * H, 3))
    q_rot, k_rot, v = vr[:, :H], vr[:, H:2 * H], vr[:, 2 * H:]
    vd = np.einsum("sij,shj->shi", rot, proj[:, 9 * H:].reshape(S, 2 * H, 3)) + trans[:, None, :]
    q_dist, k_dist = vd[:, :H], vd[:, H:]
    dist = np.sqrt(((q_dist[:, None] - k_dist[None, :]) ** 2).sum(-1))                     # [Sq, Sk, H]
    score = (np.einsum("qhc,khc->qkh", q_rot, k_rot) / sqrt(3) * np.asarray(w_rot, dtype=np.float64)
             - dist / sqrt(3) * np.asarray(w_dist, dtype=np.float64))
    out = np.zeros((S, H, 3))
    if mask.any():
        sc = score[:, mask]
        p = np.exp(sc - sc.max(1, keepdims=True))
        p /= p.sum(1, keepdims=True)
        g = np.einsum("qkh,khc->qhc", p, v[mask])
        out = np.einsum("sji,shj->shi", rot, g)                                            # R^T
        out[~mask] = 0
    return out.reshape(S, 3 * H)


def default_structure_tokens(T):
    return np.concatenate([[STRUCTURE_BOS], np.full(T - 2, STRUCTURE_MASK), [STRUCTURE_EOS]])


def numpy_forward(cfg, blob, ids, structure_tokens=None, coords=None):
    """log_softmax(sequence_logits) [T, 64] in float64 for one row of ids.  structure_tokens [T] and coords [T, >=3, 3] as the model
    gets them (the <cls> / <eos> rows non-finite); both None: sequence only."""
    D, F, V, H, L, Hv = cfg["embed_dim"], cfg["ffn_dim"], cfg["vocab"], cfg["heads"], cfg["layers"], cfg["v_heads"]
    dh = D // H
    o = 0

    def take(*shape):
        nonlocal o
        n = int(np.prod(shape))
        a = blob[o:o + n].astype(np.float64).reshape(shape)
        o += n
        return a
    ids = np.asarray(ids)
    T = len(ids)
    if structure_tokens is None:
        structure_tokens = default_structure_tokens(T)
    if coords is None:
        coords = np.full((T, 3, 3), np.nan)
    coords = np.asarray(coords, dtype=np.float64)
    plddt = np.isfinite(coords).all(-1).any(-1).astype(np.float64)
    seq_w, pl_w, pl_b, sp_w, sp_b = take(V, D), take(D, 16), take(D), take(D, 16), take(D)
    st_w, ss8_w, sasa_w = take(4101, D), take(11, D), take(19, D)
    x = (seq_w[ids] + (pl_w @ rbf16(1.0) + pl_b) + (np.stack([rbf16(p) for p in plddt]) @ sp_w.T + sp_b)
         + st_w[np.asarray(structure_tokens)] + ss8_w[0] + sasa_w[0])
    rot, trans, fmask = frames(coords)
    inv = (1.0 / (10000 ** (np.arange(0, dh, 2, dtype=np.float32) / np.float32(dh)))).astype(np.float32)
    ang = (np.arange(T, dtype=np.float32)[:, None] * inv[None, :]).astype(np.float64)
    cos, sin = np.concatenate([np.cos(ang)] * 2, -1)[:, None, :], np.concatenate([np.sin(ang)] * 2, -1)[:, None, :]

    def rotary(t):
        return t * cos + np.concatenate([-t[..., dh // 2:], t[..., :dh // 2]], -1) * sin
    s = sqrt(L / 36)
    for layer in range(L):
        ln1_w, ln1_b, wqkv = take(D), take(D), take(3 * D, D)
        q_ln, k_ln, wo = take(D), take(D), take(D, D)
        q, k, v = np.split(_layernorm(x, ln1_w, ln1_b) @ wqkv.T, 3, axis=-1)
        q, k = rotary(_layernorm(q, q_ln).reshape(T, H, dh)), rotary(_layernorm(k, k_ln).reshape(T, H, dh))
        sc = np.einsum("thd,shd->hts", q, k) / sqrt(dh)
        p = np.exp(sc - sc.max(-1, keepdims=True))
        p /= p.sum(-1, keepdims=True)
        x = x + (np.einsum("hts,shd->thd", p, v.reshape(T, H, dh)).reshape(T, D) @ wo.T) / s
        if layer == 0:
            d_scale, r_scale, g_norm, g_proj, g_out = take(Hv), take(Hv), take(D), take(15 * Hv, D), take(D, 3 * Hv)
            ctx = geom_attention(_layernorm(x, g_norm) @ g_proj.T, rot, trans, fmask, np.log1p(np.exp(r_scale)), np.log1p(np.exp(d_scale)))
            x = x + (ctx @ g_out.T) / s
        ln2_w, ln2_b = take(D), take(D)
        w1 = take(F // 32, 64, D)                     # blocks of 32 gate rows then 32 up rows
        gate_w, up_w = w1[:, :32].reshape(F, D), w1[:, 32:].reshape(F, D)
        w2 = take(D, F)
        h = _layernorm(x, ln2_w, ln2_b)
        g = h @ gate_w.T
        x = x + ((g / (1.0 + np.exp(-g))) * (h @ up_w.T) @ w2.T) / s
    x = _layernorm(x, take(D))
    w0, b0, lw, lb, w3, b3 = take(D, D), take(D), take(D), take(D), take(V, D), take(V)
    assert o == blob.size
    u = x @ w0.T + b0
    logits = _layernorm(0.5 * u * (1.0 + _erf(u / sqrt(2.0))), lw, lb) @ w3.T + b3
    logits -= logits.max(-1, keepdims=True)
    return logits - np.log(np.exp(logits).sum(-1, keepdims=True))
