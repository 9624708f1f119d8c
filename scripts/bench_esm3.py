"""Secondary measurement: ESM3 scoring with structure, end to end from mutant strings to scores (ESM3.score_mutations_with_pdb's body on
arrays: tokenizer per distinct window, masked forwards on the HIP trunk), at the released shape (48 x 1536, v_heads 256; structure
encoder 2 x 1024, v_heads 128) with seeded weights and seeded random-walk backbones.  Two targets: L = 286 with every single mutant
(one window), and L = 1100 with positions spread over ten distinct windows (T = 1024 forwards).  Prints one JSON line per target:
mutants/s, masked forwards/s, the per-class HIP-event breakdown with the geometric attention kernel's share, the structure
tokenizer's seconds per distinct window, and the same masked forwards in fp32 torch on the same GPU.

    python scripts/bench_esm3.py [--layers 48] [--no-torch]
"""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.getcwd())
from proteingym_amd import _lib, esm3, synthetic  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--layers", type=int, default=48)
ap.add_argument("--embed_dim", type=int, default=1536)
ap.add_argument("--v_heads", type=int, default=256)
ap.add_argument("--no-torch", action="store_true", help="skip the fp32 torch comparison")
ap.add_argument("--torch-rows", type=int, default=8, help="masked rows per torch forward at L = 286 (1 at T = 1024)")
args = ap.parse_args()
lib = _lib.load()
AA = "ACDEFGHIKLMNPQRSTVWY"
rng = np.random.default_rng(29)


def backbone(L):
    def unit(n):
        v = rng.standard_normal((n, 3))
        return v / np.linalg.norm(v, axis=-1, keepdims=True)
    ca = np.cumsum(3.8 * unit(L), axis=0)
    x = np.full((L, 37, 3), np.nan, dtype=np.float32)
    x[:, :3] = np.stack([ca + 1.46 * unit(L), ca, ca + 1.52 * unit(L)], axis=1)
    return x


def torch_forward(w, cfg, ids, stok, coords, rows, device):
    """The same masked forwards in fp32 torch: log-probabilities [len(rows), 64] at the masked positions (rows: positions, one
    forward each, batched by the caller)."""
    import torch
    import torch.nn.functional as TF
    D, H, L, Hv = cfg["embed_dim"], cfg["heads"], cfg["layers"], cfg["v_heads"]
    T, B, dh = len(ids), len(rows), 64
    tok = torch.from_numpy(np.repeat(ids[None], B, 0)).long().to(device)
    ar, at = torch.arange(B, device=device), torch.as_tensor(rows, device=device)
    tok[ar, at] = esm3.MASK
    rot, trans, mask = esm3.build_frames(coords)
    plddt = torch.from_numpy(esm3.per_res_plddt(coords)).float().to(device)
    R = torch.from_numpy(rot).to(device).view(T, 3, 3)
    t = torch.from_numpy(trans).to(device)
    fm = torch.from_numpy(mask).to(device)

    def rbf(v):
        c = torch.linspace(0.0, 1.0, 16, device=device)
        return torch.exp(-(((v.unsqueeze(-1) - c) * 16.0) ** 2))
    x = (w["encoder.sequence_embed.weight"][tok] + TF.linear(rbf(torch.ones(T, device=device)), w["encoder.plddt_projection.weight"], w["encoder.plddt_projection.bias"])
         + TF.linear(rbf(plddt), w["encoder.structure_per_res_plddt_projection.weight"], w["encoder.structure_per_res_plddt_projection.bias"])
         + w["encoder.structure_tokens_embed.weight"][torch.from_numpy(stok).long().to(device)] + w["encoder.ss8_embed.weight"][0] + w["encoder.sasa_embed.weight"][0])
    inv = 1.0 / (10000 ** (torch.arange(0, dh, 2, device=device).float() / dh))
    ang = torch.arange(T, device=device).float()[:, None] * inv[None]
    cos, sin = torch.cat([ang.cos()] * 2, -1)[None, :, None], torch.cat([ang.sin()] * 2, -1)[None, :, None]

    def rope(v):
        return v * cos + torch.cat([-v[..., dh // 2:], v[..., :dh // 2]], -1) * sin
    s = math.sqrt(L / 36)
    for i in range(L):
        p = f"transformer.blocks.{i}."
        q, k, v = TF.linear(TF.layer_norm(x, (D,), w[p + "attn.layernorm_qkv.0.weight"], w[p + "attn.layernorm_qkv.0.bias"]),
                            w[p + "attn.layernorm_qkv.1.weight"]).chunk(3, -1)
        q, k = TF.layer_norm(q, (D,), w[p + "attn.q_ln.weight"]), TF.layer_norm(k, (D,), w[p + "attn.k_ln.weight"])
        q, k, v = rope(q.view(B, T, H, dh)).transpose(1, 2), rope(k.view(B, T, H, dh)).transpose(1, 2), v.view(B, T, H, dh).transpose(1, 2)
        ctx = TF.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B, T, D)
        x = x + TF.linear(ctx, w[p + "attn.out_proj.weight"]) / s
        if i == 0 and mask.any():
            g = p + "geom_attn."
            pr = TF.linear(TF.layer_norm(x, (D,), w[g + "s_norm.weight"]), w[g + "proj.weight"])
            vr = torch.einsum("tij,bthj->bthi", R, pr[..., :9 * Hv].reshape(B, T, 3 * Hv, 3))
            vd = torch.einsum("tij,bthj->bthi", R, pr[..., 9 * Hv:].reshape(B, T, 2 * Hv, 3)) + t[None, :, None]
            qr, kr, vv = vr[:, :, :Hv], vr[:, :, Hv:2 * Hv], vr[:, :, 2 * Hv:]
            qd, kd = vd[:, :, :Hv].transpose(1, 2), vd[:, :, Hv:].transpose(1, 2)
            sc = (torch.einsum("bqhc,bkhc->bhqk", qr, kr) / math.sqrt(3) * TF.softplus(w[g + "rotation_scale_per_head"])[None, :, None, None]
                  - torch.cdist(qd, kd, compute_mode="donot_use_mm_for_euclid_dist") / math.sqrt(3) * TF.softplus(w[g + "distance_scale_per_head"])[None, :, None, None])
            sc = sc.masked_fill(~fm[None, None, None, :], float("-inf"))
            o = torch.einsum("bhqk,bkhc->bqhc", sc.softmax(-1), vv)
            o = torch.einsum("tji,bthj->bthi", R, o).masked_fill(~fm[None, :, None, None], 0.0).reshape(B, T, 3 * Hv)
            x = x + TF.linear(o, w[g + "out_proj.weight"]) / s
        h = TF.linear(TF.layer_norm(x, (D,), w[p + "ffn.0.weight"], w[p + "ffn.0.bias"]), w[p + "ffn.1.weight"])
        a, b = h.chunk(2, -1)
        x = x + TF.linear(TF.silu(a) * b, w[p + "ffn.3.weight"]) / s
    x = TF.layer_norm(x[ar, at], (D,), w["transformer.norm.weight"])
    o = "output_heads.sequence_head."
    x = TF.layer_norm(TF.gelu(TF.linear(x, w[o + "0.weight"], w[o + "0.bias"])), (D,), w[o + "2.weight"], w[o + "2.bias"])
    return torch.log_softmax(TF.linear(x, w[o + "3.weight"], w[o + "3.bias"]), -1)


cfg = synthetic.esm3_config(args.embed_dim, args.layers, args.v_heads)
t0 = time.perf_counter()
sd = synthetic.esm3_state_dict(cfg, seed=3)
sd = {k: sd[k] for k in esm3.expected_keys(cfg["layers"])}                 # the heads this path does not read are not needed here
enc_sd = synthetic.esm3_encoder_state_dict(synthetic.esm3_encoder_config(), seed=4)
torch_device = None
if not args.no_torch:
    import torch
    torch_device = "cuda" if torch.cuda.is_available() else None
model = esm3.ESM3(cfg, esm3.pack(cfg, sd), encoder=esm3.StructureEncoder(enc_sd, torch_device=torch_device))
print(json.dumps(dict(setup_s=round(time.perf_counter() - t0, 1))), flush=True)

targets = []
seq = "".join(rng.choice(list(AA), 286))
targets.append(("L286_all_singles", seq, [f"{seq[p]}{p + 1}{a}" for p in range(len(seq)) for a in AA if a != seq[p]]))
seq = "".join(rng.choice(list(AA), 1100))
pos = sorted(set(list(range(0, 511, 16)) + list(range(515, 589, 10)) + list(range(600, 1100, 16))))
targets.append(("L1100_ten_windows", seq, [f"{seq[p]}{p + 1}{a}" for p in pos for a in AA if a != seq[p]]))

for name, seq, muts in targets:
    atom37 = backbone(len(seq))
    parsed = esm3.parse_mutations(seq, muts)
    n_pos = len({p for _, _, _, sp, _ in parsed for p in sp})
    model._score(seq, parsed[:19], atom37, esm3.WINDOW_SIZE)               # warm-up: first launches, first torch kernels
    model.windows_encoded = 0
    t0 = time.perf_counter()
    scores = model._score(seq, parsed, atom37, esm3.WINDOW_SIZE)
    dt = time.perf_counter() - t0
    n_win = model.windows_encoded
    # the tokenizer alone, and the forwards alone under the profiler
    windows = sorted({esm3.window(p, len(seq)) for _, _, _, sp, _ in parsed for p in sp})
    t0 = time.perf_counter()
    for s_, e_ in windows:
        model.encoder.encode(atom37[s_:e_])
    tok_s = (time.perf_counter() - t0) / len(windows)
    lib.pgmi_profile_enable(model._h, 1)
    lib.pgmi_profile_reset(model._h)
    model._score(seq, parsed, atom37, esm3.WINDOW_SIZE)
    lib.pgmi_profile_enable(model._h, 0)
    prof, total = {}, 0.0
    for k, kname in enumerate(_lib.K_NAMES):
        ms, n, fl, by = C.c_double(), C.c_int64(), C.c_double(), C.c_double()
        if lib.pgmi_profile_get(model._h, k, C.byref(ms), C.byref(n), C.byref(fl), C.byref(by)) == 0 and n.value:
            prof[kname] = dict(ms=round(ms.value, 2), calls=n.value)
            total += ms.value
    out = dict(target=name, layers=cfg["layers"], embed_dim=cfg["embed_dim"], v_heads=cfg["v_heads"], L=len(seq), mutants=len(scores),
               forwards=n_pos, distinct_windows=n_win, seconds=round(dt, 3), mutants_per_s=round(len(scores) / dt, 1),
               forwards_per_s=round(n_pos / dt, 2), tokenizer_s_per_window=round(tok_s, 3), kernels_profiled=prof,
               device_ms=round(total, 1), geom_share=round(prof.get("geom", {}).get("ms", 0.0) / total, 4) if total else None)
    if not args.no_torch and torch_device:
        import torch
        w = {k: torch.from_numpy(v).to(torch_device) for k, v in sd.items()}
        s_, e_ = windows[0]
        coords, tokens = model.encoder.encode(atom37[s_:e_])
        coords, stok = esm3.pad_window(coords, tokens)
        ids = np.concatenate([[esm3.CLS], esm3.tokenize(seq)[1 + s_:1 + e_], [esm3.EOS]]).astype(np.int32)
        rows = [p - s_ + 1 for p in sorted({p for _, _, _, sp, _ in parsed for p in sp}) if esm3.window(p, len(seq)) == (s_, e_)]
        per = args.torch_rows if len(ids) < 512 else 1
        rows = rows[:4 * per]
        model.set_window(len(ids), stok, coords)
        ours = model.masked_logprobs(np.repeat(ids[None], len(rows), 0), rows)
        with torch.no_grad():
            torch_forward(w, cfg, ids, stok, coords[:, :3], rows[:per], torch_device)          # warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ref = torch.cat([torch_forward(w, cfg, ids, stok, coords[:, :3], rows[i:i + per], torch_device) for i in range(0, len(rows), per)])
            torch.cuda.synchronize()
            tdt = time.perf_counter() - t0
        t0 = time.perf_counter()
        model.masked_logprobs(np.repeat(ids[None], len(rows), 0), rows)
        odt = time.perf_counter() - t0
        out.update(torch_fp32_forwards_per_s=round(len(rows) / tdt, 2), hip_forwards_per_s_same_rows=round(len(rows) / odt, 2),
                   max_abs_diff_vs_torch_fp32=float(np.abs(ours - ref.cpu().numpy()).max()))
        del w
    print(json.dumps(out), flush=True)
model.close()
