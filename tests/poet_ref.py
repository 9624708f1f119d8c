"""TEST INFRASTRUCTURE ONLY -- a restatement of PoET (proteingym/baselines/PoET) and of its scoring arithmetic in torch on the CPU, in
float64 (what the GPU tests compare against) or float32 (the noise floor of a plain fp32 implementation).  It reads nothing of the
reference tree; tests/test_poet_host.py pins it to the live reference where that tree exists.

The model is a state dict (names as in the checkpoint, leading component stripped) and the config of proteingym_amd.poet."""
import numpy as np
import torch

MASK = 23


class PoetRef:
    def __init__(self, cfg, sd, dtype=torch.float64):
        self.cfg, self.dtype = cfg, dtype
        self.sd = {k: torch.as_tensor(np.asarray(v, dtype=np.float32)).to(dtype) for k, v in sd.items()}
        self.H = cfg["heads"]
        self.dh = cfg["embed_dim"] // self.H
        # RotaryEmbedding: inv_freq in float32, pairs (2i, 2i + 1) share a frequency; the angle is fp32 whatever the model's dtype
        r = torch.div(torch.arange(self.dh), 2, rounding_mode="floor") * 2.0 / self.dh
        self.inv_freq = (1.0 / (10000 ** r)).float()

    def _ln(self, x, name):
        return torch.nn.functional.layer_norm(x, (x.shape[-1],), self.sd[name + ".weight"], self.sd[name + ".bias"], 1e-5)

    def _rot(self, x, pos):
        """x [n, H, dh]: x cos + rotate_half(x) sin with interleaved pairs"""
        f = torch.outer(pos, self.inv_freq)
        cos, sin = torch.cos(f).to(self.dtype)[:, None, :], torch.sin(f).to(self.dtype)[:, None, :]
        x1, x2 = x[..., 0::2], x[..., 1::2]
        return x * cos + torch.stack((-x2, x1), dim=-1).flatten(-2) * sin

    def _attention(self, p, h, group, pos, memory):
        """Rows attend causally (by row order) inside their group, and to every memory row.  Returns (context, (k, v))."""
        n = h.shape[0]
        q = (h @ self.sd[p + "q_proj.weight"].T).view(n, self.H, self.dh) * self.dh ** -0.5
        k = (h @ self.sd[p + "k_proj.weight"].T).view(n, self.H, self.dh)
        v = (h @ self.sd[p + "v_proj.weight"].T).view(n, self.H, self.dh)
        q, k = self._rot(q, pos), self._rot(k, pos)
        idx = torch.arange(n)
        mask = (group[:, None] == group[None, :]) & (idx[None, :] <= idx[:, None])
        ka, va = k, v
        if memory is not None:
            ka, va = torch.cat([memory[0], k]), torch.cat([memory[1], v])
            mask = torch.cat([torch.ones(n, memory[0].shape[0], dtype=torch.bool), mask], dim=1)
        s = torch.einsum("ihd,jhd->hij", q, ka).masked_fill(~mask[None], float("-inf"))
        ctx = torch.einsum("hij,jhd->ihd", torch.softmax(s, dim=-1), va).reshape(n, -1)
        return ctx @ self.sd[p + "out_proj.weight"].T + self.sd[p + "out_proj.bias"], (k, v)

    def forward(self, tokens, seg1, seg2, pos, memory=None):
        """tokens [n]; seg1 / seg2 [n]: the group of every row in the within-sequence / sequence-of-sequences attention; memory: per
        layer (k, v) of a prompt's second attention.  Returns (log-probabilities [n, V], this call's per-layer (k, v))."""
        tokens, seg1, seg2 = (torch.as_tensor(np.asarray(a)).long() for a in (tokens, seg1, seg2))
        pos = torch.as_tensor(np.asarray(pos)).long()
        x = self.sd["token_embed.weight"][tokens]
        out_mem = []
        for l in range(self.cfg["layers"]):
            p = f"decoder.layers.{l}."
            a, _ = self._attention(p + "self_attn.", self._ln(x, p + "norm1"), seg1, pos, None)
            x = x + a
            a, kv = self._attention(p + "multihead_attn.", self._ln(x, p + "norm2"), seg2, pos, memory[l] if memory is not None else None)
            x = x + a
            out_mem.append(kv)
            h = torch.nn.functional.gelu(self._ln(x, p + "norm3") @ self.sd[p + "linear1.weight"].T + self.sd[p + "linear1.bias"])
            x = x + h @ self.sd[p + "linear2.weight"].T + self.sd[p + "linear2.bias"]
        if self.cfg["final_norm"]:
            x = self._ln(x, "norm")
        logits = x @ self.sd["linear.weight"].T + self.sd["linear.bias"]
        return torch.log_softmax(logits, dim=-1), out_mem

    def prompt(self, sequences):
        """PoET.forward / embed over a sequence-of-sequences: (log-probabilities [total, V], memory)."""
        tokens = np.concatenate(sequences)
        seg = np.concatenate([np.full(len(s), i) for i, s in enumerate(sequences)])
        pos = np.concatenate([np.arange(len(s)) for s in sequences])
        lp, mem = self.forward(tokens, seg, np.zeros_like(seg), pos)
        return lp.numpy(), mem

    def variant_logprobs(self, variant, memory):
        """PoET.logits for one variant's tokens: log-probabilities [len, V]"""
        z = np.zeros(len(variant), dtype=np.int64)
        return self.forward(variant, z, z, np.arange(len(variant)), memory)[0].numpy()

    def score(self, variant, memory):
        """scripts/score.py: sum over the targets variant[1:] of the log-probability, mask targets ignored"""
        lp = self.variant_logprobs(variant[:-1], memory)
        tgt = np.asarray(variant[1:])
        keep = tgt != MASK
        return float(lp[np.arange(len(tgt))[keep], tgt[keep]].sum())


def ensemble(ref: PoetRef, prompts, variants, relative_to_wt=False):
    """scripts/score.py main(): (forward + backward) / 2 per member, the mean over the members; every array reversed whole for the
    backward pass.  Returns (scores, per-member (forward, backward))."""
    members = []
    for prompt in prompts:
        both = []
        for flip in (False, True):
            ps = [np.ascontiguousarray(s[::-1]) if flip else s for s in prompt]
            mem = ref.prompt(ps)[1] if ps else None
            both.append(np.array([ref.score(np.ascontiguousarray(v[::-1]) if flip else v, mem) for v in variants]))
        members.append(tuple(both))
    out = np.vstack([(f + b) / 2 for f, b in members]).mean(axis=0)
    return (out[:-1] - out[-1] if relative_to_wt else out), members
