"""CARP in float64 on plain torch ops (F.embedding, F.conv1d, F.layer_norm, F.gelu), one sequence at a time at batch 1 -- the
reference for tests/test_carp_host.py and tests/test_gpu_carp.py.  It restates the ByteNetLM of sequence_models as the issue and
DESIGN.md 4.6o read it (that library is not installed here, so the live reference produced no value in this file), reads the
checkpoint's own tensor layout ([out][in][tap] convolutions, the unfolded embedding) and shares no code with proteingym_amd/carp.py's
blob or device path."""
import numpy as np
import torch
import torch.nn.functional as F

ALPHABET = "ACDEFGHIKLMNPQRSTVWYBZXJOU*-#@"
MASK_ID = ALPHABET.index("#")
EPS = 1e-5


def _t(a, dtype):
    return torch.tensor(np.asarray(a), dtype=dtype)


def n_blocks(sd):
    n = 0
    while f"embedder.layers.{n}.conv.weight" in sd:
        n += 1
    return n


def dilations(n_layers, r=128):
    cycle = int(np.log2(r)) + 1
    return [2 ** (n % cycle) for n in range(n_layers)]


def block(sd, n, x, dilation, dtype):
    """x [1, D, L] -> x + PFF2(GELU(LN3(Conv(GELU(LN2(PFF1(GELU(LN1(x))))))))); LayerNorms over the channel axis."""
    p = f"embedder.layers.{n}."

    def w(key):
        return _t(sd[p + key], dtype)

    def ln(v, key):
        return F.layer_norm(v.transpose(1, 2), (v.shape[1],), w(key + ".weight"), w(key + ".bias"), EPS).transpose(1, 2)

    h = F.gelu(ln(x, "sequence1.0"))
    h = F.conv1d(h, w("sequence1.2.conv.weight"), w("sequence1.2.conv.bias"))
    h = F.gelu(ln(h, "sequence1.3"))
    k = sd[p + "conv.weight"].shape[2]
    h = F.conv1d(h, w("conv.weight"), w("conv.bias"), dilation=dilation, padding=dilation * (k - 1) // 2)
    h = F.gelu(ln(h, "sequence2.0"))
    h = F.conv1d(h, w("sequence2.2.conv.weight"), w("sequence2.2.conv.bias"))
    return x + h


def hidden(ck, tokens, dtype=torch.float64):
    """The rows in front of last_norm, [L, D]."""
    sd = ck["model_state_dict"]
    tok = torch.as_tensor(np.asarray(tokens), dtype=torch.long)[None]
    e = F.embedding(tok, _t(sd["embedder.embedder.weight"], dtype))                       # [1, L, 8]
    x = F.conv1d(e.transpose(1, 2), _t(sd["embedder.up_embedder.conv.weight"], dtype), _t(sd["embedder.up_embedder.conv.bias"], dtype))
    for n, d in enumerate(dilations(n_blocks(sd), int(ck.get("r", 128)))):
        x = block(sd, n, x, d, dtype)
    return x[0].transpose(0, 1)


def logprobs(ck, tokens, dtype=torch.float64):
    """[L, V] log-softmax over all V columns."""
    sd = ck["model_state_dict"]
    x = hidden(ck, tokens, dtype)
    x = F.layer_norm(x, (x.shape[1],), _t(sd["last_norm.weight"], dtype), _t(sd["last_norm.bias"], dtype), EPS)
    logits = F.conv1d(x.transpose(0, 1)[None], _t(sd["decoder.conv.weight"], dtype), _t(sd["decoder.conv.bias"], dtype))[0].transpose(0, 1)
    return torch.log_softmax(logits, dim=-1).numpy()


def masked_logprobs(ck, tokens, positions, dtype=torch.float64):
    """Row i: position positions[i] of the forward with that token masked."""
    tokens = np.asarray(tokens)
    out = []
    for p in positions:
        t = tokens.copy()
        t[p] = MASK_ID
        out.append(logprobs(ck, t, dtype)[p])
    return np.stack(out)


def sequence_loglik(ck, tokens, dtype=torch.float64):
    lp = logprobs(ck, tokens, dtype)
    return float(lp[np.arange(len(tokens)), np.asarray(tokens)].sum())


def tokenize(seq):
    return np.array([ALPHABET.index(a) for a in seq], dtype=np.int64)


def label_row(rows, sequence, lp_by_pos, offset_idx=1):
    """compute_fitness.py:18-30 on a {position: row} table."""
    rows = rows.split(":")
    score = 0.0
    for row in rows:
        wt, idx, mt = row[0], int(row[1:-1]) - offset_idx, row[-1]
        assert sequence[idx] == wt, "The listed wildtype does not match the provided sequence"
        score += float(lp_by_pos[idx][ALPHABET.index(mt)] - lp_by_pos[idx][ALPHABET.index(wt)])
    return score / len(rows)


def masked_marginal_scores(ck, target_seq, mutants, offset_idx=1, dtype=torch.float64):
    """compute_fitness.py:67-93 with every position run, as the reference does."""
    tok = tokenize(target_seq)
    lp = masked_logprobs(ck, tok, range(len(tok)), dtype)
    return np.array([label_row(m, target_seq, lp, offset_idx) for m in mutants])


def pseudo_likelihood_scores(ck, seqs, dtype=torch.float64):
    """compute_fitness.py:52-66: minus CrossEntropyLoss (mean reduction) of one unmasked forward."""
    return np.array([sequence_loglik(ck, tokenize(s), dtype) / len(s) for s in seqs])


def conv_segments(x, w, bias, seg_off, dilation, dtype=torch.float64):
    """F.conv1d per segment: x [M, C], w [C out][C in][taps] -> [M, C]."""
    x, w, bias = _t(x, dtype), _t(w, dtype), _t(bias, dtype)
    k = w.shape[2]
    out = []
    for a, b in zip(seg_off[:-1], seg_off[1:]):
        out.append(F.conv1d(x[a:b].transpose(0, 1)[None], w, bias, dilation=dilation, padding=dilation * (k - 1) // 2)[0].transpose(0, 1))
    return torch.cat(out).numpy()


def ln_gelu(x, w, b, dtype=torch.float64):
    x = _t(x, dtype)
    return F.gelu(F.layer_norm(x, (x.shape[1],), _t(w, dtype), _t(b, dtype), EPS)).numpy()


class RestatedModel:
    """carp.CarpModel's scoring interface on this file (the CLI's seam in tests/test_carp_host.py)."""

    def __init__(self, ck):
        self.ck = ck

    def masked_logprobs(self, wt_tokens, positions):
        return masked_logprobs(self.ck, wt_tokens, list(positions))

    def sequence_loglik(self, token_rows):
        return np.array([sequence_loglik(self.ck, t) for t in token_rows])

    def token_logprobs(self, token_rows):
        return [logprobs(self.ck, t) for t in token_rows]

    def close(self):
        pass
