"""float64 NumPy reading of ESM-IF1's decoder (esm/inverse_folding/transformer_decoder.py, transformer_layer.py TransformerDecoderLayer,
esm/multihead_attention.py) and of its cross-attention: the reference the GPU tests compare the HIP path against.  Checked against the
reference's own float64 goldens in tests/test_esmif1_host.py."""
import numpy as np


def _softmax(a):
    a = a - a.max(-1, keepdims=True)
    e = np.exp(a)
    return e / e.sum(-1, keepdims=True)


def cross_attention(q, mem_kv, heads):
    """q [R, 64 heads] (pre-scaled), mem_kv [S, 2 * 64 heads] (k | v): every row sees all S keys.  float64 [R, 64 heads]."""
    q, mem_kv = np.asarray(q, dtype=np.float64), np.asarray(mem_kv, dtype=np.float64)
    R, Da = q.shape
    dh = Da // heads
    S = mem_kv.shape[0]
    k, v = mem_kv[:, :Da].reshape(S, heads, dh), mem_kv[:, Da:].reshape(S, heads, dh)
    p = _softmax(np.einsum("rhd,shd->hrs", q.reshape(R, heads, dh), k))
    return np.einsum("hrs,shd->rhd", p, v).reshape(R, Da)


def _ln(x, w, b, eps=1e-5):
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * w + b


def _lin(sd, name, x):
    return x @ sd[name + ".weight"].T + sd[name + ".bias"]


def _attention(sd, p, x, kv, heads, causal, softmax=_softmax):
    T, D = x.shape
    dh = D // heads
    q = (_lin(sd, p + "q_proj", x) * dh ** -0.5).reshape(T, heads, dh)
    k = _lin(sd, p + "k_proj", kv).reshape(-1, heads, dh)
    v = _lin(sd, p + "v_proj", kv).reshape(-1, heads, dh)
    a = np.einsum("thd,shd->hts", q, k)
    if causal:
        a = np.where(np.triu(np.ones((T, T), dtype=bool), 1)[None], -np.inf, a)
    return _lin(sd, p + "out_proj", np.einsum("hts,shd->thd", softmax(a), v).reshape(T, D))


def decoder_logprobs(cfg, sd, enc_out, tokens, pos_table, cross_softmax=_softmax):
    """log_softmax of the decoder's logits for every token of `tokens` [T] given the memory enc_out [S, E]; float64 [T, V].
    pos_table [>= T, D]: row t = the sinusoidal embedding of position padding_idx + 1 + t (the reference builds it in float32).
    cross_softmax: the softmax of the cross-attention scores.  The reference's encoder_attn takes multihead_attention.py's own path
    (static_kv), whose softmax is float32 whatever the model's dtype (utils_softmax, :22 / :379), while its self-attentions go through
    F.multi_head_attention_forward in the model's dtype; a test that wants the reference's float64 numbers to 1e-10 hands that float32
    softmax in, the GPU tests keep float64 throughout."""
    sd = {k: np.asarray(v, dtype=np.float64) for k, v in sd.items() if k.startswith("decoder.")}
    enc_out = np.asarray(enc_out, dtype=np.float64)
    D, H = cfg["embed_dim"], cfg["heads"]
    T = len(tokens)
    x = np.sqrt(D) * sd["decoder.embed_tokens.weight"][np.asarray(tokens)] + np.asarray(pos_table, dtype=np.float64)[:T]
    for i in range(cfg["layers"]):
        p = f"decoder.layers.{i}."
        h = _ln(x, sd[p + "self_attn_layer_norm.weight"], sd[p + "self_attn_layer_norm.bias"])
        x = x + _attention(sd, p + "self_attn.", h, h, H, True)
        h = _ln(x, sd[p + "encoder_attn_layer_norm.weight"], sd[p + "encoder_attn_layer_norm.bias"])
        x = x + _attention(sd, p + "encoder_attn.", h, enc_out, H, False, cross_softmax)
        h = _ln(x, sd[p + "final_layer_norm.weight"], sd[p + "final_layer_norm.bias"])
        x = x + _lin(sd, p + "fc2", np.maximum(_lin(sd, p + "fc1", h), 0.0))
    x = _ln(x, sd["decoder.layer_norm.weight"], sd["decoder.layer_norm.bias"])
    logits = x @ sd["decoder.output_projection.weight"].T
    m = logits.max(-1, keepdims=True)
    return logits - m - np.log(np.exp(logits - m).sum(-1, keepdims=True))


def score(lp, tokens):
    """The reference's esmif1_ll: lp [T, V] of the first T = len(tokens) - 1 tokens, targets tokens[1:]."""
    t = np.asarray(tokens)
    return float(lp[np.arange(len(t) - 1), t[1:]].mean())
