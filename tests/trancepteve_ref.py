"""float64 restatement of TranceptEVE's two device pieces (proteingym/baselines/trancepteve/trancepteve/model_pytorch.py):

``log_prior``   get_EVE_log_prior_single (:975-1001) with the decoder of trancepteve/EVE/VAE_decoder.py in eval(): per sample, a fresh
                latent and fresh decoder weights, log_softmax over the 20 letters of each position; mean and n - 1 standard deviation
                over the samples.  The noise is eve_ref's dict (tests/eve_ref.py), one per sample, for M = 1, without the keep masks.
``fuse`` / ``sequence_loglik``   the three-way fusion of :1113-1133 inside the sequence log-likelihood of
                tranception/utils/scoring_utils.py:97-128, on a table of network log-probabilities.
"""
import numpy as np

import eve_ref


def sample_logp(state, dims, mu, log_var, noise):
    """float64 [L, 20]: log_softmax(decoder(z)) of one row for one sample's noise; no dropout."""
    S = lambda k: np.asarray(state[k], dtype=np.float64)
    Z = lambda k: np.asarray(noise[k], dtype=np.float64)
    L, H = dims["seq_len"], dims["dec_sizes"][-1]
    C = dims["conv_depth"] or 20

    def draw(mean_key, lv_key, eps_key):
        return np.exp(0.5 * S(lv_key)) * Z(eps_key).reshape(S(mean_key).shape) + S(mean_key)

    h = np.exp(0.5 * log_var) * Z("z_eps").reshape(log_var.shape) + mu
    n = len(dims["dec_sizes"])
    for i in range(n):
        W = draw(f"decoder.hidden_layers_mean.{i}.weight", f"decoder.hidden_layers_log_var.{i}.weight", f"w_eps{i}")
        b = draw(f"decoder.hidden_layers_mean.{i}.bias", f"decoder.hidden_layers_log_var.{i}.bias", f"b_eps{i}")
        h = eve_ref.ACT[dims["dec_last_act"] if i == n - 1 else dims["dec_first_act"]](h @ W.T + b)
    W_out = draw("decoder.last_hidden_layer_weight_mean", "decoder.last_hidden_layer_weight_log_var", "wout_eps")
    b_out = draw("decoder.last_hidden_layer_bias_mean", "decoder.last_hidden_layer_bias_log_var", "bout_eps")
    # every reshape reinterprets row-major memory, as the reference's .view does
    if dims["conv_depth"]:
        conv = draw("decoder.output_convolution_mean.weight", "decoder.output_convolution_log_var.weight", "conv_eps")
        W_out = W_out.reshape(L * H, C) @ conv.reshape(C, 20)
    if dims["sparsity_tiles"]:
        s = draw("decoder.sparsity_weight_mean", "decoder.sparsity_weight_log_var", "sparsity_eps")
        W_out = W_out.reshape(H, L, 20) * eve_ref.ACT["sigmoid"](np.tile(s, (dims["sparsity_tiles"], 1)))[:, :, None]
    logits = h @ W_out.reshape(L * 20, H).T + b_out
    if dims["temperature"]:
        t = draw("decoder.temperature_scaler_mean", "decoder.temperature_scaler_log_var", "temp_eps")
        logits = np.log(1.0 + np.exp(t)) * logits
    x = logits.reshape(L, 20)
    mx = x.max(-1, keepdims=True)
    return x - (mx + np.log(np.exp(x - mx).sum(-1, keepdims=True)))


def log_prior(state, dims, residues, noises):
    """(mean, std, per-sample stack) float64: [L, 20], [L, 20], [n, L, 20]; ``residues`` uint8 [L], ``noises`` one dict per sample."""
    mu, log_var = eve_ref.encode(state, dims, np.asarray(residues).reshape(1, -1))
    lp = np.stack([sample_logp(state, dims, mu, log_var, nz) for nz in noises])
    return lp.mean(0), (lp.std(0, ddof=1) if len(lp) > 1 else np.zeros_like(lp[0])), lp


def noise_names(dims):
    """The tensors one log-prior sample reads: eve_ref.consumed without the dropout masks."""
    return [k for k in eve_ref.consumed(dict(dims, dropout_p=0.0))]


def numpy_noise(dims, rng):
    return eve_ref.numpy_noise(dict(dims, dropout_p=0.0), 1, rng)


def fuse(lp, m, e, alpha, beta, eve_fallback):
    """The fused log-probability of one position at the target token: (1 - beta) ((1 - alpha) lp + alpha m) + beta e, or the two-way
    value where e is -inf and eve_fallback is set; with eve_fallback unset the -inf goes through."""
    two = (1.0 - alpha) * lp + alpha * m
    if np.isneginf(e):
        return two if eve_fallback else -np.inf
    return (1.0 - beta) * two + beta * e


def sequence_loglik(logp, tokens, length, msa_prior, eve_prior, a0, row0, n, flip, alpha, beta, eve_fallback):
    """sum over t < length - 1 of the (fused) log-probability of tokens[t + 1] at logit row t.  logp float64 [T, V]; logit rows
    [a0, a0 + n) are fused with prior row row0 + i (row0 + n - 1 - i when flip); eve_prior None: the one-prior fusion."""
    total = 0.0
    for t in range(length - 1):
        tok = int(tokens[t + 1])
        v = float(logp[t, tok])
        i = t - a0
        if msa_prior is not None and 0 <= i < n:
            row = row0 + (n - 1 - i if flip else i)
            m = float(msa_prior[row, tok])
            if eve_prior is None:
                v = (1.0 - alpha) * v + alpha * m
            else:
                v = fuse(v, m, float(eve_prior[row, tok]), alpha, beta, eve_fallback)
        total += v
    return total
