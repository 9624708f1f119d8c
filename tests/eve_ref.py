"""float64 restatement of one Monte-Carlo sample of EVE's ELBO (proteingym/baselines/EVE: VAE_model.all_likelihood_components,
VAE_encoder.forward, VAE_decoder.VAE_Bayesian_MLP_decoder.forward, as compute_evol_indices_DMS.py runs them: dropout active).

The noise is an explicit dict, named in the order the reference draws it:
    z_eps [M, z]; keep0 [M, z]; then per hidden layer i: w_eps{i} [D_i, in_i], b_eps{i} [D_i], keep{i+1} [M, D_i];
    wout_eps [C L, H]; bout_eps [20 L]; conv_eps [20, C, 1]; sparsity_eps [H / tiles, L]; temp_eps [1]
(keep tensors: 1 = kept, only with dropout_p > 0; conv / sparsity / temp only when configured).  ``state`` maps the names of
VAE_model.state_dict() to arrays; ``dims`` is proteingym_amd.eve.dims_from_params' dict.
"""
import numpy as np

ACT = {
    "relu": lambda x: np.maximum(x, 0.0),
    "tanh": np.tanh,
    "sigmoid": lambda x: 1.0 / (1.0 + np.exp(-x)),
    "elu": lambda x: np.where(x > 0, x, np.expm1(np.minimum(x, 0.0))),
    "linear": lambda x: x,
}


def one_hot(residues, alphabet=20):
    """[M, L] uint8 (>= alphabet: no letter) -> float64 [M, L, alphabet]."""
    r = np.asarray(residues)
    x = np.zeros(r.shape + (alphabet,), dtype=np.float64)
    m, l = np.nonzero(r < alphabet)
    x[m, l, r[m, l]] = 1.0
    return x


def encode(state, dims, residues):
    S = lambda k: np.asarray(state[k], dtype=np.float64)
    h = one_hot(residues).reshape(len(residues), -1)
    for i in range(len(dims["enc_sizes"])):
        h = ACT[dims["enc_act"]](h @ S(f"encoder.hidden_layers.{i}.weight").T + S(f"encoder.hidden_layers.{i}.bias"))
    mu = h @ S("encoder.fc_mean.weight").T + S("encoder.fc_mean.bias")
    log_var = h @ S("encoder.fc_log_var.weight").T + S("encoder.fc_log_var.bias")
    return mu, log_var


def elbo(state, dims, residues, noise):
    """(elbo, bce, kld) float64 [M].  Every tensor of ``noise`` that the configuration draws must be present; the set of names read is
    returned by ``consumed(dims)``."""
    S = lambda k: np.asarray(state[k], dtype=np.float64)
    Z = lambda k: np.asarray(noise[k], dtype=np.float64)
    L, H, p = dims["seq_len"], dims["dec_sizes"][-1], dims["dropout_p"]
    C = dims["conv_depth"] or 20
    M = len(residues)

    def draw(mean_key, lv_key, eps_key):
        return np.exp(0.5 * S(lv_key)) * Z(eps_key).reshape(S(mean_key).shape) + S(mean_key)

    def dropout(x, key):
        return x * Z(key) / (1.0 - p) if p > 0 else x

    mu, log_var = encode(state, dims, residues)
    h = dropout(np.exp(0.5 * log_var) * Z("z_eps") + mu, "keep0")
    n = len(dims["dec_sizes"])
    for i in range(n):
        W = draw(f"decoder.hidden_layers_mean.{i}.weight", f"decoder.hidden_layers_log_var.{i}.weight", f"w_eps{i}")
        b = draw(f"decoder.hidden_layers_mean.{i}.bias", f"decoder.hidden_layers_log_var.{i}.bias", f"b_eps{i}")
        act = dims["dec_last_act"] if i == n - 1 else dims["dec_first_act"]
        h = dropout(ACT[act](h @ W.T + b), f"keep{i + 1}")
    W_out = draw("decoder.last_hidden_layer_weight_mean", "decoder.last_hidden_layer_weight_log_var", "wout_eps")
    b_out = draw("decoder.last_hidden_layer_bias_mean", "decoder.last_hidden_layer_bias_log_var", "bout_eps")
    # every reshape below reinterprets row-major memory, as the reference's .view does
    if dims["conv_depth"]:
        conv = draw("decoder.output_convolution_mean.weight", "decoder.output_convolution_log_var.weight", "conv_eps")
        W_out = W_out.reshape(L * H, C) @ conv.reshape(C, 20)
    if dims["sparsity_tiles"]:
        s = draw("decoder.sparsity_weight_mean", "decoder.sparsity_weight_log_var", "sparsity_eps")
        gate = ACT["sigmoid"](np.tile(s, (dims["sparsity_tiles"], 1)))[:, :, None]
        W_out = W_out.reshape(H, L, 20) * gate
    W_final = W_out.reshape(L * 20, H)
    logits = h @ W_final.T + b_out
    if dims["temperature"]:
        t = draw("decoder.temperature_scaler_mean", "decoder.temperature_scaler_log_var", "temp_eps")
        logits = np.log(1.0 + np.exp(t)) * logits
    x = logits.reshape(M, L, 20)
    mx = x.max(-1, keepdims=True)
    lp = x - (mx + np.log(np.exp(x - mx).sum(-1, keepdims=True)))
    # binary_cross_entropy_with_logits(lp, onehot) with lp <= 0: log1p(exp(lp)) - lp * onehot
    bce = (np.log1p(np.exp(lp)) - lp * one_hot(residues)).sum((1, 2))
    kld = -0.5 * (1.0 + log_var - mu ** 2 - np.exp(log_var)).sum(1)
    return -(bce + kld), bce, kld


def consumed(dims):
    """Names of the noise tensors one sample reads, in drawing order."""
    drop = dims["dropout_p"] > 0
    out = ["z_eps"] + (["keep0"] if drop else [])
    for i in range(len(dims["dec_sizes"])):
        out += [f"w_eps{i}", f"b_eps{i}"] + ([f"keep{i + 1}"] if drop else [])
    out += ["wout_eps", "bout_eps"]
    if dims["conv_depth"]:
        out.append("conv_eps")
    if dims["sparsity_tiles"]:
        out.append("sparsity_eps")
    if dims["temperature"]:
        out.append("temp_eps")
    return out


def numpy_noise(dims, M, rng):
    """Seeded noise of the right shapes (standard normals, Bernoulli(1 - p) keeps) for the injected-noise tests."""
    L, z, H = dims["seq_len"], dims["z_dim"], dims["dec_sizes"][-1]
    C, p = dims["conv_depth"] or 20, dims["dropout_p"]
    shapes = {"z_eps": (M, z), "keep0": (M, z), "wout_eps": (C * L, H), "bout_eps": (20 * L,), "conv_eps": (20, C, 1),
              "sparsity_eps": (H // max(dims["sparsity_tiles"], 1), L), "temp_eps": (1,)}
    fan = z
    for i, h in enumerate(dims["dec_sizes"]):
        shapes.update({f"w_eps{i}": (h, fan), f"b_eps{i}": (h,), f"keep{i + 1}": (M, h)})
        fan = h
    out = {}
    for k in consumed(dims):
        out[k] = (rng.random(shapes[k]) < 1.0 - p).astype(np.uint8) if k.startswith("keep") else rng.standard_normal(shapes[k]).astype(np.float32)
    return out
