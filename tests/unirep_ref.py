"""Float64 restatement of the reference's UniRep scorer, line by line, in numpy.

TensorFlow is not available where this suite runs, so the live reference did NOT produce any golden value here: parity is pinned by
this file, which follows proteingym/baselines/unirep/unirep.py (mLSTMCell1900, babbler1900), unirep_inference.py and
utils/data_utils.py / utils/io_utils.py with the line numbers cited at every step.  It takes the RAW checkpoint arrays (the .npy
directory's contents), not the folded blob, so the host's folding is under test as well.

``dtype=np.float32`` runs the same arithmetic in fp32 on the CPU: the distance of that run from the float64 one is the ``noise32`` of
the suite's bound (tests/axial_ref.py bound)."""
from __future__ import annotations

import os

import numpy as np

# utils/data_utils.py:16-45
AA_TO_INT = {'M': 1, 'R': 2, 'H': 3, 'K': 4, 'D': 5, 'E': 6, 'S': 7, 'T': 8, 'N': 9, 'Q': 10, 'C': 11, 'U': 12, 'G': 13, 'P': 14, 'A': 15,
             'V': 16, 'I': 17, 'F': 18, 'Y': 19, 'W': 20, 'L': 21, 'O': 22, 'X': 23, 'Z': 23, 'B': 23, 'J': 23, 'start': 24, 'stop': 25,
             '-': 26}
VALID_AAS = "MRHKDESTNQCUGPAVIFYWLO"          # utils/data_utils.py:115

CELL_FILES = ["rnn_mlstm_mlstm_wx:0.npy", "rnn_mlstm_mlstm_wh:0.npy", "rnn_mlstm_mlstm_wmx:0.npy", "rnn_mlstm_mlstm_wmh:0.npy",
              "rnn_mlstm_mlstm_b:0.npy", "rnn_mlstm_mlstm_gx:0.npy", "rnn_mlstm_mlstm_gh:0.npy", "rnn_mlstm_mlstm_gmx:0.npy",
              "rnn_mlstm_mlstm_gmh:0.npy"]     # unirep.py:89-97


def toy_checkpoint(seed, H, gain=1.0, vocab=26, embed=10):
    """Seeded arrays in the reference's naming and shapes (unirep.py:89-97, :359, :386-395).  ``gain`` scales the four weight-norm
    gains: it sets how strongly the recurrence amplifies rounding (tests derive it from the CPU fp32-vs-fp64 measurement)."""
    rng = np.random.default_rng(seed)
    f = np.float32
    return {
        "embed_matrix:0.npy": rng.normal(0, 1.0, (vocab, embed)).astype(f),
        "rnn_mlstm_mlstm_wx:0.npy": rng.normal(0, 1.0, (embed, 4 * H)).astype(f),
        "rnn_mlstm_mlstm_wh:0.npy": rng.normal(0, 1.0, (H, 4 * H)).astype(f),
        "rnn_mlstm_mlstm_wmx:0.npy": rng.normal(0, 1.0, (embed, H)).astype(f),
        "rnn_mlstm_mlstm_wmh:0.npy": rng.normal(0, 1.0, (H, H)).astype(f),
        "rnn_mlstm_mlstm_b:0.npy": rng.normal(0, 0.3, (4 * H,)).astype(f),
        "rnn_mlstm_mlstm_gx:0.npy": (gain * (1.0 + 0.2 * rng.normal(0, 1.0, (4 * H,)))).astype(f),
        "rnn_mlstm_mlstm_gh:0.npy": (gain * (1.0 + 0.2 * rng.normal(0, 1.0, (4 * H,)))).astype(f),
        "rnn_mlstm_mlstm_gmx:0.npy": (gain * (1.0 + 0.2 * rng.normal(0, 1.0, (H,)))).astype(f),
        "rnn_mlstm_mlstm_gmh:0.npy": (gain * (1.0 + 0.2 * rng.normal(0, 1.0, (H,)))).astype(f),
        "dense_kernel:0.npy": rng.normal(0, 2.0 / np.sqrt(H), (H, vocab - 1)).astype(f),
        "dense_bias:0.npy": rng.normal(0, 0.3, (vocab - 1,)).astype(f),
    }


def save_checkpoint(path, arrays):
    os.makedirs(path, exist_ok=True)
    for name, v in arrays.items():
        np.save(os.path.join(path, name), v)


def load_arrays(path):
    """np.load of every file the reference reads (unirep.py:89-97, :359, :386-395)."""
    names = CELL_FILES + ["embed_matrix:0.npy"]
    if os.path.exists(os.path.join(path, "fully_connected_weights:0.npy")):            # unirep.py:386-391
        names += ["fully_connected_weights:0.npy", "fully_connected_biases:0.npy"]
    else:
        names += ["dense_kernel:0.npy", "dense_bias:0.npy"]
    return {n: np.load(os.path.join(path, n)) for n in names}


def dense_of(arrays):
    if "fully_connected_weights:0.npy" in arrays:
        return arrays["fully_connected_weights:0.npy"], arrays["fully_connected_biases:0.npy"]
    return arrays["dense_kernel:0.npy"], arrays["dense_bias:0.npy"]


def l2_normalize(w, dtype):
    """tf.nn.l2_normalize(w, axis=0): w * rsqrt(max(sum(w^2, axis=0), epsilon = 1e-12))."""
    w = w.astype(dtype)
    return w * (dtype(1.0) / np.sqrt(np.maximum((w * w).sum(0, keepdims=True), dtype(1e-12))))


def effective_weights(arrays, dtype=np.float64):
    """unirep.py:118-122 (wn = True)."""
    g = lambda n: arrays[f"rnn_mlstm_mlstm_{n}:0.npy"]
    wx = l2_normalize(g("wx"), dtype) * g("gx").astype(dtype)
    wh = l2_normalize(g("wh"), dtype) * g("gh").astype(dtype)
    wmx = l2_normalize(g("wmx"), dtype) * g("gmx").astype(dtype)
    wmh = l2_normalize(g("wmh"), dtype) * g("gmh").astype(dtype)
    return wx, wh, wmx, wmh, g("b").astype(dtype)


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def cell_step(weights, inputs, c_prev, h_prev):
    """mLSTMCell1900.call, unirep.py:123-132.  Returns (h, c, z)."""
    wx, wh, wmx, wmh, b = weights
    m = (inputs @ wmx) * (h_prev @ wmh)                                    # :123
    z = inputs @ wx + m @ wh + b                                           # :124
    i, f, o, u = np.split(z, 4, axis=1)                                    # :125
    i, f, o, u = sigmoid(i), sigmoid(f), sigmoid(o), np.tanh(u)            # :126-129
    c = f * c_prev + i * u                                                 # :130
    h = o * np.tanh(c)                                                     # :131
    return h, c, z


def format_seq(seq):
    """data_utils.format_seq(stop=False), :82-94: [24] + residues."""
    return [24] + [AA_TO_INT[a] for a in seq.strip()]


def is_valid_seq(seq, max_len=4000):
    """utils/data_utils.py:110-119 (the one io_utils.load_and_filter_seqs calls)."""
    return len(seq) <= max_len and set(seq) <= set(VALID_AAS)


def load_and_filter_seqs(values):
    """io_utils.load_and_filter_seqs, :157-180, from the column's values."""
    out = []
    for seq in np.unique(np.asarray(values)):
        seq = seq.strip('*')
        if is_valid_seq(seq):
            out.append(seq)
    return out


def token_logprobs(arrays, x_tokens, dtype=np.float64):
    """babbler1900's graph on one input row: embedding lookup (unirep.py:361), dynamic_rnn from the zero state (:362-368, :76-79),
    Dense(25) (:396-402); returns log_softmax(logits) [T, 25]."""
    weights = effective_weights(arrays, dtype)
    E = arrays["embed_matrix:0.npy"].astype(dtype)
    Wd, bd = (a.astype(dtype) for a in dense_of(arrays))
    H = weights[3].shape[0]
    c = np.zeros((1, H), dtype)
    h = np.zeros((1, H), dtype)
    out = []
    for t in x_tokens:
        h, c, _ = cell_step(weights, E[[t]], c, h)
        logits = h @ Wd + bd
        mx = logits.max(-1, keepdims=True)
        out.append((logits - (mx + np.log(np.exp(logits - mx).sum(-1, keepdims=True))))[0])
    return np.stack(out)


def sequence_loss(lp, y_tokens, dtype=np.float64):
    """tfa.seq2seq.sequence_loss(average_across_batch=False) as unirep.py:350-355, :403-408 feeds it: sparse softmax cross-entropy
    against target - 1 (+ inverse_mask), mask = sign(target), sum(xent * mask) / (sum(mask) + 1e-12)."""
    y = np.asarray(y_tokens)
    mask = np.sign(y).astype(dtype)                                        # :350
    adj = (y - 1) + (1 - np.sign(y))                                       # :355
    xent = -lp[np.arange(len(y)), adj].astype(dtype)
    return float((xent * mask).sum() / (mask.sum() + dtype(1e-12)))


def score(arrays, seq, dtype=np.float64):
    """Unirep_score of one sequence: unirep_inference.py:44-57 (x = batch[:, :-1], y = batch[:, 1:]) for a batch of one."""
    toks = format_seq(seq.replace('-', 'X'))                               # unirep_inference.py:44-45
    lp = token_logprobs(arrays, toks[:-1], dtype)
    return sequence_loss(lp, toks[1:], dtype)


def scores(arrays, seqs, dtype=np.float64):
    return np.array([score(arrays, s, dtype) for s in seqs])
