"""Float64 reference of the scoring tail (proteingym_amd/csrc/elementwise.hip: vocab_logsoftmax_kernel, wide_logsoftmax_kernel,
group_logsoftmax_kernel, seq_loglik_kernel, seq_loglik_ragged_kernel), the inputs of tests/test_gpu_scoring_ops.py and the bounds it
asserts.  Plain NumPy; pinned against torch and plain Python loops in tests/test_scoring_ref.py, where every bound and input condition
is also rehearsed from the reference alone.

Semantics of non-finite logits: torch.log_softmax's.  A -inf logit has probability 0 and log-probability -inf, the other columns are
what they would be without it; a row of nothing but -inf is NaN, as is a row holding +inf or NaN."""
import math

import numpy as np

F32 = np.float32


def spacing32(x):
    """One fp32 unit in the last place at |x| (float64 array)."""
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(F32)).astype(np.float64)


# ---- the operations ----------------------------------------------------------------------------------------------------------------------
def log_softmax(logits):
    x = np.asarray(logits, np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        z = x - x.max(-1, keepdims=True)
        return z - np.log(np.exp(z).sum(-1, keepdims=True))


def head_logits(h, E, bias):
    return np.asarray(h, np.float64) @ np.asarray(E, np.float64).T + np.asarray(bias, np.float64)


def logsumexp(x, axis=-1):
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        m = x.max(axis, keepdims=True)
        m0 = np.where(np.isfinite(m), m, 0.0)
        return np.squeeze(m0 + np.log(np.exp(x - m0).sum(axis, keepdims=True)), axis)


def group_logprobs(logits, first, groups, width):
    """[rows][groups]: log of the summed probability of the columns first + g width .. + width."""
    x = np.asarray(logits, np.float64)
    sl = x[:, first:first + groups * width].reshape(x.shape[0], groups, width)
    with np.errstate(invalid="ignore"):
        return logsumexp(sl, -1) - logsumexp(x, -1)[:, None]


def fuse(lp, prior, alpha, eve, beta, eve_fallback):
    """(1 - alpha) lp + alpha prior, then (1 - beta) two + beta eve; an EVE value of -inf hands the position back to `two` under
    eve_fallback and goes through the arithmetic otherwise.  alpha and beta are the fp32 values the kernel receives."""
    a, b = float(F32(alpha)), float(F32(beta))
    two = (1.0 - a) * lp + a * prior
    if eve is None:
        return two
    if eve_fallback and eve == -math.inf:
        return two
    return (1.0 - b) * two + b * eve


def seq_loglik(lp, tokens, B, T, V, lens=None, seq_off=None, seq_p=None, seq_root=None, prior=None, a0=None, row0=None, n=None,
               flip=None, alpha=0.0, eve=None, beta=0.0, eve_fallback=0, terms=False):
    """out [B] float64.  lp [rows][V], tokens [rows].  Dense form (lens): sequence b owns the rows b T .. b T + T - 1 and sums the targets
    t = 0 .. lens[b] - 2: token t + 1 read from the log-probability row of token t.  Ragged form: sequence b owns the T - seq_p[b] packed
    rows from seq_off[b] on (its tokens seq_p[b] .. T - 1); token u < seq_p[b] is its root's token u; T - 1 targets.  A target t inside the
    window a0[b] <= t < a0[b] + n[b] is fused with prior (and EVE) row row0[b] + i, i = t - a0[b], or row0[b] + n[b] - 1 - i when flip[b].
    terms: also the sum of |lp| + |prior| + |eve| over the terms of each sequence (the realistic case's bound)."""
    lp = np.asarray(lp, np.float64).reshape(-1, V)
    prior = None if prior is None else np.asarray(prior, np.float64).reshape(-1, V)
    eve = None if eve is None else np.asarray(eve, np.float64).reshape(-1, V)
    out, mass = np.zeros(B, np.float64), np.zeros(B, np.float64)
    for b in range(B):
        if lens is not None:
            nt, row_of = int(lens[b]) - 1, (lambda u, b=b: b * T + u)
        else:
            p, own0, root0 = int(seq_p[b]), int(seq_off[b]) - int(seq_p[b]), int(seq_off[int(seq_root[b])])
            nt, row_of = T - 1, (lambda u, p=p, own0=own0, root0=root0: root0 + u if u < p else own0 + u)
        acc = 0.0
        for t in range(max(nt, 0)):
            tgt = int(tokens[row_of(t + 1)])
            v = lp[row_of(t), tgt]
            mass[b] += abs(v)
            if prior is not None and n[b] > 0 and a0[b] <= t < a0[b] + n[b]:
                i = t - int(a0[b])
                row = int(row0[b]) + (int(n[b]) - 1 - i if flip[b] else i)
                e = None if eve is None else eve[row, tgt]
                mass[b] += abs(prior[row, tgt]) + (abs(e) if e is not None and np.isfinite(e) else 0.0)
                with np.errstate(invalid="ignore"):
                    v = fuse(v, prior[row, tgt], alpha, e, beta, eve_fallback)
            acc += v
        out[b] = acc
    return (out, mass) if terms else out


# ---- narrow and grouped heads: inputs and bound ------------------------------------------------------------------------------------------
NARROW_CASES = [(1, 1, 1), (1, 64, 3), (2, 1, 4), (2, 63, 5), (2, 320, 9), (25, 1, 3), (25, 63, 4), (25, 64, 5), (25, 65, 9), (25, 320, 1),
                (25, 1280, 3), (25, 5120, 4), (33, 64, 9), (33, 65, 3), (33, 320, 5), (33, 1280, 4), (33, 5120, 1), (35, 63, 5),
                (35, 320, 4), (63, 1, 9), (63, 65, 4), (63, 1280, 5), (64, 64, 4), (64, 63, 3), (64, 320, 9), (64, 5120, 5)]   # (V, D, rows)
NARROW_SHIFT_CASE = (33, 320, 5)                                     # bias += 3e4 on every column

SAPROT = (446, 5, 21, 21)                                            # V, first, groups, width
GROUP_CASES = [SAPROT + (D, rows, mode) for D, rows, mode in
               ((4, 1, "both"), (256, 4, "full"), (260, 5, "group"), (480, 1, "group"), (512, 4, "both"), (516, 5, "full"),
                (1280, 1, "full"), (1284, 4, "group"), (2560, 5, "both"))] + \
              [(512, 8, 8, 63, 256, 5, "both"), (70, 3, 3, 1, 64, 4, "both")]


def head_inputs(V, D, rows, seed=0, shift=0.0):
    """h [rows][D], E [V][D], bias [V] (fp32).  h ~ N(0, 1) and E ~ N(0, 100 / D): the float64 logits of the drawn rows have a standard
    deviation of about 10.  With D >= 3 and rows >= 3 the last two features are reserved: E[v][D-1] = -bias[v], E[v][D-2] = 60 on one
    column v0, and the drawn rows are zero there; row rows-2 is the unit vector of feature D-1 (every logit is bias - bias = 0: all
    equal), row rows-1 the sum of the two unit vectors (column v0 ahead of the rest by exactly 60)."""
    rng = np.random.default_rng([seed, V, D, rows])
    h = rng.standard_normal((rows, D)).astype(F32)
    E = (rng.standard_normal((V, D)) * (10.0 / math.sqrt(D))).astype(F32)
    bias = (2.0 * rng.standard_normal(V) + shift).astype(F32)
    v0 = None
    if D >= 3 and rows >= 3:
        v0 = (7 * V) // 11
        h[:, D - 2:] = 0.0
        E[:, D - 1] = -bias
        E[:, D - 2] = 0.0
        E[v0, D - 2] = 60.0
        h[rows - 2] = 0.0
        h[rows - 2, D - 1] = 1.0
        h[rows - 1] = 0.0
        h[rows - 1, D - 2:] = 1.0
    return h, E, bias, v0


def head_bound(h, E, ref):
    """|out - ref| <= spacing32(|ref|) + 1e-12 max(1, max_v sum_i |h_i E_vi|): the kernels accumulate the logits and every log-sum-exp in
    double and round to fp32 once -- one fp32 ulp of the result plus the worst-case double dot-product error at D <= 5120
    (5120 2^-53 = 5.7e-13 relative to sum |h_i E_vi|).  Per row; -inf references carry no bound (they are compared exactly)."""
    s = (np.abs(np.asarray(h, np.float64)) @ np.abs(np.asarray(E, np.float64)).T).max(-1)
    fin = np.where(np.isfinite(ref), ref, 0.0)
    return spacing32(fin) + 1e-12 * np.maximum(1.0, s)[:, None]


# ---- wide head: inputs, bound, edge condition ---------------------------------------------------------------------------------------------
WIDE_V = [65, 255, 256, 257, 1021, 1023, 1024, 1025, 1030, 4099, 50257]
WIDE_KINDS = ["flat", "normal8", "ascending", "descending", "dominant", "offset"]


def wide_cases():
    """(V, ldl, rows, first kind): both paddings of every V; rows and the first row's kind cycle so that every kind meets every V."""
    out, i = [], 0
    for V in WIDE_V:
        for ldl in sorted({(V + 3) // 4 * 4, (V + 63) // 64 * 64}):
            if V < 50257:
                out.append((V, ldl, (1, 2, 5)[i % 3], i % len(WIDE_KINDS)))
            else:                                                    # three rows each: ascending, descending, dominant | offset, flat, normal8
                out.append((V, ldl, 3, 2 if ldl == (V + 3) // 4 * 4 else 5))
            i += 1
    return out


def wide_edge_columns(V):
    return [c for c in (0, 3, 4, V - 2, V - 1) + ((1023, 1024) if V > 1024 else ()) if 0 <= c < V]


def wide_row(V, kind, rng, edge_rank=0):
    """One row of fp32 logits.  The edge columns are raised to L - U[0, 1], L = max(largest other column, lse(other columns) - 4): within
    1 of the largest other column where that is mass enough, else (50 000 flat or evenly spread columns) above it, where each of them
    carries e^-5 of the row and stays within 1 of the row's maximum -- except in a flat row of V <= 1030, where every column qualifies as
    it is, and in the dominant row, whose dominant column is an edge column."""
    edges = wide_edge_columns(V)
    if kind == "flat":
        x = rng.uniform(-1.0, 1.0, V)
    elif kind == "normal8":
        x = 8.0 * rng.standard_normal(V)
    elif kind == "ascending":
        x = np.sort(rng.uniform(-12.0, 12.0, V))
    elif kind == "descending":
        x = np.sort(rng.uniform(-12.0, 12.0, V))[::-1].copy()
    elif kind == "dominant":
        x = rng.uniform(-1.0, 1.0, V)
        x[edges[edge_rank % len(edges)]] = 60.0
    elif kind == "offset":
        x = 1.0e4 + 8.0 * rng.standard_normal(V)
    else:
        raise ValueError(kind)
    if kind != "dominant" and not (kind == "flat" and V <= 1030):
        rest = np.delete(x, edges)
        x[edges] = max(rest.max(), logsumexp(rest) - 4.0) - rng.uniform(0.0, 1.0, len(edges))
    return x.astype(F32)


def wide_inputs(V, ldl, rows, kind0, seed=0, pad=0.0):
    """logits [rows][ldl] fp32 (row r of kind WIDE_KINDS[(kind0 + r) % 6], pad columns = pad), the kinds, tgt [rows]: columns 0, V-1, V-2 and
    an interior one in turn."""
    rng = np.random.default_rng([seed, V, rows, kind0])
    kinds = [WIDE_KINDS[(kind0 + r) % len(WIDE_KINDS)] for r in range(rows)]
    x = np.full((rows, ldl), pad, F32)
    for r, k in enumerate(kinds):
        x[r, :V] = wide_row(V, k, rng, edge_rank=kind0 + r)
    tgt = np.array([(0, V - 1, max(V - 2, 0), V // 2)[(kind0 + r) % 4] for r in range(rows)], np.int32)
    return x, kinds, tgt


def wide_bound(x, ref):
    """|out - ref| <= spacing32(|ref|) + 2^-23 sum_k p_k |x_k - max| + 2^-22 (ceil(V / 1024) + 3), x [rows][V] the logits without padding.
    The exponent rounding of __expf is <= 2^-24 |x| relative per factor and the factors of a column telescope to |x_k - max| over the
    rescales of a growing maximum; v_exp_f32 adds one ulp per factor with at most one rescale per chunk (ceil(V / 1024) chunks a thread),
    the four-term fp32 partial sum two more; the whole doubled."""
    x = np.asarray(x, np.float64)
    V = x.shape[-1]
    fin = np.isfinite(x)
    xm = np.where(fin, x, -np.inf).max(-1, keepdims=True)
    with np.errstate(invalid="ignore", over="ignore"):
        p = np.where(fin, np.exp(log_softmax(x)), 0.0)
        spread = (p * np.where(fin, np.abs(x - xm), 0.0)).sum(-1, keepdims=True)
    return spacing32(np.where(np.isfinite(ref), ref, 0.0)) + 2.0 ** -23 * spread + 2.0 ** -22 * (math.ceil(V / 1024) + 3)


def wide_edge_condition(x, kinds, ref, bound):
    """Per row: (smallest probability of a column that must qualify) / (100 x the row's largest bound); >= 1 when the condition holds.
    The columns that must qualify: the edge columns; every column in a flat row of V <= 1030; the dominant column in the dominant row."""
    V = x.shape[-1]
    out = []
    for r, k in enumerate(kinds):
        p = np.exp(ref[r])
        cols = [int(np.argmax(x[r]))] if k == "dominant" else (range(V) if (k == "flat" and V <= 1030) else wide_edge_columns(V))
        if k == "dominant":
            assert cols[0] in wide_edge_columns(V)
        out.append(min(p[c] for c in cols) / (100.0 * bound[r].max()))
    return out


# -inf patterns of the wide head, by name: (V, columns).  A thread takes the float4s i, i + 256, ...: thread 2 owns the columns 8..11 and
# 1032..1035; at V = 1023 the last, partial float4 (1020..1022) is the only chunk of thread 255.
WIDE_NEG_INF = [("single", 4099, [7]), ("aligned_group", 4099, [8, 9, 10, 11]),
                ("second_chunk_of_a_thread", 4099, [8, 9, 10, 11, 1032, 1033, 1034, 1035]),
                ("last_partial_group", 1023, [1020, 1021, 1022]), ("last_partial_group_after_chunks", 4099, [4096, 4097, 4098]),
                ("single_in_a_one_chunk_thread", 1023, [1021])]


# ---- sequence sums -----------------------------------------------------------------------------------------------------------------------
SEQ_V = 25
SEQ_T = [2, 64, 65, 66, 130, 1024]
SEQ_B = [1, 4, 5]
# (alpha, beta) of the exact cases: every value of {0, 0.25, 0.5, 1} on either side.  exact_bits() says which pairs a length allows.
EXACT_AB = [(0.25, 1.0), (0.5, 0.5), (1.0, 0.25), (0.0, 0.25), (0.25, 0.0), (0.5, 1.0), (1.0, 0.5), (0.25, 0.25), (0.5, 0.25), (0.25, 0.5)]


def frac_bits(v):
    """Fractional bits of a dyadic v in [0, 1]."""
    k = 0
    while v != int(v):
        v, k = v * 2, k + 1
    return k


def exact_bits(alpha, beta, T, with_eve):
    """Bits an fp32 partial sum may need when lp / prior / eve are multiples of 2^-8 in [-16, 0): a fused term is a multiple of
    2^-(8 + f), f the fractional bits of the weights in force, below 16 in magnitude; any partial sum of at most T - 1 terms is a multiple
    of the same unit below 16 (T - 1).  At most 24 bits: every product, fused term and partial sum is exact in fp32 in any order (the
    products of a 12-bit value and a 2-bit weight and their two-term sums need 8 + f + 4 <= 24 bits as well)."""
    f = max(frac_bits(alpha), frac_bits(1 - alpha)) + (max(frac_bits(beta), frac_bits(1 - beta)) if with_eve else 0)
    return 8 + f + math.ceil(math.log2(16 * max(T - 1, 1)))


def quantized(rng, shape):
    """Multiples of 2^-8 in [-16, 0)."""
    return (-rng.integers(1, 4097, shape) / 256.0).astype(F32)


def seq_lens(B, T, k):
    pool = [0, 1, 2, T - 1, T]
    return np.array([min(max(pool[(k + b) % 5], 0), T) for b in range(B)], np.int32)


def seq_windows(rng, B, T, lens, k, spare=1):
    """Prior windows: n from {0, 1, 64, 65} and a0 from {0, 1, 63, 64, len - 1 - n} in turn, cut to what the T - 1 targets allow (the
    entry's rule is a0 + n <= T - 1); flip alternates; row0 walks through one shared table, which ends in `spare` rows no window uses."""
    a0, row0, n, flip = (np.zeros(B, np.int32) for _ in range(4))
    rows = 0
    for b in range(B):
        nb = min((0, 1, 64, 65)[(k + b) % 4], T - 1)
        cand = (0, 1, 63, 64, int(lens[b]) - 1 - nb)[(k + 2 * b) % 5]
        a0[b] = min(max(cand, 0), T - 1 - nb)
        n[b], flip[b], row0[b] = nb, (k + b) & 1, rows
        rows += nb
    return a0, row0, n, flip, rows + spare


def seq_dense_case(B, T, k, exact=True, with_prior=True, with_eve=False, eve_holes=False):
    """A dense case: dict of the op's arguments (arrays fp32 / int32)."""
    rng = np.random.default_rng([5, B, T, k])
    V = SEQ_V
    draw = (lambda s: quantized(rng, s)) if exact else (lambda s: (-rng.gamma(2.0, 1.5, s)).astype(F32))
    c = dict(B=B, T=T, V=V, lp=draw((B * T, V)), tokens=rng.integers(0, V, B * T).astype(np.int32), lens=seq_lens(B, T, k))
    if with_prior:
        c["a0"], c["row0"], c["n"], c["flip"], npr = seq_windows(rng, B, T, c["lens"], k)
        c["prior"] = draw((npr, V))
        if with_eve:
            c["eve"] = draw((npr, V))
            if eve_holes:
                c["eve"][:, rng.permutation(V)[:6]] = -np.inf                  # columns EVE does not model
    return c


def seq_ragged_case(T, k, exact=True, with_prior=True, with_eve=False):
    """A root and children sharing prefixes of seq_p in {0, 1, 31, 64, T - 1} (cut to T - 1) with it: the dense layout (every sequence all
    its T rows; a child's rows and tokens before seq_p are the root's) and the packed layout of the same values."""
    rng = np.random.default_rng([9, T, k])
    V = SEQ_V
    ps = [0] + [min(p, T - 1) for p in (0, 1, 31, 64, T - 1)]
    B = len(ps)
    draw = (lambda s: quantized(rng, s)) if exact else (lambda s: (-rng.gamma(2.0, 1.5, s)).astype(F32))
    lp = draw((B, T, V))
    tok = rng.integers(0, V, (B, T)).astype(np.int32)
    for b, p in enumerate(ps):
        lp[b, :p], tok[b, :p] = lp[0, :p], tok[0, :p]
    lens = np.full(B, T, np.int32)
    dense = dict(B=B, T=T, V=V, lp=lp.reshape(B * T, V).copy(), tokens=tok.reshape(-1).copy(), lens=lens)
    off = np.cumsum([0] + [T - p for p in ps]).astype(np.int32)
    ragged = dict(B=B, T=T, V=V, lp=np.concatenate([lp[b, p:] for b, p in enumerate(ps)]), tokens=np.concatenate([tok[b, p:] for b, p in enumerate(ps)]),
                  seq_off=off[:-1].copy(), seq_p=np.array(ps, np.int32), seq_root=np.zeros(B, np.int32))
    if with_prior:
        a0, row0, n, flip, npr = seq_windows(rng, B, T, lens, k)
        extra = dict(a0=a0, row0=row0, n=n, flip=flip, prior=draw((npr, V)))
        if with_eve:
            extra["eve"] = draw((npr, V))
        dense.update(extra)
        ragged.update(extra)
    return dense, ragged


def seq_reference(c, alpha=0.0, beta=0.0, eve_fallback=0, terms=False):
    keys = ("lens", "seq_off", "seq_p", "seq_root", "prior", "a0", "row0", "n", "flip", "eve")
    return seq_loglik(c["lp"], c["tokens"], c["B"], c["T"], c["V"], alpha=alpha, beta=beta, eve_fallback=eve_fallback, terms=terms,
                      **{k: c.get(k) for k in keys})


def seq_realistic_bound(lens, mass):
    """2^-23 (ceil(len / 64) + 12) sum_t (|lp_t| + |prior_t| + |eve_t|): the fp32 lane partials (ceil(len / 64) additions a lane), the
    six-step wave tree and the fusion arithmetic (two products and an addition per prior, fp32 weights)."""
    return 2.0 ** -23 * (np.ceil(np.asarray(lens, np.float64) / 64) + 12) * mass
