"""scoring_ref.py pinned on the CPU: against torch.log_softmax / torch.logsumexp and plain Python loops in float64, and every bound and
input condition of tests/test_gpu_scoring_ops.py rehearsed from the reference alone, so that they are known before a GPU runs."""
import math

import numpy as np
import pytest
import torch

import scoring_ref as sr


def _t(a):
    return torch.from_numpy(np.asarray(a, np.float64))


def test_log_softmax_and_groups_match_torch_in_float64():
    rng = np.random.default_rng(0)
    x = 10.0 * rng.standard_normal((7, 446))
    x[1, 5] = -np.inf
    x[2, 26:47] = -np.inf                                            # one whole group
    x[3] = -np.inf
    x[4, 9] = np.inf
    x[5, 11] = np.nan
    want = torch.log_softmax(_t(x), -1).numpy()
    got = sr.log_softmax(x)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.array_equal(np.isneginf(got), np.isneginf(want))
    fin = ok & np.isfinite(want)
    assert np.abs(got[fin] - want[fin]).max() < 1e-13
    assert np.isnan(got[3]).all() and np.isnan(got[4]).all() and np.isnan(got[5]).all()
    V, first, groups, width = sr.SAPROT
    g = sr.group_logprobs(x[:3], first, groups, width)
    for r in range(3):
        for k in range(groups):
            w = (torch.logsumexp(_t(x[r, first + k * width:first + (k + 1) * width]), 0) - torch.logsumexp(_t(x[r]), 0)).item()
            assert (g[r, k] == w) or abs(g[r, k] - w) < 1e-13 or (math.isnan(w) and math.isnan(g[r, k])), (r, k, g[r, k], w)
    assert g[2, 1] == -np.inf
    h, E, b, _ = sr.head_inputs(33, 65, 4)
    assert np.abs(sr.head_logits(h, E, b) - (_t(h) @ _t(E).T + _t(b)).numpy()).max() < 1e-12


def _loop_dense(c, alpha, beta, fb):
    out = []
    for b in range(c["B"]):
        s = 0.0
        for t in range(int(c["lens"][b]) - 1):
            tgt = int(c["tokens"][b * c["T"] + t + 1])
            v = float(c["lp"][b * c["T"] + t, tgt])
            if "prior" in c and c["n"][b] > 0 and c["a0"][b] <= t < c["a0"][b] + c["n"][b]:
                i = t - c["a0"][b]
                row = c["row0"][b] + (c["n"][b] - 1 - i if c["flip"][b] else i)
                v = (1 - alpha) * v + alpha * float(c["prior"][row, tgt])
                if "eve" in c:
                    e = float(c["eve"][row, tgt])
                    if not (fb and e == -math.inf):
                        v = (1 - beta) * v + beta * e
            s += v
        out.append(s)
    return np.array(out)


def test_sequence_sums_match_a_plain_loop_and_the_ragged_form_matches_the_dense_one():
    for B, T, k in ((4, 66, 0), (5, 130, 3), (1, 2, 1), (5, 65, 2)):
        c = sr.seq_dense_case(B, T, k, with_eve=True, eve_holes=True)
        for fb in (0, 1):
            got = sr.seq_reference(c, 0.5, 0.5, fb)
            want = _loop_dense(c, 0.5, 0.5, fb)
            assert np.array_equal(got, want), (B, T, k, fb, got, want)
    for T in (66, 130):
        dense, ragged = sr.seq_ragged_case(T, 1, with_eve=True)
        assert np.array_equal(sr.seq_reference(dense, 0.25, 1.0), sr.seq_reference(ragged, 0.25, 1.0))
        assert np.array_equal(sr.seq_reference(dense, 0.25, 1.0), _loop_dense(dense, 0.25, 1.0, 0))
        # the packed layout really is shorter, and a child's own rows start at its first own token
        assert len(ragged["tokens"]) == sum(T - p for p in ragged["seq_p"]) < len(dense["tokens"])


@pytest.mark.parametrize("V,D,rows", sr.NARROW_CASES + [sr.NARROW_SHIFT_CASE])
def test_narrow_inputs_meet_their_conditions(V, D, rows):
    shift = 3e4 if (V, D, rows) == sr.NARROW_SHIFT_CASE else 0.0
    h, E, bias, v0 = sr.head_inputs(V, D, rows, shift=shift)
    x = sr.head_logits(h, E, bias)
    ref = sr.log_softmax(x)
    bound = sr.head_bound(h, E, ref)
    assert np.isfinite(ref).all() and (bound > 0).all() and bound.max() < 1e-5
    assert np.abs(np.exp(ref).sum(-1) - 1).max() < 1e-12
    drawn = x[:rows - 2] if v0 is not None else x
    if drawn.size >= 50:
        sd = (drawn - (shift and bias.astype(np.float64))).std()
        assert 6.0 < sd < 15.0, sd
    if v0 is not None:
        assert np.all(x[rows - 2] == x[rows - 2, 0])                                      # all logits equal
        assert np.abs(ref[rows - 2] + math.log(V)).max() < 1e-12
        if V > 1:
            assert x[rows - 1, v0] - np.delete(x[rows - 1], v0).max() == 60.0               # one column ahead by 60
    # fp32 round-off of the reference itself stays inside the bound (the kernel's one rounding)
    assert np.all(np.abs(ref.astype(np.float32).astype(np.float64) - ref) <= bound)


@pytest.mark.parametrize("V,first,groups,width,D,rows,mode", sr.GROUP_CASES)
def test_group_inputs_meet_their_conditions(V, first, groups, width, D, rows, mode):
    h, E, bias, v0 = sr.head_inputs(V, D, rows, seed=1)
    x = sr.head_logits(h, E, bias)
    ref, g = sr.log_softmax(x), sr.group_logprobs(x, first, groups, width)
    assert np.isfinite(ref).all() and np.isfinite(g).all()
    assert sr.head_bound(h, E, g).max() < 1e-5
    nv = (D // 4 + 63) // 64
    assert D % 4 == 0 and nv <= 10 and first + groups * width <= V
    # the groups and the special columns share the row's mass: exp(lse_g(group)) = 1 - p(specials), compared as masses (the logarithm of
    # 1 - p is ill-conditioned where the specials hold nearly everything) -- and so lse_g(group) <= 0 up to the rounding of what is summed
    special = np.r_[0:first, first + groups * width:V]
    assert np.abs(np.exp(sr.logsumexp(g, -1)) + np.exp(ref[:, special]).sum(-1) - 1.0).max() < 1e-13


def test_group_cases_cover_every_instantiation_and_both_sides_of_its_guard():
    saprot = [c for c in sr.GROUP_CASES if c[:4] == sr.SAPROT]
    nvs = {(c[4] // 4 + 63) // 64 for c in saprot}
    assert nvs == {1, 2, 3, 5, 6, 10} and {c[4] for c in saprot} == {4, 256, 260, 480, 512, 516, 1280, 1284, 2560}
    assert {c[5] for c in sr.GROUP_CASES} == {1, 4, 5} and {c[6] for c in sr.GROUP_CASES} == {"full", "group", "both"}


@pytest.mark.parametrize("V,ldl,rows,kind0", sr.wide_cases())
def test_wide_inputs_meet_the_edge_condition(V, ldl, rows, kind0):
    x, kinds, tgt = sr.wide_inputs(V, ldl, rows, kind0)
    assert ldl % 4 == 0 and ldl >= V and x.shape == (rows, ldl)
    ref = sr.log_softmax(x[:, :V])
    bound = sr.wide_bound(x[:, :V], ref)
    ratio = sr.wide_edge_condition(x[:, :V], kinds, ref, bound)
    print(f"wide V={V} ldl={ldl} rows={rows} kinds={kinds} bound max={bound.max():.3e} edge mass / (100 bound) min={min(ratio):.2f}")
    assert min(ratio) >= 1.0, (kinds, ratio)
    assert bound.max() < 2.5e-5
    for r, k in enumerate(kinds):                                     # within 2 of the maximum (asked for at V = 50 257; true everywhere)
        if k != "dominant" and not (k == "flat" and V <= 1030):
            assert np.all(x[r, :V].max() - x[r, sr.wide_edge_columns(V)] <= 2.0)
    assert np.all((tgt >= 0) & (tgt < V))


def test_wide_cases_cover_the_issue():
    cases = sr.wide_cases()
    assert {c[0] for c in cases} == set(sr.WIDE_V)
    for V in sr.WIDE_V:
        assert {c[1] for c in cases if c[0] == V} == {(V + 3) // 4 * 4, (V + 63) // 64 * 64}
    assert {c[2] for c in cases if c[0] < 50257} == {1, 2, 5} and max(c[2] for c in cases if c[0] == 50257) <= 3
    seen = {(V, sr.WIDE_KINDS[(k0 + r) % 6]) for V, _, rows, k0 in cases for r in range(rows)}
    assert {k for _, k in seen} == set(sr.WIDE_KINDS)
    assert (50257, "ascending") in seen
    tg = set()
    for V, ldl, rows, k0 in cases:
        tg |= {("0", "V-1", "V-2", "mid")[(k0 + r) % 4] for r in range(rows)}
    assert len(tg) == 4


def test_wide_neg_inf_patterns_sit_where_their_names_say():
    for name, V, cols in sr.WIDE_NEG_INF:
        assert all(0 <= c < V for c in cols)
        threads = {(c // 4) % 256 for c in cols}
        if name == "second_chunk_of_a_thread":
            assert threads == {2} and {c // 4 for c in cols} == {2, 258}
        if name == "last_partial_group":
            assert V % 4 == 3 and {c // 4 for c in cols} == {(V + 3) // 4 - 1} and (V + 3) // 4 <= 256
        x, _, _ = sr.wide_inputs(V, (V + 3) // 4 * 4, 2, 1)
        x[:, cols] = -np.inf
        ref = sr.log_softmax(x[:, :V])
        want = torch.log_softmax(_t(x[:, :V]), -1).numpy()
        assert np.array_equal(np.isneginf(ref), np.isneginf(want)) and np.isneginf(ref[:, cols]).all()
        keep = np.isfinite(want)
        assert keep.sum() == 2 * (V - len(cols)) and np.abs(ref[keep] - want[keep]).max() < 1e-12


def test_exact_sequence_cases_are_exact_in_fp32():
    """Every (alpha, beta) the GPU cases use at a length fits 24 bits, and the set covers {0, 0.25, 0.5, 1} on both sides."""
    assert {a for a, _ in sr.EXACT_AB} == {0.0, 0.25, 0.5, 1.0} == {b for _, b in sr.EXACT_AB}
    for T in sr.SEQ_T:
        ok = [ab for ab in sr.EXACT_AB if sr.exact_bits(*ab, T, True) <= 24]
        assert len(ok) >= 4, (T, ok)
        assert all(sr.exact_bits(a, 0.0, T, False) <= 24 for a in (0.0, 0.25, 0.5, 1.0)), T
    # a fused term computed in fp32 is the float64 value, in every order of the products
    rng = np.random.default_rng(3)
    lp, pr, ev = (sr.quantized(rng, 4096) for _ in range(3))
    for a, b in sr.EXACT_AB:
        a32, b32 = np.float32(a), np.float32(b)
        two = (np.float32(1) - a32) * lp + a32 * pr
        f = (np.float32(1) - b32) * two + b32 * ev
        want = (1 - b) * ((1 - a) * lp.astype(np.float64) + a * pr.astype(np.float64)) + b * ev.astype(np.float64)
        assert f.dtype == np.float32 and np.array_equal(f.astype(np.float64), want)


def test_sequence_cases_reach_the_index_edges():
    a0s, ns, flips, lens_seen = set(), set(), set(), set()
    for T in sr.SEQ_T:
        for B in sr.SEQ_B:
            for k in range(5):
                c = sr.seq_dense_case(B, T, k)
                assert np.all(c["a0"] + c["n"] <= T - 1) and np.all(c["row0"] + c["n"] < len(c["prior"]))    # a spare row stays
                for b in range(B):
                    lens_seen.add((int(c["lens"][b]) - T) if c["lens"][b] >= T - 1 and T > 3 else int(c["lens"][b]))
                    if c["n"][b]:
                        a0s.add(int(c["a0"][b]))
                        ns.add(int(c["n"][b]))
                        flips.add(int(c["flip"][b]))
                assert (c["n"] == 0).any() or B == 1 or T == 2
    assert {0, 1, 63, 64} <= a0s and {1, 64, 65} <= ns and flips == {0, 1} and {0, 1, 2, -1} <= lens_seen
    dense, ragged = sr.seq_ragged_case(130, 0)
    assert list(ragged["seq_p"]) == [0, 0, 1, 31, 64, 129]


def test_realistic_sequence_bound_covers_fp32_summation():
    c = sr.seq_dense_case(4, 1024, 4, exact=False, with_eve=True)
    ref, mass = sr.seq_reference(c, 0.6, 0.3, 0, terms=True)
    bound = sr.seq_realistic_bound(c["lens"], mass)
    # the same sum carried in fp32 left to right: a worse order than the kernel's lanes and tree, still far inside the bound's scale
    a, b = np.float32(0.6), np.float32(0.3)
    for s in range(4):
        acc = np.float32(0)
        for t in range(int(c["lens"][s]) - 1):
            tgt = c["tokens"][s * 1024 + t + 1]
            v = c["lp"][s * 1024 + t, tgt]
            if c["n"][s] > 0 and c["a0"][s] <= t < c["a0"][s] + c["n"][s]:
                i = t - c["a0"][s]
                row = c["row0"][s] + (c["n"][s] - 1 - i if c["flip"][s] else i)
                v = (np.float32(1) - a) * v + a * c["prior"][row, tgt]
                v = (np.float32(1) - b) * v + b * c["eve"][row, tgt]
            acc = np.float32(acc + v)
        print(f"seq {s} len {c['lens'][s]} fp32 left-to-right err {abs(float(acc) - ref[s]):.3e} bound {bound[s]:.3e}")
        assert bound[s] == 0 or bound[s] < 1e-2 * max(1.0, abs(ref[s]))
