"""The scoring tail op by op (pgmi_op_vocab_logsoftmax / pgmi_op_wide_logsoftmax / pgmi_op_group_logsoftmax / pgmi_op_seq_loglik: the
production launchers on the entries' own buffers) against the float64 reference of scoring_ref.py.

Inputs, bounds and input conditions are scoring_ref's and are rehearsed on the CPU in test_scoring_ref.py; nothing here is derived from
what the kernels return.  Every output buffer starts as 0xFF bytes, so a skipped element is NaN, and carries a guard the entry checks, so
a write past the end fails the call.  Every case prints its shape, error and bound before it asserts.

Contract checked beside the values: -inf logits follow torch.log_softmax (probability 0, the other columns unchanged; a row of nothing
but -inf is NaN); the non-finite flag is set exactly when a written output is non-finite; pad columns are excluded by index, never by
value; a row's bits depend on the row alone; the ragged sequence sum has the dense kernel's bits on the same row values."""
import functools
import hashlib

import numpy as np
import pytest

import scoring_ref as sr
from proteingym_amd import _lib

pytestmark = pytest.mark.gpu

NEG_INF = -np.inf


def _p(a):
    return a.ctypes.data_as(_lib._f32p) if a is not None else None


def _i(a):
    return a.ctypes.data_as(_lib._i32p) if a is not None else None


def _frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.flags.writeable = False
    return arrays


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- runners -----------------------------------------------------------------------------------------------------------------------------
def run_narrow(lib, h, E, bias):
    rows, D = h.shape
    V = E.shape[0]
    out = np.full((rows, V), 12345.0, np.float32)
    flag = np.full(1, -1, np.int32)
    _lib.check(lib.pgmi_op_vocab_logsoftmax(0, _p(h), _p(E), _p(bias), rows, D, V, _p(out), _i(flag)))
    return out, int(flag[0])


def run_wide(lib, x, V, tgt=None):
    rows, ldl = x.shape
    out = np.full(rows if tgt is not None else (rows, V), 12345.0, np.float32)
    flag = np.full(1, -1, np.int32)
    _lib.check(lib.pgmi_op_wide_logsoftmax(0, _p(x), ldl, rows, V, _i(tgt), _p(out), _i(flag)))
    return out, int(flag[0])


def run_group(lib, h, E, bias, first, groups, width, mode="both"):
    rows, D = h.shape
    V = E.shape[0]
    full = np.full((rows, V), 12345.0, np.float32) if mode in ("full", "both") else None
    group = np.full((rows, groups), 12345.0, np.float32) if mode in ("group", "both") else None
    flag = np.full(1, -1, np.int32)
    _lib.check(lib.pgmi_op_group_logsoftmax(0, _p(h), _p(E), _p(bias), rows, D, V, first, groups, width, _p(full), _p(group), _i(flag)))
    return full, group, int(flag[0])


def run_seq(lib, c, alpha=0.0, beta=0.0, eve_fallback=0):
    out = np.full(c["B"], 12345.0, np.float32)
    g = c.get
    _lib.check(lib.pgmi_op_seq_loglik(0, _p(c["lp"]), _i(c["tokens"]), c["B"], c["T"], c["V"], _i(g("lens")), _i(g("seq_off")), _i(g("seq_p")),
                                      _i(g("seq_root")), len(c["tokens"]), _p(g("prior")), len(c["prior"]) if "prior" in c else 0,
                                      _i(g("a0")), _i(g("row0")), _i(g("n")), _i(g("flip")), alpha, _p(g("eve")), beta, eve_fallback, _p(out)))
    return out


def compare(tag, out, ref, bound):
    """(err, bound there) at the worst error / bound over the finite references.  A -inf reference must come back as -inf and a NaN as NaN:
    where the patterns differ the error is inf, so that the caller's assertion fails after it has printed."""
    out64 = out.astype(np.float64)
    fin = np.isfinite(ref)
    if not (np.array_equal(np.isneginf(out64), np.isneginf(ref)) and np.array_equal(np.isnan(out64), np.isnan(ref))):
        print(f"{tag}: non-finite pattern differs: out has {int(np.isnan(out64).sum())} NaN, {int(np.isneginf(out64).sum())} -inf; "
              f"reference {int(np.isnan(ref).sum())} NaN, {int(np.isneginf(ref).sum())} -inf")
        return np.inf, 1.0
    if not fin.any():
        return 0.0, np.inf
    err = np.where(fin, np.abs(np.where(fin, out64, 0.0) - np.where(fin, ref, 0.0)), 0.0)
    ratio = np.where(fin, err / np.broadcast_to(bound, err.shape), 0.0)
    k = np.unravel_index(np.argmax(ratio), ratio.shape)
    return float(err[k]), float(np.broadcast_to(bound, err.shape)[k])


# ---- narrow head -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def narrow_case(V, D, rows, shift=0.0):
    h, E, bias, v0 = sr.head_inputs(V, D, rows, shift=shift)
    ref = sr.log_softmax(sr.head_logits(h, E, bias))
    bound = sr.head_bound(h, E, ref)
    _frozen(h, E, bias, ref, bound)
    return h, E, bias, ref, bound


def check_narrow(lib, V, D, rows, shift=0.0):
    h, E, bias, ref, bound = narrow_case(V, D, rows, shift)
    out, flag = run_narrow(lib, h, E, bias)
    err, b = compare("narrow", out, ref, bound)
    rowsum = float(np.abs(np.exp(out.astype(np.float64)).sum(-1) - 1.0).max())
    print(f"narrow V={V} D={D} rows={rows}{' bias+3e4' if shift else ''} err={err:.3e} bound={b:.3e} err/bound={err / b:.3f} "
          f"|sum exp - 1|={rowsum:.2e} flag={flag}")
    assert np.isfinite(out).all()
    assert err <= b, (V, D, rows, err, b)
    assert rowsum <= 1e-6
    assert flag == 0
    return out


@pytest.mark.parametrize("V,D,rows", sr.NARROW_CASES)
def test_narrow_head_vs_fp64(lib, V, D, rows):
    check_narrow(lib, V, D, rows)


def test_narrow_head_shift_invariance(lib):
    """bias + 3e4 on every column: the log-softmax is that of the shifted fp32 biases (the reference adds them in float64)."""
    check_narrow(lib, *sr.NARROW_SHIFT_CASE, shift=3e4)


# ---- wide head ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def wide_case(V, ldl, rows, kind0):
    x, kinds, tgt = sr.wide_inputs(V, ldl, rows, kind0)
    ref = sr.log_softmax(x[:, :V])
    bound = sr.wide_bound(x[:, :V], ref)
    cond = sr.wide_edge_condition(x[:, :V], kinds, ref, bound)
    _frozen(x, tgt, ref, bound)
    return x, tuple(kinds), tgt, ref, bound, min(cond)


@pytest.mark.parametrize("V,ldl,rows,kind0", sr.wide_cases())
def test_wide_head_vs_fp64_and_pad_columns(lib, V, ldl, rows, kind0):
    """Both forms against float64; pad columns of 0, NaN and +3e38 give the same bits.  The sha256 of the raw output bytes of each form is
    printed: the record that a change of the kernel leaves finite rows bit for bit alone."""
    x, kinds, tgt, ref, bound, cond = wide_case(V, ldl, rows, kind0)
    assert cond >= 1.0                                                # every edge column carries >= 100 x the bound in mass
    full, flag = run_wide(lib, x, V)
    picked, flag_t = run_wide(lib, x, V, tgt)
    r = np.arange(rows)
    err, b = compare("wide", full, ref, bound)
    err_t, b_t = compare("wide tgt", picked, ref[r, tgt], bound[r, tgt])
    print(f"wide V={V} ldl={ldl} rows={rows} kinds={','.join(kinds)} err={err:.3e} bound={b:.3e} err/bound={err / b:.3f} | tgt={list(tgt)} "
          f"err={err_t:.3e} bound={b_t:.3e} err/bound={err_t / b_t:.3f} | edge mass/(100 bound)={cond:.2f} flags={flag},{flag_t} "
          f"sha256 full={hashlib.sha256(full.tobytes()).hexdigest()} tgt={hashlib.sha256(picked.tobytes()).hexdigest()}")
    assert np.isfinite(full).all() and np.isfinite(picked).all()
    assert err <= b and err_t <= b_t, (V, ldl, rows, kinds, err, b, err_t, b_t)
    assert np.array_equal(_bits(picked), _bits(full[r, tgt]))           # the scoring form reads the same row statistics
    assert flag == 0 and flag_t == 0
    if ldl > V:
        for pad in (np.nan, 3e38):
            y = x.copy()
            y[:, V:] = pad
            full_p, flag_p = run_wide(lib, y, V)
            picked_p, flag_tp = run_wide(lib, y, V, tgt)
            assert np.array_equal(_bits(full_p), _bits(full)) and np.array_equal(_bits(picked_p), _bits(picked)), (V, ldl, pad)
            assert flag_p == 0 and flag_tp == 0


@pytest.mark.parametrize("name,V,cols", sr.WIDE_NEG_INF)
def test_wide_head_neg_inf_columns(lib, name, V, cols):
    """-inf logits as torch.log_softmax treats them: those columns are -inf, the others what float64 gives without them."""
    ldl = (V + 3) // 4 * 4
    x, kinds, tgt, _, _, _ = wide_case(V, ldl, 2, 1)
    y = x.copy()
    y[:, cols] = NEG_INF
    ref = sr.log_softmax(y[:, :V])
    bound = sr.wide_bound(y[:, :V], ref)
    full, flag = run_wide(lib, y, V)
    nan = int(np.isnan(full).sum())
    tgt = np.array([V // 2, V // 2 + 1], np.int32)                    # non-target -inf columns
    picked, flag_t = run_wide(lib, y, V, tgt)
    print(f"wide -inf {name} V={V} cols={cols}: NaN outputs {nan} of {full.size}, -inf outputs {int(np.isneginf(full).sum())}, "
          f"tgt form {picked}, flags={flag},{flag_t}")
    err, b = compare("wide -inf " + name, full, ref, bound)
    err_t, b_t = compare("wide -inf tgt " + name, picked, ref[np.arange(2), tgt], bound[np.arange(2), tgt])
    print(f"wide -inf {name} err={err:.3e} bound={b:.3e} | tgt err={err_t:.3e} bound={b_t:.3e}")
    assert err <= b and err_t <= b_t
    assert flag == 1                                                   # -inf outputs were written
    assert flag_t == 0                                                 # the written outputs are finite


def test_wide_head_all_neg_inf_row_is_nan(lib):
    x, *_ = wide_case(1023, 1024, 2, 1)
    y = x.copy()
    y[1, :] = NEG_INF
    ref = sr.log_softmax(y[:, :1023])
    full, flag = run_wide(lib, y, 1023)
    print(f"wide all -inf row: NaN {int(np.isnan(full[1]).sum())} of 1023; row 0 NaN {int(np.isnan(full[0]).sum())}, flag={flag}")
    assert np.isnan(full[1]).all() and np.isnan(ref[1]).all() and flag == 1
    err, b = compare("wide beside all -inf", full[:1], ref[:1], sr.wide_bound(y[:1, :1023], ref[:1]))
    assert err <= b


@pytest.mark.parametrize("V", [1025, 4099])
def test_wide_head_maxima_2000_apart(lib, V):
    """One column at +1000, the others in [-1000, -999]: the threads' running maxima lie 2000 apart, so a merge that rescales towards the
    smaller maximum overflows even in double (exp(709) is the limit) -- at V >= 1024, where every thread holds columns, that is the only
    place where such a merge and the right one differ by more than rounding."""
    rng = np.random.default_rng(V)
    x = np.zeros((2, (V + 3) // 4 * 4), np.float32)
    x[:, :V] = rng.uniform(-1000.0, -999.0, (2, V))
    x[0, V // 3], x[1, V - 1] = 1000.0, 1000.0
    ref = sr.log_softmax(x[:, :V])
    bound = sr.wide_bound(x[:, :V], ref)
    full, flag = run_wide(lib, x, V)
    err, b = compare("wide 2000 apart", full, ref, bound)
    print(f"wide maxima 2000 apart V={V} err={err:.3e} bound={b:.3e} err/bound={err / b:.3f} flag={flag}")
    assert err <= b and flag == 0


# ---- grouped head ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def group_case(V, first, groups, width, D, rows):
    h, E, bias, v0 = sr.head_inputs(V, D, rows, seed=1)
    x = sr.head_logits(h, E, bias)
    ref, g = sr.log_softmax(x), sr.group_logprobs(x, first, groups, width)
    _frozen(h, E, bias, ref, g)
    return h, E, bias, ref, g, sr.head_bound(h, E, ref), sr.head_bound(h, E, g)


@pytest.mark.parametrize("V,first,groups,width,D,rows,mode", sr.GROUP_CASES)
def test_group_head_vs_fp64(lib, V, first, groups, width, D, rows, mode):
    h, E, bias, ref, gref, bound, gbound = group_case(V, first, groups, width, D, rows)
    full, group, flag = run_group(lib, h, E, bias, first, groups, width, mode)
    msg = f"group V={V} first={first} {groups}x{width} D={D} (NV {(D // 4 + 63) // 64}) rows={rows} {mode}:"
    if full is not None:
        err, b = compare("group full", full, ref, bound)
        msg += f" full err={err:.3e} bound={b:.3e} err/bound={err / b:.3f}"
    if group is not None:
        gerr, gb = compare("group", group, gref, gbound)
        special = np.r_[0:first, first + groups * width:V]
        lse = sr.logsumexp(group.astype(np.float64), -1)
        # the groups' mass and the specials' add up to 1: an error d of the group values moves the groups' mass by at most d of itself
        mass = np.abs(np.exp(lse) + np.exp(ref[:, special]).sum(-1) - 1.0)
        tol = gbound.max(-1) + 1e-12
        msg += f" group err={gerr:.3e} bound={gb:.3e} err/bound={gerr / gb:.3f} lse_g max={lse.max():.3e} |mass - 1| max={mass.max():.3e}"
    print(msg + f" flag={flag}")
    if full is not None:
        assert np.isfinite(full).all() and err <= b
    if group is not None:
        assert np.isfinite(group).all() and gerr <= gb
        assert np.all(lse <= tol) and np.all(mass <= tol), (lse, mass, tol)
    assert flag == 0


def test_group_head_modes_share_their_bits(lib):
    V, first, groups, width = sr.SAPROT
    h, E, bias, *_ = group_case(V, first, groups, width, 516, 5)
    full, group, _ = run_group(lib, h, E, bias, first, groups, width, "both")
    full1, _, _ = run_group(lib, h, E, bias, first, groups, width, "full")
    _, group1, _ = run_group(lib, h, E, bias, first, groups, width, "group")
    assert np.array_equal(_bits(full), _bits(full1)) and np.array_equal(_bits(group), _bits(group1))


# ---- -inf through a -inf bias, narrow and grouped ---------------------------------------------------------------------------------------
def test_narrow_head_neg_inf_bias(lib):
    h, E, bias, _, _ = narrow_case(33, 320, 5)
    b2 = bias.copy()
    b2[[0, 7, 32]] = NEG_INF
    ref = sr.log_softmax(sr.head_logits(h, E, b2))
    out, flag = run_narrow(lib, h, E, b2)
    err, b = compare("narrow -inf", out, ref, sr.head_bound(h, E, ref))
    print(f"narrow -inf bias on columns 0, 7, 32: -inf outputs {int(np.isneginf(out).sum())} NaN {int(np.isnan(out).sum())} err={err:.3e} bound={b:.3e} flag={flag}")
    assert err <= b and flag == 1
    out, flag = run_narrow(lib, h, E, np.full_like(bias, NEG_INF))
    assert np.isnan(out).all() and flag == 1                          # nothing but -inf: NaN


def test_group_head_neg_inf_bias(lib):
    V, first, groups, width = sr.SAPROT
    h, E, bias, *_ = group_case(V, first, groups, width, 260, 5)
    b2 = bias.copy()
    b2[[2, 30, 445]] = NEG_INF                                         # a special, one column of group 1, the last column
    b2[first + 3 * width:first + 4 * width] = NEG_INF                  # all of group 3
    x = sr.head_logits(h, E, b2)
    ref, gref = sr.log_softmax(x), sr.group_logprobs(x, first, groups, width)
    full, group, flag = run_group(lib, h, E, b2, first, groups, width)
    err, b = compare("group full -inf", full, ref, sr.head_bound(h, E, ref))
    gerr, gb = compare("group -inf", group, gref, sr.head_bound(h, E, gref))
    print(f"group -inf bias: full -inf {int(np.isneginf(full).sum())} err={err:.3e} bound={b:.3e} | group -inf {int(np.isneginf(group).sum())} "
          f"err={gerr:.3e} bound={gb:.3e} flag={flag}")
    assert err <= b and gerr <= gb and flag == 1
    assert np.isneginf(group[:, 3]).all() and np.isfinite(np.delete(group, 3, 1)).all()
    _, group, flag = run_group(lib, h, E, b2 * 1, first, groups, width, "group")
    assert flag == 1                                                   # group 3 is a written -inf


# ---- the non-finite flag -----------------------------------------------------------------------------------------------------------------
def test_flag_is_set_exactly_when_a_written_output_is_non_finite(lib):
    h, E, bias, _, _ = narrow_case(25, 65, 9)
    for what, (hh, bb) in {"NaN hidden": (h.copy(), bias), "+inf bias": (h, bias.copy())}.items():
        if what == "NaN hidden":
            hh[4, 17] = np.nan
        else:
            bb[3] = np.inf
        out, flag = run_narrow(lib, hh, E, bb)
        bad = ~np.isfinite(out)
        print(f"flag narrow {what}: non-finite outputs {int(bad.sum())} flag={flag}")
        assert flag == 1 and bad.any()
        if what == "NaN hidden":
            assert bad[4].all() and not np.delete(bad, 4, 0).any()    # the other rows are untouched
    V, first, groups, width = sr.SAPROT
    h, E, bias, *_ = group_case(V, first, groups, width, 256, 4)
    hh = h.copy()
    hh[2, 100] = np.nan
    for mode in ("full", "group", "both"):
        full, group, flag = run_group(lib, hh, E, bias, first, groups, width, mode)
        for o in (full, group):
            assert o is None or (np.isnan(o[2]).all() and np.isfinite(np.delete(o, 2, 0)).all())
        assert flag == 1
    bb = bias.copy()
    bb[440] = np.inf
    full, group, flag = run_group(lib, h, E, bb, first, groups, width, "both")
    assert flag == 1 and np.isnan(full).all()
    x, _, tgt, *_ = wide_case(4099, 4160, 5, 2)
    for what, val, col in (("NaN logit", np.nan, 2050), ("+inf logit", np.inf, 4098)):
        y = x.copy()
        y[3, col] = val
        full, flag = run_wide(lib, y, 4099)
        picked, flag_t = run_wide(lib, y, 4099, tgt)
        print(f"flag wide {what}: non-finite rows {sorted(set(np.nonzero(~np.isfinite(full))[0]))} flags={flag},{flag_t}")
        assert flag == 1 and flag_t == 1
        assert np.isnan(full[3]).all() and np.isfinite(np.delete(full, 3, 0)).all()
        assert np.isnan(picked[3]) and np.isfinite(np.delete(picked, 3)).all()


# ---- row independence --------------------------------------------------------------------------------------------------------------------
def _launch_views(buf9, probe):
    """The launches of a comparison, all views of ONE buffer of 9 rows whose rows 0, 3, 4 and 8 (and so twice and more) hold the probe
    row: the 9-row launch and the probe alone (row 0 as a launch of one)."""
    for r in (0, 3, 4, 8):
        buf9[r] = probe
    return buf9, buf9[:1]


def test_a_rows_bits_do_not_depend_on_the_launch_narrow(lib):
    h, E, bias, _, _ = narrow_case(33, 320, 9)
    hh = h.copy()
    all9, alone = _launch_views(hh, h[5].copy())
    out9, _ = run_narrow(lib, all9, E, bias)
    out1, _ = run_narrow(lib, alone, E, bias)
    for r in (0, 3, 4, 8):
        assert np.array_equal(_bits(out9[r]), _bits(out1[0])), r
    assert not np.array_equal(_bits(out9[1]), _bits(out1[0]))


def test_a_rows_bits_do_not_depend_on_the_launch_group(lib):
    V, first, groups, width = sr.SAPROT
    h, E, bias, _ = sr.head_inputs(V, 260, 9, seed=1)
    hh = h.copy()
    all9, alone = _launch_views(hh, h[5].copy())
    f9, g9, _ = run_group(lib, all9, E, bias, first, groups, width)
    f1, g1, _ = run_group(lib, alone, E, bias, first, groups, width)
    for r in (0, 3, 4, 8):
        assert np.array_equal(_bits(f9[r]), _bits(f1[0])) and np.array_equal(_bits(g9[r]), _bits(g1[0])), r
    assert not np.array_equal(_bits(f9[1]), _bits(f1[0]))


@pytest.mark.parametrize("V,ldl", [(1030, 1088), (4099, 4100)])
def test_a_rows_bits_do_not_depend_on_the_launch_wide(lib, V, ldl):
    rng = np.random.default_rng(V)
    buf = np.stack([np.pad(sr.wide_row(V, sr.WIDE_KINDS[r % 6], rng), (0, ldl - V)) for r in range(9)])
    all9, alone = _launch_views(buf, buf[5].copy())
    tgt = np.full(9, V - 1, np.int32)
    out9, _ = run_wide(lib, all9, V)
    out1, _ = run_wide(lib, alone, V)
    t9, _ = run_wide(lib, all9, V, tgt)
    t1, _ = run_wide(lib, alone, V, tgt[:1])
    for r in (0, 3, 4, 8):
        assert np.array_equal(_bits(out9[r]), _bits(out1[0])) and _bits(t9)[r] == _bits(t1)[0], r
    assert not np.array_equal(_bits(out9[1]), _bits(out1[0]))


# ---- sequence sums -----------------------------------------------------------------------------------------------------------------------
def _exact_ab(T, k, with_eve):
    ok = [ab for ab in sr.EXACT_AB if sr.exact_bits(*ab, T, with_eve) <= 24]
    return ok[k % len(ok)]


@pytest.mark.parametrize("T", sr.SEQ_T)
@pytest.mark.parametrize("B", sr.SEQ_B)
def test_sequence_sums_exact(lib, B, T):
    """lp, prior and eve in multiples of 2^-8 and dyadic weights: every product and partial sum is exact in fp32 in any order
    (scoring_ref.exact_bits), so the kernel equals float64 exactly and only the index logic is on trial."""
    for k in range(5):
        plain = sr.seq_dense_case(B, T, k, with_prior=False)
        assert np.array_equal(run_seq(lib, plain).astype(np.float64), sr.seq_reference(plain)), (B, T, k, "no prior")
        for with_eve in (False, True):
            c = sr.seq_dense_case(B, T, k, with_eve=with_eve)
            a, b = _exact_ab(T, k + B, with_eve)
            assert sr.exact_bits(a, b, T, with_eve) <= 24
            out = run_seq(lib, c, a, b)
            ref = sr.seq_reference(c, a, b)
            if k == 0:
                print(f"seq exact B={B} T={T} lens={list(c['lens'])} a0={list(c['a0'])} n={list(c['n'])} flip={list(c['flip'])} "
                      f"alpha={a} beta={b if with_eve else None}: out={out} ref={ref}")
            assert np.array_equal(out.astype(np.float64), ref), (B, T, k, with_eve, a, b, out, ref)


@pytest.mark.parametrize("B,T", [(4, 66), (5, 130), (5, 1024)])
def test_sequence_sums_eve_holes(lib, B, T):
    """EVE columns of -inf: under eve_fallback the position is `two` exactly; without it the sum is -inf when a target hits such a column
    inside a window and is unchanged when none does."""
    hit_any = miss_any = False
    for k in range(5):
        c = sr.seq_dense_case(B, T, k, with_eve=True, eve_holes=True)
        a, b = _exact_ab(T, k, True)
        if not 0 < b < 1:
            a, b = 0.5, 0.5
        for fb in (1, 0):
            out = run_seq(lib, c, a, b, fb).astype(np.float64)
            ref = sr.seq_reference(c, a, b, fb)
            assert np.array_equal(out, ref), (B, T, k, fb, out, ref)
        hit_any |= bool(np.isneginf(ref).any())
        miss_any |= bool(np.isfinite(ref[c["n"] > 0]).any())
        print(f"seq eve holes B={B} T={T} k={k} alpha={a} beta={b}: no fallback {ref}")
    assert hit_any and miss_any


def test_sequence_sums_realistic(lib):
    c = sr.seq_dense_case(4, 1024, 4, exact=False, with_eve=True)
    c["lens"] = np.array([1024, 1023, 700, 66], np.int32)
    c["a0"], c["n"] = np.array([0, 64, 100, 0], np.int32), np.array([65, 65, 64, 65], np.int32)
    c["row0"] = np.array([0, 0, 65, 1], np.int32)
    assert np.all(c["row0"] + c["n"] < len(c["prior"]))
    ref, mass = sr.seq_reference(c, 0.6, 0.3, 0, terms=True)
    bound = sr.seq_realistic_bound(c["lens"], mass)
    out = run_seq(lib, c, 0.6, 0.3, 0)
    err = np.abs(out.astype(np.float64) - ref)
    print(f"seq realistic T=1024 lens={list(c['lens'])} alpha=0.6 beta=0.3: err={err} bound={bound} err/bound={err / bound}")
    assert np.all(err <= bound)


@pytest.mark.parametrize("T", [66, 130, 1024])
def test_ragged_sums_have_the_dense_bits(lib, T):
    for exact in (True, False):
        for with_prior, with_eve in ((False, False), (True, False), (True, True)):
            dense, ragged = sr.seq_ragged_case(T, T % 5, exact=exact, with_prior=with_prior, with_eve=with_eve)
            a, b = _exact_ab(T, 1, with_eve) if exact else (0.6, 0.3)
            d, r = run_seq(lib, dense, a, b), run_seq(lib, ragged, a, b)
            print(f"ragged T={T} exact={exact} prior={with_prior} eve={with_eve} seq_p={list(ragged['seq_p'])}: {r}")
            assert np.array_equal(_bits(d), _bits(r)), (T, exact, with_prior, with_eve, d, r)
            if exact:
                assert np.array_equal(r.astype(np.float64), sr.seq_reference(ragged, a, b))
