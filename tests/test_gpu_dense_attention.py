"""The encoder's dense attention chain, op by op (pgmi_op_dense_attention: the launchers and the argument pattern of one run_encoder
layer) against the float64 reference of attention_ref.py: the fused QKV epilogue (ESM2's rotary with one and two table rows per token,
q times log2 e, split q | k planes, transposed key-permuted V^T planes), attention_f16x3_v2_kernel at 64 and 128 lanes and the pipelined
attention_f16x3_v3_kernel on those operands with a device kv_len, and the three context stores (fp32, split planes, bf16).

Inputs in the manner of test_gpu_causal_attention.py (its make_fused is used as it is): q scaled to the same score spread at every width,
one spiky query row among the checked rows of sequence 0, V rows offset by 0 / 1e-3 / 5, and in every sequence with kv_len[b] < T the
first masked key t = kv_len[b] is spiky with a V row of 5 -- a leaked pad key moves the rows by O(1).  zero_lanes reproduces head dims
16 / 24 / 32 inside 64 lanes (active slots i < dh / 2 and 32 + i).  The reference always forms X W^T + b in float64 itself.

Tolerances.  (a) context values, rows t < kv_len[b]: 64 lanes below T = 1024: test_attention's 2e-5 max(1, |ref|max); 128 lanes and
T = 1024: max(that, 3 noise32), noise32 = the same reference evaluated in plain fp32 NumPy against its float64 value (the rule of
test_gpu_causal_attention.py), computed from the reference alone; the bf16 output adds 2^-8 |ref| element by element (bf16 keeps 8
significant bits: half an ulp is 2^-9 |x|).  (b) operand planes: test_gemm_f16x3's 2e-5 sqrt(K / 128) relative to max(1, the row's
max |x|), plus 2^-21 |value| for the split (hi + lo keeps 22 bits).  (c) - (e) are equalities of bits: all three stores form
fmaf(oc, inv_lo, om) * inv (attention_f16_common.h), the v3 kernel walks a row through the v2 kernel's arithmetic, a block order does not
touch it, a masked key has P = 0 exactly and the GEMM is row-local.  Every case prints its figures before it asserts."""
import numpy as np
import pytest

import attention_ref as ar
from proteingym_amd import _lib
from test_attention_ref import esm2_tables, esm_slots
from test_gpu_causal_attention import make_fused

pytestmark = pytest.mark.gpu

LOG2E = 1.4426950408889634
TS = [1, 31, 32, 33, 64, 97, 128, 129, 160, 193, 224, 257, 288, 1024]     # 193: the first length the default rule gives to v3; 288: the benchmark's
ALL_OUTS_AT = (33, 97, 193, 288)
F32, SPLIT, BF16 = 0, 1, 2
OUT_NAME = {F32: "f32", SPLIT: "split", BF16: "bf16"}
FLAVOURS = [(64, "none"), (64, "esm2"), (128, "esm2")]                   # ESM-1v, ESM2, ESM2-15B (the dh-128 table: two rows per token)


def _p(a, ty=_lib._f32p):
    return a.ctypes.data_as(ty) if a is not None else None


def full(B, T):
    return (T,) * B


def ragged(B, T):
    return (T, (T + 1) // 2, 1) if B == 3 else ((T + 1) // 2,) * B


def make_rows(rng, B, T, heads, lanes, kv_len):
    """q | k | v rows [B, T, 3 Da] with the properties of the module docstring."""
    Da = heads * lanes
    x = rng.standard_normal((B, T, 3 * Da)).astype(np.float32)
    x[..., :Da] *= 0.4 * np.sqrt(64 / lanes)
    x[0, min((2 * T) // 3, kv_len[0] - 1), :Da] *= 6.0                     # the running maximum jumps, in a row that is checked
    x[..., 2 * Da:] += rng.choice([0.0, 1e-3, 5.0], size=(B, T, 1)).astype(np.float32)
    for b in range(B):
        if kv_len[b] < T:
            x[b, kv_len[b], Da:2 * Da] *= 6.0                              # the first masked key is spiky ...
            x[b, kv_len[b], 2 * Da:] = 5.0                                 # ... and its V row is 5
    return x


def hole_columns(dh, heads):
    """Attention columns of `heads` 64-lane heads that no model dim of a dh-wide head takes."""
    holes = np.setdiff1d(np.arange(64), esm_slots(dh))
    assert len(holes) == 64 - dh
    return np.concatenate([h * 64 + holes for h in range(heads)])


def make_case(seed, B, T, heads, lanes, rot, kv_len, dh=None):
    """(X, W, bias, cos, sin, kv_len int32 [B]) of one case; dh: a head dim below 64 inside 64 lanes (zero weight rows, its own table)."""
    rng = np.random.default_rng(seed)
    X, W, bias = make_fused(rng, make_rows(rng, B, T, heads, lanes, kv_len), hole_columns(dh, heads) if dh else None)
    cos, sin = esm2_tables(T, dh or lanes) if rot == "esm2" else (None, None)
    return X, W, bias, cos, sin, np.asarray(kv_len, np.int32)


def run(lib, case, B, T, heads, lanes, out, operands=False, kv_null=False):
    X, W, bias, cos, sin, kv = case
    Da = heads * lanes
    ctx = np.full((B, T, Da), np.nan, np.float32)
    qk = np.full((B * T, 2 * Da), np.nan, np.float32) if operands else None
    v = np.full((B * T, Da), np.nan, np.float32) if operands else None
    _lib.check(lib.pgmi_op_dense_attention(0, lanes, _p(X), _p(W), _p(bias), X.shape[1], _p(cos), _p(sin),
                                           None if kv_null else _p(kv, _lib._i32p), B, T, heads, out, _p(ctx), _p(qk), _p(v)))
    return (ctx, qk, v) if operands else ctx


def valid_rows(kv, T):
    return np.arange(T)[None, :] < np.asarray(kv)[:, None]                # [B, T]: query rows t < kv_len[b]


def rne_bf16(x):
    """fp32 -> bf16 (round to nearest even) -> fp32, on finite values."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32)


# ---- (a) values against float64 ---------------------------------------------------------------------------------------------------------
def _value_cases():
    cases = []
    for T in TS:
        B = 1 if T == 1024 else 3
        outs = (SPLIT, F32, BF16) if T in ALL_OUTS_AT else (SPLIT,)
        for lanes, rot in FLAVOURS:
            kvs = [full(B, T), ragged(B, T)] + ([(32, 33, 64)] if T in (97, 160, 288) else [])     # the tile-edge set
            cases += [(lanes, rot, B, T, 2, kv, outs, None) for kv in dict.fromkeys(kvs)]          # T = 1: ragged is full
    for T in (97, 288):
        cases += [(64, "esm2", 3, T, 2, ragged(3, T), (SPLIT,), dh) for dh in (16, 24, 32)]
    cases.append((64, "esm2", 3, 160, 3, ragged(3, 160), (SPLIT,), None))   # 9 (sequence, head) pairs: the last XCD-local group of 8 is padded
    return cases


def _case_id(c):
    lanes, rot, B, T, heads, kv, outs, dh = c
    return f"{lanes}-{rot}-B{B}-T{T}-h{heads}-kv{'_'.join(map(str, kv))}" + (f"-dh{dh}" if dh else "")


@pytest.mark.parametrize("case", _value_cases(), ids=_case_id)
def test_context_vs_fp64(lib, case):
    lanes, rot, B, T, heads, kv, outs, dh = case
    c = make_case(7 * T + lanes + heads + sum(kv) + (dh or 0), B, T, heads, lanes, rot, kv, dh)
    ref = ar.dense_fused_reference(*c[:3], B, T, heads, lanes, kv, c[3], c[4])[0]
    ok = valid_rows(kv, T)
    noise32 = float(np.abs(ar.dense_fused_reference(*c[:3], B, T, heads, lanes, kv, c[3], c[4], dtype=np.float32)[0] - ref)[ok].max())
    base = 2e-5 * max(1.0, float(np.abs(ref[ok]).max()))
    tol = base if lanes == 64 and T < 1024 else max(base, 3.0 * noise32)
    for out in outs:
        ctx = run(lib, c, B, T, heads, lanes, out)
        d = np.abs(ctx - ref)[ok]
        allow = tol + (2.0 ** -8 * np.abs(ref[ok]) if out == BF16 else 0.0)
        err, worst = float(d.max()), float((d / allow).max())
        print(f"dense_att values {_case_id(case)} out={OUT_NAME[out]} err={err:.3e} noise32={noise32:.3e} bound={tol:.3e} err/bound={worst:.3f}")
        assert np.isfinite(ctx).all(), (case, out)                           # rows t >= kv_len[b] included: a padded batch carries them on
        assert worst < 1.0, (case, out, err, tol)
        if dh:
            cols = hole_columns(dh, heads)
            assert np.all(ctx[..., cols] == 0.0), (case, out)                # the padded context lanes: exact zeros
            assert np.abs(ctx[..., np.setdiff1d(np.arange(heads * 64), cols)]).min() > 0.0


# ---- (b) the QKV epilogue alone ---------------------------------------------------------------------------------------------------------
def make_gemm_case(seed, B, T, heads, lanes, rot, K=160):
    """Inputs in the manner of test_gemm_f16x3: rows of magnitude 0.01 / 1 / 30, W / sqrt(K), a unit bias."""
    rng = np.random.default_rng(seed)
    Da = heads * lanes
    X = (rng.standard_normal((B * T, K)) * rng.choice([0.01, 1.0, 30.0], size=(B * T, 1))).astype(np.float32)
    W = (rng.standard_normal((3 * Da, K)) / np.sqrt(K)).astype(np.float32)
    bias = rng.standard_normal(3 * Da).astype(np.float32)
    cos, sin = esm2_tables(T, lanes) if rot == "esm2" else (None, None)
    return X, W, bias, cos, sin, np.full(B, T, np.int32)


# M = B T: 1; 291 (one full 256-row tile, then a guarded one); 576; 2300 (every tile as two half-height items)
@pytest.mark.parametrize("lanes", [64, 128])
@pytest.mark.parametrize("rot", ["none", "esm2"])
@pytest.mark.parametrize("B,T", [(1, 1), (3, 97), (2, 288), (23, 100)])
def test_qkv_epilogue_operands_vs_fp64(lib, B, T, rot, lanes):
    heads = 2
    Da = heads * lanes
    c = make_gemm_case(B * T + lanes, B, T, heads, lanes, rot)
    X, K = c[0], c[0].shape[1]
    _, qk, v = run(lib, c, B, T, heads, lanes, SPLIT, operands=True)
    _, qk_ref, v_ref = ar.dense_fused_reference(*c[:3], B, T, heads, lanes, None, c[3], c[4])
    qk_ref = qk_ref.copy()
    qk_ref[:, :Da] *= LOG2E                                                 # the attention's softmax is base 2: q carries log2(e)
    row = 2e-5 * np.sqrt(K / 128) * np.maximum(1.0, np.abs(X).max(1, keepdims=True))
    assert np.isfinite(qk).all() and np.isfinite(v).all()                   # the planes start as 0xFF bytes: every element was written
    worst = {}
    for name, got, want in (("q", qk[:, :Da], qk_ref[:, :Da]), ("k", qk[:, Da:], qk_ref[:, Da:]), ("v", v, v_ref)):
        d = np.abs(got - want)
        worst[name] = (float(d.max()), float((d / (row + 2.0 ** -21 * np.abs(want))).max()))
    print(f"dense_att operands lanes={lanes} rot={rot} B={B} T={T} K={K} " +
          " ".join(f"{n}: err={e:.3e} err/bound={r:.3f}" for n, (e, r) in worst.items()))
    for name, (e, r) in worst.items():
        assert r < 1.0, (name, lanes, rot, B, T, e)


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("lanes", [64, 128])
def test_qkv_epilogue_item_kinds_and_launch_parameters_keep_the_bits(lib, monkeypatch, lanes):
    """PGMI_GEMM_HALF_TAIL 0 / 1 and PGMI_GEMM_VARIANT 0 / 1002 / 1008 at 2300 rows, with rotary: the same operand planes and context."""
    B, T, heads = 23, 100, 2
    c = make_gemm_case(lanes, B, T, heads, lanes, "esm2")
    monkeypatch.setenv("PGMI_GEMM_VARIANT", "0")
    monkeypatch.setenv("PGMI_GEMM_HALF_TAIL", "1")
    base = run(lib, c, B, T, heads, lanes, SPLIT, operands=True)
    assert all(np.isfinite(t).all() for t in base)
    monkeypatch.setenv("PGMI_GEMM_HALF_TAIL", "0")
    half = _same(run(lib, c, B, T, heads, lanes, SPLIT, operands=True), base)
    monkeypatch.setenv("PGMI_GEMM_HALF_TAIL", "1")
    variants = {}
    for variant in (1002, 1008):
        monkeypatch.setenv("PGMI_GEMM_VARIANT", str(variant))
        variants[variant] = _same(run(lib, c, B, T, heads, lanes, SPLIT, operands=True), base)
    print(f"dense_att operands bits lanes={lanes} rows={B * T} half_tail_0_equals_1={half} variants_equal_0={variants}")
    assert half and all(variants.values()), (half, variants)


@pytest.mark.parametrize("rot", ["none", "esm2"])
@pytest.mark.parametrize("lanes", [64, 128])
def test_qkv_epilogue_interior_rows_equal_guarded_rows(lib, lanes, rot):
    """The first 97 rows of the 3 x 97 launch (inside a full 256-row tile: the interior path) against the same rows computed as B = 1 (a tile
    with rows past M: the guarded path)."""
    B, T, heads = 3, 97, 2
    c = make_gemm_case(97 + lanes, B, T, heads, lanes, rot)
    ctx3, qk3, v3 = run(lib, c, B, T, heads, lanes, SPLIT, operands=True)
    one = (np.ascontiguousarray(c[0][:T]),) + c[1:5] + (c[5][:1],)
    ctx1, qk1, v1 = run(lib, one, 1, T, heads, lanes, SPLIT, operands=True)
    eq = [bool(np.array_equal(a, b)) for a, b in ((qk3[:T], qk1), (v3[:T], v1), (ctx3[0], ctx1[0]))]
    print(f"dense_att operands interior_vs_guarded lanes={lanes} rot={rot} qk={eq[0]} v={eq[1]} ctx={eq[2]}")
    assert np.isfinite(ctx1).all() and np.isfinite(qk1).all() and np.isfinite(v1).all()
    assert all(eq), eq


# ---- (c) one value, three stores --------------------------------------------------------------------------------------------------------
def _store_cases():
    cases = [(64, T, v3, rg) for T in (33, 97, 160, 288) for v3 in (0, 1) for rg in (False, True)]
    return cases + [(128, T, -1, rg) for T in (97, 288) for rg in (False, True)]


@pytest.mark.parametrize("lanes,T,v3,is_ragged", _store_cases())
def test_three_stores_hold_one_value(lib, lanes, T, v3, is_ragged):
    """bf16 context == rne_bf16(fp32 context) bit for bit, |split - fp32| <= 2^-21 |fp32|max, on every row; at 64 lanes under both kernels."""
    B, heads = 3, 2
    kv = ragged(B, T) if is_ragged else full(B, T)
    c = make_case(T + lanes, B, T, heads, lanes, "esm2", kv)
    try:
        _lib.check(lib.pgmi_set_option(b"att_v3", v3))
        f32, split, bf16 = (run(lib, c, B, T, heads, lanes, out) for out in (F32, SPLIT, BF16))
    finally:
        lib.pgmi_set_option(b"att_v3", -1)
    assert np.isfinite(f32).all() and np.isfinite(split).all() and np.isfinite(bf16).all()
    want = rne_bf16(f32)
    n_bf = int((bf16.view(np.uint32) != want.view(np.uint32)).sum())
    d_split, allow = float(np.abs(split - f32).max()), 2.0 ** -21 * float(np.abs(f32).max())
    print(f"dense_att stores lanes={lanes} T={T} att_v3={v3} kv={kv} bf16_mismatches={n_bf} |split-f32|max={d_split:.3e} bound={allow:.3e}")
    assert n_bf == 0, (lanes, T, v3, kv, np.argwhere(bf16.view(np.uint32) != want.view(np.uint32))[:8])
    assert d_split <= allow, (lanes, T, v3, kv, d_split, allow)


# ---- (d) v3 == v2 and the XCD-local order, through the fused operands -------------------------------------------------------------------
@pytest.mark.parametrize("is_ragged", [False, True])
@pytest.mark.parametrize("T", [5, 33, 97, 160, 224, 288, 737])
def test_v3_equals_v2_on_fused_operands(lib, T, is_ragged):
    B, heads, lanes = 3, 2, 64
    kv = ragged(B, T) if is_ragged else full(B, T)
    c = make_case(3 * T + 1, B, T, heads, lanes, "esm2", kv)
    try:
        _lib.check(lib.pgmi_set_option(b"att_v3", 0))
        base = {out: run(lib, c, B, T, heads, lanes, out) for out in (SPLIT, BF16)}
        _lib.check(lib.pgmi_set_option(b"att_v3", 1))
        got = {out: run(lib, c, B, T, heads, lanes, out) for out in (SPLIT, BF16)}
    finally:
        lib.pgmi_set_option(b"att_v3", -1)
    eq = {OUT_NAME[out]: bool(np.array_equal(base[out], got[out])) for out in base}
    print(f"dense_att v3_vs_v2 T={T} kv={kv} bit_identical={eq}")
    assert all(np.isfinite(t).all() for t in base.values())
    assert all(eq.values()), (T, kv, eq)


@pytest.mark.parametrize("B,heads,T", [(3, 3, 160), (2, 2, 288)])
def test_block_order_keeps_the_bits(lib, B, heads, T):
    """att_xcd_local 0 / 1 / -1, split output; a NULL kv_len is the full one."""
    kv = full(B, T)
    c = make_case(T + B, B, T, heads, 64, "esm2", kv)
    try:
        _lib.check(lib.pgmi_set_option(b"att_xcd_local", 0))
        base = run(lib, c, B, T, heads, 64, SPLIT)
        eq = {}
        for value in (1, -1):
            _lib.check(lib.pgmi_set_option(b"att_xcd_local", value))
            eq[value] = bool(np.array_equal(run(lib, c, B, T, heads, 64, SPLIT), base))
        eq["kv_len NULL"] = bool(np.array_equal(run(lib, c, B, T, heads, 64, SPLIT, kv_null=True), base))
    finally:
        lib.pgmi_set_option(b"att_xcd_local", -1)
    print(f"dense_att block_order B={B} heads={heads} T={T} bit_identical_to_grid_order={eq}")
    assert np.isfinite(base).all()
    assert all(eq.values()), eq


# ---- (e) masking is exact ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes,T", [(64, 97), (64, 288), (128, 160)])
def test_masked_rows_and_other_sequences_do_not_reach_a_row(lib, lanes, T):
    """Every X row t >= kv_len[b] replaced by other finite values: the rows t < kv_len[b] of every sequence keep their bits (P = 0 exactly,
    the GEMM is row-local); another sequence's rows replaced: a sequence's bits stay."""
    B, heads = 3, 2
    kv = ragged(B, T)
    c = make_case(T + lanes + 1, B, T, heads, lanes, "esm2", kv)
    ok = valid_rows(kv, T)
    base = run(lib, c, B, T, heads, lanes, SPLIT)
    rng = np.random.default_rng(T)
    X = c[0].reshape(B, T, -1).copy()
    X[~ok] = (3.0 * rng.standard_normal((int((~ok).sum()), X.shape[-1])) + 2.0).astype(np.float32)
    loud = run(lib, (np.ascontiguousarray(X.reshape(B * T, -1)),) + c[1:], B, T, heads, lanes, SPLIT)
    masked = bool(np.array_equal(loud[ok], base[ok]))
    X = c[0].reshape(B, T, -1).copy()
    X[0] = rng.standard_normal(X[0].shape).astype(np.float32)
    other = run(lib, (np.ascontiguousarray(X.reshape(B * T, -1)),) + c[1:], B, T, heads, lanes, SPLIT)
    batch = bool(np.array_equal(other[1:], base[1:]))
    print(f"dense_att masking lanes={lanes} T={T} kv={kv} masked_rows_replaced_bits_kept={masked} other_sequence_replaced_bits_kept={batch}")
    assert np.isfinite(base).all() and np.isfinite(loud).all() and np.isfinite(other).all()
    assert masked and batch and not np.array_equal(other[0], base[0])


# ---- (f) refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_come_back_as_einval(lib):
    B, T, heads = 2, 40, 2
    c = make_case(1, B, T, heads, 64, "esm2", full(B, T))
    X, W, bias, cos, sin, kv = c

    def refused(msg, case, lanes=64, out=SPLIT, heads=heads):
        with pytest.raises(_lib.PgmiError, match=msg) as e:
            run(lib, case, B, T, heads, lanes, out)
        assert e.value.code == _lib.EINVAL

    c96 = make_case(2, B, T, heads, 96, "none", full(B, T))
    refused("lanes = 96", c96, lanes=96)
    refused("multiple of 32", (np.zeros((B * T, 40), np.float32), np.zeros((3 * heads * 64, 40), np.float32), bias, cos, sin, kv))
    refused("rot_cos and rot_sin", (X, W, bias, cos, None, kv))
    refused("rot_cos and rot_sin", (X, W, bias, None, sin, kv))
    refused(r"kv_len\[1\] = 0 ", (X, W, bias, cos, sin, np.array([T, 0], np.int32)))
    refused(rf"kv_len\[0\] = {T + 1} ", (X, W, bias, cos, sin, np.array([T + 1, T], np.int32)))
    refused("attention_f16x3_v2: bad arguments .* out=3", c, out=3)              # the launcher's own message
    assert np.isfinite(run(lib, c, B, T, heads, 64, SPLIT)).all()               # and the library goes on working
