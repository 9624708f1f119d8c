"""The causal flavours of attention_f16x3_v2_kernel, the fused QKV epilogue with rot_halves 1 / 2 / 4 and Tranception's depth-wise
prep pass, op by op (pgmi_op_causal_attention: the launchers and the argument pattern of run_decoder) against the float64 reference
of attention_ref.py, on every row.

Inputs in the manner of test_gpu_ops.py::test_attention: q scaled to the same score spread at every width, one spiky query row, V
rows offset by 0 / 1e-3 / 5, and one spiky key with a V row of 5 near the end of every sequence -- a key leaked from above the
diagonal then moves early rows by O(1).  The fused form multiplies them by a near-identity weight; the reference always forms
X W^T + b in float64 itself.

Tolerances.  64 lanes, fused form, no ALiBi at T >= 1024: test_attention's |ctx - ref|max < 2e-5 max(1, |ref|max).  The 128- / 256-lane,
ALiBi-at-1024 and conv cases: max(that, 3 noise32), noise32 = the same reference evaluated in plain fp32 NumPy against its float64 value
(the rule of test_gpu_progen2.py::test_token_logprobs_real_width), computed here from the reference alone.  Every case prints its error,
noise32 and bound before it asserts.

Bit-identity of the prefix property rests on this reading of the kernel: a wave owns 32 query rows at q0 = 32 (block * WPB + wave), walks
the key tiles 0, 1, ... in that order whatever T is, and skips those above its diagonal (wanted); T only moves the block's tile count nkt
(tiles a row never uses), the clamped K rows / zero V^T columns of pad keys (masked to -inf, P = 0 exactly) and the grid.  The per-row
running reference of the deferred rescale depends on the row's own scores only.  So with the same instantiation (the same
att16_waves_per_block at 64 lanes; always at 128 / 256 lanes, which have one) a row's arithmetic is the same sequence of operations."""
import numpy as np
import pytest

import attention_ref as ar
from proteingym_amd import _lib

pytestmark = pytest.mark.gpu

LOG2E = 1.4426950408889634
TS = [1, 31, 32, 33, 64, 95, 96, 97, 127, 128, 129, 160, 257, 1024]


def _p(a):
    return a.ctypes.data_as(_lib._f32p) if a is not None else None


def waves_per_block(T):
    """att16_waves_per_block (attention_f16.hip): the 64-lane instantiation a sequence length selects."""
    n32 = (T + 31) // 32
    nblk = (n32 + 3) // 4
    wpb = (n32 + nblk - 1) // nblk
    return 4 if wpb == 3 else wpb


def same_instantiation(lanes, Ta, Tb):
    return lanes > 64 or waves_per_block(Ta) == waves_per_block(Tb)


def tranception_slopes(heads):
    """alibi_slopes(heads / 4) tiled four times (api_tranception.hip; a power of two here)."""
    n = heads // 4
    start = 2.0 ** (-(2.0 ** -(np.log2(n) - 3)))
    return np.tile(start ** np.arange(1, n + 1), 4).astype(np.float32)


def rotary_tables(kind, T, lanes):
    """cos / sin fp32 [T, lanes / 64, 64].  full: the same 32 frequencies in every slot group; group: pair position p = 32 g + i has its
    own frequency; partial: as group with angle 0 from pair rotary_dim / 2 on (32 of 128 lanes, 64 of 256: ProGen2's)."""
    if kind == "none":
        return None, None
    G = lanes // 64
    g, i = np.meshgrid(np.arange(G), np.arange(32), indexing="ij")
    if kind == "full":
        inv = (1.0 / 10000 ** (2 * i / 64)).astype(np.float32)
    else:
        rd = {64: 32, 128: 32, 256: 64}[lanes] if kind == "partial" else lanes
        p = 32 * g + i
        inv = np.where(2 * p < rd, 1.0 / 10000 ** (2 * p / rd), 0.0).astype(np.float32)
    ang = np.arange(T, dtype=np.float32)[:, None, None] * inv[None]                   # fp32 angles
    return tuple(np.ascontiguousarray(np.concatenate([f(ang)] * 2, -1), dtype=np.float32) for f in (np.cos, np.sin))


def make_rows(rng, B, T, heads, lanes):
    """q | k | v rows [B, T, 3 Da] with the properties of the module docstring."""
    Da = heads * lanes
    x = rng.standard_normal((B, T, 3 * Da)).astype(np.float32)
    x[..., :Da] *= 0.4 * np.sqrt(64 / lanes)
    x[0, (2 * T) // 3, :Da] *= 6.0                                                     # the running maximum jumps
    x[..., 2 * Da:] += rng.choice([0.0, 1e-3, 5.0], size=(B, T, 1)).astype(np.float32)
    te = max(T - 2, 0)
    x[:, te, Da:2 * Da] *= 6.0                                                         # a spiky key near the end of every sequence ...
    x[:, te, 2 * Da:] = 5.0                                                            # ... whose V row is 5
    return x


def make_fused(rng, rows, zero_lanes=None):
    """X = the rows, W [3 Da, 3 Da] = a diagonal in [0.8, 1.2] + 2e-4 dense noise, a small bias; zero_lanes: attention columns whose q, k
    and v are exact zeros (zero weight rows, zero bias)."""
    B, T, K = rows.shape
    W = (2e-4 * rng.standard_normal((K, K))).astype(np.float32)
    W[np.arange(K), np.arange(K)] += rng.uniform(0.8, 1.2, K).astype(np.float32)
    bias = (0.05 * rng.standard_normal(K)).astype(np.float32)
    bias[:K // 3] *= 0.1
    if zero_lanes is not None:
        for which in range(3):
            W[which * (K // 3) + zero_lanes] = 0.0
            bias[which * (K // 3) + zero_lanes] = 0.0
    return np.ascontiguousarray(rows.reshape(B * T, K)), W, bias


def make_conv(rng):
    """conv [3, 4, 64, 8]: group 0 the identity, groups 1..3 three / five / seven right-aligned random taps and a random bias."""
    conv = np.zeros((3, 4, 64, 8), np.float32)
    conv[:, 0, :, 6] = 1.0
    for g in (1, 2, 3):
        n = 2 * g + 1
        conv[:, g, :, 7 - n:7] = (rng.standard_normal((3, 64, n)) / np.sqrt(n)).astype(np.float32)
        conv[:, g, :, 7] = (0.1 * rng.standard_normal((3, 64))).astype(np.float32)
    return conv


def run_fused(lib, X, W, bias, B, T, heads, lanes, slopes, cos=None, sin=None):
    ctx = np.full((B, T, heads * lanes), np.nan, np.float32)
    _lib.check(lib.pgmi_op_causal_attention(0, lanes, _p(X), _p(W), _p(bias), X.shape[1], None, None, _p(cos), _p(sin), _p(slopes),
                                            B, T, heads, _p(ctx)))
    return ctx


def run_conv(lib, qkv, conv, B, T, heads, slopes, lanes=64):
    ctx = np.full((B, T, heads * lanes), np.nan, np.float32)
    _lib.check(lib.pgmi_op_causal_attention(0, lanes, None, None, None, 0, _p(qkv), _p(conv), None, None, _p(slopes), B, T, heads, _p(ctx)))
    return ctx


def bound(ref, noise32, strict):
    base = 2e-5 * max(1.0, float(np.abs(ref).max()))
    return base if strict else max(base, 3.0 * noise32)


def check_fused(lib, tag, rng, B, T, heads, lanes, rot, slopes, strict, zero_lanes=None):
    X, W, bias = make_fused(rng, make_rows(rng, B, T, heads, lanes), zero_lanes)
    cos, sin = rotary_tables(rot, T, lanes)
    ctx = run_fused(lib, X, W, bias, B, T, heads, lanes, slopes, cos, sin)
    ref = ar.fused_reference(X, W, bias, B, T, heads, lanes, slopes, cos, sin)
    noise32 = float(np.abs(ar.fused_reference(X, W, bias, B, T, heads, lanes, slopes, cos, sin, dtype=np.float32) - ref).max())
    err, tol = float(np.abs(ctx - ref).max()), bound(ref, noise32, strict)
    print(f"causal_att {tag} lanes={lanes} heads={heads} B={B} T={T} rot={rot} err={err:.3e} noise32={noise32:.3e} tol={tol:.3e}")
    assert np.isfinite(ctx).all()
    assert err < tol, (tag, lanes, heads, B, T, rot, err, tol)
    return ctx


def _sweep():
    rots = {64: ["none", "full"], 128: ["none", "full", "partial", "group"], 256: ["full", "none", "group", "partial"]}
    cases = []
    for li, lanes in enumerate((64, 128, 256)):
        odd = 5 if lanes == 64 else 3
        for i, T in enumerate(TS + ([2048] if lanes == 64 else [])):
            for rep in range(1 if T == 2048 else 2):      # two draws of (heads, B, rotary) per width and length
                heads, B = (1, 2, odd)[(i + li + rep) % 3], (1, 2)[(i // 3 + li + rep) % 2]
                if T == 1024:
                    heads, B = (3, 1) if rep == 0 else (2, 2)     # 3 heads: multi-block launches with a partial last group of 8 pairs
                if T == 2048:
                    heads, B = 1, 1
                cases.append((lanes, heads, B, T, rots[lanes][(i + 3 * rep) % len(rots[lanes])]))
        cases.append((lanes, 2, 9, 33, rots[lanes][1]))                                # more than 8 sequences
    cases.append((64, 1, 11, 160, "none"))
    return cases


@pytest.mark.parametrize("lanes,heads,B,T,rot", _sweep())
def test_fused_vs_fp64(lib, lanes, heads, B, T, rot):
    """Every length class (1 / 2 / 4 waves per block, ring wrap, a last query block with fewer tiles than waves, a partial last key tile)
    at every width, no ALiBi (all-zero slopes: RITA, ProtGPT2, ProGen2)."""
    rng = np.random.default_rng(1000 * lanes + 7 * T + heads + B)
    check_fused(lib, "fused", rng, B, T, heads, lanes, rot, np.zeros(heads, np.float32), strict=lanes == 64)


def pg2_holes(dh):
    """Slots of a 128-lane head that no model dim takes (rotate_half_slot, dh > 64 branch, model.h)."""
    taken = {(((j >> 5) & 1)) * 64 + ((j >> 6) << 5) + (j & 31) for j in range(dh)}
    return np.array(sorted(set(range(128)) - taken))


@pytest.mark.parametrize("dh,T", [(80, 97), (96, 257)])
def test_zero_padded_lanes_stay_exactly_zero(lib, dh, T):
    heads, B, lanes = 2, 2, 128
    holes = pg2_holes(dh)
    assert len(holes) == 128 - dh
    cols = np.concatenate([h * lanes + holes for h in range(heads)])
    ctx = check_fused(lib, f"pad{dh}", np.random.default_rng(dh), B, T, heads, lanes, "partial", np.zeros(heads, np.float32), strict=False,
                      zero_lanes=cols)
    assert np.all(ctx[..., cols] == 0.0)
    keep = np.setdiff1d(np.arange(heads * lanes), cols)
    assert np.abs(ctx[..., keep]).min() > 0.0


ALIBI = {
    "tranception8": lambda: tranception_slopes(8),
    # base-2 maximum per 32-key tile: + ~1 and + ~3.9 (below kAttDefer = 4: the rescale is deferred for tiles on end), + 11.5 (every tile), 0
    "defer": lambda: np.array([1.0 / (32 * LOG2E), 3.9 / (32 * LOG2E), 0.25, 0.0], np.float32),
}


@pytest.mark.parametrize("name", list(ALIBI))
def test_alibi_at_1024_vs_fp64(lib, name):
    slopes = ALIBI[name]()
    check_fused(lib, "alibi_" + name, np.random.default_rng(len(name)), 1, 1024, len(slopes), 64, "none", slopes, strict=False)


@pytest.mark.parametrize("heads", [4, 8])
@pytest.mark.parametrize("T", [33, 70, 129, 1024])
def test_conv_form_vs_fp64(lib, heads, T):
    """Tranception: the depth-wise prep pass (tile edges, the start of sequences 1 .. B - 1) and its grouped ALiBi."""
    B = 3
    rng = np.random.default_rng(10 * T + heads)
    qkv = np.ascontiguousarray(make_rows(rng, B, T, heads, 64).reshape(B * T, -1))
    conv, slopes = make_conv(rng), tranception_slopes(heads)
    ctx = run_conv(lib, qkv, conv, B, T, heads, slopes)
    ref = ar.conv_reference(qkv, conv, B, T, heads, slopes)
    noise32 = float(np.abs(ar.conv_reference(qkv, conv, B, T, heads, slopes, dtype=np.float32) - ref).max())
    err, tol = float(np.abs(ctx - ref).max()), bound(ref, noise32, False)
    head = float(np.abs(ctx[1:, :7] - ref[1:, :7]).max())
    print(f"causal_att conv lanes=64 heads={heads} B={B} T={T} err={err:.3e} rows0-6_of_seq1+={head:.3e} noise32={noise32:.3e} tol={tol:.3e}")
    assert np.isfinite(ctx).all()
    assert head < tol, (heads, T, head, tol)          # no history from the previous sequence's tail
    assert err < tol, (heads, T, err, tol)


def _flavour(lib, flavour, rng, B, T, heads=None):
    """(run(rows) -> ctx, rows, reference(rows, dtype)) of one flavour: fused at 64 (Tranception's slopes) / 128 / 256 lanes, or conv."""
    if flavour == "conv":
        heads = heads or 4
        conv, slopes = make_conv(rng), tranception_slopes(heads)
        rows = make_rows(rng, B, T, heads, 64)

        def run(r):
            return run_conv(lib, np.ascontiguousarray(r.reshape(-1, r.shape[-1])), conv, r.shape[0], r.shape[1], heads, slopes)

        def ref(r, dtype=np.float64):
            return ar.conv_reference(r.reshape(-1, r.shape[-1]), conv, r.shape[0], r.shape[1], heads, slopes, dtype)
        return run, rows, ref
    lanes = int(flavour)
    heads = heads or (4 if lanes == 64 else 2)
    slopes = tranception_slopes(4)[:heads].copy() if lanes == 64 else np.zeros(heads, np.float32)
    rows = make_rows(rng, B, T, heads, lanes)
    _, W, bias = make_fused(rng, rows)
    cos, sin = rotary_tables("group" if lanes > 64 else "full", T, lanes)

    def run(r):
        Tr = r.shape[1]
        return run_fused(lib, np.ascontiguousarray(r.reshape(-1, r.shape[-1])), W, bias, r.shape[0], Tr, heads, lanes, slopes,
                         np.ascontiguousarray(cos[:Tr]), np.ascontiguousarray(sin[:Tr]))

    def ref(r, dtype=np.float64):
        return ar.fused_reference(r.reshape(-1, r.shape[-1]), W, bias, r.shape[0], r.shape[1], heads, lanes, slopes, cos[:r.shape[1]],
                                  sin[:r.shape[1]], dtype)
    return run, rows, ref


FLAVOURS = ["64", "128", "256", "conv"]


@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("Tp,T", [(32, 33), (96, 97), (128, 257), (129, 1024)])
def test_prefix_property(lib, flavour, Tp, T):
    """Rows [0, T') of a run at T against a run at T' on the truncated input: within the bound, and bit for bit where both lengths select
    the same kernel instantiation (module docstring)."""
    run, rows, ref = _flavour(lib, flavour, np.random.default_rng(T + Tp), 2, T)
    short = np.ascontiguousarray(rows[:, :Tp])
    a, b = run(rows)[:, :Tp], run(short)
    r64 = ref(short)
    tol = bound(r64, float(np.abs(ref(short, np.float32) - r64).max()), False)
    diff = float(np.abs(a - b).max())
    lanes = 64 if flavour == "conv" else int(flavour)
    bits = same_instantiation(lanes, Tp, T)
    print(f"causal_att prefix {flavour} T'={Tp} T={T} |diff|max={diff:.3e} tol={tol:.3e} bits_required={bits}")
    assert diff < tol, (flavour, Tp, T, diff, tol)
    if bits:
        assert np.array_equal(a, b), (flavour, Tp, T, diff)


@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("t0", [0, 30, 31, 32, 127])
def test_future_independence(lib, flavour, t0):
    """q, k, v of the tokens after t0 replaced by 1e3: rows <= t0 keep their bits."""
    T = 160
    run, rows, _ = _flavour(lib, flavour, np.random.default_rng(t0), 2, T)
    loud = rows.copy()
    loud[:, t0 + 1:] = 1e3
    a, b = run(rows), run(loud)
    assert np.isfinite(a).all() and np.isfinite(b[:, :t0 + 1]).all()
    assert np.array_equal(a[:, :t0 + 1], b[:, :t0 + 1]), (flavour, t0, float(np.abs(a[:, :t0 + 1] - b[:, :t0 + 1]).max()))


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_batch_invariance(lib, flavour):
    """Sequence b alone has the bits it has inside the batch."""
    run, rows, _ = _flavour(lib, flavour, np.random.default_rng(5), 3, 129)
    full = run(rows)
    for b in range(3):
        assert np.array_equal(full[b], run(np.ascontiguousarray(rows[b:b + 1]))[0]), (flavour, b)


@pytest.mark.parametrize("flavour", ["64", "128", "256"])
def test_grid_order_keeps_the_bits(lib, flavour):
    """att_xcd_local 0 / 1 / -1 on a causal launch of three query blocks, 3 or 4 heads x 3 sequences (a partial last group of 8 pairs)."""
    run, rows, _ = _flavour(lib, flavour, np.random.default_rng(6), 3, 257, heads=3 if flavour != "64" else 4)
    try:
        _lib.check(lib.pgmi_set_option(b"att_xcd_local", 0))
        base = run(rows)
        for value in (1, -1):
            _lib.check(lib.pgmi_set_option(b"att_xcd_local", value))
            assert np.array_equal(run(rows), base), (flavour, value)
    finally:
        lib.pgmi_set_option(b"att_xcd_local", -1)


def test_launcher_refusals_come_back_as_einval(lib):
    rng = np.random.default_rng(7)
    B, T = 1, 40
    conv = make_conv(rng)
    for heads, lanes, msg in ((3, 64, "not a multiple of 4"), (4, 128, "head_dim 128 needs operands from the fused QKV projection"),
                              (2, 256, "head_dim 256 is the causal, fused-QKV")):
        qkv = rng.standard_normal((B * T, 3 * heads * lanes)).astype(np.float32)
        with pytest.raises(_lib.PgmiError, match=msg) as e:
            run_conv(lib, qkv, conv, B, T, heads, np.zeros(heads, np.float32), lanes=lanes)
        assert e.value.code == _lib.EINVAL
    X, W, bias = make_fused(rng, make_rows(rng, B, T, 2, 96))
    with pytest.raises(_lib.PgmiError, match="head_dim=96") as e:
        run_fused(lib, X, W, bias, B, T, 2, 96, np.zeros(2, np.float32))
    assert e.value.code == _lib.EINVAL
    with pytest.raises(_lib.PgmiError, match="multiple of 32") as e:
        run_fused(lib, np.zeros((B * T, 40), np.float32), np.zeros((192, 40), np.float32), np.zeros(192, np.float32), B, T, 1, 64,
                  np.zeros(1, np.float32))
    assert e.value.code == _lib.EINVAL
