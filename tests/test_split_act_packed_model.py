"""The f16x3 activation split, one value at a time (common.h split_act) and four at a time (split_act4), as numpy models of the two
instruction sequences: identical (hi, lo) pairs.

split_act:   hi = |x| < 2^-14 ? 0 : fp16(x);        lo = fp16((x - hi) * 2^11)                     (fp32 subtract, fp32 multiply)
split_act4:  hi = fp16(|x| < 2^-14 ? 0 : x);        lo = fp16(fma(hi, -2^11, x * 2^11))            (fp32 multiply, one fused multiply-add)

x - hi is exact in fp32 (hi is x rounded to 11 bits, or 0) and so are both scalings by 2^11, so the fma has nothing to round.  The
one place where the forms part is |x| >= 2^117, where x * 2^11 overflows: hi is +-inf in both, lo is -+inf in the old form and NaN in the
new one -- non-finite either way, which is all the fp16 range guard downstream asks of a value 30 orders of magnitude beyond fp16."""
import numpy as np

TINY = np.float32(2.0 ** -14)
K = np.float32(2048.0)


def split_old(x):
    with np.errstate(all="ignore"):
        hi = np.where(np.abs(x) < TINY, np.float16(0), x.astype(np.float16))
        lo = ((x - hi.astype(np.float32)) * K).astype(np.float16)
    return hi, lo


def split_new(x):
    with np.errstate(all="ignore"):
        hi = np.where(np.abs(x) < TINY, np.float32(0), x).astype(np.float16)
        xs = x * K                                                              # fp32
        # fma(hi, -2048, xs): the product is exact in float64 and so is its sum with xs (both are fp32 values whose exponents lie within
        # 53 bits of each other whenever the sum is not simply one of them), so ONE rounding to fp32 -- what the fused operation does
        lo32 = (hi.astype(np.float64) * -2048.0 + xs.astype(np.float64)).astype(np.float32)
        lo = lo32.astype(np.float16)
    return hi, lo


def same(a, b):
    """bit-identical, any NaN equal to any NaN"""
    nan = np.isnan(a) & np.isnan(b)
    return bool((nan | (a.view(np.uint16) == b.view(np.uint16))).all())


def edge_values():
    f = np.float32
    vals = [0.0, -0.0, 1e-45, -1e-45, 1e-40, 2.0 ** -126, 2.0 ** -36, 2.0 ** -26, 2.0 ** -25, 2.0 ** -24, 3e-8, 2.0 ** -15,
            1.0, 1.0 + 2.0 ** -11, 1.0 + 2.0 ** -12, 1.0 - 2.0 ** -12, 0.1, 1 / 3, 2047.5, 65504.0, 65519.99, 65520.0, 65536.0, 1e5, 1e10,
            1e30, 2.0 ** 116, np.inf, np.nan]
    for c in (2.0 ** -14, 65504.0, 65520.0, 2.0 ** -25):                        # +- 1, 2 ulp around the thresholds
        for steps in (-2, -1, 1, 2):
            v = f(c)
            for _ in range(abs(steps)):
                v = np.nextafter(v, f(np.inf) if steps > 0 else f(0))
            vals.append(float(v))
    x = np.array(vals, np.float32)
    return np.concatenate([x, -x])


def test_packed_split_gives_the_pairs_of_the_scalar_split():
    rng = np.random.default_rng(0)
    bits = rng.integers(0, 2 ** 32, size=500_000, dtype=np.uint64).astype(np.uint32).view(np.float32)      # every exponent, NaNs, infinities
    bits = bits[~(np.abs(bits) >= np.float32(2.0 ** 117))]                                                  # the documented overflow region: below
    acts = (rng.standard_normal(300_000) * rng.choice([1e-6, 1e-4, 1e-2, 1.0, 30.0, 3e4], size=300_000)).astype(np.float32)
    near = (rng.uniform(-2.0, 2.0, 300_000) * 2.0 ** -14).astype(np.float32)                                # around the flush threshold
    x = np.concatenate([bits, acts, near, edge_values()])
    assert x.size >= 10 ** 6
    (h0, l0), (h1, l1) = split_old(x), split_new(x)
    assert same(h0, h1) and same(l0, l1)
    # what the split is for: hi + lo 2^-11 gives x back to 22 bits wherever fp16 holds it
    ok = np.isfinite(x) & (np.abs(x) <= 65504) & (np.abs(x) >= 2.0 ** -14)
    back = h1[ok].astype(np.float64) + l1[ok].astype(np.float64) / 2048.0
    assert (np.abs(back - x[ok]) <= np.abs(x[ok]) * 2.0 ** -22).all()
    assert not (h1[np.abs(x) < TINY] != 0).any()                                                            # flushed, never an fp16 subnormal


def test_beyond_the_scaling_range_both_splits_are_non_finite():
    x = np.array([2.0 ** 117, 3e38, -(2.0 ** 117), -3e38, np.inf, -np.inf, np.nan], np.float32)
    for hi, lo in (split_old(x), split_new(x)):
        assert not np.isfinite(hi).any() and not np.isfinite(lo).any()
