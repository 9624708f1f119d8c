"""PoET on the GPU (toy checkpoint of tests/golden/PoET_toy only): the prefix attention op by op against float64, the prompt's own
log-probabilities, variant log-probabilities and scores with and without a prompt against the float64 restatement (tests/poet_ref.py,
pinned to the live reference by tests/test_poet_host.py), bit-identity of a variant's score across batch composition and chunking, the
neighbour counts against the recorded ones, and the CLI's CSV against the recorded reference CSV.

Bounds.  Log-probability rows against float64: flat 1e-4.  Sums over a variant's targets: max(1e-4, 3 noise32), noise32 = the same sums
from the restatement in plain fp32 against float64 (the rule of tests/test_gpu_causal_lm.py).  Context values of the attention op:
max(2e-5 max(1, |ref|max), 3 noise32) with noise32 from the fp32 evaluation of the same attention (the rule of
tests/test_gpu_causal_attention.py).  Every test prints its figures before it asserts."""
import ctypes as C
import os

import numpy as np
import pandas as pd
import pytest
import torch

import poet_ref
from proteingym_amd import _lib, poet

pytestmark = pytest.mark.gpu
TOY = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "PoET_toy")
CONTEXT_LENGTHS = (60, 150, 400)
LENS = (1, 2, 31, 32, 33, 70)


def _p(a):
    return None if a is None else a.ctypes.data_as(_lib._f32p if a.dtype == np.float32 else _lib._i32p)


# ---- the attention op ------------------------------------------------------------------------------------------------------
def att_reference(qkv, seg_off, prefix, heads, dtype):
    """ctx [rows, heads * 64]: per segment, softmax over [the prefix keys, the segment's keys up to the query]"""
    Da = heads * 64
    x = qkv.astype(dtype)
    out = np.empty((x.shape[0], Da), dtype)
    pk = prefix.astype(dtype)[:, :Da] if prefix is not None else np.zeros((0, Da), dtype)
    pv = prefix.astype(dtype)[:, Da:] if prefix is not None else np.zeros((0, Da), dtype)
    P = pk.shape[0]
    for b in range(len(seg_off) - 1):
        s, e = seg_off[b], seg_off[b + 1]
        n = e - s
        for h in range(heads):
            c = slice(h * 64, h * 64 + 64)
            q = x[s:e, c]
            k = np.concatenate([pk[:, c], x[s:e, Da:2 * Da][:, c]])
            v = np.concatenate([pv[:, c], x[s:e, 2 * Da:][:, c]])
            sc = q @ k.T
            mask = np.concatenate([np.ones((n, P), bool), np.tril(np.ones((n, n), bool))], axis=1)
            sc = np.where(mask, sc, -np.inf)
            p = np.exp(sc - sc.max(axis=1, keepdims=True))
            out[s:e, c] = (p / p.sum(axis=1, keepdims=True)) @ v
    return out


def att_rows(rng, n, heads, spike=True):
    Da = heads * 64
    x = rng.standard_normal((n, 3 * Da)).astype(np.float32)
    x[:, :Da] *= 0.4
    x[:, 2 * Da:] += rng.choice([0.0, 1e-3, 5.0], size=(n, 1)).astype(np.float32)
    if spike and n > 2:
        x[(2 * n) // 3, :Da] *= 6.0                              # the running maximum jumps
        x[n - 2, Da:2 * Da] *= 6.0                               # a spiky key near the end ...
        x[n - 2, 2 * Da:] = 5.0                                  # ... whose V row is 5
    return x


def run_att(lib, qkv, seg_off, prefix, heads, split):
    ctx = np.full((qkv.shape[0], heads * 64), np.nan, np.float32)
    so = np.ascontiguousarray(seg_off, dtype=np.int32)
    _lib.check(lib.pgmi_op_prefix_attention(0, _p(qkv), _p(so), len(so) - 1, _p(prefix), 0 if prefix is None else prefix.shape[0], heads,
                                            int(split), _p(ctx)))
    return ctx


def check_att(lib, tag, rng, lens, P, heads, split):
    seg_off = np.concatenate([[0], np.cumsum(lens)])
    qkv = np.concatenate([att_rows(rng, n, heads) for n in lens])
    prefix = np.ascontiguousarray(att_rows(rng, P, heads)[:, heads * 64:]) if P else None
    ctx = run_att(lib, qkv, seg_off, prefix, heads, split)
    ref = att_reference(qkv, seg_off, prefix, heads, np.float64)
    noise32 = float(np.abs(att_reference(qkv, seg_off, prefix, heads, np.float32) - ref).max())
    err, tol = float(np.abs(ctx - ref).max()), max(2e-5 * max(1.0, float(np.abs(ref).max())), 3.0 * noise32)
    print(f"prefix_att {tag} P={P} lens={list(lens)} heads={heads} split={split} err={err:.3e} noise32={noise32:.3e} tol={tol:.3e}")
    assert np.isfinite(ctx).all(), (tag, P, lens)
    assert err < tol, (tag, P, lens, heads, split, err, tol)
    return qkv, prefix, ctx


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("P", [0, 1, 31, 32, 33, 97])
def test_prefix_attention_against_float64(lib, P, split):
    """B = 1 at every own length, B = 5 and all six lengths mixed in one launch; 3 heads (a padded head group of the XCD-local order)."""
    rng = np.random.default_rng(1000 + 7 * P + split)
    for n in LENS:
        check_att(lib, "single", rng, [n], P, 3, split)
    check_att(lib, "mixed5", rng, [70, 1, 33, 2, 32], P, 3, split)
    check_att(lib, "mixed6", rng, [33, 70, 2, 31, 1, 32], P, 3, split)


def test_prefix_attention_many_short_segments_and_more_than_eight_heads(lib):
    """A prompt-like launch of many one- and two-token segments (every query tile holds one or two rows), and 9 heads (two head groups)."""
    rng = np.random.default_rng(5)
    check_att(lib, "short", rng, [1, 2] * 20 + [1], 0, 3, 1)
    check_att(lib, "short+prefix", rng, [2, 1] * 9, 33, 3, 1)
    check_att(lib, "heads9", rng, [33, 2, 70], 97, 9, 1)
    check_att(lib, "long", rng, [300], 200, 2, 0)               # ten own key tiles, seven prefix tiles: the LDS stages wrap


def test_prefix_attention_row_does_not_depend_on_its_neighbours(lib):
    """A segment alone, first, last and in the middle of a launch: the same bits."""
    rng = np.random.default_rng(9)
    heads, P = 2, 97
    prefix = np.ascontiguousarray(att_rows(rng, P, heads)[:, heads * 64:])
    segs = [att_rows(rng, n, heads) for n in (33, 70, 5, 64)]
    alone = [run_att(lib, s, [0, len(s)], prefix, heads, 1) for s in segs]
    for order in ([0, 1, 2, 3], [3, 2, 1, 0], [1, 0, 3]):
        off = np.concatenate([[0], np.cumsum([len(segs[i]) for i in order])])
        ctx = run_att(lib, np.concatenate([segs[i] for i in order]), off, prefix, heads, 1)
        for j, i in enumerate(order):
            assert np.array_equal(ctx[off[j]:off[j + 1]], alone[i]), (order, i)


def test_prefix_attention_refuses_bad_arguments(lib):
    q = np.zeros((4, 3 * 64), np.float32)
    assert lib.pgmi_op_prefix_attention(0, _p(q), _p(np.array([0, 2, 2, 4], np.int32)), 3, None, 0, 1, 0, _p(np.zeros((4, 64), np.float32))) == _lib.EINVAL
    assert b"empty" in lib.pgmi_last_error()


# ---- the model -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def toy():
    ckpt = torch.load(os.path.join(TOY, "poet_toy.ckpt"), map_location="cpu", weights_only=True)
    sd = {k.split(".", 1)[1]: v.float().numpy() for k, v in ckpt["state_dict"].items()}
    cfg, blob = poet.load_checkpoint(os.path.join(TOY, "poet_toy.ckpt"))
    g = np.load(os.path.join(TOY, "golden_poet.npz"))
    variants = [poet.frame(s) for s in pd.read_csv(os.path.join(TOY, "TOY_POET.csv"))["mutated_sequence"]]
    prompts = {k: np.split(g[f"prompt_tokens_{k}"], np.cumsum(g[f"prompt_lens_{k}"])[:-1]) for k in (0, 7, 12)}
    return dict(cfg=cfg, blob=blob, g=g, variants=variants, prompts=prompts, ref64=poet_ref.PoetRef(cfg, sd, torch.float64),
                ref32=poet_ref.PoetRef(cfg, sd, torch.float32))


@pytest.fixture(scope="module")
def model(toy):
    m = poet.PoetModel(toy["cfg"], toy["blob"], max_rows=4096, max_prompt=1024)
    yield m
    m.close()


@pytest.fixture(scope="module")
def refs(toy):
    """The float64 / fp32 restatement of prompt 12 (417 tokens, 10 sequences): computed once, shared, never changed."""
    p = toy["prompts"][12]
    lp64, mem64 = toy["ref64"].prompt(p)
    lp32, mem32 = toy["ref32"].prompt(p)
    return dict(prompt=p, lp64=lp64, mem64=mem64, lp32=lp32, mem32=mem32)


def test_prompt_logprobs(model, toy, refs):
    model.set_prompt(refs["prompt"])
    lp = model.prompt_logprobs()
    err = float(np.abs(lp - refs["lp64"]).max())
    print(f"poet prompt logprobs rows={lp.shape[0]} err={err:.3e} noise32={float(np.abs(refs['lp32'] - refs['lp64']).max()):.3e}")
    assert lp.shape == refs["lp64"].shape and err <= 1e-4, err


def test_prompt_of_one_and_two_token_sequences(model, toy):
    """Segments shorter than any tile, and a prompt that is one single sequence."""
    rng = np.random.default_rng(2)
    for tag, p in (("short", [rng.integers(0, 20, n).astype(np.int64) for n in [1, 2] * 17 + [1]]),
                   ("one", [poet.frame("ACDEFGHIKLMNPQRSTVWY" * 4).astype(np.int64)])):
        model.set_prompt(p)
        ref = toy["ref64"].prompt(p)[0]
        err = float(np.abs(model.prompt_logprobs() - ref).max())
        print(f"poet prompt {tag} rows={ref.shape[0]} err={err:.3e}")
        assert err <= 1e-4, (tag, err)


@pytest.mark.parametrize("with_prompt", [True, False])
def test_variant_logprobs_and_scores(model, toy, refs, with_prompt):
    model.set_prompt(refs["prompt"] if with_prompt else [])
    mem64, mem32 = (refs["mem64"], refs["mem32"]) if with_prompt else (None, None)
    V = toy["variants"]
    lp = model.token_logprobs(V)
    s = model.sequence_loglik(V)
    for i, v in enumerate(V):
        ref = toy["ref64"].variant_logprobs(v, mem64)
        err = float(np.abs(lp[i, :len(v)] - ref).max())
        want, want32 = toy["ref64"].score(v, mem64), toy["ref32"].score(v, mem32)
        noise32 = abs(want32 - want)
        serr, tol = abs(s[i] - want), max(1e-4, 3 * noise32)
        print(f"poet variant {i} prompt={with_prompt} len={len(v)} lp_err={err:.3e} score_err={serr:.3e} noise32={noise32:.3e} tol={tol:.3e}")
        assert err <= 1e-4, (i, err)
        assert np.isnan(lp[i, len(v):]).all()
        assert serr <= tol, (i, serr, tol)


def test_score_bits_do_not_depend_on_batch_or_chunking(toy, refs):
    """One variant alone, among others in either order, twice in one call, and with a workspace so small that the call is cut into
    several chunks: the same float64 bits."""
    V = toy["variants"]
    big = poet.PoetModel(toy["cfg"], toy["blob"], max_rows=4096, max_prompt=1024)
    small = poet.PoetModel(toy["cfg"], toy["blob"], max_rows=2048, max_prompt=1024)
    try:
        for m in (big, small):
            m.set_prompt(refs["prompt"])
        alone = big.sequence_loglik([V[5]])[0]
        mixed = big.sequence_loglik(V + [V[5]])
        rev = big.sequence_loglik(V[::-1])
        many = V * 6                                             # 66 variants of ~42 rows, 64 padded key rows each: 3 chunks at 2048 rows
        chunked = small.sequence_loglik(many)
        assert alone == mixed[5] == mixed[-1] == rev[len(V) - 1 - 5], (alone, mixed[5], mixed[-1], rev[len(V) - 1 - 5])
        assert np.array_equal(chunked, np.tile(mixed[:len(V)], 6))
        assert np.array_equal(big.score(V), mixed[:len(V)].astype(np.float32))
    finally:
        big.close()
        small.close()


def test_prompt_longer_than_announced_is_refused(toy):
    m = poet.PoetModel(toy["cfg"], toy["blob"], max_rows=2048, max_prompt=100)
    try:
        with pytest.raises(_lib.PgmiError, match="max_positions = 100") as e:
            m.set_prompt(toy["prompts"][7])
        assert e.value.code == _lib.EINVAL
        m.set_prompt(toy["prompts"][0])                          # 84 tokens fit
        assert m.prompt_logprobs().shape == (84, 24)
    finally:
        m.close()


def test_head_dim_128_is_refused(toy):
    cfg = dict(toy["cfg"], heads=1)
    with pytest.raises(_lib.PgmiError, match="head dims up to 64"):
        poet.PoetModel(cfg, toy["blob"], max_rows=2048)


def test_neighbor_counts_equal_the_recorded_ones(toy):
    msa = toy["g"]["msa"]
    assert np.array_equal(poet.neighbor_counts(msa), toy["g"]["neighbors"])
    for theta in (0.0, 0.35, 1.0):                               # the float64 predicate itself, at other thresholds
        m = msa.astype(np.int64)
        masked = np.where(m == poet.GAP, 255, m)
        sim = (m[:, None] == masked).sum(axis=2) / (m != poet.GAP).sum(axis=1, keepdims=True)
        assert np.array_equal(poet.neighbor_counts(msa, theta), ((1 - sim) <= theta).sum(axis=1)), theta
    gaps = msa.copy()
    gaps[3] = poet.GAP
    with pytest.raises(_lib.PgmiError, match="no non-gap symbol"):
        poet.neighbor_counts(gaps)


@pytest.mark.parametrize("relative", [False, True])
def test_cli_csv_matches_the_recorded_reference(toy, tmp_path, relative):
    from proteingym_amd import score_poet_proteingym as cli
    argv = ["--checkpoint", os.path.join(TOY, "poet_toy.ckpt"), "--DMS_reference_file_path", os.path.join(TOY, "TOY_POET_REFERENCE.csv"),
            "--DMS_data_folder", TOY, "--DMS_index", "0", "--output_scores_folder", str(tmp_path), "--MSA_folder", TOY,
            "--context_lengths", *map(str, CONTEXT_LENGTHS), "--batch_size", "8"] + (["--relative_to_wt"] if relative else [])
    out = cli.main(argv)
    assert out == os.path.join(str(tmp_path), "TOY_POET.csv")
    df = pd.read_csv(out)
    want = pd.read_csv(os.path.join(TOY, "TOY_POET_scores_relative.csv" if relative else "TOY_POET_scores.csv"))
    assert list(df.columns) == ["mutated_sequence", "PoET_score"] and list(df["mutated_sequence"]) == list(want["mutated_sequence"])
    err = float(np.abs(df["PoET_score"].to_numpy() - want["PoET_score"].to_numpy()).max())
    print(f"poet cli relative={relative} err={err:.3e}")
    # a mean of 30 sums of ~40 fp32-class terms each, reported in float32 (ulp 1.5e-5 at 137): the bound on sums, 1e-4
    assert err <= 1e-4, err


def test_ensemble_members_forward_and_backward(model, toy):
    """Every member's forward and backward sums against the reference's recorded float64 ones (members 0, 7, 12)."""
    V = toy["variants"] + [poet.frame(str(pd.read_csv(os.path.join(TOY, "TOY_POET_REFERENCE.csv"))["target_seq"][0][2:42]))]
    g = toy["g"]
    for k, p in toy["prompts"].items():
        members = []
        poet.ensemble_scores(model, [(None, p)], V, members_out=members)
        fwd, bwd = members[0]
        ef, eb = float(np.abs(fwd - g[f"fwd_{k}"]).max()), float(np.abs(bwd - g[f"bwd_{k}"]).max())
        print(f"poet member {k} fwd_err={ef:.3e} bwd_err={eb:.3e}")
        assert ef <= 1e-4 and eb <= 1e-4, (k, ef, eb)
