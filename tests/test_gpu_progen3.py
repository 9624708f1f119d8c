"""ProGen3 on the GPU (toy checkpoints of tests/golden/ProGen3_toy only): the RMSNorm and the routed expert block op by op against
float64, the model's token log-probabilities, chosen experts and sequence scores against the recording of the live reference, bit-identity
of a row across batch composition, and the CLI's CSV against the recorded scores.

Bounds.  Op outputs and token log-probabilities: the suite's rule bound(ref, noise32) = max(2e-5 max(1, |ref|max), 3 noise32)
(tests/axial_ref.py), with noise32 = the error against float64 of the same computation in fp32 on the same inputs -- for the expert
block the torch fp32 restatement of the reference's eager block, for the model the recorded fp32 reference itself against the float64
restatement (tests/progen3_ref.py).  Chosen experts: equal to the float64 restatement's / the recording's, exactly -- every input keeps
the k-th and the (k+1)-th router probability at least 1e-3 apart (progen3_ref.moe_inputs, make_golden_progen3.py), so no case is left
out.  Sequence scores: the project's flat 1e-4.  Every test prints its figures before it asserts."""
import os

import numpy as np
import pandas as pd
import pytest
import torch

import progen3_ref as R
from axial_ref import bound
from proteingym_amd import _lib, progen3 as pg3

pytestmark = pytest.mark.gpu
TOY = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ProGen3_toy")


def _p(a):
    return None if a is None else a.ctypes.data_as(_lib._f32p if a.dtype == np.float32 else _lib._i32p)


# ---- RMSNorm ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [128, 1280])
@pytest.mark.parametrize("rows", [1, 67])
def test_op_rmsnorm(lib, D, rows):
    rng = np.random.default_rng(31 * D + rows)
    w = (1.0 + 0.2 * rng.standard_normal(D)).astype(np.float32)
    eps = 1e-5
    # rows = 67: row 3 has magnitude 1e-4 (below eps: the output shrinks with it), row 5 magnitude 1e3; rows = 1: the three magnitudes in turn
    for scale in ((1.0,) if rows > 1 else (1.0, 1e-4, 1e3)):
        x = (rng.standard_normal((rows, D)) * scale).astype(np.float32)
        if rows > 1:
            x[3] *= 1e-4
            x[5] *= 1e3
        y = np.empty_like(x)
        _lib.check(lib.pgmi_op_rmsnorm(0, _p(x), _p(w), rows, D, eps, _p(y)))
        ref = R.rmsnorm(x.astype(np.float64), w.astype(np.float64), eps)
        r32 = R.rmsnorm(x, w, np.float32(eps))
        for r in range(rows):
            noise = float(np.abs(r32[r] - ref[r]).max())
            err, b = float(np.abs(y[r] - ref[r]).max()), bound(ref[r], noise)
            if r in (0, 3, 5):
                print(f"rmsnorm D={D} rows={rows} scale={scale:g} row {r}: |ref|max {np.abs(ref[r]).max():.3g} err {err:.3g} noise32 {noise:.3g} bound {b:.3g}")
            assert err <= b, (r, err, b)


# ---- the expert block ------------------------------------------------------------------------------------------------------
def torch_eager_block(h, gate, w1, w3, w2, top_k, gated):
    """model/moe.py SparseMoeBlock.forward restated in torch fp32 on the CPU.  With n_experts == top_k the eager block takes a dense
    shortcut that pairs the j-th LARGEST weight with expert j's output; the sparse loop below, which is also what the megablocks block
    the checkpoints are trained with computes, pairs every weight with its own expert, and that is what the product runs."""
    h, w1, w2 = torch.from_numpy(h), torch.from_numpy(w1), torch.from_numpy(w2)
    w3 = torch.from_numpy(w3) if gated else None
    F = torch.nn.functional

    def mlp(e, x):
        a = F.silu(x @ w1[e].T)
        return (a * (x @ w3[e].T) if gated else a) @ w2[e].T
    E = w1.shape[0]
    if E == 1:
        return mlp(0, h).numpy()
    p = F.softmax(h @ torch.from_numpy(gate).T, dim=-1, dtype=torch.float32)
    wt, sel = torch.topk(p, top_k, dim=-1)
    wt = wt / wt.sum(dim=-1, keepdim=True)
    out = torch.zeros_like(h)
    mask = F.one_hot(sel, num_classes=E).permute(2, 1, 0)
    for e in range(E):
        idx, top_x = torch.where(mask[e])
        if top_x.shape[0]:
            out.index_add_(0, top_x, mlp(e, h[top_x]) * wt[top_x, idx, None])
    return out.numpy()


def run_moe(lib, h, gate, w1, w3, w2, E, k, gated):
    M, D = h.shape
    Fh = w1.shape[1]
    out = np.empty((M, D), np.float32)
    ids = np.full((M, k), -7, np.int32)
    wts = np.empty((M, k), np.float32)
    _lib.check(lib.pgmi_op_moe(0, _p(h), _p(np.ascontiguousarray(gate)), _p(np.ascontiguousarray(w1)), _p(np.ascontiguousarray(w3)),
                               _p(np.ascontiguousarray(w2)), M, D, Fh, E, k, gated, _p(out), _p(ids), _p(wts)))
    return out, ids, wts


@pytest.fixture(scope="module")
def moe_cases():
    """Inputs and references of every op case, computed once."""
    cache = {}

    def get(case):
        if case not in cache:
            M, E, k, gated, special = case
            inp = R.moe_inputs(M, E, k, gated, special)
            ref = R.moe_block(*inp, k, gated)
            n32 = float(np.abs(torch_eager_block(*inp, k, gated) - ref[0]).max())
            cache[case] = (inp, ref, n32)
        return cache[case]
    return get


@pytest.mark.parametrize("case", R.OP_CASES, ids=lambda c: f"M{c[0]}-E{c[1]}k{c[2]}-{'glu' if c[3] else 'mlp'}" + (f"-{c[4]}" if c[4] else ""))
def test_op_moe(lib, moe_cases, case):
    M, E, k, gated, special = case
    (h, gate, w1, w3, w2), (ref, p, ref_ids, ref_w), n32 = moe_cases(case)
    out, ids, wts = run_moe(lib, h, gate, w1, w3, w2, E, k, gated)
    err, b = float(np.abs(out - ref).max()), bound(ref, n32)
    print(f"moe {case}: |ref|max {np.abs(ref).max():.3g} err {err:.3g} noise32 {n32:.3g} bound {b:.3g}"
          + ("" if E == 1 else f" gap {R.router_gap(p, k):.3g} weight err {np.abs(wts - ref_w).max():.3g}"))
    if E > 1:
        assert np.array_equal(ids, ref_ids)
        assert np.abs(wts - ref_w).max() <= 1e-6          # fp32 softmax of O(1) logits and one division: a few ulp of values <= 1
        if special == "empty_expert":
            assert not (ids == 1).any()
        if special == "same_pair":
            assert (np.sort(ids, axis=1) == np.array([2, 5])).all()        # the pair, whichever of the two leads in a row
    assert err <= b


def test_moe_rows_do_not_depend_on_the_batch(lib, moe_cases):
    """The same rows in a batch of 200 and alone give the same bits; two identical runs give the same bits."""
    for case in ((200, 4, 2, 1, None), (200, 8, 2, 0, None)):
        M, E, k, gated, _ = case
        (h, gate, w1, w3, w2), _, _ = moe_cases(case)
        full, ids, wts = run_moe(lib, h, gate, w1, w3, w2, E, k, gated)
        again = run_moe(lib, h, gate, w1, w3, w2, E, k, gated)
        assert np.array_equal(full.view(np.uint32), again[0].view(np.uint32)) and np.array_equal(ids, again[1]) and np.array_equal(wts, again[2])
        for sl in (slice(0, 1), slice(17, 50), slice(199, 200), slice(100, 200, 3)):
            part = run_moe(lib, np.ascontiguousarray(h[sl]), gate, w1, w3, w2, E, k, gated)
            assert np.array_equal(part[0].view(np.uint32), full[sl].view(np.uint32)), sl
            assert np.array_equal(part[1], ids[sl]) and np.array_equal(part[2], wts[sl])


# ---- the model -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(TOY, "golden_progen3.npz"))


@pytest.fixture(scope="module", params=["A", "B"])
def toy(request, lib, golden):
    """(name, model, per direction the float64 restatement's log-probs of every fixture sequence)."""
    name = request.param
    d = os.path.join(TOY, name)
    model = pg3.from_pretrained(d, max_rows=2048)
    c, sd = pg3.load_directory(d)
    cfg = pg3.config_from_json(c)
    sd = {k: np.asarray(v, np.float32) for k, v in sd.items()}
    ref64 = {tag: [R.forward(sd, cfg, pg3.encode(s, rev))[0] for s in golden["sequences"]] for tag, rev in (("fwd", False), ("rev", True))}
    yield name, model, ref64
    model.close()


@pytest.mark.parametrize("tag", ["fwd", "rev"])
def test_token_logprobs_and_experts_match_the_recording(toy, golden, tag):
    name, model, ref64 = toy
    ids, rec = golden[f"ids_{tag}"], golden[f"{name}_logprobs_{tag}"]
    B, T = ids.shape
    lp = model.token_logprobs(ids)
    real = ids != pg3.PAD_ID
    noise = max(float(np.abs(rec[b, :len(r)] - r).max()) for b, r in enumerate(ref64[tag]))
    err, bd = float(np.abs(lp[real] - rec[real]).max()), bound(rec[real], noise)
    print(f"ProGen3 {name} {tag}: |ref|max {np.abs(rec[real]).max():.3g} err {err:.3g} noise32 {noise:.3g} bound {bd:.3g}")
    experts = golden[f"{name}_experts_{tag}"]
    for layer in range(model.cfg["layers"]):
        chosen, w = model.routing(layer, B * T)
        assert np.array_equal(chosen[real.reshape(-1)], experts[layer][real.reshape(-1)]), layer
        assert (chosen[~real.reshape(-1)] == -1).all()                       # <pad> rows are not routed
        p = golden[f"{name}_router_{tag}"][layer].astype(np.float64)
        pw = np.take_along_axis(p, experts[layer], axis=-1)
        assert np.abs(w[real.reshape(-1)] - (pw / pw.sum(-1, keepdims=True))[real.reshape(-1)]).max() <= 1e-5
    assert err <= bd


def test_sequence_scores_match_the_recorded_reference(toy):
    name, model, _ = toy
    for kind in ("sub", "indel"):
        rec = pd.read_csv(os.path.join(TOY, f"scores_{name}_{kind}.csv"))
        dms = pd.read_csv(os.path.join(TOY, f"TOY_PG3_{kind.upper()}.csv"))
        target = pd.read_csv(os.path.join(TOY, "TOY_PG3_REFERENCE.csv"))["target_seq"][0]
        from proteingym_amd.causal_lm import get_mutated_sequence
        seqs = list(dms["mutated_sequence"]) if kind == "indel" else [get_mutated_sequence(target, m) for m in dms["mutant"]]
        ll, ppl = model.score(seqs)
        err = float(np.abs(ll - rec["log_likelihood"].to_numpy()).max())
        print(f"ProGen3 {name} {kind}: max |log_likelihood - reference| {err:.3g}")
        assert err <= 1e-4
        assert np.allclose(ppl, np.exp(-ll.astype(np.float32)), rtol=1e-6)
        small = model.score(seqs, max_batch_tokens=40)                       # another batching: the same bits
        assert np.array_equal(small[0], ll)


def test_a_padded_batch_equals_its_rows_scored_alone(toy, golden):
    name, model, _ = toy
    rows = [pg3.encode(s, rev) for s in golden["sequences"] for rev in (False, True)]
    assert len({len(r) for r in rows}) > 2                                  # unequal lengths: right-padded in one call
    sums, n = model.sequence_loglik(rows)
    for j, r in enumerate(rows):
        s1, n1 = model.sequence_loglik([r])
        assert s1[0].tobytes() == sums[j].tobytes() and n1[0] == n[j] == len(r) - 1, j


@pytest.mark.parametrize("kind", ["sub", "indel"])
def test_cli_csv_matches_the_recorded_reference(lib, tmp_path, kind):
    from proteingym_amd import score_progen3_proteingym as cli
    argv = ["--Progen3_model_name_or_path", os.path.join(TOY, "A_megablocks"), "--DMS_reference_file_path", os.path.join(TOY, "TOY_PG3_REFERENCE.csv"),
            "--DMS_data_folder", TOY, "--DMS_index", "0" if kind == "sub" else "1", "--output_scores_folder", str(tmp_path), "--max_rows", "2048"]
    out = cli.main(argv + (["--indel_mode"] if kind == "indel" else []))
    got, rec = pd.read_csv(out), pd.read_csv(os.path.join(TOY, f"scores_A_{kind}.csv"))
    assert list(got.columns) == ["mutant", "log_likelihood", "perplexity", "DMS_score"] and list(got["mutant"]) == list(rec["mutant"])
    err = float(np.abs(got["log_likelihood"] - rec["log_likelihood"]).max())
    print(f"ProGen3 CLI {kind}: max |log_likelihood - reference| {err:.3g}")
    assert err <= 1e-4
    assert np.allclose(got["perplexity"], rec["perplexity"], rtol=2e-4)      # exp of a value within 1e-4
    assert np.array_equal(got["DMS_score"], rec["DMS_score"])
