"""UniRep on the GPU: pgmi_unirep_* and pgmi_op_mlstm_step against tests/unirep_ref.py in float64.

The live reference did not produce the expected values: TensorFlow is not available where this suite runs, so parity is pinned by the
restatement, which follows the reference's unirep.py / unirep_inference.py line by line from the raw checkpoint arrays (the folding is
under test too).  Checkpoints are seeded (unirep_ref.toy_checkpoint) with gain 1.5, the value tests/test_unirep_host.py derives from
the CPU fp32-vs-fp64 distance of the score.

Bounds: per-op and token quantities within the suite's rule max(2e-5 max(1, |ref|max), 3 noise32) (tests/axial_ref.py bound), noise32 =
the restatement in fp32 on the CPU against itself in float64; Unirep_score within the project's flat 1e-4 of float64.  The prefix
start and the row invariance are equalities of bits."""
import os

import numpy as np
import pandas as pd
import pytest

import unirep_ref as R
from axial_ref import bound
from proteingym_amd import _lib, unirep as ur, score_unirep_proteingym as cli
from test_unirep_host import TARGET, cli_argv, make_toy_assay

pytestmark = pytest.mark.gpu

GAIN = 1.5
AAS = list(R.VALID_AAS)
_files, _models, _refs = {}, {}, {}


def files_of(H):
    if H not in _files:
        _files[H] = R.toy_checkpoint(11 + H, H, GAIN)
    return _files[H]


def model_of(lib, H, precision):
    if (H, precision) not in _models:
        _models[(H, precision)] = ur.UniRepModel(ur.arrays_from_files(files_of(H)), precision=precision)
    return _models[(H, precision)]


@pytest.fixture(scope="module", autouse=True)
def _close_models():
    yield
    for m in _models.values():
        m.close()
    _models.clear()


def seqs_of(seed, lengths):
    rng = np.random.default_rng(seed)
    return ["".join(rng.choice(AAS, L)) for L in lengths]


def model_reference(H, lengths):
    """(sequences, float64 and fp32 token log-probs per sequence, float64 scores), once per shape."""
    key = (H, tuple(lengths))
    if key not in _refs:
        f = files_of(H)
        seqs = seqs_of(100 + H, lengths)
        lp64 = [R.token_logprobs(f, R.format_seq(s)[:-1]) for s in seqs]
        lp32 = [R.token_logprobs(f, R.format_seq(s)[:-1], np.float32) for s in seqs]
        sc = np.array([R.sequence_loss(lp, R.format_seq(s)[1:]) for lp, s in zip(lp64, seqs)])
        _refs[key] = (seqs, lp64, lp32, sc)
    return _refs[key]


def step_reference(H, rows):
    key = ("step", H, rows)
    if key not in _refs:
        f = files_of(H)
        rng = np.random.default_rng(rows * 1000 + H)
        h = rng.uniform(-1, 1, (rows, H)).astype(np.float32)
        c = (rng.choice([-5.0, 5.0], (rows, H)) + rng.normal(0, 0.5, (rows, H))).astype(np.float32)      # saturated tanh
        h[::2] = 0.0                                                                                     # first-step rows
        c[::2] = 0.0
        tok = rng.integers(0, 26, rows).astype(np.int32)
        tok[:3] = [24, 0, 23][:rows]
        E = f["embed_matrix:0.npy"]
        out = {}
        for dt in (np.float64, np.float32):
            out[dt] = R.cell_step(R.effective_weights(f, dt), E[tok].astype(dt), c.astype(dt), h.astype(dt))
        _refs[key] = (h, c, tok, out[np.float64], out[np.float32])
    return _refs[key]


@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
@pytest.mark.parametrize("rows", [1, 3, 130])
@pytest.mark.parametrize("H", [76, 128])
def test_mlstm_step_against_float64(lib, H, rows, precision):
    h0, c0, tok, ref, ref32 = step_reference(H, rows)
    m = model_of(lib, H, precision)
    h, c, z = m.step(h0, c0, tok)
    assert m.Hp == (96 if H == 76 else 128)
    z_ref = np.stack(np.split(ref[2], 4, axis=1), 1)
    z_32 = np.stack(np.split(ref32[2], 4, axis=1), 1)
    for name, got, r64, r32 in (("z", z[:, :, :H], z_ref, z_32), ("c", c[:, :H], ref[1], ref32[1]), ("h", h[:, :H], ref[0], ref32[0])):
        noise = float(np.abs(r32 - r64).max())
        err, tol = float(np.abs(got - r64).max()), bound(r64, noise)
        print(f"mlstm_step {precision} H={H} rows={rows} {name}: err={err:.3e} noise32={noise:.3e} tol={tol:.3e}")
        assert np.isfinite(got).all() and err < tol, (name, err, tol)
    # the padded units stay exactly 0
    assert not h[:, H:].any() and not c[:, H:].any() and not z[:, :, H:].any()


LENGTHS = [1, 2, 37, 37, 5]


@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
@pytest.mark.parametrize("H", [76, 128])
def test_model_against_float64(lib, H, precision):
    seqs, lp64, lp32, sc = model_reference(H, LENGTHS)
    m = model_of(lib, H, precision)
    m.set_target(None)
    for s, r64, r32 in zip(seqs[:3], lp64, lp32):
        got = m.token_logprobs(R.format_seq(s)[:-1])
        noise = float(np.abs(r32 - r64).max())
        err, tol = float(np.abs(got - r64).max()), bound(r64, noise)
        print(f"unirep {precision} H={H} L={len(s)} token log-probs: err={err:.3e} noise32={noise:.3e} tol={tol:.3e}")
        assert got.shape == (len(s), 25) and err < tol
    got = m.nll(seqs)                                     # mixed lengths in one call
    err = float(np.abs(got - sc).max())
    print(f"unirep {precision} H={H} lengths={LENGTHS} scores: err={err:.3e} (bar 1e-4)")
    assert err < 1e-4 and m.last_row_steps == sum(LENGTHS)
    one = np.array([m.nll([s])[0] for s in seqs])
    assert np.array_equal(one, got)


@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
def test_real_width(lib, precision):
    """H = 1900 (padded to 1920), the released shape."""
    seqs, lp64, lp32, sc = model_reference(1900, [24] * 5)
    m = model_of(lib, 1900, precision)
    assert m.Hp == 1920
    got = m.nll(seqs)
    err = float(np.abs(got - sc).max())
    print(f"unirep {precision} H=1900 L=24 scores: err={err:.3e} (bar 1e-4)")
    assert err < 1e-4
    lp = m.token_logprobs(R.format_seq(seqs[0])[:-1])
    noise = float(np.abs(lp32[0] - lp64[0]).max())
    e, tol = float(np.abs(lp - lp64[0]).max()), bound(lp64[0], noise)
    print(f"unirep {precision} H=1900 L=24 token log-probs: err={e:.3e} noise32={noise:.3e} tol={tol:.3e}")
    assert e < tol


def prefix_variants():
    rng = np.random.default_rng(9)
    L = len(TARGET)

    def sub(s, i):
        return s[:i] + str(rng.choice([a for a in AAS if a != s[i]])) + s[i + 1:]

    out = [TARGET, sub(TARGET, 0), sub(TARGET, L - 1), sub(TARGET, L // 2), TARGET[:12] + "W" + TARGET[12:], TARGET[:20] + TARGET[21:]]
    out += [sub(TARGET, int(i)) for i in rng.integers(0, L, 34)]
    for _ in range(20):
        s = TARGET
        for i in rng.choice(L, 3, replace=False):
            s = sub(s, int(i))
        out.append(s)
    return out


@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
def test_prefix_start_is_exact(lib, precision):
    m = model_of(lib, 76, precision)
    seqs = prefix_variants()
    assert len(seqs) == 60
    m.set_target(TARGET)
    shared = m.nll(seqs)
    n_shared = m.last_row_steps
    scratch = m.nll(seqs, from_scratch=True)
    n_scratch = m.last_row_steps
    p_shared, p_scratch = m.plan(seqs), m.plan(seqs, from_scratch=True)
    print(f"unirep {precision} prefix start: row-steps {n_shared} shared, {n_scratch} from scratch (planner {p_shared.row_steps}, "
          f"{p_scratch.row_steps}); max |score - float64| = {np.abs(shared - R.scores(files_of(76), seqs)).max():.3e}")
    assert np.array_equal(shared, scratch)
    assert n_shared == p_shared.row_steps and n_scratch == p_scratch.row_steps == sum(len(s) for s in seqs)
    assert n_shared < n_scratch
    assert np.abs(shared - R.scores(files_of(76), seqs)).max() < 1e-4
    m.set_target(None)
    assert np.array_equal(m.nll(seqs), scratch) and m.last_row_steps == n_scratch


@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
def test_row_invariance(lib, precision):
    m = model_of(lib, 76, precision)
    m.set_target(None)
    seqs = seqs_of(3, [37] * 130)
    batch = m.nll(seqs)
    assert m.nll([seqs[0]])[0] == batch[0] and m.nll([seqs[77]])[0] == batch[77]
    assert np.array_equal(m.nll(seqs[::-1])[::-1], batch)
    try:
        _lib.check(lib.pgmi_set_option(b"unirep_max_rows", 17))          # several chunks
        assert np.array_equal(m.nll(seqs), batch)
        m.set_target(seqs[5])
        assert np.array_equal(m.nll(seqs), batch)
    finally:
        lib.pgmi_set_option(b"unirep_max_rows", 0)
        m.set_target(None)


@pytest.mark.parametrize("evotune", [False, True])
def test_cli_end_to_end(lib, tmp_path, evotune):
    root = str(tmp_path / "toy")
    make_toy_assay(root, H=44)
    out = cli.main(cli_argv(root, "evo" if evotune else "base", str(tmp_path / "out"), *(["--evotune"] if evotune else [])))
    got = pd.read_csv(out)
    path = os.path.join(root, "evo", "TOY_UR_MSA") if evotune else os.path.join(root, "base")
    ref = R.scores(R.load_arrays(path), list(got["mutated_sequence"]))
    err = float(np.abs(got["Unirep_score"].values - ref).max())
    print(f"unirep CLI evotune={evotune}: {len(got)} sequences, max |score - float64| = {err:.3e}")
    assert list(got.columns) == ["mutated_sequence", "Unirep_score"] and os.path.basename(out) == "TOY_UR.csv" and err < 1e-4


def test_refusals(lib, tmp_path):
    arrays = ur.arrays_from_files(files_of(76))
    with pytest.raises(_lib.PgmiError, match="bf16"):
        ur.UniRepModel(arrays, precision="bf16")
    bad = dict(arrays, wh=arrays["wh"][:, :-1])
    with pytest.raises(_lib.PgmiError, match="shape"):
        ur.UniRepModel(bad)
    R.save_checkpoint(str(tmp_path / "ck"), {k: v for k, v in files_of(76).items() if "gmx" not in k})
    with pytest.raises(_lib.PgmiError, match="gmx"):
        ur.from_pretrained(str(tmp_path / "ck"))
    m = model_of(lib, 76, "f16x3")
    for toks in ([24, 1, 26], [24, -1, 3]):
        with pytest.raises(_lib.PgmiError, match="token") as e:
            m.nll_tokens([np.array(toks)])
        assert e.value.code == _lib.EINVAL
    with pytest.raises(_lib.PgmiError, match="token"):
        m.token_logprobs([24, 30])
    with pytest.raises(_lib.PgmiError, match="tokens"):
        m.nll_tokens([np.array([24])])
    assert np.isfinite(m.nll(["MKV"])).all()                  # the handle still works
