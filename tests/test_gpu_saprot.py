"""SaProt on the MI355X against the unmodified reference (Hugging Face EsmForMaskedLM, fp32, CPU) at every frozen shape: the full
log-softmax, the group table of the position-set forwards and the scores; the bits of the kept-row and chunked evaluations; a sequence
that holds token id 32; the CLI end to end on the toy assays through the stand-in Foldseek; the length limit and the fp16 range guard.

Bounds: 1e-4 on every log-probability (DESIGN.md section 3's flat bar).  A score is a sum over its sub-mutations of a difference of two
table entries, each held to 1e-4: 2e-4 x number of sub-mutations."""
import os

import numpy as np
import pandas as pd
import pytest

import saprot_ref
from proteingym_amd import _lib, saprot, synthetic as S
from proteingym_amd import score_saprot_proteingym as cli

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOY_DIR = os.path.join(GOLDEN, "SaProt_toy")
STRUCT_DIR = os.path.join(GOLDEN, "SaProt_structures")
SHAPES = ["toy", "h24", "w650"]
TOL = 1e-4


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLDEN, "golden_saprot.npz"))


def build(g, name, precision="f16x3", max_rows=0, scale_fc1=None):
    if name == "toy" and scale_fc1 is None:
        return saprot.from_pretrained(TOY_DIR, precision=precision, max_rows=max_rows)
    D, H, F, layers, seed = (int(v) for v in g[f"{name}_cfg"])
    cfg = S.saprot_config(D, H, layers, F)
    sd = S.saprot_state_dict(cfg, seed)
    if scale_fc1 is not None:
        sd["esm.encoder.layer.0.intermediate.dense.weight"] = sd["esm.encoder.layer.0.intermediate.dense.weight"] * np.float32(scale_fc1)
    return saprot.from_state_dict(cfg, sd, precision=precision, max_rows=max_rows)


def parsed(g, name):
    muts, seq = [str(m) for m in g[f"{name}_mutants"]], str(g[f"{name}_seq"])
    return saprot.parse_chunk(muts, seq, 1, len(seq))


def all_sets(g, name):
    """The golden's position sets plus one set per residue: several device chunks at 2048 workspace rows."""
    L = len(g[f"{name}_ids"]) - 2
    set_off, set_pos = g[f"{name}_set_off"], g[f"{name}_set_pos"]
    return (np.concatenate([set_off, set_off[-1] + 1 + np.arange(L)]).astype(np.int32),
            np.concatenate([set_pos, 1 + np.arange(L)]).astype(np.int32))


@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
@pytest.mark.parametrize("name", SHAPES)
def test_logprobs_table_and_scores_match_reference(lib, g, name, precision):
    model = build(g, name, precision)
    ids = g[f"{name}_ids"]
    assert (ids == 32).any()                                # an ordinary residue token at ESM's <mask> id
    lp = model.token_logprobs(ids[None])[0]
    err = np.abs(lp - g[f"{name}_lp"]).max()
    print(f"{name} {precision}: max|log-softmax - reference| = {err:.3e}")
    assert err <= TOL
    table = model.group_logprobs(ids, g[f"{name}_set_off"], g[f"{name}_set_pos"])
    err = np.abs(table - g[f"{name}_group_lp"]).max()
    print(f"{name} {precision}: max|group table - reference| = {err:.3e}")
    assert err <= TOL
    pos, wt, mt, off = parsed(g, name)
    scores = model.score_chunk(ids, pos, wt, mt, off)
    excess = np.abs(scores - g[f"{name}_scores"]) / np.diff(off)
    print(f"{name} {precision}: max|score - reference| / sub-mutations = {excess.max():.3e}")
    assert (excess <= 2e-4).all()
    model.close()


def test_bf16_error_is_reported_not_gated(lib, g):
    model = build(g, "toy", "bf16")
    table = model.group_logprobs(g["toy_ids"], g["toy_set_off"], g["toy_set_pos"])
    print(f"toy bf16: max|group table - reference| = {np.abs(table - g['toy_group_lp']).max():.3e} (reported, not gated)")
    assert np.isfinite(table).all()
    model.close()


@pytest.mark.parametrize("name", ["toy", "h24"])
def test_kept_rows_and_chunks_have_the_same_bits(lib, g, name, monkeypatch):
    """The last layer's row-local stages on the kept rows only (the default) against the full evaluation (PGMI_KEEP_ROWS=0, read at
    model creation), and 2048 workspace rows (several device chunks) against the default (one): array_equal."""
    ids = g[f"{name}_ids"]
    set_off, set_pos = all_sets(g, name)
    T64 = (len(ids) + 31) // 32 * 32
    assert (len(set_off) - 1) * T64 > 2 * 2048              # at least three chunks at 2048 rows
    model = build(g, name)
    table = model.group_logprobs(ids, set_off, set_pos)
    model.close()
    n = len(g[f"{name}_set_pos"])
    assert np.abs(table[:n] - g[f"{name}_group_lp"]).max() <= TOL
    small = build(g, name, max_rows=2048)
    assert np.array_equal(small.group_logprobs(ids, set_off, set_pos), table)
    # an entry's bits do not depend on the other sets of the call
    assert np.array_equal(small.group_logprobs(ids, g[f"{name}_set_off"], g[f"{name}_set_pos"]), table[:n])
    small.close()
    monkeypatch.setenv("PGMI_KEEP_ROWS", "0")
    full = build(g, name)
    assert np.array_equal(full.group_logprobs(ids, set_off, set_pos), table)
    full.close()


def test_token_id_32_is_a_residue_not_a_mask(lib, g):
    """Position 4 of the toy sequence holds id 32 ("Ch").  Unmasked, its row matches the reference; in a set of its own it is replaced by
    "#h" like any residue, and the table entry matches the float64 forward of that masked row."""
    ids = g["toy_ids"]
    assert ids[4] == 32
    model = saprot.from_pretrained(TOY_DIR)
    lp = model.token_logprobs(ids[None])[0]
    assert np.abs(lp - g["toy_lp"])[[3, 4, 5]].max() <= TOL
    table = model.group_logprobs(ids, np.array([0, 1, 3], np.int32), np.array([4, 4, 9], np.int32))
    model.close()
    cfg, sd = saprot.load_checkpoint(TOY_DIR)
    blob = saprot.pack(cfg, sd)
    for rows, ps in ((slice(0, 1), [4]), (slice(1, 3), [4, 9])):
        masked = ids.copy()
        masked[ps] = saprot.masked_ids()[ids[ps]]
        want = saprot_ref.group_logprobs(saprot_ref.numpy_forward(cfg, blob, masked))[ps]
        assert np.abs(table[rows] - want).max() <= TOL


def run_cli(tmp_path, index, *extra, reference=None):
    foldseek = saprot_ref.write_stand_in_foldseek(tmp_path)
    dms = tmp_path / "dms"
    dms.mkdir(exist_ok=True)
    for n in ("TOY_SAPROT_ONE", "TOY_SAPROT_TWO"):
        pd.read_csv(os.path.join(GOLDEN, n + ".csv"))[["mutant", "DMS_score"]].to_csv(dms / f"{n}.csv", index=False)
    out = tmp_path / "out"
    rc = cli.main(["--foldseek_bin", foldseek, "--SaProt_model_name_or_path", TOY_DIR, "--DMS_reference_file_path",
                   reference or os.path.join(GOLDEN, "TOY_SAPROT_REFERENCE.csv"), "--DMS_data_folder", str(dms),
                   "--structure_data_folder", STRUCT_DIR, "--DMS_index", str(index), "--output_scores_folder", str(out), *extra])
    assert rc == 0
    return out


@pytest.mark.parametrize("index, name", [(0, "TOY_SAPROT_ONE"), (1, "TOY_SAPROT_TWO")])
def test_cli_matches_reference_csvs(lib, tmp_path, index, name):
    """TOY_SAPROT_TWO's rows alternate between its two chunks: the scores are assigned positionally in chunk order, as the reference
    does, so the golden's row order holds only if that is reproduced."""
    out = run_cli(tmp_path, index)
    got, ref = pd.read_csv(out / f"{name}.csv"), pd.read_csv(os.path.join(GOLDEN, name + ".csv"))
    assert list(got.columns) == list(ref.columns) == ["mutant", "SaProt_score", "DMS_score"]
    assert got["mutant"].tolist() == ref["mutant"].tolist() and got["DMS_score"].tolist() == ref["DMS_score"].tolist()
    if name == "TOY_SAPROT_TWO":                            # per row, the bound of the mutant whose score the row received
        first = np.array([int(m.split(":")[0][1:-1]) for m in ref["mutant"]])
        order = np.concatenate([np.flatnonzero(first <= 40), np.flatnonzero(first > 40)])
        assert not np.array_equal(order, np.arange(len(order)))
        n_sub = np.array([ref["mutant"][i].count(":") + 1 for i in order])
    else:
        n_sub = np.array([m.count(":") + 1 for m in ref["mutant"]])
    assert (np.abs(got["SaProt_score"] - ref["SaProt_score"]).to_numpy() <= 2e-4 * n_sub).all()
    # an existing file is reported and overwritten; fp32 is available from the command line
    again = run_cli(tmp_path, index, "--precision", "fp32")
    assert (np.abs(pd.read_csv(again / f"{name}.csv")["SaProt_score"] - ref["SaProt_score"]).to_numpy() <= 2e-4 * n_sub).all()


def test_cli_row_in_no_chunk_is_a_value_error(lib, tmp_path):
    ref = pd.read_csv(os.path.join(GOLDEN, "TOY_SAPROT_REFERENCE.csv"))
    ref.loc[1, "pdb_file"], ref.loc[1, "pdb_range"] = "toy_saprot_two_1.pdb", "1-40"
    ref.to_csv(tmp_path / "ref.csv", index=False)
    with pytest.raises(ValueError, match="does not match length of index"):
        run_cli(tmp_path, 1, reference=str(tmp_path / "ref.csv"))


def test_over_long_sequence_names_the_limit(lib, g):
    model = build(g, "toy", max_rows=2048)
    ids = np.concatenate([[0], np.resize(g["toy_ids"][1:-1], 2100), [2]]).astype(np.int32)
    for call in (lambda: model.token_logprobs(ids[None]), lambda: model.group_logprobs(ids, [0, 1], [5])):
        with pytest.raises(_lib.PgmiError, match="exceeds workspace rows 2048") as e:
            call()
        assert e.value.code == _lib.EINVAL
    # and the ESM entries refuse the model rather than read its ids as the ESM alphabet's
    out = np.empty((1, 8, 33), dtype=np.float32)
    t = _lib.as_i32(g["toy_ids"][None, :8])
    assert lib.pgmi_token_logprobs(model._h, _lib.ptr(t, _lib._i32p), 1, 8, _lib.ptr(out, _lib._f32p)) == _lib.EINVAL
    model.close()


def test_overflow_through_fc1_trips_the_range_guard(lib, g):
    """FC1 weights of the first layer times 1e6 (its pre-activations are then ~ N(0, 1e12): LayerNorm's unit-variance rows against
    N(0, 1/D) weights): GELU's output, FC2's operand, leaves fp16's 65 504; the NaN / Inf it carries reaches the grouped log-softmax
    and the call returns PGMI_EOVERFLOW (no wrong finite number).  The same weights score in fp32."""
    model = build(g, "h24", scale_fc1=1e6)
    ids = g["h24_ids"]
    for call in (lambda: model.group_logprobs(ids, g["h24_set_off"], g["h24_set_pos"]), lambda: model.token_logprobs(ids[None])):
        with pytest.raises(_lib.PgmiError) as e:
            call()
        assert e.value.code == _lib.EOVERFLOW
    model.close()
    ok = build(g, "h24", "fp32", scale_fc1=1e6)
    assert np.isfinite(ok.group_logprobs(ids, g["h24_set_off"], g["h24_set_pos"])).all()
    ok.close()


def test_create_refusals(lib):
    import ctypes as C
    w = np.zeros(1, dtype=np.float32)
    base = dict(abi_version=_lib.ABI_VERSION, arch=_lib.ARCH_SAPROT, layers=1, embed_dim=128, heads=2, ffn_dim=256, vocab=446,
                precision=_lib.PREC_F16X3)
    h = C.c_void_p()
    assert lib.pgmi_model_create(C.byref(_lib.Config(**base)), _lib.ptr(w, _lib._f32p), 1, 0, C.byref(h)) == _lib.EINVAL
    assert b"pgmi_saprot_model_create" in lib.pgmi_last_error()
    assert lib.pgmi_saprot_model_create(C.byref(_lib.Config(**dict(base, vocab=33))), 4, _lib.ptr(w, _lib._f32p), 1, 0, C.byref(h)) == _lib.EINVAL
    assert b"vocab" in lib.pgmi_last_error()
    cfg = S.saprot_config(64, 1, 1, 64)
    blob = saprot.pack(cfg, S.saprot_state_dict(cfg, 1))
    c = _lib.Config(**dict(base, embed_dim=64, heads=1, ffn_dim=64))
    assert lib.pgmi_saprot_model_create(C.byref(c), 32, _lib.ptr(blob, _lib._f32p), blob.size, 0, C.byref(h)) == _lib.EINVAL
    assert b"<mask> id" in lib.pgmi_last_error()
