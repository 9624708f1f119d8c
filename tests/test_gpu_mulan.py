"""MULAN on the MI355X against the float64 restatement (tests/mulan_ref.py; test_mulan_host.py pins it to the installed transformers'
ESM modules): the log-probability tables of the position-set forwards and the scores on both toy checkpoints at T = 19 and T = 70 (the
second crosses a 64-key attention tile); the adapter alone in front of a one-layer stack, zeroed and not, against the restatement with
and without rotary in the adapter; the bits of the explicit-row, kept-row and chunked evaluations; a masked low-pLDDT residue; the
CLI end to end from the structure files and from the cached dataset folder; the refusals.

Bounds: 1e-4 on every log-probability (DESIGN.md section 3's flat bar).  A score is a sum over its sub-mutations of a difference of two
table entries, each held to 1e-4: 2e-4 x number of sub-mutations."""
import ctypes as C
import os

import numpy as np
import pandas as pd
import pytest

import mulan_ref
from proteingym_amd import _lib, esm as pesm, mulan, saprot, synthetic as S
from proteingym_amd import score_mulan_proteingym as cli

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOY = os.path.join(GOLDEN, "MULAN_toy")
STRUCT_DIR = os.path.join(GOLDEN, "MULAN_structures")
DATASET = os.path.join(GOLDEN, "MULAN_dataset")
REFERENCE = os.path.join(GOLDEN, "TOY_MULAN_REFERENCE.csv")
TOL = 1e-4
# (checkpoint, dataset entry): T = 19 and T = 70 for each
CASES = [("plain", "toy_mulan_a"), ("plain", "toy_mulan_b"), ("foldseek", "toy_mulan_a"), ("foldseek", "toy_mulan_c")]
# residues with pLDDT <= 70 per entry (make_golden_mulan.py), 0-based; the sets below mask some of them
LOW = {"toy_mulan_a": [3, 4, 9], "toy_mulan_b": [0, 20, 21, 50, 67], "toy_mulan_c": [5, 6, 44]}


def sets_of(entry, L):
    """Singles (among them low-pLDDT residues, the first and the last residue), doubles and triples that share positions: CSR over
    token positions (1 + residue index)."""
    low = LOW[entry]
    groups = [[1], [L], [low[0] + 1], [low[1] + 1], [2], [L // 2], [low[0] + 1, low[1] + 1], [2, low[0] + 1, L // 2], [1, L], [2, L // 2],
              [low[1] + 1, low[2] + 1, L]]
    groups = [sorted(set(g)) for g in groups]
    off = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int32)
    return off, np.concatenate(groups).astype(np.int32)


class Case:
    """One (checkpoint, structure) pair with its float64 tables, computed once for the module."""

    def __init__(self, name, entry):
        self.name, self.entry, self.fs = name, entry, name == "foldseek"
        self.cfg, self.sd = mulan.load_checkpoint(os.path.join(TOY, name), self.fs)
        self.blob = mulan.pack(self.cfg, self.sd)
        seq, rows = mulan.load_dataset_folder(DATASET, self.fs)[entry]
        self.ids = mulan.tokenize(seq, self.fs)
        self.angles, self.plddt = mulan.chunk_features(rows)
        self.L = len(self.ids) - 2
        self.set_off, self.set_pos = sets_of(entry, self.L)
        self.table = mulan_ref.set_table(self.cfg, self.blob, self.ids, self.angles, self.plddt, self.set_off, self.set_pos)
        self.lp = mulan_ref.log_softmax(mulan_ref.numpy_logits(self.cfg, self.blob, self.ids, mulan_ref.collate(self.angles, self.plddt)))
        letters = seq[0::2] if self.fs else seq
        aas = "ACDEFGHIKLMNPQRSTVWY"
        self.target = letters.replace("X", "M")
        sub = lambda p: f"{self.target[p - 1]}{p}{aas[(aas.index(self.target[p - 1]) + 3) % 20]}"          # noqa: E731
        self.mutants = [":".join(sub(int(p)) for p in self.set_pos[self.set_off[s]:self.set_off[s + 1]]) for s in range(len(self.set_off) - 1)]
        vocab = saprot.vocabulary() if self.fs else list(pesm.VOCABULARY)
        self.scores = mulan_ref.scores(self.cfg, self.blob, self.ids, self.angles, self.plddt, self.mutants, 1, vocab)

    def build(self, precision="f16x3", max_rows=0):
        m = mulan.Mulan(self.cfg, self.blob, precision=precision, max_rows=max_rows)
        m.set_structure(self.angles, self.plddt)
        return m


@pytest.fixture(scope="module")
def cases():
    return {c: Case(*c) for c in CASES}


@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-{c[1][-1]}")
def test_tables_and_scores_match_the_restatement(lib, cases, case, precision):
    c = cases[case]
    assert len(c.ids) == (19 if case[1].endswith("a") else 70)
    model = c.build(precision)
    lp = model.token_logprobs(c.ids[None])[0]
    err = np.abs(lp - c.lp).max()
    print(f"{case} {precision}: max|log-softmax - restatement| = {err:.3e}")
    assert err <= TOL
    table = model.set_logprobs(c.ids, c.set_off, c.set_pos)
    assert table.shape == c.table.shape == (len(c.set_pos), 21 if c.fs else 33)
    err = np.abs(table - c.table).max()
    print(f"{case} {precision}: max|set table - restatement| = {err:.3e}")
    assert err <= TOL
    parsed = mulan.parse_chunk(c.mutants, c.target, 1, c.L, c.fs)
    scores = model.score_chunk(c.ids, c.angles, c.plddt, *parsed)
    excess = np.abs(scores - c.scores) / np.diff(parsed[3])
    print(f"{case} {precision}: max|score - restatement| / sub-mutations = {excess.max():.3e}")
    assert (excess <= 2e-4).all()
    model.close()


def test_bf16_error_is_reported_not_gated(lib, cases):
    c = cases[("plain", "toy_mulan_b")]
    model = c.build("bf16")
    table = model.set_logprobs(c.ids, c.set_off, c.set_pos)
    print(f"plain T=70 bf16: max|set table - restatement| = {np.abs(table - c.table).max():.3e} (reported, not gated)")
    assert np.isfinite(table).all()
    model.close()


@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
def test_adapter_alone_contributes_and_has_no_rotary(lib, cases, precision):
    """A one-layer main stack behind the adapter (a stack of no layers is not constructible).  With the adapter's final LayerNorm
    zeroed the structure rows are exactly 0 and the model is its main stack; with it on, the device follows the restatement WITHOUT
    rotary in the adapter and is far from the one with it, on the same input."""
    c = cases[("plain", "toy_mulan_b")]
    cfg = S.mulan_config(64, 4, 1, 256)
    masked = [3, 21, 40]
    ids = c.ids.copy()
    ids[masked] = cfg["mask_token_id"]
    struct_inputs = mulan_ref.collate(c.angles, c.plddt, masked)
    off, pos = np.array([0, 3], np.int32), np.array(masked, np.int32)
    out = {}
    for scale in (0.0, 1.0):
        blob = mulan.pack(cfg, S.mulan_state_dict(cfg, 31, adapter_scale=scale))
        model = mulan.Mulan(cfg, blob, precision=precision)
        model.set_structure(c.angles, c.plddt)
        out[scale] = model.token_logprobs(ids[None], off, pos)[0]
        model.close()
        want = mulan_ref.log_softmax(mulan_ref.numpy_logits(cfg, blob, ids, struct_inputs))
        err = np.abs(out[scale] - want).max()
        print(f"adapter x{scale} {precision}: max|log-softmax - restatement| = {err:.3e}")
        assert err <= TOL
        if scale:
            wrong = mulan_ref.log_softmax(mulan_ref.numpy_logits(cfg, blob, ids, struct_inputs, adapter_rotary=True))
            print(f"adapter x{scale} {precision}: distance to the rotary-adapter model = {np.abs(out[scale] - wrong).max():.3e}")
            assert np.abs(out[scale] - wrong).max() >= 100 * TOL
    assert np.abs(out[1.0] - out[0.0]).max() >= 100 * TOL    # the adapter contributes


@pytest.mark.parametrize("name", ["plain", "foldseek"])
def test_explicit_rows_kept_rows_and_chunks_have_the_same_bits(lib, cases, name, monkeypatch):
    """set_logprobs against token_logprobs on the explicitly masked rows (plain: the table rows are rows of the full log-softmax; the
    Foldseek table is a group reduction, so it is compared across the evaluations only); 2048 workspace rows (several device chunks)
    against the default (one); PGMI_KEEP_ROWS=0 (read at model creation) against the kept-row last layer: array_equal."""
    c = cases[(name, "toy_mulan_b" if name == "plain" else "toy_mulan_c")]
    L = c.L
    set_off = np.concatenate([c.set_off, c.set_off[-1] + 1 + np.arange(L)]).astype(np.int32)        # plus one set per residue
    set_pos = np.concatenate([c.set_pos, 1 + np.arange(L)]).astype(np.int32)
    n_sets = len(set_off) - 1
    assert n_sets * 96 > 2 * 2048                           # at least three chunks at 2048 rows (T = 70 takes 96)
    model = c.build()
    table = model.set_logprobs(c.ids, set_off, set_pos)
    n = len(c.set_pos)
    assert np.abs(table[:n] - c.table).max() <= TOL
    if name == "plain":
        rows = np.repeat(c.ids[None], n_sets, axis=0)
        for s in range(n_sets):
            rows[s, set_pos[set_off[s]:set_off[s + 1]]] = c.cfg["mask_token_id"]
        full = model.token_logprobs(rows, set_off, set_pos)
        picked = np.concatenate([full[s, set_pos[set_off[s]:set_off[s + 1]]] for s in range(n_sets)])
        assert np.array_equal(picked, table)
    model.close()
    small = c.build(max_rows=2048)
    assert np.array_equal(small.set_logprobs(c.ids, set_off, set_pos), table)
    assert np.array_equal(small.set_logprobs(c.ids, c.set_off, c.set_pos), table[:n])       # an entry's bits do not depend on the other sets
    small.close()
    monkeypatch.setenv("PGMI_KEEP_ROWS", "0")
    full_model = c.build()
    assert np.array_equal(full_model.set_logprobs(c.ids, set_off, set_pos), table)
    full_model.close()


def test_a_masked_low_plddt_residue_gets_minus_four(lib, cases):
    """Residue 21 of toy_mulan_b has pLDDT 70.0: its row is 4.0 unmasked; in a set, -4 wins.  The restatement where 4 wins instead is a
    different model by far more than the tolerance, and the device follows the reference's order."""
    c = cases[("plain", "toy_mulan_b")]
    p = LOW["toy_mulan_b"][1] + 1
    assert c.plddt[p] == 70.0
    model = c.build()
    got = model.set_logprobs(c.ids, [0, 1], [p])[0]
    model.close()
    ids = c.ids.copy()
    ids[p] = c.cfg["mask_token_id"]
    want = mulan_ref.log_softmax(mulan_ref.numpy_logits(c.cfg, c.blob, ids, mulan_ref.collate(c.angles, c.plddt, [p])))[p]
    four = mulan_ref.log_softmax(mulan_ref.numpy_logits(c.cfg, c.blob, ids, mulan_ref.collate(c.angles, c.plddt)))[p]
    assert np.abs(got - want).max() <= TOL and np.abs(got - four).max() >= 100 * TOL


@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
def test_profiled_call_counts_nested_scopes(lib, cases, precision):
    """The adapter's layer runs inside run_encoder's embed scope and is the first thing to grow the model's event list: the outer scope
    must survive that.  One chunk of 11 sets on the 2-layer toy: the rows kernel and the embed step (2 embed scopes), the adapter's and
    the first main layer's QKV / attention / out / FC1 / FC2 (2 each; the last layer's tail is one kept-rows scope), 5 LayerNorm scopes
    (two per full layer, one in the last), one head.  The table has the bits of the unprofiled call."""
    c = cases[("plain", "toy_mulan_b")]
    model = c.build(precision)
    table = model.set_logprobs(c.ids, c.set_off, c.set_pos)
    model.profile_enable(True)
    for _ in range(2):                                      # the first call creates the events, the second reuses them
        model.profile_reset()
        assert np.array_equal(model.set_logprobs(c.ids, c.set_off, c.set_pos), table)
        prof = model.profile()
        calls = {k: v["launches"] for k, v in prof.items() if v["launches"]}
        assert calls == dict(embed=2, layernorm=5, gemm_qkv=3, attention=3, gemm_out=2, gemm_fc1=2, gemm_fc2=2, kept_rows=1, head=1)
        assert all(np.isfinite(v["ms"]) and v["ms"] >= 0.0 for v in prof.values())
        inner = sum(prof[k]["ms"] for k in ("layernorm", "gemm_qkv", "attention", "gemm_out", "gemm_fc1", "gemm_fc2"))
        assert 0.0 < prof["embed"]["ms"] < inner + prof["embed"]["ms"]
    model.profile_enable(False)
    model.close()


def run_cli(tmp_path, index, *extra):
    dms = tmp_path / "dms"
    dms.mkdir(exist_ok=True)
    for n in ("TOY_MULAN_TWO", "TOY_MULAN_FS"):
        pd.read_csv(os.path.join(GOLDEN, n + ".csv"))[["mutant", "DMS_score"]].to_csv(dms / f"{n}.csv", index=False)
    out = tmp_path / f"out{len(list(tmp_path.iterdir()))}"
    fs = index == 1
    rc = cli.main(["--MULAN_model_name_or_path", os.path.join(TOY, "foldseek" if fs else "plain"), "--DMS_reference_file_path", REFERENCE,
                   "--DMS_data_folder", str(dms), "--structure_data_folder", STRUCT_DIR, "--DMS_index", str(index),
                   "--output_scores_folder", str(out), *(["--use_foldseek"] if fs else []), *extra])
    assert rc == 0
    return out


def check_csv(out, name, order=None):
    got, ref = pd.read_csv(out / f"{name}.csv"), pd.read_csv(os.path.join(GOLDEN, name + ".csv"))
    assert list(got.columns) == list(ref.columns) == ["mutant", "MULAN_score", "DMS_score"]
    assert got["mutant"].tolist() == ref["mutant"].tolist() and got["DMS_score"].tolist() == ref["DMS_score"].tolist()
    muts = ref["mutant"].tolist() if order is None else [ref["mutant"][i] for i in order]
    n_sub = np.array([m.count(":") + 1 for m in muts])      # per row, the bound of the mutant whose score the row received
    assert (np.abs(got["MULAN_score"] - ref["MULAN_score"]).to_numpy() <= 2e-4 * n_sub).all()


def test_cli_two_chunks_from_structure_files_and_from_the_dataset_folder(lib, tmp_path):
    """TOY_MULAN_TWO's rows are interleaved between its two chunks: the scores are assigned positionally in chunk order, as the
    reference does, so the recorded row order holds only if that is reproduced.  An existing output is left as it is."""
    first = np.array([int(m.split(":")[0][1:-1]) for m in pd.read_csv(os.path.join(GOLDEN, "TOY_MULAN_TWO.csv"))["mutant"]])
    order = np.concatenate([np.flatnonzero(first <= 17), np.flatnonzero(first > 17)])
    assert not np.array_equal(order, np.arange(len(order)))
    out = run_cli(tmp_path, 0)
    check_csv(out, "TOY_MULAN_TWO", order)
    check_csv(run_cli(tmp_path, 0, "--output_dataset_folder", DATASET, "--precision", "fp32"), "TOY_MULAN_TWO", order)
    before = (out / "TOY_MULAN_TWO.csv").read_bytes()
    (out / "TOY_MULAN_TWO.csv").write_bytes(before + b"# kept\n")
    assert cli.main(["--MULAN_model_name_or_path", os.path.join(TOY, "plain"), "--DMS_reference_file_path", REFERENCE, "--DMS_data_folder",
                     str(tmp_path / "dms"), "--structure_data_folder", STRUCT_DIR, "--DMS_index", "0", "--output_scores_folder", str(out)]) == 0
    assert (out / "TOY_MULAN_TWO.csv").read_bytes() == before + b"# kept\n"


def test_cli_foldseek_model_from_the_dataset_folder(lib, tmp_path):
    check_csv(run_cli(tmp_path, 1, "--output_dataset_folder", DATASET), "TOY_MULAN_FS")


def test_refusals(lib, cases):
    c = cases[("plain", "toy_mulan_a")]
    model = mulan.Mulan(c.cfg, c.blob, max_rows=2048)
    with pytest.raises(_lib.PgmiError, match="no structure bound"):
        model.set_logprobs(c.ids, [0, 1], [3])
    model.set_structure(c.angles, c.plddt)
    for off, pos, message in (([0, 2], [5, 3], "not ascending"), ([0, 2], [3, 3], "not ascending"), ([1, 2], [3, 4], r"set_off\[0\] must be 0"),
                              ([0, 0], [3], "empty"), ([0, 1], [19], "out of range"), ([0, 1], [0], "special token"),
                              ([0, 1], [18], "special token")):
        with pytest.raises(_lib.PgmiError, match=message) as e:
            model.set_logprobs(c.ids, off, pos)
        assert e.value.code == _lib.EINVAL
    with pytest.raises(_lib.PgmiError, match="bound structure has 19 tokens"):
        model.set_logprobs(c.ids[:-1], [0, 1], [3])
    with pytest.raises(_lib.PgmiError, match="<pad>"):
        model.token_logprobs(np.where(np.arange(19) == 18, 1, c.ids)[None])
    # sequences are not windowed: the limit is named
    long_ids = np.concatenate([[0], np.resize(c.ids[1:-1], 2100), [2]]).astype(np.int32)
    with pytest.raises(_lib.PgmiError, match="exceeds workspace rows 2048") as e:
        model.set_structure(np.zeros((len(long_ids), 7), np.float32), np.full(len(long_ids), 90.0, np.float32))
    assert e.value.code == _lib.EINVAL
    with pytest.raises(_lib.PgmiError, match="exceeds workspace rows 2048"):
        model.set_logprobs(long_ids, [0, 1], [5])
    with pytest.raises(_lib.PgmiError, match="non-finite"):
        model.set_structure(np.full((19, 7), np.nan, np.float32), c.plddt)
    # wrong arch, both ways: the ESM entries refuse a MULAN model, the MULAN entries any other
    out = np.empty((1, 19, 33), dtype=np.float32)
    t = _lib.as_i32(c.ids[None])
    assert lib.pgmi_token_logprobs(model._h, _lib.ptr(t, _lib._i32p), 1, 19, _lib.ptr(out, _lib._f32p)) == _lib.EINVAL
    assert b"pgmi_mulan_token_logprobs" in lib.pgmi_last_error()
    model.close()
    sa_cfg = S.saprot_config(64, 4, 1, 64)
    sa = saprot.from_state_dict(sa_cfg, S.saprot_state_dict(sa_cfg, 1))
    so, sp = _lib.as_i32([0, 1]), _lib.as_i32([3])
    table = np.empty((1, 446), dtype=np.float32)
    assert lib.pgmi_mulan_set_logprobs(sa._h, _lib.ptr(t, _lib._i32p), 19, _lib.ptr(so, _lib._i32p), _lib.ptr(sp, _lib._i32p), 1,
                                       _lib.ptr(table, _lib._f32p)) == _lib.EINVAL
    assert b"not a MULAN model" in lib.pgmi_last_error()
    a, p = _lib.as_f32(c.angles), _lib.as_f32(c.plddt)
    assert lib.pgmi_mulan_set_structure(sa._h, _lib.ptr(a, _lib._f32p), _lib.ptr(p, _lib._f32p), 19) == _lib.EINVAL
    sa.close()


def test_create_refusals(lib, cases):
    c = cases[("plain", "toy_mulan_a")]
    w = _lib.as_f32(c.blob)
    base = dict(abi_version=_lib.ABI_VERSION, arch=_lib.ARCH_MULAN, layers=2, embed_dim=64, heads=4, ffn_dim=256, vocab=33,
                token_dropout=1, precision=_lib.PREC_F16X3)
    h = C.c_void_p()
    wp = _lib.ptr(w, _lib._f32p)
    assert lib.pgmi_mulan_weight_count(C.byref(_lib.Config(**base))) == w.size
    assert lib.pgmi_weight_count(C.byref(_lib.Config(**base))) == -1
    assert lib.pgmi_model_create(C.byref(_lib.Config(**base)), wp, w.size, 0, C.byref(h)) == _lib.EINVAL
    assert b"pgmi_mulan_model_create" in lib.pgmi_last_error()
    assert lib.pgmi_mulan_model_create(C.byref(_lib.Config(**base)), 32, 21, wp, w.size, 0, C.byref(h)) == _lib.EINVAL
    assert b"groups 21 with vocab 33" in lib.pgmi_last_error()
    assert lib.pgmi_mulan_model_create(C.byref(_lib.Config(**dict(base, vocab=64))), 32, 0, wp, w.size, 0, C.byref(h)) == _lib.EINVAL
    assert lib.pgmi_mulan_model_create(C.byref(_lib.Config(**dict(base, arch=_lib.ARCH_ESM2))), 32, 0, wp, w.size, 0, C.byref(h)) == _lib.EINVAL
    assert b"PGMI_ARCH_MULAN" in lib.pgmi_last_error()
    assert lib.pgmi_mulan_model_create(C.byref(_lib.Config(**base)), 7, 0, wp, w.size, 0, C.byref(h)) == _lib.EINVAL
    assert b"<mask> id" in lib.pgmi_last_error()
    assert lib.pgmi_mulan_model_create(C.byref(_lib.Config(**base)), 32, 0, wp, w.size - 1, 0, C.byref(h)) == _lib.EINVAL
    assert b"weight blob" in lib.pgmi_last_error()
    assert lib.pgmi_mulan_model_create(C.byref(_lib.Config(**base)), 32, 0, wp, w.size, 0, C.byref(h)) == 0
    lib.pgmi_model_destroy(h)
