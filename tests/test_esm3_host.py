"""ESM3 host logic without a GPU: the float64 numpy forward over the packed blob against the reference's goldens (with structure and
sequence only), the blob round trip and the key check against the reference's own key list, the frames and the coordinate
normalisation, the PDB reader on hand-written PDB text, the position mapping with and without pdb_range, window slicing with one
tokenizer pass per distinct window, the structure tokenizer (its attention replaced by the float64 formula) against the
reference's tokens, and the CLI over a NumPy stand-in model."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pandas as pd
import pytest

import esm3_cases as K
import esm3_ref
from proteingym_amd import esm3, synthetic as S
from proteingym_amd import score_esm3_proteingym as cli

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLDEN, "golden_esm3.npz"))


@pytest.fixture(scope="module")
def ref_keys():
    with open(os.path.join(GOLDEN, "esm3_state_dict_keys.json")) as f:
        return json.load(f)


def numpy_attention(proj, rot, trans, mask, w_rot, w_dist):
    return np.stack([esm3_ref.geom_attention(proj[b], rot[b], trans[b], mask[b], w_rot, w_dist) for b in range(len(proj))]).astype(np.float32)


# -- forward -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["d128", "d1536"])
def test_numpy_forward_over_blob_matches_reference(g, name):
    cfg, sd = K.trunk_model(name)
    blob = esm3.pack(cfg, sd)
    ids = g[f"{name}_ids"]
    for tag, tokens, coords in (("st", g[f"{name}_structure_tokens"], g[f"{name}_coords"]), ("seq", None, None)):
        for p, ref in zip(g[f"{name}_mask_pos"], g[f"{name}_{tag}_mask_lp"]):
            t = ids.copy()
            t[p] = esm3.MASK
            assert np.abs(esm3_ref.numpy_forward(cfg, blob, t, tokens, coords)[p] - ref).max() < 2e-4
    assert np.abs(g[f"{name}_st_mask_lp"] - g[f"{name}_seq_mask_lp"]).max() > 1e-2         # the goldens' structure path was live


def test_golden_inputs_are_what_the_host_builds(g):
    """The coordinates and structure tokens the reference's encode() handed its trunk are pad_window(normalize_coordinates(...)) of
    the toy backbone: the <cls> / <eos> rows infinite, the BOS / EOS structure tokens around the residues."""
    D, layers, Hv, seed, L, bseed, nan_at = K.TRUNK["d128"]
    coords, _ = esm3.pad_window(esm3.normalize_coordinates(K.toy_backbone(bseed, L, (nan_at,))), np.zeros(L, np.int32))
    want = g["d128_coords"]
    assert np.isinf(coords[[0, -1], :3]).all() and np.isinf(want[[0, -1]]).all() and np.isnan(want[1 + nan_at]).all()
    ok = np.isfinite(want)
    assert np.array_equal(np.isfinite(coords[:, :3]), ok) and np.abs(coords[:, :3][ok] - want[ok]).max() < 1e-4
    st = g["d128_structure_tokens"]
    assert st[0] == esm3.STRUCTURE_BOS and st[-1] == esm3.STRUCTURE_EOS and st[1:-1].max() < 4096
    assert g["d128_ids"][0] == esm3.CLS and g["d128_ids"][-1] == esm3.EOS


def test_frames():
    x = K.toy_backbone(5, 12, (4,))
    coords, _ = esm3.pad_window(x, np.zeros(12, np.int32))
    rot, trans, mask = esm3.build_frames(coords)
    assert mask.tolist() == [False] + [i != 4 for i in range(12)] + [False]             # <cls>, <eos> and the empty residue: frameless
    R = rot.reshape(-1, 3, 3)
    assert np.abs(np.einsum("nij,nkj->nik", R, R) - np.eye(3)).max() < 1e-5 and np.abs(np.linalg.det(R) - 1).max() < 1e-5
    r64, t64, m64 = esm3_ref.frames(coords)
    assert np.array_equal(mask, m64) and np.abs(R - r64).max() < 1e-5 and np.abs(trans - t64).max() < 1e-4
    assert np.array_equal(trans[mask], coords[mask, 1])                                  # origin at CA
    assert np.all(R[~mask] == R[0]) and np.all(trans[~mask] == trans[0])                 # the frame of the mean N / CA / C
    # the frame's x axis runs from C to CA; N lies in its xy plane on the positive-y side
    local_n = np.einsum("nji,nj->ni", R[mask], coords[mask, 0] - coords[mask, 1])
    local_c = np.einsum("nji,nj->ni", R[mask], coords[mask, 2] - coords[mask, 1])
    assert np.abs(local_c[:, 1:]).max() < 1e-4 and (local_c[:, 0] < 0).all() and np.abs(local_n[:, 2]).max() < 1e-4 and (local_n[:, 1] > 0).all()
    rot0, trans0, mask0 = esm3.build_frames(np.full((5, 3, 3), np.nan, np.float32))
    assert not mask0.any() and np.all(rot0.reshape(-1, 3, 3) == np.eye(3)) and np.all(trans0 == 0)
    assert esm3.per_res_plddt(coords).tolist() == [0] + [int(i != 4) for i in range(12)] + [0]


# -- checkpoint --------------------------------------------------------------------------------------------------------------
def test_keys_are_the_reference_state_dict(ref_keys):
    rel = esm3.RELEASED["esm3_open"]
    want = ref_keys["esm3_open"]
    assert sorted(esm3.state_dict_keys(rel["layers"])) == sorted(k for k, _ in want)
    ref_shapes = {k: tuple(s) for k, s in want}
    shapes = {k: np.broadcast_to(np.float32(0), s) for k, s in ref_shapes.items()}
    cfg = esm3.config_from_state_dict(shapes, "esm3_open")
    assert cfg == dict(layers=48, embed_dim=1536, heads=24, ffn_dim=esm3.swiglu_hidden(1536), vocab=64, v_heads=256) == S.esm3_config()
    assert all(ref_shapes[k] == s for k, s in esm3.shapes(cfg).items())
    assert esm3.check_state_dict(shapes) == cfg
    enc = ref_keys["structure_encoder"]
    assert sorted(esm3.encoder_state_dict_keys(esm3.RELEASED_ENCODER["layers"])) == sorted(k for k, _ in enc)
    ecfg = esm3.encoder_config_from_state_dict({k: np.broadcast_to(np.float32(0), tuple(s)) for k, s in enc})
    assert ecfg == S.esm3_encoder_config() and {k: ecfg[k] for k in esm3.RELEASED_ENCODER} == esm3.RELEASED_ENCODER
    esd = S.esm3_encoder_state_dict(S.esm3_encoder_config(64, 8, 2, 32, 64), 1)
    assert sorted(esd) == sorted(esm3.encoder_state_dict_keys(2))


def test_synthetic_state_dict_and_blob_round_trip():
    cfg = S.esm3_config(128, 2, 16)
    sd = S.esm3_state_dict(cfg, 3)
    assert sorted(sd) == sorted(esm3.state_dict_keys(2)) and esm3.check_state_dict(sd) == cfg
    p = "transformer.blocks.0.geom_attn."
    assert np.all(sd[p + "rotation_scale_per_head"] != 0) and np.all(sd[p + "distance_scale_per_head"] != 0)
    assert not any(k.startswith("transformer.blocks.1.geom_attn") for k in sd)
    blob = esm3.pack(cfg, sd)
    assert blob.size == esm3.weight_count(cfg)
    back = esm3.unpack(cfg, blob)
    assert list(back) == esm3.expected_keys(2) and all(np.array_equal(back[k], sd[k]) for k in back)
    bad = dict(sd)
    bad["transformer.extra"] = np.zeros(1, np.float32)
    with pytest.raises(ValueError, match="unexpected"):
        esm3.check_state_dict(bad)
    bad = dict(sd)
    del bad["output_heads.structure_head.0.bias"]
    with pytest.raises(ValueError, match="missing"):
        esm3.check_state_dict(bad)
    bad = dict(sd)
    bad["encoder.ss8_embed.weight"] = bad["encoder.ss8_embed.weight"][:8]
    with pytest.raises(ValueError, match="shape"):
        esm3.check_state_dict(bad)
    bad = dict(sd)
    bad["encoder.function_embed.3.weight"] = bad["encoder.function_embed.3.weight"] + 1
    with pytest.raises(ValueError, match="padding row"):
        esm3.check_state_dict(bad)


def test_weight_count_matches_library(lib):
    from proteingym_amd import _lib
    for D, L, Hv in ((128, 2, 16), (1536, 48, 256)):
        cfg = S.esm3_config(D, L, Hv)
        c = _lib.Config(abi_version=_lib.ABI_VERSION, arch=_lib.ARCH_ESM3, layers=L, embed_dim=D, heads=D // 64, ffn_dim=cfg["ffn_dim"],
                        vocab=64, precision=_lib.PREC_F16X3)
        assert lib.pgmi_esm3_weight_count(C.byref(c), Hv) == esm3.weight_count(cfg)
        assert lib.pgmi_weight_count(C.byref(c)) == -1


@pytest.mark.parametrize("form", ["dir", "file"])
def test_loader_snapshot_dir_and_file(tmp_path, form):
    torch = pytest.importorskip("torch")
    cfg, sd = K.trunk_model("d128")
    esd = K.encoder_model()[1]
    wdir = tmp_path / "data" / "weights" if form == "dir" else tmp_path
    wdir.mkdir(parents=True, exist_ok=True)
    torch.save({k: torch.from_numpy(v).to(torch.bfloat16 if "ffn" in k else torch.float32) for k, v in sd.items()}, wdir / "esm3_sm_open_v1.pth")
    path = str(tmp_path if form == "dir" else wdir / "esm3_sm_open_v1.pth")
    got, enc = esm3.load_state_dicts(path)
    assert enc is None and sorted(got) == sorted(sd) and all(v.dtype == np.float32 for v in got.values())
    assert np.array_equal(got["encoder.sequence_embed.weight"], sd["encoder.sequence_embed.weight"])
    torch.save({k: torch.from_numpy(v) for k, v in esd.items()}, wdir / "esm3_structure_encoder_v0.pth")
    got, enc = esm3.load_state_dicts(path)
    assert sorted(enc) == sorted(esd) and esm3.encoder_config_from_state_dict(enc) == K.encoder_model()[0]
    with pytest.raises(FileNotFoundError):
        esm3.load_state_dicts(str(tmp_path / "nothing_here"))


# -- PDB ---------------------------------------------------------------------------------------------------------------------
def atom(serial, name, res, chain, num, xyz, ins=" ", rec="ATOM", alt=" "):
    return "%-6s%5d %-4s%1s%3s %1s%4d%1s   %8.3f%8.3f%8.3f  1.00  0.00" % (rec, serial, name if len(name) == 4 else " " + name, alt, res, chain,
                                                                         num, ins, *xyz)


PDB_TEXT = [
    "HEADER    HAND-WRITTEN",
    atom(1, "O", "HOH", "B", 900, (9, 9, 9), rec="HETATM"),            # the first atom record names the first chain: B
    atom(2, "N", "GLY", "B", 1, (0, 0, 0)), atom(3, "CA", "GLY", "B", 1, (1, 0, 0)), atom(4, "C", "GLY", "B", 1, (2, 0, 0)),
    atom(5, "N", "ALA", "A", 10, (0, 1, 0)), atom(6, "CA", "ALA", "A", 10, (1, 1, 0)), atom(7, "C", "ALA", "A", 10, (2, 1, 0)),
    atom(8, "CA", "ALA", "A", 10, (5, 5, 5), alt="B"),                 # a second alternate location: ignored
    atom(9, "N", "MSE", "A", 11, (0, 2, 0)), atom(10, "CA", "MSE", "A", 11, (1, 2, 0)), atom(11, "C", "MSE", "A", 11, (2, 2, 0)),
    atom(12, "SE", "MSE", "A", 11, (3, 2, 1)),
    atom(13, "N", "TRP", "A", 11, (0, 3, 0), ins="A"), atom(14, "CA", "TRP", "A", 11, (1, 3, 0), ins="A"),
    atom(15, "N", "LYS", "A", 12, (0, 4, 0)), atom(16, "C", "LYS", "A", 12, (2, 4, 0)), atom(17, "CB", "LYS", "A", 12, (1, 4, 1)),
    atom(18, "ZN", " ZN", "A", 300, (7, 7, 7), rec="HETATM"),
    atom(19, "N", "MSE", "A", 13, (0, 5, 0), rec="HETATM"),           # a hetero residue: not part of the chain
    atom(20, "N", "ABC", "A", 14, (0, 6, 0)), atom(21, "CA", "ABC", "A", 14, (1, 6, 0)), atom(22, "C", "ABC", "A", 14, (2, 6, 0)),
    atom(23, "P", " DA", "A", 15, (0, 7, 0)),
    "ENDMDL",
    atom(24, "N", "VAL", "A", 16, (0, 8, 0)),                          # model 2: not read
]


def test_pdb_reader_on_hand_written_text():
    a = esm3.read_pdb(PDB_TEXT, "A")
    assert a.sequence == "AMWKX" and a.residue_index.tolist() == [10, 11, 11, 12, 14] and a.insertion_code.tolist() == ["", "", "A", "", ""]
    assert a.atom37_positions.shape == (5, 37, 3) and a.atom37_positions.dtype == np.float32
    o = esm3.ATOM_ORDER
    assert a.atom37_positions[0, o["CA"]].tolist() == [1, 1, 0]                          # the first alternate location
    assert a.atom37_positions[1, o["SD"]].tolist() == [3, 2, 1]                          # MSE's selenium in the SD column
    assert np.isnan(a.atom37_positions[3, o["CA"]]).all() and a.atom37_positions[3, o["CB"]].tolist() == [1, 4, 1]   # a residue missing CA
    assert np.isnan(a.atom37_positions[2, o["C"]]).all()
    _, _, mask = esm3.build_frames(a.atom37_positions)
    assert mask.tolist() == [True, True, False, False, True] and esm3.per_res_plddt(a.atom37_positions).tolist() == [1, 1, 1, 1, 1]
    b = esm3.read_pdb(PDB_TEXT)                                                          # the first chain of the file
    assert b.sequence == "G" and b.residue_index.tolist() == [1]
    with pytest.raises(ValueError):                                                      # the reference's int("11A")
        esm3.residue_map(a)


def test_toy_pdb_files_read_back():
    for fname, (L, seed, hole, first) in K.TOY_PDBS.items():
        chain = esm3.read_pdb(os.path.join(GOLDEN, "ESM3_structures", fname), "A")
        want = K.toy_backbone(seed, L, (hole,))
        assert chain.sequence == K.sequence_of(seed, L) and chain.residue_index.tolist() == list(range(first, first + L))
        ok = np.isfinite(want)
        assert np.array_equal(chain.atom37_positions[ok], want[ok]) and np.isnan(chain.atom37_positions[hole, :3]).all()
        assert np.isfinite(chain.atom37_positions[hole, esm3.ATOM_ORDER["CB"]]).all()


def test_position_mapping_with_and_without_pdb_range(capsys):
    chain = esm3.Chain("ACDE", None, np.array([5, 6, 8, 9]), np.array(["", "", "", ""]))
    assert esm3.residue_map(chain) == {5: 0, 6: 1, 8: 2, 9: 3}
    assert esm3.residue_map(chain, "11-50") == {15: 0, 16: 1, 18: 2, 19: 3}
    assert esm3.residue_map(chain, float("nan")) == esm3.residue_map(chain, "") == esm3.residue_map(chain)
    assert esm3.residue_map(chain, "11:50") == esm3.residue_map(chain) and "Could not parse pdb_range" in capsys.readouterr().out
    ids = esm3.residue_map(chain, "11-50")
    parsed = esm3.parse_mutations_pdb(["A15G", "W16C", "A17C", "A15G:D18E", "A15G:D17E:E19A", "x15G", "A15G:bad"], ids)
    # no wild-type check on this path (W16C is scored); a position outside the PDB or an unparsable part drops the whole mutant
    assert [p[4] for p in parsed] == ["A15G", "W16C", "A15G:D18E"]
    assert parsed[2][:4] == ("AD", [15, 18], "GE", [0, 2])


# -- scoring -----------------------------------------------------------------------------------------------------------------
class NumpyESM3:
    """The device model's scoring on the float64 numpy forward (fp32 log-probabilities)."""

    def __init__(self, cfg, blob, encoder=None):
        self.cfg, self.blob, self.encoder, self.windows_encoded, self.bound = cfg, blob, encoder, 0, []

    def set_window(self, T, structure_tokens=None, coords=None):
        self.window = (structure_tokens, coords)
        self.bound.append((T, structure_tokens is not None))

    def masked_logprobs(self, tokens, mask):
        out = []
        for row, p in zip(tokens, mask):
            t = row.copy()
            t[p] = esm3.MASK
            out.append(esm3_ref.numpy_forward(self.cfg, self.blob, t, *self.window)[p])
        return np.array(out, dtype=np.float32)

    _score = esm3.ESM3._score
    score_mutations = esm3.ESM3.score_mutations
    score_mutations_with_pdb = esm3.ESM3.score_mutations_with_pdb

    def close(self):
        pass


@pytest.fixture(scope="module")
def numpy_model():
    cfg, sd = K.trunk_model(K.TOY_MODEL[0])
    return NumpyESM3(cfg, esm3.pack(cfg, sd), esm3.StructureEncoder(K.encoder_model()[1], attention=numpy_attention))


@pytest.mark.parametrize("name", list(K.TOKENIZER))
def test_structure_tokenizer_against_reference(g, numpy_model, name):
    """The tokenizer's host side (k-NN, neighbourhood frames, relative positions, blocks, nearest code) with the float64 formula in
    the attention's place; the conditioned equality of test_gpu_esm3.py."""
    L, seed, missing = K.TOKENIZER[name]
    coords, tokens = numpy_model.encoder.encode(K.toy_backbone(seed, L, missing))
    sure = g[f"tok_{name}_margin"] >= 100 * float(g["tok_dev"])
    assert (~sure).mean() <= 0.10 and np.array_equal(tokens[sure], g[f"tok_{name}_tokens"][sure])
    assert coords.shape == (L, 37, 3) and coords.dtype == np.float32


def test_knn_edges():
    ca = K.toy_backbone(3, 30)[:, 1]
    mask = np.ones(30, bool)
    mask[7] = False
    e = esm3.StructureEncoder.knn_edges(ca, mask)
    assert e.shape == (30, 16) and e[:, 0].tolist() == list(range(30))                   # a residue is its own nearest neighbour
    d = np.linalg.norm(ca[:, None] - ca[None], axis=-1)
    for i in (0, 12, 29):
        assert 7 not in e[i] and sorted(e[i]) == sorted(np.argsort(np.where(mask, d[i], np.inf))[:16])
    assert esm3.StructureEncoder.knn_edges(ca[:5], mask[:5]).shape == (5, 5)


def test_scores_match_reference_on_the_toy_assays(numpy_model):
    ref = pd.read_csv(os.path.join(GOLDEN, "TOY_ESM3_REFERENCE.csv")).set_index("DMS_id")
    for name in ("TOY_ESM3_STRUCT", "TOY_ESM3_RANGE", "TOY_ESM3_SEQONLY"):
        want = pd.read_csv(os.path.join(GOLDEN, name + ".csv"))
        if name == "TOY_ESM3_SEQONLY":
            scores = numpy_model.score_mutations(ref.loc[name, "target_seq"], want["mutant"].tolist())
        else:
            scores = numpy_model.score_mutations_with_pdb(os.path.join(GOLDEN, "ESM3_structures", ref.loc[name, "pdb_file"]), want["mutant"].tolist(),
                                                          "A", pdb_range=ref.loc[name, "pdb_range"])
        got = want["mutant"].map(lambda x: scores.get(x, np.nan))
        assert got.isna().tolist() == want["esm3_open_score"].isna().tolist()
        ok = want["esm3_open_score"].notna()
        assert np.abs(got[ok] - want["esm3_open_score"][ok]).max() < 2e-4
    assert pd.read_csv(os.path.join(GOLDEN, "TOY_ESM3_RANGE.csv"))["esm3_open_score"].isna().sum() == 4     # positions absent from the PDB
    with pytest.raises(KeyError):                                                        # aa_to_token has the 20 standard letters only
        numpy_model.score_mutations("ACDEFGHIKL", ["C2B"])


class CountingEncoder:
    def __init__(self):
        self.seen = []

    def encode(self, atom37):
        self.seen.append(atom37[:, 1, 0].copy())
        return atom37, np.zeros(len(atom37), np.int32)


def test_window_slicing_encodes_each_distinct_window_once():
    """compute_fitness.py:366-401 with the coordinates sliced like the sequence; one tokenizer pass per distinct (start, end)."""
    L, W = 60, 22                                       # windows of 20 residues
    seq = K.sequence_of(9, L)
    atom37 = np.zeros((L, 37, 3), np.float32)
    atom37[:, :, 0] = np.arange(L)[:, None]             # residue i's x coordinates are i: a window shows where it was cut
    calls = []

    class Fake(NumpyESM3):
        def masked_logprobs(self, tokens, mask):
            if self.window[1] is not None:
                calls.append((self.window[1][1:-1, 1, 0].copy(), tokens.copy(), np.asarray(mask).copy()))
            return np.zeros((len(tokens), 64), np.float32)
    enc = CountingEncoder()
    m = Fake(None, None, enc)
    positions = [0, 3, 10, 11, 30, 49, 50, 59]
    parsed = [(seq[p], [p + 1], "A" if seq[p] != "A" else "C", [p], f"m{p}") for p in positions]
    m._score(seq, parsed, atom37, W)
    want = {}
    for p in positions:
        want.setdefault(esm3.window(p, L, W), []).append(p)
    assert list(want) == [(0, 20), (1, 21), (20, 40), (39, 59), (40, 60)] and m.windows_encoded == len(want) == len(enc.seen)
    for (s, e), (xs, tokens, mask), ps in zip(want, calls, want.values()):
        assert xs.tolist() == list(range(s, e))                                          # the coordinates of exactly this window
        assert tokens.shape == (len(ps), e - s + 2) and mask.tolist() == [p - s + 1 for p in ps]
        assert all(np.array_equal(row, esm3.tokenize(seq[s:e])) for row in tokens)
    assert m.bound == [(22, True)] * 5
    m2 = Fake(None, None, None)                         # sequence only: no coordinates, no tokenizer
    m2._score(seq, parsed, None, W)
    assert m2.bound == [(22, False)] * 5 and m2.windows_encoded == 0
    with pytest.raises(ValueError, match="structure encoder"):
        m2._score(seq, parsed, atom37, W)


# -- CLI -------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def assays(tmp_path):
    dms = tmp_path / "dms"
    dms.mkdir()
    for n in ("TOY_ESM3_STRUCT", "TOY_ESM3_RANGE", "TOY_ESM3_SEQONLY"):
        pd.read_csv(os.path.join(GOLDEN, n + ".csv"))[["mutant", "DMS_score"]].to_csv(dms / f"{n}.csv", index=False)
    pd.DataFrame({"mutant": ["A1C", "C2B"], "DMS_score": [0.1, 0.2]}).to_csv(dms / "TOY_ESM3_BADLETTER.csv", index=False)
    ref = pd.read_csv(os.path.join(GOLDEN, "TOY_ESM3_REFERENCE.csv"))
    extra = pd.DataFrame({"DMS_id": ["TOY_ESM3_NOPDB", "TOY_ESM3_NOCSV", "TOY_ESM3_BADLETTER"], "target_seq": ["ACD"] * 3,
                          "pdb_file": ["missing.pdb", "toy_esm3.pdb", "toy_esm3.pdb"], "pdb_range": [""] * 3})
    pd.concat([ref, extra]).to_csv(tmp_path / "ref.csv", index=False)
    return tmp_path


@pytest.fixture
def fake_model(monkeypatch, numpy_model):
    made = []

    def from_pretrained(path, model_type=None, device=0, max_rows=0):
        made.append((path, model_type))
        return numpy_model
    monkeypatch.setattr(esm3, "from_pretrained", from_pretrained)
    return made


def run_cli(assays, *extra, ref="ref.csv"):
    return cli.main(["--reference_csv", str(assays / ref), "--dms_dir", str(assays / "dms"), "--output_dir", str(assays / "out"),
                     "--model_path", "/nonexistent", *extra])


def test_cli_with_structure(assays, fake_model):
    assert run_cli(assays, "--use_structure", "--pdb_dir", os.path.join(GOLDEN, "ESM3_structures")) == 0
    assert fake_model == [("/nonexistent", "esm3_open")]
    for n in ("TOY_ESM3_STRUCT", "TOY_ESM3_RANGE"):
        out, want = pd.read_csv(assays / "out" / f"{n}.csv"), pd.read_csv(os.path.join(GOLDEN, n + ".csv"))
        assert list(out.columns) == ["mutant", "DMS_score", "esm3_open_score"] and out["mutant"].tolist() == want["mutant"].tolist()
        assert out["esm3_open_score"].isna().tolist() == want["esm3_open_score"].isna().tolist()
        ok = want["esm3_open_score"].notna()
        assert np.abs(out["esm3_open_score"][ok] - want["esm3_open_score"][ok]).max() < 2e-4
    # a missing PDB and a missing assay CSV: skipped, no summary row; a failing assay: NaN summary row, no CSV
    assert not (assays / "out" / "TOY_ESM3_NOPDB.csv").exists() and not (assays / "out" / "TOY_ESM3_BADLETTER.csv").exists()
    summary = pd.read_csv(assays / "out" / "correlation_summary_esm3_open.csv")
    assert summary["assay"].tolist() == ["TOY_ESM3_STRUCT", "TOY_ESM3_RANGE", "TOY_ESM3_SEQONLY", "TOY_ESM3_BADLETTER"]
    assert summary["correlation"].notna().tolist() == [True, True, True, False]
    assert run_cli(assays, "--use_structure", "--pdb_dir", os.path.join(GOLDEN, "ESM3_structures"), "--DMS_index", "1") == 0    # appended
    assert pd.read_csv(assays / "out" / "correlation_summary_esm3_open.csv")["assay"].tolist()[4:] == ["TOY_ESM3_RANGE"]


def test_cli_sequence_only(assays, fake_model):
    assert run_cli(assays, "--DMS_index", "2") == 0
    out, want = pd.read_csv(assays / "out" / "TOY_ESM3_SEQONLY.csv"), pd.read_csv(os.path.join(GOLDEN, "TOY_ESM3_SEQONLY.csv"))
    assert out["esm3_open_score"].isna().tolist() == want["esm3_open_score"].isna().tolist()
    ok = want["esm3_open_score"].notna()
    assert np.abs(out["esm3_open_score"][ok] - want["esm3_open_score"][ok]).max() < 2e-4
    assert pd.read_csv(assays / "out" / "correlation_summary_esm3_open.csv")["assay"].tolist() == ["TOY_ESM3_SEQONLY"]


def test_cli_flags_and_refusals(assays, fake_model, capsys):
    a = cli.parser().parse_args(["--reference_csv", "r", "--dms_dir", "d", "--output_dir", "o"])
    assert (a.model_type, a.model_path, a.pdb_dir, a.use_structure, a.DMS_index) == ("esm3_open", None, None, False, -1)
    assert run_cli(assays, "--model_type", "esmc_300M") == 2 and "score_esmc_proteingym" in capsys.readouterr().err
    assert run_cli(assays, "--use_structure") == 2 and "--pdb_dir must be provided" in capsys.readouterr().err
    assert cli.main(["--reference_csv", str(assays / "ref.csv"), "--dms_dir", "d", "--output_dir", str(assays / "o2")]) == 2
    assert "--model_path is required" in capsys.readouterr().err
    pd.read_csv(assays / "ref.csv").drop(columns=["pdb_file"]).to_csv(assays / "nopdb.csv", index=False)
    with pytest.raises(ValueError, match="pdb_file"):
        run_cli(assays, "--use_structure", "--pdb_dir", "p", ref="nopdb.csv")
    assert fake_model == []
    from proteingym_amd import score_esmc_proteingym as esmc_cli                      # the ESM C entry keeps refusing esm3_open
    assert esmc_cli.main(["--reference_csv", "r", "--dms_dir", "d", "--output_dir", "o", "--model_type", "esm3_open"]) == 2


def test_launcher_builds_a_valid_command_line(tmp_path):
    cfg_dir = tmp_path / "scripts"
    (cfg_dir / "scoring_DMS_zero_shot").mkdir(parents=True)
    (cfg_dir / "zero_shot_config.sh").write_text(
        'export DMS_data_folder_subs="/data/pg/DMS_ProteinGym_substitutions/"\n'
        'export DMS_structure_folder="/data/pg/ProteinGym_AF2_structures/"\n'
        'export DMS_reference_file_path_subs=../../reference_files/DMS_substitutions.csv\n'
        'export DMS_output_score_folder_subs="/data/pg/zero_shot_substitutions_scores/"\n')
    script = os.path.join(ROOT, "scripts", "scoring_DMS_zero_shot", "scoring_ESM3_substitutions.sh")
    for use, index in (("1", "-1"), ("0", "4")):
        env = dict(os.environ, ZERO_SHOT_CONFIG=str(cfg_dir / "zero_shot_config.sh"), PGMI_LAUNCH_ECHO="1", ESM3_model_path="/w/esm3",
                   ESM3_use_structure=use, DMS_index=index)
        out = subprocess.run(["bash", script], env=env, capture_output=True, text=True, cwd=str(tmp_path))
        assert out.returncode == 0, out.stderr
        argv = out.stdout.strip().split("\n")
        assert argv[0] == "proteingym_amd.score_esm3_proteingym"
        a = cli.parser().parse_args(argv[1:])
        assert (a.model_type, a.model_path, str(a.DMS_index)) == ("esm3_open", "/w/esm3", index)
        assert a.use_structure == (use == "1") and a.pdb_dir == ("/data/pg/ProteinGym_AF2_structures/" if use == "1" else None)
        assert a.output_dir == "/data/pg/zero_shot_substitutions_scores//ESM3/" and a.reference_csv.endswith("reference_files/DMS_substitutions.csv")
