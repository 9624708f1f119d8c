"""SaProt, host side (no GPU): tokenisation, the masked-id map and the vocabulary check against the Hugging Face tokenizer's frozen ids,
position sets and the entry map, the pLDDT parser and the Foldseek command line against the reference's, the blob packing and a
float64 forward over it against the reference's frozen logits, loader refusals and the CLI's exit codes and errors."""
import json
import os
import shutil

import numpy as np
import pandas as pd
import pytest

import saprot_ref
from proteingym_amd import saprot, synthetic as S
from proteingym_amd import score_saprot_proteingym as cli

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOY_DIR = os.path.join(GOLDEN, "SaProt_toy")
STRUCT_DIR = os.path.join(GOLDEN, "SaProt_structures")
TOL = 1e-4                                                  # the project's parity bar


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLDEN, "golden_saprot.npz"))


def test_tokenisation_and_masked_ids_match_hf(g):
    pairs = [str(p) for p in g["tok_pairs"]]
    ids = saprot.tokenize("".join(p[0] for p in pairs), "".join(p[1] for p in pairs))
    assert np.array_equal(ids, g["tok_ids"])
    assert np.array_equal(saprot.masked_ids()[ids], g["tok_masked"])       # specials stay, a residue token becomes '#' + its structure letter
    assert saprot.vocabulary() == saprot.read_vocab(os.path.join(TOY_DIR, "vocab.txt"))
    assert saprot.vocabulary()[32] == "Ch"                                 # ESM's <mask> id is an ordinary residue token here
    for name in ("toy", "h24", "w650"):
        assert np.array_equal(saprot.tokenize(str(g[f"{name}_seq"]), str(g[f"{name}_struc"])), g[f"{name}_ids"])
    with pytest.raises(ValueError, match="not a SaProt token"):
        saprot.tokenize("AXA", "ppp")
    with pytest.raises(ValueError, match="structure string"):
        saprot.tokenize("AAA", "pp")


def test_vocabulary_layout_check_rejects_a_shuffled_vocab(tmp_path):
    v = saprot.vocabulary()
    saprot.check_vocabulary(v)
    swapped = list(v)
    swapped[40], swapped[41] = swapped[41], swapped[40]
    for bad in (swapped, v[:-1], v[:4] + v[5:] + ["<mask>"], [v[0]] + v):
        with pytest.raises(ValueError, match="layout"):
            saprot.check_vocabulary(bad)
    d = tmp_path / "ckpt"
    shutil.copytree(TOY_DIR, d)
    (d / "vocab.txt").write_text("\n".join(swapped) + "\n")
    with pytest.raises(ValueError, match="layout"):
        saprot.load_checkpoint(str(d))


def test_position_sets_and_entry_map(lib, g):
    for name in ("toy", "h24", "w650"):
        muts, seq = [str(m) for m in g[f"{name}_mutants"]], str(g[f"{name}_seq"])
        pos, wt, mt, off = saprot.parse_chunk(muts, seq, 1, len(seq))
        set_off, set_pos, entry = saprot.position_sets(pos, off)
        assert np.array_equal(set_off, g[f"{name}_set_off"]) and np.array_equal(set_pos, g[f"{name}_set_pos"])
        assert np.array_equal(entry, g[f"{name}_entry"])
        sets = [tuple(set_pos[a:b]) for a, b in zip(set_off[:-1], set_off[1:])]
        assert len(set(sets)) == len(sets)                                 # every set once
        for i, m in enumerate(muts):
            want = tuple(sorted({int(s[1:-1]) for s in m.split(":")}))
            for k, s in zip(range(off[i], off[i + 1]), m.split(":")):
                e = entry[k]
                si = int(np.searchsorted(set_off, e, side="right")) - 1
                assert sets[si] == want and set_pos[e] == int(s[1:-1]) == pos[k]
                assert saprot.AA_LETTERS[wt[k]] == s[0] and saprot.AA_LETTERS[mt[k]] == s[-1]
        # the table the reference's own forwards give, through the entry map and pgmi_score_mutants, gives its scores
        sc = saprot.pesm.score_parsed(g[f"{name}_group_lp"], entry, wt, mt, off)
        assert np.abs(sc - g[f"{name}_scores"]).max() <= 1e-5
    # singles take the vectorised path: the same sets as the general one
    pos = np.array([7, 3, 7, 9, 3, 1], dtype=np.int32)
    so, sp, en = saprot.position_sets(pos, np.arange(7))
    assert so.tolist() == [0, 1, 2, 3, 4] and sp.tolist() == [7, 3, 9, 1] and en.tolist() == [0, 1, 0, 2, 1, 3]
    # a repeated position is masked once and counted twice; a chunk's positions are rebased
    so, sp, en = saprot.position_sets(np.array([5, 5, 9, 2, 9], dtype=np.int32), np.array([0, 2, 5]))
    assert so.tolist() == [0, 1, 3] and sp.tolist() == [5, 2, 9] and en.tolist() == [0, 0, 2, 1, 2]
    seq = str(g["toy_seq"])
    pos, _, _, _ = saprot.parse_chunk([f"{seq[44]}45A" if seq[44] != "A" else f"{seq[44]}45C"], seq, 41, 10)
    assert pos.tolist() == [5]


def test_parse_chunk_assertions(lib, g):
    seq = str(g["toy_seq"])
    wrong = next(a for a in S.AA if a != seq[4])
    with pytest.raises(AssertionError):
        saprot.parse_chunk([f"{wrong}5A"], seq, 1, len(seq))               # get_mutated_sequence: wild-type letter
    with pytest.raises(AssertionError, match="to_AA"):
        saprot.parse_chunk([f"{seq[4]}5B"], seq, 1, len(seq))              # ... and the target letter among the 20
    a, b = (f"{seq[p]}{p + 1}{'A' if seq[p] != 'A' else 'C'}" for p in (44, 3))
    with pytest.raises(ValueError, match=a + ":" + b):
        saprot.parse_chunk([a + ":" + b], seq, 41, 10)                     # the second sub-mutation lies before the chunk


def test_plddt_parser_and_foldseek_command(g, tmp_path):
    for n in ("toy_saprot_one", "toy_saprot_two_1", "toy_saprot_two_2"):
        got = saprot.extract_plddt(os.path.join(STRUCT_DIR, n + ".pdb"))
        assert got.dtype == np.float64 and np.array_equal(got, g[f"plddt_{n}"])
    text = open(os.path.join(STRUCT_DIR, "toy_saprot_two_2.pdb")).read()
    assert " A1000 " in text and " A 999 " in text                         # chain and number fused from 1000 on
    assert saprot.foldseek_command("/opt/fs/foldseek", "x/y.pdb", "t/out.tsv") == \
        "/opt/fs/foldseek structureto3didescriptor -v 0 --threads 1 --chain-name-mode 1 x/y.pdb t/out.tsv"
    # through the stand-in: chain A's record (the file's second), lower-cased, '#' where the mean pLDDT is below 70
    foldseek = saprot_ref.write_stand_in_foldseek(tmp_path)
    cwd = set(os.listdir("."))
    struc = saprot.structure_sequence(foldseek, os.path.join(STRUCT_DIR, "toy_saprot_one.pdb"))
    assert set(os.listdir(".")) == cwd                                     # nothing written into the working directory
    raw = open(os.path.join(STRUCT_DIR, "toy_saprot_one.tsv")).read().splitlines()[1].split("\t")[2]
    low = g["plddt_toy_saprot_one"] < 70
    assert low.any() and not low.all() and len(struc) == len(raw)
    assert struc == "".join("#" if m else c.lower() for c, m in zip(raw, low))
    with pytest.raises(KeyError):
        saprot.structure_sequence(foldseek, os.path.join(STRUCT_DIR, "toy_saprot_one.pdb"), chain="C")


def test_numpy_forward_over_the_packed_blob_matches_reference_logits(g):
    """Blob order, name mapping, rotary and the 0.88 factor, read independently in float64: within 1e-4 of the reference's fp32 logits
    (observed maxima: profiles/saprot/README.md)."""
    cfg, sd = saprot.load_checkpoint(TOY_DIR)
    assert cfg["layers"] == 2 and cfg["embed_dim"] == 128 and cfg["token_dropout"] == 1
    blob = saprot.pack(cfg, sd)
    assert blob.size == saprot.weight_count(cfg)
    err = np.abs(saprot_ref.numpy_logits(cfg, blob, g["toy_ids"]) - g["toy_logits"]).max()
    print(f"toy: max|numpy float64 - reference logits| = {err:.3e}")
    assert err <= TOL
    D, H, F, layers, seed = (int(v) for v in g["h24_cfg"])
    cfg = S.saprot_config(D, H, layers, F)
    blob = saprot.pack(cfg, S.saprot_state_dict(cfg, seed))
    lp = saprot_ref.numpy_forward(cfg, blob, g["h24_ids"])
    err = np.abs(lp - g["h24_lp"]).max()
    print(f"h24: max|numpy float64 - reference log-probabilities| = {err:.3e}")
    assert err <= TOL
    # the group table of the unmasked row from those log-probabilities: 21 columns that sum (with the specials) to one
    gl = saprot_ref.group_logprobs(lp)
    assert gl.shape == (len(g["h24_ids"]), 21) and np.abs(np.exp(gl).sum(-1) + np.exp(lp[:, :5]).sum(-1) - 1).max() < 1e-12


def test_pack_accepts_hf_extras_and_refuses_others():
    cfg = S.saprot_config(64, 1, 1, 64)
    sd = S.saprot_state_dict(cfg, 1)
    blob = saprot.pack(cfg, sd)
    extra = dict(sd)
    extra["lm_head.decoder.bias"] = extra.pop("lm_head.bias")
    extra.update({"esm.contact_head.regression.weight": np.zeros((1, 2), np.float32), "lm_head.decoder.weight": sd["esm.embeddings.word_embeddings.weight"],
                  "esm.encoder.layer.0.attention.self.rotary_embeddings.inv_freq": np.zeros(32, np.float32),
                  "esm.embeddings.position_embeddings.weight": np.zeros((1026, 64), np.float32)})
    assert np.array_equal(saprot.pack(cfg, extra), blob)
    with pytest.raises(ValueError, match="unexpected"):
        saprot.pack(cfg, dict(sd, **{"esm.pooler.dense.weight": np.zeros((64, 64), np.float32)}))
    missing = dict(sd)
    del missing["esm.encoder.layer.0.LayerNorm.bias"]
    with pytest.raises(ValueError, match="missing"):
        saprot.pack(cfg, missing)


@pytest.mark.parametrize("change, message", [({"layer_norm_eps": 1e-12}, "layer_norm_eps"), ({"position_embedding_type": "absolute"}, "rotary"),
                                             ({"emb_layer_norm_before": True}, "emb_layer_norm_before"), ({"vocab_size": 33}, "vocab_size"),
                                             ({"mask_token_id": 32}, "mask_token_id")])
def test_loader_refusals(tmp_path, change, message):
    d = tmp_path / "ckpt"
    shutil.copytree(TOY_DIR, d)
    c = json.load(open(d / "config.json"))
    c.update(change)
    json.dump(c, open(d / "config.json", "w"))
    with pytest.raises(ValueError, match=message):
        saprot.load_checkpoint(str(d))


def test_loader_needs_a_local_directory():
    with pytest.raises(ValueError, match="local directory"):
        saprot.from_pretrained("westlake-repl/SaProt_650M_AF2")


def test_cli_exit_codes_and_errors(lib, g, tmp_path, capsys):
    assert cli.main(["--indel_mode", "--DMS_index", "0", "--output_scores_folder", str(tmp_path)]) == 2
    assert "indel" in capsys.readouterr().err
    assert cli.main(["--output_scores_folder", str(tmp_path)]) == 2
    assert [a.dest for a in cli.parser()._actions[1:9]] == ["foldseek_bin", "SaProt_model_name_or_path", "DMS_reference_file_path",
                                                           "DMS_data_folder", "structure_data_folder", "DMS_index",
                                                           "output_scores_folder", "indel_mode"]
    foldseek = saprot_ref.write_stand_in_foldseek(tmp_path)
    ref = pd.read_csv(os.path.join(GOLDEN, "TOY_SAPROT_REFERENCE.csv")).set_index("DMS_id")
    two = ref.loc["TOY_SAPROT_TWO"]
    muts = pd.read_csv(os.path.join(GOLDEN, "TOY_SAPROT_TWO.csv"))["mutant"].tolist()
    seq = two["target_seq"]
    # both errors come before any forward: no model is needed to meet them
    with pytest.raises(ValueError, match="structure string has 40 letters"):
        cli.score_assay(None, foldseek, STRUCT_DIR, seq, two["pdb_file"].split("|"), ["1-39", "41-80"], muts)
    a, b = (f"{seq[p]}{p + 1}{'A' if seq[p] != 'A' else 'C'}" for p in (50, 10))
    with pytest.raises(ValueError, match=f"mutant {a}:{b}"):
        cli.score_assay(None, foldseek, STRUCT_DIR, seq, two["pdb_file"].split("|"), two["pdb_range"].split("|"), [a + ":" + b])
