"""ESM-IF1's host side on the CPU against the reference's recorded numbers (tests/golden/golden_esmif1.npz, written by
tests/golden/make_golden_esmif1.py from the unmodified reference): the torch restatement of the encoder in float64 and float32, the NaN-CA
backbone, the direction of the GVP messages, the checkpoint's key renaming and key / shape check, the decoder blob against the library's
count, the CLI's flags against the reference parser's, the backbone reader on the toy PDB, and tests/esmif1_ref.py (the float64 NumPy
decoder the GPU tests use) against the goldens.

Bounds.  float64 against the reference's float64: 1e-10 (the bound of tests/test_poet_host.py).  float32 against its float32: 1e-5.
The reference's cross-attention takes multihead_attention.py's own path, whose softmax is float32 in every run, so its "float64"
log-probabilities carry that rounding: with that float32 softmax handed in, esmif1_ref reproduces them to 1e-10; in float64 throughout
(as the GPU tests use it) it must stay within the reference's own |float32 run - float64 run|, which holds that rounding and more."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import esmif1_cases as K
import esmif1_ref
from proteingym_amd import _lib, esmif1, score_esmif1_proteingym

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(GOLDEN, "golden_esmif1.npz")))


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "esmif1_state_dict_keys.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def toy():
    cfg = esmif1.config_from_args(K.toy_args())
    return cfg, K.state_dict(cfg)


def _pos_table(cfg, n):
    return esmif1._sinusoid(torch.arange(n) + esmif1.PAD + 1, cfg["embed_dim"], esmif1.PAD).numpy()


def _softmax32(a):
    return torch.softmax(torch.from_numpy(a), -1, dtype=torch.float32).double().numpy()


@pytest.mark.parametrize("name", list(K.CASES))
def test_float64_restatement_against_the_reference(toy, golden, name):
    """encoder_out of the restatement, and the log-probabilities / scores of the NumPy decoder on THAT encoder output; `nanca` is the
    backbone with a residue whose CA is NaN."""
    cfg, sd = toy
    coords, seqs = K.case(name)
    enc = esmif1.Encoder(cfg, sd, "cpu", torch.float64).encode(coords)
    assert enc.shape == (len(coords) + 2, cfg["enc_dim"])
    err = float(np.abs(enc - golden[f"{name}_enc64"]).max())
    print(f"esmif1 float64 {name} encoder_out err={err:.3e}")
    assert err < 1e-10
    for i, s in enumerate(seqs):
        t = esmif1.tokenize(s)
        lp = esmif1_ref.decoder_logprobs(cfg, sd, enc, t[:-1], _pos_table(cfg, len(s)), cross_softmax=_softmax32)
        err, serr = float(np.abs(lp - golden[f"{name}_lp64_{i}"]).max()), abs(esmif1_ref.score(lp, t) - golden[f"{name}_ll64"][i])
        print(f"esmif1 float64 {name} seq {i} lp err={err:.3e} score err={serr:.3e}")
        assert err < 1e-10 and serr < 1e-10


@pytest.mark.parametrize("name", list(K.CASES))
def test_float32_restatement_against_the_reference(toy, golden, name):
    cfg, sd = toy
    coords, _ = K.case(name)
    enc = esmif1.Encoder(cfg, sd, "cpu", torch.float32).encode(coords)
    err = float(np.abs(enc - golden[f"{name}_enc32"]).max())
    print(f"esmif1 float32 {name} encoder_out err={err:.3e}")
    assert err < 1e-5


@pytest.mark.parametrize("name", list(K.CASES))
def test_numpy_decoder_in_float64_throughout(toy, golden, name):
    cfg, sd = toy
    _, seqs = K.case(name)
    for i, s in enumerate(seqs):
        t = esmif1.tokenize(s)
        lp = esmif1_ref.decoder_logprobs(cfg, sd, golden[f"{name}_enc64"], t[:-1], _pos_table(cfg, len(s)))
        own = float(np.abs(golden[f"{name}_lp32_{i}"] - golden[f"{name}_lp64_{i}"]).max())
        err = float(np.abs(lp - golden[f"{name}_lp64_{i}"]).max())
        print(f"esmif1 numpy float64 {name} seq {i} err={err:.3e} reference float32 - float64={own:.3e}")
        assert err < own


def test_nan_ca_residue_gets_no_edges_and_confidence_zero(toy):
    """The NaN-CA residue and the two end rows keep no edge at all; every other residue keeps its own (self) edge."""
    cfg, sd = toy
    coords, _ = K.case("nanca")
    nan_at = K.CASES["nanca"][2][0] + 1                        # + 1: the converter's leading inf row
    enc = esmif1.Encoder(cfg, sd, "cpu", torch.float64)
    c = torch.nn.functional.pad(torch.as_tensor(coords, dtype=torch.float64), (0, 0, 0, 0, 1, 1), value=float("inf"))
    mask = torch.isfinite(c).all(-1).all(-1)
    node, nb, dist = enc.graph(torch.where(torch.isfinite(c), c, torch.zeros((), dtype=c.dtype)), mask, torch.zeros(len(c), dtype=torch.bool))
    S = len(c)
    dropped = {0, nan_at, S - 1}
    assert not dropped & set(node.tolist()) and not dropped & set(nb.tolist())
    assert all((node == i).sum() == min(cfg["top_k"], S - 3) and ((node == i) & (nb == i)).sum() == 1 for i in set(range(S)) - dropped)
    assert float(dist.max()) < 5e7


def test_messages_are_averaged_at_the_neighbour(toy):
    """edge_index[0] is the node and edge_index[1] its neighbour; the mean lands at edge_index[1], and a node that no neighbour list
    contains receives a zero message."""
    cfg, sd = toy
    enc = esmif1.Encoder(cfg, sd, "cpu", torch.float64)
    g = torch.Generator().manual_seed(1)
    n, ns, nv, es, ev = 5, cfg["node_s"], cfg["node_v"], cfg["edge_s"], cfg["edge_v"]
    s, v = torch.randn(n, ns, generator=g, dtype=torch.float64), torch.randn(n, nv, 3, generator=g, dtype=torch.float64)
    node, nb = torch.tensor([0, 0, 2, 4]), torch.tensor([1, 2, 1, 4])          # nodes 0 and 3 are in nobody's list
    e_s, e_v = torch.randn(4, es, generator=g, dtype=torch.float64), torch.randn(4, ev, 3, generator=g, dtype=torch.float64)
    p = "encoder.gvp_encoder.encoder_layers.0.conv."
    out_s, out_v = enc.message(p, s, v, e_s, e_v, node, nb)
    assert torch.all(out_s[[0, 3]] == 0) and torch.all(out_v[[0, 3]] == 0)
    assert all(out_s[i].abs().max() > 0 for i in (1, 2, 4))
    one_s, _ = enc.message(p, s, v, e_s[[0, 2]], e_v[[0, 2]], node[[0, 2]], nb[[0, 2]])       # the two edges that point at node 1
    assert torch.allclose(one_s[1], out_s[1], rtol=0, atol=1e-14) and torch.all(one_s[[0, 2, 3, 4]] == 0)
    a, _ = enc.message(p, s, v, e_s[[0]], e_v[[0]], node[[0]], nb[[0]])
    b, _ = enc.message(p, s, v, e_s[[2]], e_v[[2]], node[[2]], nb[[2]])
    assert torch.allclose(out_s[1], (a[1] + b[1]) / 2, rtol=0, atol=1e-14)                  # the mean, not the sum


def test_expected_keys_are_the_reference_models_keys(recorded):
    for name, args in (("toy", K.TOY_ARGS), ("released", K.RELEASED_ARGS)):
        want = {k: tuple(s) for k, s in recorded[name] if not k.endswith("_float_tensor")}
        assert esmif1.expected_shapes(esmif1.config_from_args(args)) == want, name
        assert sum(k.endswith("_float_tensor") for k, _ in recorded[name]) == 2


OLD_NAMES = (("encoder.gvp_encoder.embed_graph.embed_confidence.", "encoder.gvp_encoder.embed_score."),
             ("encoder.embed_confidence", "encoder.embed_scores.0"), ("embed_graph.embed_node", "W_v"), ("embed_graph.embed_edge", "W_e"),
             ("decoder.output_projection", "decoder.seq_logits_projection.output_projection"), ("embed_dihedrals", "embed_ingraham_features"),
             ("embed_gvp_output", "embed_gvp_in_local_frame.0"), ("embed_gvp_input_features", "embed_features_in_local_frame.0"))


def _released_style(sd):
    out = {}
    for k, v in sd.items():
        for new, old in OLD_NAMES:
            k = k.replace(new, old)
        out[k] = v
    out["decoder.version"] = np.zeros(1, np.float32)
    out["encoder.embed_positions._float_tensor"] = np.zeros(1, np.float32)
    return out


def test_key_renaming_and_strict_check(toy):
    cfg, sd = toy
    old = _released_style(sd)
    assert "encoder.gvp_encoder.W_v.0.wh.weight" in old and "encoder.embed_scores.0.weight" in old and set(old) != set(sd)
    checked = esmif1.check_state_dict(cfg, esmif1.rename_state_dict(old))
    assert set(checked) == set(sd) and all(checked[k] is sd[k] for k in sd)
    missing = dict(old)
    del missing["decoder.layers.1.encoder_attn.k_proj.weight"]
    with pytest.raises(RuntimeError, match="Missing key"):
        esmif1.check_state_dict(cfg, esmif1.rename_state_dict(missing))
    with pytest.raises(RuntimeError, match="Unexpected key"):
        esmif1.check_state_dict(cfg, esmif1.rename_state_dict(dict(old, **{"decoder.layers.0.extra.weight": np.zeros(1)})))
    wrong = dict(sd, **{"decoder.layers.0.fc1.weight": np.zeros((3, 3), np.float32)})
    with pytest.raises(RuntimeError, match="shape"):
        esmif1.check_state_dict(cfg, wrong)
    with pytest.raises(ValueError, match="not an ESM-IF1"):
        esmif1.config_from_args(dict(K.TOY_ARGS, arch="roberta_large"))


def test_blob_order_and_size_against_the_library(toy):
    cfg, sd = toy
    blob = esmif1.pack_decoder(cfg, sd)
    c = _lib.Config(abi_version=_lib.ABI_VERSION, arch=_lib.ARCH_ESMIF1, layers=cfg["layers"], embed_dim=cfg["embed_dim"], heads=cfg["heads"],
                    ffn_dim=cfg["ffn_dim"], vocab=cfg["vocab"], max_positions=64, precision=_lib.PREC_F16X3)
    assert _lib.load().pgmi_esmif1_weight_count(C.byref(c), cfg["enc_dim"]) == blob.size == esmif1.weight_count(cfg)
    assert _lib.load().pgmi_weight_count(C.byref(c)) == -1
    rel = esmif1.config_from_args(K.RELEASED_ARGS)
    c.layers, c.embed_dim, c.heads, c.ffn_dim = rel["layers"], rel["embed_dim"], rel["heads"], rel["ffn_dim"]
    assert _lib.load().pgmi_esmif1_weight_count(C.byref(c), rel["enc_dim"]) == esmif1.weight_count(rel)
    o = 0
    for k in esmif1.decoder_keys(cfg):                          # the documented order: every tensor where the header says it is
        assert np.array_equal(blob[o:o + sd[k].size], sd[k].ravel()), k
        o += sd[k].size
    keys = esmif1.decoder_keys(cfg)
    assert keys[0] == "decoder.embed_tokens.weight" and keys[-1] == "decoder.output_projection.weight"
    p = "decoder.layers.0."
    assert keys[1:11] == [p + "self_attn_layer_norm.weight", p + "self_attn_layer_norm.bias"] + \
        [p + f"self_attn.{n}_proj.{w}" for n in ("q", "k", "v", "out") for w in ("weight", "bias")]
    assert set(keys) == {k for k in sd if k.startswith("decoder.")}


def test_cli_flags_are_the_reference_parsers(recorded):
    mine = {s for a in score_esmif1_proteingym.parser()._actions for s in a.option_strings}
    assert set(recorded["cli_flags"]) <= mine
    assert mine - set(recorded["cli_flags"]) == {"-h", "--help", "--device", "--max_batch", "--max_rows"}
    args = score_esmif1_proteingym.parser().parse_args(["--multichain-backbone", "--chain", "B"])
    assert args.multichain_backbone and args.chain == "B" and args.batch_size == 1
    with pytest.raises(SystemExit, match="nogpu"):
        score_esmif1_proteingym.main(["--nogpu"])


def test_backbone_reader_on_the_toy_pdb():
    fname, L, seed, nan_ca, first = K.TOY_PDB
    coords, seq = esmif1.read_backbone(os.path.join(GOLDEN, "ESMIF1_structures", fname), "A")
    want = K.backbone(seed, L, nan_ca)
    assert coords.shape == (L, 3, 3) and seq == K.sequence_of(seed, L)
    assert np.array_equal(np.isnan(coords), np.isnan(want)) and np.isnan(coords[nan_ca[0], 1]).all()
    assert np.allclose(coords[np.isfinite(want)], want[np.isfinite(want)], rtol=0, atol=5e-4)
    with pytest.raises(ValueError, match="Chain B not found"):
        esmif1.read_backbone(os.path.join(GOLDEN, "ESMIF1_structures", fname), "B")
    lines = open(os.path.join(GOLDEN, "ESMIF1_structures", fname)).read().splitlines()
    other = [ln[:21] + "B" + ln[22:] for ln in lines[:6]]                              # a second chain and a hetero atom are left out
    both, _ = esmif1.read_backbone(other + ["HETATM" + lines[0][6:]] + lines, "A")
    assert np.array_equal(np.isnan(both), np.isnan(coords)) and np.array_equal(both[np.isfinite(both)], coords[np.isfinite(coords)])
    every, _ = esmif1.read_backbone(other + lines, None)
    assert len(every) == L + 2


def test_tokens():
    assert esmif1.N_VOCAB == 35 and (esmif1.PAD, esmif1.MASK, esmif1.CATH) == (1, 32, 33)
    assert esmif1.tokenize("LAJ").tolist() == [33, 4, 5, 3]
