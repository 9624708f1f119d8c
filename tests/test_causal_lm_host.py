"""RITA / ProtGPT2 host logic without a GPU: tokenization against the reference's PreTrainedTokenizerFast on both stand-in
tokenizers, the chunk / mirror plan of compute_fitness.py and its degenerate chunks, the batching, the packed blob (a float64 numpy
forward against the reference's golden output), the config checks, the CLIs' flags and the launchers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from causal_lm_ref import numpy_forward
from proteingym_amd import _lib, causal_lm as clm, synthetic as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RITA_TOK = os.path.join(GOLDEN, "rita_toy_tokenizer")
GPT2_TOK = os.path.join(GOLDEN, "protgpt2_toy_tokenizer")
RITA_TOY = {"h32": (128, 4, 21), "h64": (256, 4, 22), "h128": (256, 2, 23)}
GPT2_TOY = {"h32": (128, 4, 31), "h64": (128, 2, 32)}


@pytest.fixture(scope="module")
def g_rita():
    return np.load(os.path.join(GOLDEN, "golden_rita.npz"))


@pytest.fixture(scope="module")
def g_gpt2():
    return np.load(os.path.join(GOLDEN, "golden_protgpt2.npz"))


@pytest.mark.parametrize("which", ["rita", "gpt2"])
def test_tokenization_matches_frozen_reference(which, g_rita, g_gpt2):
    g = g_rita if which == "rita" else g_gpt2
    encode = clm.load_tokenizer(RITA_TOK if which == "rita" else GPT2_TOK)
    for k in range(5):
        assert encode(str(g[f"tok_text_{k}"])).tolist() == g[f"tok_ids_{k}"].tolist(), (which, k)


@pytest.mark.parametrize("which", ["rita", "gpt2"])
def test_tokenization_matches_pretrained_tokenizer_fast(which):
    """The reference's AutoTokenizer is a PreTrainedTokenizerFast over the same file: forward, reversed and multi-chunk text."""
    transformers = pytest.importorskip("transformers")
    path = RITA_TOK if which == "rita" else GPT2_TOK
    ref = transformers.PreTrainedTokenizerFast(tokenizer_file=os.path.join(path, "tokenizer.json"))
    encode = clm.load_tokenizer(path)
    rng = np.random.default_rng(4)
    prot = "".join(rng.choice(list("ACDEFGHIKLMNPQRSTVWY"), 2500))
    for chunk in clm.chunks(prot):
        for p in (chunk, chunk[::-1]):
            assert encode(p).tolist() == ref.encode(p)


def test_bpe_from_vocab_and_merges_equals_tokenizer_json():
    a = clm.load_tokenizer(GPT2_TOK)
    b = clm.load_tokenizer(os.path.join(GPT2_TOK, "tokenizer.json"))
    import shutil, tempfile
    with tempfile.TemporaryDirectory() as d:
        for f in ("vocab.json", "merges.txt"):
            shutil.copy(os.path.join(GPT2_TOK, f), d)
        c = clm.load_tokenizer(d)
        for p in ("MKTAYIAKQRQISFVKSHFSRQ", "QRSFHSKVFSIQRQKAIYATKM"):
            assert a(p).tolist() == b(p).tolist() == c(p).tolist()


def test_chunk_mirror_plan():
    enc = lambda p: np.arange(len(p) + 1, dtype=np.int32)            # noqa: E731  a stand-in adding one special token
    plan = clm.scoring_plan(["ACD", "A" * 25], enc, 10)
    # 25 >= 10: 1 + int(25 / 10) = 3 windows (10, 10, 5), each followed by its reverse
    assert [ids.size for _, ids in plan] == [4, 4, 11, 11, 11, 11, 6, 6]
    assert [i for i, _ in plan] == [0, 0, 1, 1, 1, 1, 1, 1]
    assert clm.chunks("A" * 20, 10) == ["A" * 10, "A" * 10, ""]
    assert clm.chunks("A" * 1022) == ["A" * 1022] and len(clm.chunks("A" * 1023)) == 2


def test_degenerate_chunk_raises_naming_the_sequence():
    enc = clm.load_tokenizer(GPT2_TOK)
    # a length that is a multiple of 1023 leaves an empty last window: zero tokens, the reference's mean CE over nothing is NaN
    with pytest.raises(ValueError, match=r"sequence 1 \(length 2046\)"):
        clm.scoring_plan(["MKT", "A" * 2046], enc)
    with pytest.raises(ValueError, match=r"sequence 0 \(length 1\)"):
        clm.scoring_plan(["A"], enc)                                  # one BPE token, no target


def test_combine_sum_and_mean():
    plan = [(0, None)] * 2 + [(1, None)] * 4
    sums, n = np.array([-4.0, -6.0, -1.0, -2.0, -3.0, -4.0]), np.array([2, 3, 1, 1, 1, 1])
    assert clm.combine(2, plan, sums, n, "rita").tolist() == [-4.0, -10.0]
    assert clm.combine(2, plan, sums, n, "gpt2").tolist() == [-2.0, -2.5]


def test_batches_sort_and_cut_at_tiles():
    lens = [40, 5, 33, 34, 100, 2]
    b = clm.batches(lens)
    assert sorted(j for x in b for j in x) == list(range(6))
    assert [[lens[j] for j in x] for x in b] == [[2, 5, 33], [34, 40], [100]]


@pytest.mark.parametrize("name", list(RITA_TOY))
def test_rita_packed_blob_numpy_forward_matches_reference(g_rita, name):
    D, H, seed = RITA_TOY[name]
    cfg = S.rita_config(2, D, H)
    blob = clm.pack(cfg, S.rita_state_dict(cfg, seed))
    assert blob.size == clm.weight_count(cfg)
    for T in (20, 77):
        ids, ref = g_rita[f"{name}_T{T}_ids"], g_rita[f"{name}_T{T}_lp"]
        for b in range(ids.shape[0]):
            err = np.abs(numpy_forward(cfg, blob, ids[b]) - ref[b]).max()
            assert err < 2e-5, (name, T, b, err)                     # the golden rows are fp32: what is left is their rounding


@pytest.mark.parametrize("name", list(GPT2_TOY))
def test_gpt2_packed_blob_numpy_forward_matches_reference(g_gpt2, name):
    D, H, seed = GPT2_TOY[name]
    cfg = S.gpt2_config(2, D, H, int(g_gpt2["vocab_size"]))
    sd = S.gpt2_state_dict(cfg, seed)
    blob = clm.pack(cfg, sd)
    for T in (20, 77):
        ids, ref = g_gpt2[f"{name}_T{T}_ids"], g_gpt2[f"{name}_T{T}_lp"]
        for b in range(ids.shape[0]):
            err = np.abs(numpy_forward(cfg, blob, ids[b]) - ref[b]).max()
            assert err < 2e-5, (name, T, b, err)


def test_gpt2_packed_blob_matches_float64_transformers_model():
    """1e-6 against transformers' GPT2LMHeadModel run in float64 on the same weights: the Conv1D transposes and the c_attn split."""
    torch = pytest.importorskip("torch")
    transformers = pytest.importorskip("transformers")
    cfg = S.gpt2_config(2, 128, 2, 300, max_positions=128)
    sd = S.gpt2_state_dict(cfg, 5)
    conf = transformers.GPT2Config(vocab_size=300, n_positions=128, n_embd=128, n_layer=2, n_head=2, activation_function="gelu_new",
                                   resid_pdrop=0.0, embd_pdrop=0.0, attn_pdrop=0.0)
    model = transformers.GPT2LMHeadModel(conf)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    model = model.double().eval()
    ids = np.random.default_rng(1).integers(0, 300, 45)
    with torch.no_grad():
        ref = torch.log_softmax(model(torch.tensor(ids)[None]).logits[0], -1).numpy()
    err = np.abs(numpy_forward(cfg, clm.pack(cfg, sd), ids) - ref).max()
    assert err < 1e-6, err


def test_rita_inv_freq_checked():
    cfg = S.rita_config(1, 128, 2)
    sd = S.rita_state_dict(cfg, 1)
    sd["transformer.layers.0.self_attention.rotary_embedding.inv_freq"] = sd["transformer.layers.0.self_attention.rotary_embedding.inv_freq"] * 1.01
    with pytest.raises(ValueError, match="inv_freq"):
        clm.pack(cfg, sd)


def test_config_from_json():
    r = clm.config_from_json(dict(model_type="rita", d_model=2048, num_layers=24, num_heads=16, vocab_size=26, max_seq_len=1024, ff_ratio=4))
    assert (r["family"], r["embed_dim"], r["ffn_dim"], r["embed_dim"] // r["heads"]) == ("rita", 2048, 8192, 128)
    base = dict(model_type="gpt2", n_embd=1280, n_layer=36, n_head=20, vocab_size=50257, n_positions=1024, activation_function="gelu_new")
    g = clm.config_from_json(base)
    assert (g["family"], g["ffn_dim"], g["vocab"], g["max_positions"]) == ("gpt2", 5120, 50257, 1024)
    for bad in (dict(activation_function="relu"), dict(scale_attn_by_inverse_layer_idx=True), dict(reorder_and_upcast_attn=True)):
        with pytest.raises(ValueError):
            clm.config_from_json({**base, **bad})


def test_library_checks_the_config():
    lib = _lib.load() if os.path.exists(_lib.LIB_PATH) else pytest.skip("libpgmi.so not built")
    c = _lib.Config(abi_version=_lib.ABI_VERSION, arch=_lib.ARCH_GPT, layers=2, embed_dim=128, heads=2, ffn_dim=512, vocab=300,
                    max_positions=128, precision=_lib.PREC_F16X3)
    cfg = S.gpt2_config(2, 128, 2, 300, max_positions=128)
    assert lib.pgmi_gpt_weight_count(C.byref(c), _lib.GPT_POS_LEARNED) == clm.weight_count(cfg)
    assert lib.pgmi_gpt_weight_count(C.byref(c), _lib.GPT_POS_ROTARY) == clm.weight_count(dict(cfg, family="rita"))
    assert lib.pgmi_gpt_weight_count(C.byref(c), 7) < 0
    w = np.zeros(clm.weight_count(cfg), np.float32)
    h = C.c_void_p()
    c.precision = _lib.PREC_BF16
    assert lib.pgmi_gpt_model_create(C.byref(c), _lib.GPT_POS_LEARNED, _lib.ptr(w, _lib._f32p), w.size, 0, C.byref(h)) == _lib.EINVAL
    assert b"f16x3" in lib.pgmi_last_error()


@pytest.mark.parametrize("which", ["rita", "protgpt2"])
def test_cli_flags_match_reference_parser(which):
    """Every flag of the reference's parser exists here with the same dest; the additions are --tokenizer_path, --device and
    --max_rows."""
    import ast
    from proteingym_amd import score_protgpt2_proteingym as gcli, score_rita_proteingym as rcli
    ours = {a.dest for a in (rcli if which == "rita" else gcli).parser()._actions} - {"help"}
    ref_flags = {"rita": {"RITA_model_name_or_path"}, "protgpt2": {"ProtGPT2_model_name_or_path"}}[which] | {
        "DMS_reference_file_path", "DMS_data_folder", "DMS_index", "output_scores_folder", "indel_mode"}
    from oracle import ref_harness
    src = os.path.join(ref_harness.REF_ROOT, "proteingym", "baselines", which, "compute_fitness.py")
    if os.path.exists(src):                                          # the reference's own parser, read from its source
        tree = ast.parse(open(src).read())
        ref_flags = {n.args[0].value.lstrip("-") for n in ast.walk(tree) if isinstance(n, ast.Call)
                     and getattr(n.func, "attr", "") == "add_argument"}
    assert ours - ref_flags == {"tokenizer_path", "device", "max_rows"}
    assert ref_flags <= ours


LAUNCHERS = ["scoring_RITA_substitutions.sh", "scoring_RITA_indels.sh", "scoring_ProtGPT2_substitutions.sh", "scoring_ProtGPT2_indels.sh"]


@pytest.mark.parametrize("script", LAUNCHERS)
def test_launchers_echo_a_valid_command_line(script, tmp_path):
    from proteingym_amd import score_protgpt2_proteingym as gcli, score_rita_proteingym as rcli
    root = os.path.dirname(GOLDEN.rstrip("/"))
    root = os.path.dirname(root)
    cfg_dir = tmp_path / "scripts"
    (cfg_dir / "scoring_DMS_zero_shot").mkdir(parents=True)
    (cfg_dir / "zero_shot_config.sh").write_text(
        'export PROTEINGYM_CACHE="/data/pg"\n'
        'export DMS_data_folder_subs="${PROTEINGYM_CACHE}/DMS_ProteinGym_substitutions/"\n'
        'export DMS_data_folder_indels="${PROTEINGYM_CACHE}/DMS_ProteinGym_indels/"\n'
        'export DMS_reference_file_path_subs=../../reference_files/DMS_substitutions.csv\n'
        'export DMS_reference_file_path_indels=../../reference_files/DMS_indels.csv\n'
        'export DMS_output_score_folder_subs="${PROTEINGYM_CACHE}/zero_shot_substitutions_scores/"\n'
        'export DMS_output_score_folder_indels="${PROTEINGYM_CACHE}/zero_shot_indels_scores/"\n')
    env = dict(os.environ, ZERO_SHOT_CONFIG=str(cfg_dir / "zero_shot_config.sh"), PGMI_LAUNCH_ECHO="1", DMS_index="5",
               RITA_tokenizer_path="/models/rita_tok")
    out = subprocess.run(["bash", os.path.join(root, "scripts", "scoring_DMS_zero_shot", script)], env=env, capture_output=True,
                         text=True, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr
    module, *argv = out.stdout.strip().split("\n")
    rita = "RITA" in script
    assert module == ("proteingym_amd.score_rita_proteingym" if rita else "proteingym_amd.score_protgpt2_proteingym")
    a = (rcli if rita else gcli).parser().parse_args(argv)
    indels = "indels" in script
    assert a.DMS_index == 5 and bool(a.indel_mode) == indels
    assert a.DMS_reference_file_path.endswith("DMS_indels.csv" if indels else "DMS_substitutions.csv")
    assert os.path.isabs(a.DMS_reference_file_path)
    assert a.DMS_data_folder.startswith("/data/pg/DMS_ProteinGym_" + ("indels" if indels else "substitutions"))
    assert a.output_scores_folder.startswith("/data/pg/zero_shot_" + ("indels" if indels else "substitutions") + "_scores/")
    assert a.tokenizer_path == ("/models/rita_tok" if rita else None)
