"""ProGen2 host logic without a GPU: tokenizer, the chunk / mirror / terminal plan of compute_fitness.py, the terminal rule keyed on
the mutated_sequence column, weight packing (a float64 numpy forward over the packed blob against the reference's golden output),
the CLI's flags and the library's configuration check."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pandas as pd
import pytest

from proteingym_amd import _lib, progen2 as pg, synthetic as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOY = {"h32": (256, 8, 16, 11), "h64": (512, 8, 32, 12), "h64_full_rotary": (512, 8, 64, 13), "h80": (640, 8, 32, 14),
       "h96": (768, 8, 48, 15), "h128": (1024, 8, 64, 16),
       "h256": (2048, 8, 64, 17), "h256_full_rotary": (2048, 8, 256, 18)}


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "golden_progen2.npz"))


def test_tokenizer_matches_frozen_reference_table(golden):
    chars = [str(c) for c in golden["tok_chars"]]
    assert [pg.TOKENS[c] for c in chars] == golden["tok_ids"].tolist()
    assert pg.encode(str(golden["tok_text"])).tolist() == golden["tok_text_ids"].tolist()
    assert len(pg.TOKENS) == 27 and "J" not in pg.TOKENS
    with pytest.raises(ValueError, match="vocabulary"):
        pg.encode("MKJ")


def test_chunk_mirror_plan():
    plan = pg.scoring_plan(["1ABC2", "A" * 20], 16)
    # short sequence: itself then its reverse; 20 >= 16: two chunks (16 + 4), each followed by its reverse
    assert [len(ids) for _, ids in plan] == [5, 5, 16, 16, 4, 4]
    assert plan[1][1].tolist() == pg.encode("2CBA1").tolist()
    assert [i for i, _ in plan] == [0, 0, 1, 1, 1, 1]
    assert pg.kept_targets(pg.encode("1ABC2")) == 3 and pg.kept_targets(pg.encode("2CBA1")) == 3
    assert pg.kept_targets(pg.encode("ABC")) == 2
    # the reference builds 1 + int(len / n) chunks: len 32 at n = 16 gives a third, empty chunk
    assert pg.chunks("A" * 32, 16) == ["A" * 16, "A" * 16, ""]


@pytest.mark.parametrize("length", [16, 17])
def test_degenerate_chunk_raises_naming_the_row(length):
    with pytest.raises(ValueError, match=r"sequence 1 \(length %d\)" % length):
        pg.scoring_plan(["ACD", "A" * length], 16)


def test_interior_terminal_raises_naming_the_row():
    # a mutated_sequence column scored as it is: a '2' inside the chunk is a target the reference's assertion refuses
    with pytest.raises(ValueError, match=r"sequence 2: a '1' / '2' terminal at position 2"):
        pg.scoring_plan(["ACD", "1ACD2", "AC2DE"], 16)


def test_zero_kept_targets_give_nan():
    # "A2": one target, the terminal '2', dropped -> an empty mean (NaN in the reference); "2A" keeps its target
    plan = pg.scoring_plan(["A2"], 16)
    kept = [pg.kept_targets(ids) for _, ids in plan]
    assert kept == [0, 1]
    assert np.isnan(pg.combine(["A2"], plan, np.array([0.0, -1.0], np.float32), np.array(kept))[0])
    s = pg.combine(["AC"], pg.scoring_plan(["AC"], 16), np.array([-1.0, -3.0], np.float32), np.array([1, 1]))
    assert s[0] == pytest.approx((-1.0 - 3.0) / 2 / 2)


def test_terminals_only_without_mutated_sequence_column():
    df = pd.DataFrame({"mutant": ["A1C", "C2A"]})
    assert pg.sequences_to_score(df, "ACD", indel_mode=False) == ["1CCD2", "1AAD2"]
    df2 = df.assign(mutated_sequence=["CCD", "AAD"])
    assert pg.sequences_to_score(df2, "ACD", indel_mode=False) == ["CCD", "AAD"]
    assert pg.sequences_to_score(df2, "ACD", indel_mode=True) == ["CCD", "AAD"]


def _layernorm(x, w, b, eps):
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * w + b


def numpy_forward(cfg, blob, ids):
    """float64 ProGen2 forward over the C ABI blob (include/pgmi.h order, q | k | v projection): log-softmax [T, 32]."""
    D, F, V, H, L = cfg["embed_dim"], cfg["ffn_dim"], cfg["vocab"], cfg["heads"], cfg["layers"]
    dh, rd, eps = D // H, cfg["rotary_dim"], cfg["ln_eps"]
    w = blob.astype(np.float64)
    o = 0

    def take(*shape):
        nonlocal o
        n = int(np.prod(shape))
        a = w[o:o + n].reshape(shape)
        o += n
        return a
    wte = take(V, D)
    T = len(ids)
    x = wte[ids]
    inv = (1.0 / np.power(np.float32(10000.0), (np.arange(0, rd, 2) / np.float32(rd)).astype(np.float32))).astype(np.float32)
    ang = (np.arange(T, dtype=np.float32)[:, None] * inv[None, :]).astype(np.float64)   # fp32 angle, as the reference
    sin, cos = np.repeat(np.sin(ang), 2, -1)[:, None, :], np.repeat(np.cos(ang), 2, -1)[:, None, :]

    def rot(t):
        r, p = t[..., :rd], t[..., rd:]
        r2 = np.stack([-r[..., 1::2], r[..., ::2]], -1).reshape(r.shape)
        return np.concatenate([r * cos + r2 * sin, p], -1)
    mask = np.tril(np.ones((T, T), bool))
    for _ in range(L):
        ln_w, ln_b = take(D), take(D)
        wqkv, wo = take(3 * D, D), take(D, D)
        w1, b1, w2, b2 = take(F, D), take(F), take(D, F), take(D)
        h = _layernorm(x, ln_w, ln_b, eps)
        qkv = h @ wqkv.T
        q, k, v = (qkv[:, i * D:(i + 1) * D].reshape(T, H, dh) for i in range(3))
        q, k = rot(q), rot(k)
        s = np.einsum("thd,shd->hts", q, k) / np.sqrt(dh)
        s = np.where(mask[None], s, -1e9)
        p = np.exp(s - s.max(-1, keepdims=True))
        p /= p.sum(-1, keepdims=True)
        a = np.einsum("hts,shd->thd", p, v).reshape(T, D) @ wo.T
        u = h @ w1.T + b1
        g = 0.5 * u * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) * (u + 0.044715 * u ** 3)))
        x = x + a + (g @ w2.T + b2)
    lnf_w, lnf_b = take(D), take(D)
    head_w, head_b = take(V, D), take(V)
    assert o == w.size
    logits = _layernorm(x, lnf_w, lnf_b, eps) @ head_w.T + head_b
    logits -= logits.max(-1, keepdims=True)
    return logits - np.log(np.exp(logits).sum(-1, keepdims=True))


@pytest.mark.parametrize("name", ["h32", "h64_full_rotary", "h80", "h96", "h256"])
def test_packed_blob_numpy_forward_matches_reference(golden, name):
    D, H, rd, seed = TOY[name]
    cfg = S.progen2_config(2, D, H, rd, n_positions=96)
    blob = pg.pack(cfg, S.progen2_state_dict(cfg, seed))
    assert blob.size == pg.weight_count(cfg)
    for T in (20, 77):
        ids, ref = golden[f"{name}_T{T}_ids"], golden[f"{name}_T{T}_lp"]
        for b in range(ids.shape[0]):
            lp = numpy_forward(cfg, blob, ids[b])
            # the golden rows are the reference's fp32 output: what is left is its own rounding
            assert np.abs(lp - ref[b]).max() < 2e-5, (name, T, b, np.abs(lp - ref[b]).max())


def test_qkv_reorder_is_the_mp8_split():
    D, H = 64, 8
    dh = D // H
    w = np.arange(3 * D, dtype=np.float32)[:, None] * np.ones((1, D), np.float32)
    r = pg.qkv_to_qkv_order(w, H)[:, 0].astype(int)
    local = D // 8
    for h in range(H):
        b, hl = divmod(h, H // 8)
        for j in range(dh):
            base = b * 3 * local + hl * dh + j
            assert r[h * dh + j] == base                       # q: first block of each mp shard
            assert r[D + h * dh + j] == base + 2 * local       # k: third
            assert r[2 * D + h * dh + j] == base + local       # v: second


def test_cli_flags_superset_of_reference():
    from proteingym_amd import score_progen2_proteingym as cli
    ref_flags = {"--Progen2_model_name_or_path", "--DMS_reference_file_path", "--DMS_data_folder", "--DMS_index",
                 "--output_scores_folder", "--indel_mode", "--fp16", "--test"}
    ours = set(re.findall(r"--[A-Za-z0-9_]+", inspect.getsource(cli.parser)))
    assert ref_flags <= ours
    a = cli.parser().parse_args(["--Progen2_model_name_or_path", "x", "--DMS_index", "0", "--indel_mode", "--fp16", "--test"])
    assert a.indel_mode and a.fp16 and a.test and a.DMS_index == 0


def _create_error(D, H, arch=_lib.ARCH_PROGEN2, vocab=32, rotary=16, F=None):
    lib = _lib.load()
    c = _lib.Config(abi_version=_lib.ABI_VERSION, arch=arch, layers=2, embed_dim=D, heads=H, ffn_dim=F or 4 * D, vocab=vocab,
                    max_positions=1024, precision=_lib.PREC_F16X3)
    h = C.c_void_p()
    # no weights: a configuration the check accepts fails on the blob next, before any device is touched
    rc = lib.pgmi_pg2_model_create(C.byref(c), rotary, None, 0, 0, C.byref(h))
    assert rc != 0 and not h.value
    return lib.pgmi_last_error().decode()


@pytest.mark.parametrize("D,H", [(1024, 16), (1536, 16), (2560, 32), (4096, 16), (512, 8), (256, 8)])
def test_check_cfg_accepts_progen2_shapes(D, H):
    assert "weight blob" in _create_error(D, H)


def test_check_cfg_rejects():
    assert "unsupported head_dim 320" in _create_error(5120, 16)           # beyond the four 64-lane slot groups of head_dim 256
    assert "multiple of 8" in _create_error(512, 4)                         # mp_num = 8
    assert "vocab" in _create_error(1024, 16, vocab=33)
    # the other archs keep their rules: head_dim 96 is still refused for ESM2 and Tranception
    lib = _lib.load()
    for arch, vocab in ((_lib.ARCH_ESM2, 33), (_lib.ARCH_TRANCEPTION, 25)):
        c = _lib.Config(abi_version=_lib.ABI_VERSION, arch=arch, layers=2, embed_dim=1536, heads=16, ffn_dim=6144, vocab=vocab,
                        max_positions=1024, precision=_lib.PREC_F16X3)
        h = C.c_void_p()
        assert lib.pgmi_model_create(C.byref(c), None, 0, 0, C.byref(h)) != 0
        assert "unsupported head_dim 96" in lib.pgmi_last_error().decode()
    # a ProGen2 config through the generic entry is refused (it needs rotary_dim)
    c = _lib.Config(abi_version=_lib.ABI_VERSION, arch=_lib.ARCH_PROGEN2, layers=2, embed_dim=1024, heads=16, ffn_dim=4096, vocab=32,
                    max_positions=1024, precision=_lib.PREC_F16X3)
    assert lib.pgmi_model_create(C.byref(c), None, 0, 0, C.byref(C.c_void_p())) != 0
    assert "pgmi_pg2_model_create" in lib.pgmi_last_error().decode()
