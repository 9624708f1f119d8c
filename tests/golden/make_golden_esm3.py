"""Writes tests/golden/golden_esm3.npz, esm3_state_dict_keys.json, ESM3_structures/*.pdb and the TOY_ESM3_* CSVs from the UNMODIFIED
reference ESM3 (proteingym/baselines/evoscale: compute_fitness.py, esm/models/{esm3,vqvae}.py, esm/layers/geom_attention.py) on CPU
in fp32.

    python tests/golden/make_golden_esm3.py

Weights are proteingym_amd.synthetic.esm3_state_dict / esm3_encoder_state_dict(cfg, seed) and the structures tests/esm3_cases.py's
seeded backbones: the tests rebuild them, so no checkpoint is committed.  Modules the image lacks are stubbed empty as in
make_golden_esmc.py.  Nothing here reaches data_root(): the tokenizer collection is built by hand (sequence and structure
tokenizers only) and the structure encoder is handed in as structure_encoder_fn.

ProteinChain.from_pdb needs biotite, which the image lacks, so the reference's own PDB reading cannot run.  For the TOY_ESM3_*
assays the module attribute compute_fitness.ProteinChain is replaced by a loader that returns proteingym_amd.esm3.read_pdb's
sequence, atom37_positions, residue_index and insertion_code for the committed toy PDB; everything after that line of
score_mutations_with_pdb runs unmodified.  The PDB-to-arrays step therefore has no executable oracle here.

What the file holds besides the reference's outputs:
  op_dev_<case>   max |fp32 - float64| of GeometricReasoningOriginalImpl.forward on the op case's inputs (its s_norm, proj and out_proj
                  replaced by nn.Identity on the instance, so that the inputs are the projection's output): the op test's tolerance
                  is 4 x this.
  tok_<case>_*    the reference's structure tokens, the relative margin (second-best - best) / best of the codebook distances, and
                  tok_dev: the largest |fp32 - float64| distance over the best distance.  Token equality is required where the margin
                  is at least 100 x tok_dev; the script asserts that at most 10 % of a case's positions fall below that, and none of a
                  toy assay's structures.
Needs the reference tree and torch (build container only).
"""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import esm3_cases as K  # noqa: E402
from make_golden_esmc import EVOSCALE, _StubFinder  # noqa: E402
from proteingym_amd import esm3 as E  # noqa: E402

AA = K.AA


def reference():
    sys.meta_path.insert(0, _StubFinder())
    sys.path.insert(0, EVOSCALE)
    import compute_fitness as cf
    from esm.layers.geom_attention import GeometricReasoningOriginalImpl
    from esm.models.esm3 import ESM3
    from esm.models.vqvae import StructureTokenEncoder
    from esm.tokenization import EsmSequenceTokenizer, StructureTokenizer
    from esm.utils.structure.affine3d import Affine3D, RotationMatrix
    return types.SimpleNamespace(cf=cf, Geom=GeometricReasoningOriginalImpl, ESM3=ESM3, Encoder=StructureTokenEncoder, Seq=EsmSequenceTokenizer,
                                 Struct=StructureTokenizer, Affine3D=Affine3D, RotationMatrix=RotationMatrix)


def load(module, sd):
    import torch
    module.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return module.eval()


def build_encoder(R):
    cfg, sd = K.encoder_model()
    return load(R.Encoder(cfg["d_model"], 1, cfg["v_heads"], cfg["layers"], cfg["d_out"], cfg["n_codes"]), sd)


def build_model(R, name, enc):
    cfg, sd = K.trunk_model(name)
    tok = types.SimpleNamespace(sequence=R.Seq(), structure=R.Struct())
    return load(R.ESM3(cfg["embed_dim"], cfg["heads"], cfg["v_heads"], cfg["layers"], lambda device: enc, None, None, tok), sd)


def float64_reference(on):
    """Two places of the reference pin fp32 and stop a float64 run: geom_attention.py:61 fills its float32 bias with
    finfo(s.dtype).min, which overflows for float64 activations, and RotationMatrix.__init__ casts every rotation to torch.float32.
    While `on`, the `torch` global of those two modules is a proxy whose finfo is float32's (the same fill value as in the fp32 run;
    exp() of it is 0 either way) and whose float32 is float64.  The reference's files are untouched."""
    import torch
    import esm.layers.geom_attention as ga
    import esm.utils.structure.affine3d as a3

    class _Torch:
        float32 = torch.float64

        def __getattr__(self, a):
            return getattr(torch, a)

        @staticmethod
        def finfo(_dtype):
            return torch.finfo(torch.float32)
    ga.torch = a3.torch = _Torch() if on else torch


def op_deviation(R, name):
    import torch
    proj, rot, trans, mask, w_rot, w_dist = K.op_case(name)
    B, S, W = proj.shape
    H = W // 15
    n = rot.shape[0]
    out = {}
    for dt in (torch.float32, torch.float64):
        float64_reference(dt == torch.float64)
        mod = R.Geom(c_s=W, v_heads=H)
        mod.s_norm, mod.proj, mod.out_proj = torch.nn.Identity(), torch.nn.Identity(), torch.nn.Identity()
        # softplus^-1 of the case's weights, so that the module's own softplus gives them back
        mod.rotation_scale_per_head.data = torch.log(torch.expm1(torch.from_numpy(w_rot.astype(np.float64))))
        mod.distance_scale_per_head.data = torch.log(torch.expm1(torch.from_numpy(w_dist.astype(np.float64))))
        mod = mod.to(dt)
        r = torch.from_numpy(np.broadcast_to(rot, (B,) + rot.shape[1:]).copy() if n == 1 else rot).to(dt).reshape(B, S, 3, 3)
        t = torch.from_numpy(np.broadcast_to(trans, (B,) + trans.shape[1:]).copy() if n == 1 else trans).to(dt)
        m = torch.from_numpy(np.broadcast_to(mask, (B, S)).copy() if n == 1 else mask).bool()
        with torch.no_grad():
            out[dt] = mod(torch.from_numpy(proj).to(dt), R.Affine3D(t, R.RotationMatrix(r)), m, None, torch.zeros(B, S, dtype=torch.int64)).double()
    float64_reference(False)
    import esm3_ref
    ours = np.stack([esm3_ref.geom_attention(proj[b], rot[b if n > 1 else 0].reshape(S, 3, 3), trans[b if n > 1 else 0], mask[b if n > 1 else 0],
                                             w_rot, w_dist) for b in range(B)])
    ref64 = out[torch.float64].numpy()
    framed = np.broadcast_to(mask, (B, S)).astype(bool) if n == 1 else mask.astype(bool)
    # the float64 numpy reading of the formula equals the module in float64 wherever the query has a frame (frameless rows: zero)
    assert np.abs(ours - ref64)[framed].max() < 1e-9, (name, np.abs(ours - ref64)[framed].max())
    assert np.all(ref64[~framed] == 0) and np.all(ours[~framed] == 0)
    return float((out[torch.float32] - out[torch.float64]).abs().max())


def tokenizer_case(R, enc, atom37):
    """Reference tokens, margins and the fp32-vs-float64 distance deviation for one chain [L,37,3]."""
    import copy

    import torch
    from esm.utils.structure.protein_chain import ProteinChain
    chain = ProteinChain.from_atom37(torch.from_numpy(atom37))
    coords, _, residue_index = chain.to_structure_encoder_inputs()
    grabbed = {}

    def run(e, c):
        orig = e.codebook.forward

        def fwd(z):
            flat = z.view(-1, e.codebook.embedding_dim)
            grabbed["d"] = ((flat ** 2).sum(dim=1, keepdim=True) - 2 * flat @ e.codebook.embeddings.t()
                            + (e.codebook.embeddings.t() ** 2).sum(dim=0, keepdim=True)).double().numpy()
            return orig(z)
        e.codebook.forward = fwd
        with torch.no_grad():
            _, tok = e.encode(c, residue_index=residue_index)
        e.codebook.forward = orig
        return tok[0].numpy(), grabbed["d"]
    tok32, d32 = run(enc, coords)
    float64_reference(True)
    _, d64 = run(copy.deepcopy(enc).double(), coords.double())
    float64_reference(False)
    assert np.array_equal(tok32, d32.argmin(1))
    srt = np.sort(d64, axis=1)
    best = srt[:, 0]
    margin = (srt[:, 1] - best) / best
    dev = float((np.abs(d32 - d64).max(1) / best).max())
    return tok32.astype(np.int32), margin, dev, bool(np.array_equal(tok32, d64.argmin(1)))


def main():
    import pandas as pd
    import torch
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    R = reference()
    cf = R.cf
    out = {}

    # the reference's key names and shapes at the released configurations (meta tensors: no weights allocated)
    tok = types.SimpleNamespace(sequence=R.Seq(), structure=R.Struct())
    with torch.device("meta"):
        m = R.ESM3(1536, 24, 256, 48, lambda device: None, None, None, tok)
        e = R.Encoder(d_model=1024, n_heads=1, v_heads=128, n_layers=2, d_out=128, n_codes=4096)
    keys = {"esm3_open": [[k, list(v.shape)] for k, v in m.state_dict().items()],
            "structure_encoder": [[k, list(v.shape)] for k, v in e.state_dict().items()]}
    with open(os.path.join(HERE, "esm3_state_dict_keys.json"), "w") as f:
        json.dump(keys, f, indent=0)

    for name in K.OP_CASES:
        out[f"op_dev_{name}"] = np.float64(op_deviation(R, name))
        print("op", name, out[f"op_dev_{name}"], flush=True)

    enc = build_encoder(R)
    devs = []
    for name, (L, seed, missing) in K.TOKENIZER.items():
        tokens, margin, dev, same64 = tokenizer_case(R, enc, K.toy_backbone(seed, L, missing))
        out[f"tok_{name}_tokens"], out[f"tok_{name}_margin"] = tokens, margin
        devs.append(dev)
        print("tokenizer", name, "dev", dev, "min margin", margin.min(), "fp32 == float64 argmin", same64, flush=True)
    out["tok_dev"] = np.float64(max(devs))
    for name in K.TOKENIZER:
        below = float((out[f"tok_{name}_margin"] < 100 * out["tok_dev"]).mean())
        print("tokenizer", name, "share below 100 x tok_dev:", below, flush=True)
        assert below <= 0.10, (name, below)

    # trunk: masked-row log-probabilities with the structure (tokens and coordinates as the model gets them) and sequence only
    rng = np.random.default_rng(2026)
    for name, (D, layers, Hv, seed, L, bseed, nan_at) in K.TRUNK.items():
        model = build_model(R, name, enc)
        seq = K.sequence_of(bseed, L)
        from esm.sdk.api import ESMProtein, LogitsConfig
        import attr
        pos = np.array(sorted(rng.choice(np.arange(1, L + 1), 4, replace=False)), dtype=np.int32)
        for tag, protein in (("st", ESMProtein(sequence=seq, coordinates=torch.from_numpy(K.toy_backbone(bseed, L, (nan_at,))))),
                             ("seq", ESMProtein(sequence=seq))):
            pt = model.encode(protein)
            mlp = []
            for p in pos:
                t = pt.sequence.clone()
                t[p] = 32
                lo = model.logits(attr.evolve(pt, sequence=t), LogitsConfig(sequence=True))
                mlp.append(torch.log_softmax(lo.logits.sequence[0, p], -1).numpy())
            out[f"{name}_{tag}_mask_lp"] = np.stack(mlp).astype(np.float32)
            if tag == "st":
                out[f"{name}_ids"] = pt.sequence.numpy().astype(np.int32)
                out[f"{name}_structure_tokens"] = pt.structure.numpy().astype(np.int32)
                out[f"{name}_coords"] = pt.coordinates[:, :3, :].numpy().astype(np.float32)
        out[f"{name}_mask_pos"] = pos
        assert np.abs(out[f"{name}_st_mask_lp"] - out[f"{name}_seq_mask_lp"]).max() > 1e-2          # the structure path is live
        print(name, "done", flush=True)
        del model
    np.savez_compressed(os.path.join(HERE, "golden_esm3.npz"), **out)

    # toy assays through compute_fitness.score_mutations_with_pdb / score_mutations
    os.makedirs(os.path.join(HERE, "ESM3_structures"), exist_ok=True)
    model = build_model(R, K.TOY_MODEL[0], enc)
    cf.ProteinChain = types.SimpleNamespace(from_pdb=lambda path, chain_id=None: E.read_pdb(path, chain_id))
    srng = np.random.default_rng(12)
    seqs = {}
    for fname, (L, seed, hole, first) in K.TOY_PDBS.items():
        seqs[fname] = K.sequence_of(seed, L)
        atom37 = K.toy_backbone(seed, L, (hole,))
        with open(os.path.join(HERE, "ESM3_structures", fname), "w") as f:
            f.write(K.pdb_text(seqs[fname], atom37, first))
        chain = E.read_pdb(os.path.join(HERE, "ESM3_structures", fname))
        _, margin, dev, _ = tokenizer_case(R, enc, chain.atom37_positions)
        thr = 100 * max(dev, float(out["tok_dev"]))
        framed = np.isfinite(chain.atom37_positions[:, :3]).all(-1).all(-1)
        print(fname, "min margin of framed residues", margin[framed].min(), "threshold", thr, flush=True)
        assert margin[framed].min() >= thr, "pick another backbone seed"

    def sub(tgt, p, number):
        return f"{tgt[p]}{number}{srng.choice([a for a in AA if a != tgt[p]])}"
    s0, s1 = seqs["toy_esm3.pdb"], seqs["toy_esm3_range.pdb"]
    # STRUCT: PDB numbering = target numbering; singles, multis, a position outside the PDB, an unparsable part, a wrong wild type
    # (no wild-type check on this path: it is scored), the residue without a frame
    m0 = [sub(s0, int(p), int(p) + 1) for p in srng.choice(40, 10, replace=False)]
    m0 += [":".join(sub(s0, int(p), int(p) + 1) for p in sorted(srng.choice(40, k, replace=False))) for k in (2, 3)]
    m0 += [m0[0], f"{s0[3]}41C", f"{s0[2]}3D:{s0[9]}99E", "x3Y", f"{next(a for a in AA if a != s0[4])}5A", sub(s0, 12, 13)]
    # RANGE: the PDB numbers residues 5 .. 40 and covers target positions 15 .. 50 (pdb_range 11-50: offset 10)
    tgt1 = K.sequence_of(83, 14) + s1 + K.sequence_of(84, 10)
    m1 = [sub(s1, int(p), int(p) + 5 + 10) for p in srng.choice(36, 8, replace=False)]
    m1 += [f"{tgt1[3]}4A", f"{tgt1[13]}14C", f"{tgt1[50]}51D", sub(s1, 0, 15) + ":" + sub(s1, 35, 50), sub(s1, 1, 16) + ":" + f"{tgt1[2]}3A"]
    m2 = [sub(s0, int(p), int(p) + 1) for p in srng.choice(40, 8, replace=False)] + [f"{next(a for a in AA if a != s0[4])}5A", f"{s0[0]}41C"]
    files = [("TOY_ESM3_STRUCT", m0, s0, "toy_esm3.pdb", ""), ("TOY_ESM3_RANGE", m1, tgt1, "toy_esm3_range.pdb", "11-50"),
             ("TOY_ESM3_SEQONLY", m2, s0, "toy_esm3.pdb", "")]
    pd.DataFrame({"DMS_id": [f[0] for f in files], "target_seq": [f[2] for f in files], "pdb_file": [f[3] for f in files],
                  "pdb_range": [f[4] for f in files]}).to_csv(os.path.join(HERE, "TOY_ESM3_REFERENCE.csv"), index=False)
    for dms_id, mm, tgt, pdb, rng_ in files:
        df = pd.DataFrame({"mutant": mm, "DMS_score": srng.standard_normal(len(mm)).round(4)})
        if dms_id == "TOY_ESM3_SEQONLY":
            scores = cf.score_mutations(tgt, mm, model=model, model_type="esm3_open", window_size=1024)
        else:
            scores = cf.score_mutations_with_pdb(os.path.join(HERE, "ESM3_structures", pdb), mm, "A", model, model_type="esm3_open",
                                                 use_structure=True, window_size=1024, pdb_range=rng_ or None)
        df["esm3_open_score"] = df["mutant"].map(lambda x: scores.get(x, np.nan))
        df.to_csv(os.path.join(HERE, dms_id + ".csv"), index=False)
        print(dms_id, df["esm3_open_score"].values, flush=True)


if __name__ == "__main__":
    main()
