"""Writes tests/golden/golden_esmc.npz, esmc_state_dict_keys.json and the TOY_ESMC_* CSVs from the UNMODIFIED reference ESM C
(proteingym/baselines/evoscale: compute_fitness.py, esm/models/esmc.py, esm/tokenization) on CPU in fp32 (use_flash_attn=False).

    python tests/golden/make_golden_esmc.py

Weights are proteingym_amd.synthetic.esmc_state_dict(cfg, seed): the tests rebuild them from (cfg, seed), so no checkpoint is
committed.  Modules the image lacks and the ESM C path never calls (zstd, cloudpathlib, Bio, biotite, brotli, msgpack,
msgpack_numpy, tenacity) are stubbed empty.  Needs the reference tree and torch (build container only).
"""
import importlib.machinery
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from proteingym_amd import synthetic as S  # noqa: E402

from oracle.ref_harness import REF_ROOT  # noqa: E402

EVOSCALE = os.path.join(REF_ROOT, "proteingym", "baselines", "evoscale")
STUBBED = ("zstd", "cloudpathlib", "Bio", "biotite", "brotli", "msgpack", "msgpack_numpy", "tenacity")
AA = "ACDEFGHIKLMNPQRSTVWY"

# (name, d_model, layers, seed, sequence length): toy widths, both released widths at reduced depth, and 300M's width at full depth
SHAPES = [("d128", 128, 2, 31, 45), ("d192", 192, 2, 32, 70), ("d960", 960, 2, 33, 100), ("d1152", 1152, 2, 34, 100),
          ("d960_full", 960, 30, 35, 40)]
TOY_MODEL = ("d128", 128, 2, 31)              # the model of the TOY_ESMC_* assays


class _Stub(types.ModuleType):
    __path__ = []

    def __getattr__(self, attr):
        if attr.startswith("__"):
            raise AttributeError(attr)
        v = type(attr, (), {"__init__": lambda self, *a, **k: None})
        setattr(self, attr, v)
        return v


class _StubFinder:
    def find_spec(self, name, path=None, target=None):
        return importlib.machinery.ModuleSpec(name, self) if name.split(".")[0] in STUBBED else None

    def create_module(self, spec):
        return _Stub(spec.name)

    def exec_module(self, module):
        pass


def reference():
    sys.meta_path.insert(0, _StubFinder())
    sys.path.insert(0, EVOSCALE)
    import compute_fitness as cf
    from esm.models.esmc import ESMC
    from esm.tokenization import EsmSequenceTokenizer
    return cf, ESMC, EsmSequenceTokenizer


def build_model(D, layers, seed, ESMC, Tok):
    import torch
    cfg = S.esmc_config(D, layers)
    model = ESMC(D, cfg["heads"], layers, Tok(), use_flash_attn=False).eval()
    sd = S.esmc_state_dict(cfg, seed)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return model


def main():
    import pandas as pd
    import torch
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    cf, ESMC, Tok = reference()
    out = {}

    # the reference's key names and shapes for both released configurations (meta tensors: no weights allocated)
    keys = {}
    for name, (D, H, L) in {"esmc_300M": (960, 15, 30), "esmc_600M": (1152, 18, 36)}.items():
        with torch.device("meta"):
            m = ESMC(D, H, L, Tok(), use_flash_attn=False)
        keys[name] = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    with open(os.path.join(HERE, "esmc_state_dict_keys.json"), "w") as f:
        json.dump(keys, f, indent=0)

    tok = Tok()
    out["tok_chars"] = np.array(list(AA + "XBUZO"))
    out["tok_ids"] = np.array([tok.convert_tokens_to_ids(c) for c in out["tok_chars"]], dtype=np.int32)
    rng = np.random.default_rng(2025)
    for name, D, layers, seed, L in SHAPES:
        model = build_model(D, layers, seed, ESMC, Tok)
        seq = "".join(rng.choice(list(AA), L))
        ids = model._tokenize([seq])[0]
        with torch.no_grad():
            lp = torch.log_softmax(model(sequence_tokens=ids[None]).sequence_logits[0], -1).numpy()
            pos = np.array(sorted(rng.choice(np.arange(1, L + 1), 4, replace=False)), dtype=np.int32)
            mlp = []
            for p in pos:
                t = ids.clone()
                t[p] = 32
                mlp.append(torch.log_softmax(model(sequence_tokens=t[None]).sequence_logits[0, p], -1).numpy())
        out[f"{name}_cfg"] = np.array([D, layers, seed], dtype=np.int64)
        out[f"{name}_ids"] = ids.numpy().astype(np.int32)
        out[f"{name}_lp"] = lp.astype(np.float32)
        out[f"{name}_mask_pos"] = pos
        out[f"{name}_mask_lp"] = np.stack(mlp).astype(np.float32)
        print(name, "done", flush=True)
        del model
    np.savez_compressed(os.path.join(HERE, "golden_esmc.npz"), **out)

    # toy assays: singles + multis + a wild-type mismatch + an out-of-range position + an unparsable part; a 1100-residue target
    # (the window branch); a non-standard mutant letter (KeyError in aa_to_token: no CSV)
    _, D, layers, seed = TOY_MODEL
    model = build_model(D, layers, seed, ESMC, Tok)
    srng = np.random.default_rng(11)
    short = "".join(srng.choice(list(AA), 60))
    long_ = "".join(srng.choice(list(AA), 1100))

    def sub(tgt, p):
        return f"{tgt[p]}{p + 1}{srng.choice([a for a in AA if a != tgt[p]])}"

    muts = [sub(short, int(p)) for p in srng.choice(60, 10, replace=False)]
    muts += [":".join(sub(short, int(p)) for p in sorted(srng.choice(60, k, replace=False))) for k in (2, 2, 3)]
    muts += [muts[0]]                                                          # a duplicate row
    bad_wt = next(a for a in AA if a != short[4])
    muts += [f"{bad_wt}5A", f"{short[0]}61C", f"{short[2]}3D:{short[9]}99E", "A0C", "x3Y", f"{short[7]}8{short[7]}"]
    lpos = [0, 1, 5, 510, 511, 512, 549, 550, 600, 1000, 1098, 1099]
    long_muts = [sub(long_, p) for p in lpos] + [f"{sub(long_, 3)}:{sub(long_, 1097)}"]
    bad = [sub(short, 1), f"{short[3]}4B", sub(short, 5)]
    files = [("TOY_ESMC_SHORT", muts, short), ("TOY_ESMC_LONG", long_muts, long_), ("TOY_ESMC_BADLETTER", bad, short)]
    pd.DataFrame({"DMS_id": [f[0] for f in files], "target_seq": [f[2] for f in files]}).to_csv(
        os.path.join(HERE, "TOY_ESMC_REFERENCE.csv"), index=False)
    for dms_id, mm, tgt in files:
        df = pd.DataFrame({"mutant": mm, "DMS_score": srng.standard_normal(len(mm)).round(4)})
        try:
            scores = cf.score_mutations(tgt, mm, model=model, model_type="esmc_300M", window_size=1024)
        except KeyError as e:                                                  # compute_fitness.py:724: NaN summary row, no CSV
            print(dms_id, "KeyError", e, flush=True)
            df.to_csv(os.path.join(HERE, dms_id + ".csv"), index=False)
            continue
        df["esmc_300M_score"] = df["mutant"].map(lambda x: scores.get(x, np.nan))   # compute_fitness.py:592
        df.to_csv(os.path.join(HERE, dms_id + ".csv"), index=False)
        print(dms_id, df["esmc_300M_score"].values[:4], flush=True)


if __name__ == "__main__":
    main()
