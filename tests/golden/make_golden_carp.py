"""Records tests/golden/CARP_toy/: a seeded toy CARP checkpoint in the released format, a toy substitution assay and a toy indel
assay with their reference CSV, and the float64 tables and scores of tests/carp_ref.py on them.

    python tests/golden/make_golden_carp.py

sequence_models is not installed, so the expected values come from the float64 restatement (tests/carp_ref.py: F.conv1d,
F.layer_norm, F.gelu at batch 1), not from the library; DESIGN.md 4.6o lists what that restatement takes from the library's documented
behaviour.  No test imports this file; only the files it writes are committed."""
import os
import sys

import numpy as np
import pandas as pd
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import carp_ref as R  # noqa: E402

OUT = os.path.join(HERE, "CARP_toy")
TARGET = "MKVLAAGIVRHDESTNQCGPAVIFYWLMKRHDESTNQ"          # 37 residues
D, LAYERS, SLIM = 64, 3, True


def toy_checkpoint(seed):
    g = torch.Generator().manual_seed(seed)
    V, H, k = len(R.ALPHABET), D // 2 if SLIM else D, 5

    def rand(*shape, scale=1.0):
        return torch.randn(*shape, generator=g) * scale

    sd = {"embedder.embedder.weight": rand(V, 8)}
    sd["embedder.embedder.weight"][R.MASK_ID] = 0.0                     # the padding row
    sd["embedder.up_embedder.conv.weight"], sd["embedder.up_embedder.conv.bias"] = rand(D, 8, 1, scale=8 ** -0.5), rand(D, scale=0.1)
    for n in range(LAYERS):
        p = f"embedder.layers.{n}."
        for key, width in (("sequence1.0", D), ("sequence1.3", H), ("sequence2.0", H)):
            sd[p + key + ".weight"], sd[p + key + ".bias"] = 1.0 + rand(width, scale=0.1), rand(width, scale=0.1)
        sd[p + "sequence1.2.conv.weight"], sd[p + "sequence1.2.conv.bias"] = rand(H, D, 1, scale=D ** -0.5), rand(H, scale=0.1)
        sd[p + "conv.weight"], sd[p + "conv.bias"] = rand(H, H, k, scale=(H * k) ** -0.5), rand(H, scale=0.1)
        sd[p + "sequence2.2.conv.weight"], sd[p + "sequence2.2.conv.bias"] = rand(D, H, 1, scale=H ** -0.5), rand(D, scale=0.1)
    sd["last_norm.weight"], sd["last_norm.bias"] = 1.0 + rand(D, scale=0.1), rand(D, scale=0.1)
    sd["decoder.conv.weight"], sd["decoder.conv.bias"] = rand(V, D, 1, scale=D ** -0.5), rand(V, scale=0.1)
    return {"model": "carp_toy", "d_embed": 8, "d_model": D, "n_layers": LAYERS, "kernel_size": k, "r": 128, "activation": "gelu",
            "slim": SLIM, "model_state_dict": sd}


def main():
    os.makedirs(OUT, exist_ok=True)
    ck = toy_checkpoint(2024)
    torch.save(ck, os.path.join(OUT, "carp_toy.pt"))
    rng = np.random.default_rng(7)
    aas = R.ALPHABET[:20]
    singles = []
    for pos in (1, 2, 5, 17, 18, 30, 37):                               # both ends, neighbours, the middle
        for mt in rng.choice([a for a in aas if a != TARGET[pos - 1]], 2, replace=False):
            singles.append(f"{TARGET[pos - 1]}{pos}{mt}")
    multis = [f"{singles[0]}:{singles[5]}", f"{singles[2]}:{singles[7]}:{singles[12]}", f"{singles[13]}:{singles[3]}"]
    mutants = singles + multis
    score = rng.normal(0, 1, len(mutants)).round(4)
    pd.DataFrame({"mutant": mutants, "DMS_score": score}).to_csv(os.path.join(OUT, "TOY_CARP.csv"), index=False)
    indels = [TARGET[:10] + TARGET[11:], TARGET[:20] + "W" + TARGET[20:], TARGET[:5], TARGET + "AC", "M"]
    pd.DataFrame({"mutant": indels, "DMS_score": rng.normal(0, 1, len(indels)).round(4)}).to_csv(os.path.join(OUT, "TOY_CARP_INDELS.csv"),
                                                                                             index=False)
    pd.DataFrame({"DMS_id": ["TOY_CARP", "TOY_CARP_INDELS"], "DMS_filename": ["TOY_CARP.csv", "TOY_CARP_INDELS.csv"],
                  "target_seq": [TARGET, TARGET]}).to_csv(os.path.join(OUT, "reference.csv"), index=False)
    tok = R.tokenize(TARGET)
    np.savez(os.path.join(OUT, "expected.npz"),
             masked_lp=R.masked_logprobs(ck, tok, range(len(tok))), token_lp=R.logprobs(ck, tok),
             mm_scores=R.masked_marginal_scores(ck, TARGET, mutants),
             pl_scores=R.pseudo_likelihood_scores(ck, [_mutate(m) for m in mutants]),
             indel_scores=R.pseudo_likelihood_scores(ck, indels))
    print(f"wrote {OUT}")


def _mutate(mutant):
    s = list(TARGET)
    for row in mutant.split(":"):
        assert s[int(row[1:-1]) - 1] == row[0]
        s[int(row[1:-1]) - 1] = row[-1]
    return "".join(s)


if __name__ == "__main__":
    main()
