"""float64 restatement of VespaG (proteingym/baselines/vespag/vespag) on plain torch ops, for the tests.  Shares no code with
proteingym_amd/vespag.py.  Every rule cites the reference's file and line.

One stated deviation from the reference: mask_non_mutations raises on a wild-type letter outside the 20; here, as on
the device path, that row stays unmasked.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

import protssn_ref

AMINO_ACIDS = "ACDEFGHIKLMNPQRSTVWY"          # utils/utils.py:15
# the small seeded ESM2 of tests/test_gpu_vespag.py: 2 layers, D = 128, 4 heads (head_dim 32)
TOY_ESM = dict(layers=2, embed_dim=128, heads=4, ffn_dim=512, max_positions=0, token_dropout=1, emb_layer_norm_before=0)
TOY_HEAD = dict(seed=21, input_dim=128, hidden=256, gain=1.0, bias_std=0.05)


def fnn(sd, x, slope=0.01, dtype=torch.float64):
    """FNN([hidden], input_dim, 20, dropout_rate=0.2).eval(): models/utils.py:19-30 builds Linear, Dropout, LeakyReLU, Linear (the last
    activation and dropout removed); nn.LeakyReLU() has slope 0.01; Dropout is the identity in eval; models/fnn.py:51 squeezes nothing
    at 20 columns."""
    w = {k: torch.as_tensor(np.array(v)).to(dtype) for k, v in sd.items()}
    h = F.linear(torch.as_tensor(np.array(x)).to(dtype), w["net.0.weight"], w["net.0.bias"])
    h = F.leaky_relu(h, slope)
    return F.linear(h, w["net.3.weight"], w["net.3.bias"])


def mask_non_mutations(y, sequence):
    """utils/mutations.py:69-80, in place: y[i, AMINO_ACIDS.index(wt_i)] = 0.0 (a letter outside the 20: the row is left alone)."""
    for i, aa in enumerate(sequence):
        if aa in AMINO_ACIDS:
            y[i, AMINO_ACIDS.index(aa)] = 0.0
    return y


def landscape_y(sd, rows, sequence, dtype=torch.float64):
    """runner/predict.py:182-183: y = model(embedding); y = mask_non_mutations(y, sequence).  A numpy array of `dtype`."""
    return mask_non_mutations(fnn(sd, rows, dtype=dtype), sequence).numpy()


def parse(mutant, one_indexed=True):
    """utils/mutations.py:24-32 and :49-57: ':'-joined <from><position><to>; [(zero-indexed position, to_aa)]; from_aa is never read."""
    out = []
    for s in mutant.split(":"):
        position = int(s[1:-1])
        if one_indexed:
            position -= 1
        out.append((position, s[-1]))
    return out


def full_landscape(sequence, one_indexed=True):
    """runner/predict.py:155-163 with SAV.__str__ (utils/mutations.py:34-38): the mutant strings, position-major, AMINO_ACIDS order, the
    wild type skipped."""
    return [f"{wt}{i + 1 if one_indexed else i}{aa}" for i, wt in enumerate(sequence) for aa in AMINO_ACIDS if aa != wt]


def score(y, mutant, one_indexed=True, normalize=True):
    """utils/mutations.py:95-115: sum of y[position][alphabet.index(to_aa)].item() over the SAVs, then 1 / (1 + exp(-score))."""
    s = sum([y[p][AMINO_ACIDS.index(a)].item() for p, a in parse(mutant, one_indexed)])
    return 1 / (1 + math.exp(-s)) if normalize else s


def scores(y, mutants, one_indexed=True, normalize=True):
    return np.array([score(y, m, one_indexed, normalize) for m in mutants], dtype=np.float64)


# -- ESM2 rows: data/embeddings.py:83-104, one sequence at a time at batch 1, unpadded, float64, on the CPU --------------------------
def toy_esm(seed=3):
    """(cfg, blob) of the seeded small ESM2."""
    from proteingym_amd import _lib, synthetic
    cfg = dict(TOY_ESM, arch=_lib.ARCH_ESM2)
    return cfg, synthetic.random_weights(cfg, seed=seed)


def hf_model(cfg, blob):
    """The same weights as a float64 Hugging Face EsmModel."""
    from proteingym_amd import synthetic
    return protssn_ref.fair_to_hf(synthetic.blob_to_arrays(cfg, blob), cfg)


ESM_IDS = {a: i for i, a in enumerate(("<cls>", "<pad>", "<eos>", "<unk>", "L", "A", "G", "V", "S", "E", "R", "T", "I", "D", "P", "K", "Q", "N",
                                       "F", "Y", "M", "H", "W", "C", "X", "B", "U", "Z", "O", ".", "-", "<null_1>", "<mask>"))}


def hf_rows(model, sequence):
    """data/embeddings.py:84 (U Z O B -> X), the ESM tokenizer's <cls> ... <eos>, :97 last_hidden_state[0, 1 : L + 1]."""
    s = "".join("X" if a in "UZOB" else a for a in sequence)
    tokens = [ESM_IDS["<cls>"]] + [ESM_IDS[a] for a in s] + [ESM_IDS["<eos>"]]
    return protssn_ref.hf_residue_rows(model, tokens)

