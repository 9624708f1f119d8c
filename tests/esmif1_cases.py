"""Shared by make_golden_esmif1.py and the ESM-IF1 tests: the toy model (seeded, so that no checkpoint is committed), the seeded
backbones and sequences of the golden cases, and the toy assay's PDB text."""
import argparse

import numpy as np

from esm3_cases import THREE, random_walk

AA = "ACDEFGHIKLMNPQRSTVWY"

# D 128, 2 heads of 64, 2 + 2 layers, small GVP widths, 5 neighbours
TOY_ARGS = dict(arch="gvp_transformer_invariant_gvp", encoder_embed_dim=128, encoder_layers=2, encoder_attention_heads=2, encoder_ffn_embed_dim=256,
                decoder_embed_dim=128, decoder_layers=2, decoder_attention_heads=2, decoder_ffn_embed_dim=256,
                gvp_node_hidden_dim_scalar=32, gvp_node_hidden_dim_vector=8, gvp_edge_hidden_dim_scalar=16, gvp_edge_hidden_dim_vector=1,
                gvp_num_encoder_layers=2, gvp_top_k_neighbors=5, gvp_dropout=0.1, dropout=0.1, attention_dropout=0.1)
# the released esm_if1_gvp4_t16_142M_UR50 widths (esm/inverse_folding and the checkpoint's args)
RELEASED_ARGS = dict(TOY_ARGS, encoder_embed_dim=512, encoder_layers=8, encoder_attention_heads=8, encoder_ffn_embed_dim=2048,
                     decoder_embed_dim=512, decoder_layers=8, decoder_attention_heads=8, decoder_ffn_embed_dim=2048,
                     gvp_node_hidden_dim_scalar=1024, gvp_node_hidden_dim_vector=256, gvp_edge_hidden_dim_scalar=32,
                     gvp_edge_hidden_dim_vector=1, gvp_num_encoder_layers=4, gvp_top_k_neighbors=30)
MODEL_SEED = 41

# case -> (residues in the backbone, backbone seed, residues whose CA is NaN, lengths of the scored sequences)
CASES = {
    "L30": (30, 301, (), (30, 30)),
    "L31": (31, 302, (), (31, 17)),          # the second sequence: T != S - 2
    "L70": (70, 303, (), (70, 70)),
    "nanca": (33, 304, (11,), (33, 33)),
}
TOY_PDB = ("toy_esmif1.pdb", 36, 305, (7,), 3)          # file, residues, seed, residues without CA, first residue number


def toy_args():
    return argparse.Namespace(**TOY_ARGS)


def state_dict(cfg, seed=MODEL_SEED):
    """float32 numpy weights for every key of esmif1.expected_shapes(cfg), seeded per key order."""
    from proteingym_amd import esmif1
    rng = np.random.default_rng(seed)
    sd = {}
    for k, shp in sorted(esmif1.expected_shapes(cfg).items()):
        if len(shp) == 2:
            w = rng.standard_normal(shp) / np.sqrt(shp[1])
        elif k.endswith(("norm.weight", "norm_nodes.gain")):
            w = 1.0 + 0.1 * rng.standard_normal(shp)
        else:
            w = 0.1 * rng.standard_normal(shp)
        sd[k] = w.astype(np.float32)
    return sd


def backbone(seed, L, nan_ca=()):
    """N, CA, C of a seeded random walk, float32 [L, 3, 3], rounded to a PDB file's three decimals; CA of the residues in nan_ca is NaN."""
    x = np.round(random_walk(np.random.default_rng(seed), L), 3).astype(np.float32)
    for i in nan_ca:
        x[i, 1] = np.nan
    return x


def sequence_of(seed, L):
    return "".join(np.random.default_rng(seed).choice(list(AA), L))


def case(name):
    L, seed, nan_ca, lens = CASES[name]
    return backbone(seed, L, nan_ca), [sequence_of(seed * 10 + i, n) for i, n in enumerate(lens)]


def pdb_text(sequence, coords, first=1, chain="A"):
    """ATOM records for the finite N / CA / C atoms."""
    lines, serial = [], 1
    for i, aa in enumerate(sequence):
        for j, name in enumerate(("N", "CA", "C")):
            if not np.isfinite(coords[i, j]).all():
                continue
            x = coords[i, j]
            lines.append("ATOM  %5d  %-3s %3s %1s%4d    %8.3f%8.3f%8.3f  1.00  0.00           %1s" %
                         (serial, name, THREE[aa], chain, first + i, x[0], x[1], x[2], name[0]))
            serial += 1
    return "\n".join(lines + ["END"]) + "\n"
