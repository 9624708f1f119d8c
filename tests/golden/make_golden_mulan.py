"""Writes the MULAN fixtures: two seeded toy checkpoints (MULAN_toy/plain: 2 layers, D = 64, 4 heads of 16, F = 256, ESM2's 33
tokens; MULAN_toy/foldseek: 2 layers, D = 96, 4 heads of 24, F = 192, SaProt's 446 tokens, stored in fp16 to stay under the SaProt
toy's size), three constructed structure files (17, 68 and 68 residues: T = 19 and T = 70; residues with pLDDT <= 70, one of them
exactly 70; a 2.5 A chain break; one MSE), the dataset folder the reference would cache for them, and the assays with the scores the
float64 restatement (tests/mulan_ref.py) gives: TOY_MULAN_TWO (two chunks, rows interleaved between them; plain model) and
TOY_MULAN_FS (one chunk; Foldseek model).  Run from the repository root: python tests/golden/make_golden_mulan.py"""
import json
import os
import sys

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import mulan_ref                                            # noqa: E402
from proteingym_amd import esm as pesm, mulan, saprot, synthetic as S       # noqa: E402

ONE_TO_THREE = {v: k for k, v in mulan.THREE_TO_ONE.items()}
SEED_PLAIN, SEED_FS = 20261, 20262


def write_checkpoint(path, cfg, sd, half):
    from safetensors.numpy import save_file
    os.makedirs(path, exist_ok=True)
    hf = dict(architectures=["StructEsmForMaskedLM"], model_type="esm", hidden_size=cfg["embed_dim"], num_hidden_layers=cfg["layers"],
              num_attention_heads=cfg["heads"], intermediate_size=cfg["ffn_dim"], vocab_size=cfg["vocab"], pad_token_id=1,
              mask_token_id=cfg["mask_token_id"], position_embedding_type="rotary", layer_norm_eps=1e-5, hidden_act="gelu",
              token_dropout=True, emb_layer_norm_before=False, max_position_embeddings=1026)
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(hf, f, indent=1)
    save_file({k: np.ascontiguousarray(v.astype(np.float16) if half else v) for k, v in sd.items()}, os.path.join(path, "model.safetensors"))


def checkpoints():
    out = {}
    for name, cfg, seed, half in (("plain", S.mulan_config(64, 4, 2, 256), SEED_PLAIN, False),
                                  ("foldseek", S.mulan_config(96, 4, 2, 192, use_foldseek=True), SEED_FS, True)):
        sd = S.mulan_state_dict(cfg, seed)
        if half:                                            # what the file holds is what every reader sees
            sd = {k: v.astype(np.float16).astype(np.float32) for k, v in sd.items()}
        write_checkpoint(os.path.join(HERE, "MULAN_toy", name), cfg, sd, half)
        out[name] = (cfg, mulan.pack(cfg, sd))
    return out


def write_structure(path, seq, seed, low, brk, mse=None):
    """A chain of random geometry: backbone atoms 1.4 A apart along a random walk (every peptide bond inside 1.8 A, except a 2.5 A
    one after residue `brk`), side chains as random 1.5 A steps from CA.  B-factors 70 + (0.5 .. 25), `low`: residue -> its B-factor."""
    rng = np.random.default_rng(seed)

    def step(length):
        v = rng.standard_normal(3)
        return v / np.linalg.norm(v) * length
    lines, serial, pos = ["HEADER    TOY STRUCTURE FOR THE MULAN TESTS"], 1, np.zeros(3)
    for i, a in enumerate(seq):
        name = "MSE" if mse == i else ONE_TO_THREE[a]
        b = low.get(i, 70.0 + float(rng.uniform(0.5, 25.0)))
        atoms = {}
        for k in ("N", "CA", "C"):
            pos = pos + step(2.5 if (k == "N" and brk is not None and i == brk + 1) else 1.4)
            atoms[k] = pos
        side = atoms["CA"]
        for k in mulan.CHI_ATOMS.get(name, ())[2:]:
            side = side + step(1.5)
            atoms[k] = side
        for k, xyz in atoms.items():
            rec = "HETATM" if name == "MSE" else "ATOM  "
            lines.append(f"{rec}{serial:5d} {k:<4s} {name} A{i + 1:4d}    {xyz[0]:8.3f}{xyz[1]:8.3f}{xyz[2]:8.3f}  1.00{b:6.2f}          {k[0]:>2s}")
            serial += 1
    lines.append("END")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def random_mutants(rng, seq, lo, n_single, multi):
    """Mutants in the assay's numbering on a chunk that starts at `lo`; `multi`: tuples of 0-based residue indices."""
    aas = "ACDEFGHIKLMNPQRSTVWY"

    def sub(i):
        return f"{seq[i]}{lo + i}{rng.choice([c for c in aas if c != seq[i]])}"
    singles = [sub(int(i)) for i in rng.choice(len(seq), size=n_single, replace=False)]
    return singles + [":".join(sub(i) for i in m) for m in multi]


def main():
    rng = np.random.default_rng(7)
    ck = checkpoints()
    sdir = os.path.join(HERE, "MULAN_structures")
    os.makedirs(sdir, exist_ok=True)
    aas = np.array(list("ACDEFGHIKLMNPQRSTVWY"))
    seq_a = "R" + "".join(rng.choice(aas, 16))                # starts with the five-chi residue
    seq_b = "".join(rng.choice(aas, 30)) + "M" + "".join(rng.choice(aas, 37))
    seq_c = "".join(rng.choice(aas, 68))
    write_structure(os.path.join(sdir, "toy_mulan_a.pdb"), seq_a, 11, {3: 70.0, 4: 55.25, 9: 12.5}, brk=7)
    write_structure(os.path.join(sdir, "toy_mulan_b.pdb"), seq_b, 12, {0: 40.0, 20: 70.0, 21: 69.99, 50: 33.0, 67: 60.0}, brk=40, mse=30)
    write_structure(os.path.join(sdir, "toy_mulan_c.pdb"), seq_c, 13, {5: 70.0, 6: 10.0, 44: 65.5}, brk=None)
    entries = []
    for n in "abc":
        seq, rows = mulan.structure_rows(os.path.join(sdir, f"toy_mulan_{n}.pdb"))
        entries.append((f"toy_mulan_{n}", seq, rows))
    assert entries[0][1] == seq_a and entries[1][1] == seq_b[:30] + "X" + seq_b[31:] and entries[2][1] == seq_c
    struc = []
    for _, seq, rows in entries:                            # 3Di letters, '#' where pLDDT < 70 (get_struc_seq's plddt_mask)
        s = rng.choice(list(saprot.STRUC_LETTERS[:20]), len(seq))
        s[rows[:, 0] < 70.0] = "#"
        struc.append("".join(a + b for a, b in zip(seq, s)))
    mulan.save_dataset_folder(os.path.join(HERE, "MULAN_dataset"), entries, struc)

    # TOY_MULAN_TWO: chunk a = 1-17, chunk b = 18-85; singles, doubles and triples that share positions, low-pLDDT residues among them
    target = seq_a + seq_b
    muts_a = random_mutants(rng, seq_a, 1, 8, [(3, 9), (3, 4, 9), (0, 16), (4,), (3,)])
    muts_b = random_mutants(rng, seq_b, 18, 14, [(20, 21), (20, 21, 50), (0, 67), (5, 20), (21,), (29, 31, 64), (50,)])
    order = rng.permutation(len(muts_a) + len(muts_b))
    mutants = [(muts_a + muts_b)[i] for i in order]
    cfg, blob = ck["plain"]
    vocab = list(pesm.VOCABULARY)
    per_chunk = []
    for (name, seq, rows), lo, hi in ((entries[0], 1, 17), (entries[1], 18, 85)):
        angles, plddt = mulan.chunk_features(rows)
        mine = [m for m in mutants if lo <= int(m.split(":")[0][1:-1]) <= hi]
        per_chunk.append(mulan_ref.scores(cfg, blob, mulan.tokenize(seq, False), angles, plddt, mine, lo, vocab))
    two = pd.DataFrame({"mutant": mutants, "MULAN_score": np.concatenate(per_chunk), "DMS_score": np.round(rng.standard_normal(len(mutants)), 3)})
    two.to_csv(os.path.join(HERE, "TOY_MULAN_TWO.csv"), index=False)

    # TOY_MULAN_FS: chunk c = 1-68 on the Foldseek model
    muts_c = random_mutants(rng, seq_c, 1, 12, [(5, 6), (5, 6, 44), (1, 66), (6,)])
    cfg, blob = ck["foldseek"]
    angles, plddt = mulan.chunk_features(entries[2][2])
    sc = mulan_ref.scores(cfg, blob, mulan.tokenize(struc[2], True), angles, plddt, muts_c, 1, saprot.vocabulary())
    pd.DataFrame({"mutant": muts_c, "MULAN_score": sc, "DMS_score": np.round(rng.standard_normal(len(muts_c)), 3)}).to_csv(
        os.path.join(HERE, "TOY_MULAN_FS.csv"), index=False)
    pd.DataFrame({"DMS_id": ["TOY_MULAN_TWO", "TOY_MULAN_FS"], "DMS_filename": ["TOY_MULAN_TWO.csv", "TOY_MULAN_FS.csv"],
                  "target_seq": [target, seq_c], "pdb_file": ["toy_mulan_a.pdb|toy_mulan_b.pdb", "toy_mulan_c.pdb"],
                  "pdb_range": ["1-17|18-85", "1-68"]}).to_csv(os.path.join(HERE, "TOY_MULAN_REFERENCE.csv"), index=False)


if __name__ == "__main__":
    main()
