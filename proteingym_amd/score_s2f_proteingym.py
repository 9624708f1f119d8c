"""Drop-in for ``proteingym/baselines/S3F/compute_fitness.py`` on MI355X, for the S2F configuration (config/evaluate/s2f.yaml).

Same flags.  The yaml is read after plain substitution of its ``{{ }}`` placeholders and only for the fields this path needs; what it
does not compute is refused (proteingym_amd.s2f.check_yaml): S3F's surface branch (a ``surface_path``, a ``SurfGVP`` structure model),
other dimensions, other graph construction.  Per assay: the wild-type structure's C-alpha atoms (``pdb_file``, ``|``-separated files
concatenated) over ``pdb_range``, the mutants in the reference's sorted order, one forward per distinct (window, set of sites), and the
reference's CSV in ``<output_scores_folder>/<DMS_filename>``: a leading empty column, then mutant, mutated_sequence (empty), DMS_score,
``<config name>_score`` and, with --MSA_retrieval_location, ``<config name>_MSA_score`` -- the mutants shared with the EVE file, in the
EVE file's order, both scores standardised with the unbiased standard deviation and averaged.  An existing output file is skipped.

Divergences, deliberate: the reference's ``if args.DMS_index:`` treats index 0 as "all assays"; here --DMS_index 0 scores assay 0 and
leaving the flag out scores them all.  results_*.csv aggregate files are not written.  Additive flags: --device, --precision,
--max_rows, --surfdir (refused when set), --esm_dims (a test hook: the ESM2 dimensions of a checkpoint that is not ESM-2-650M).
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import pandas as pd

from . import _lib, s2f, synthetic


def parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="S2F scoring (HIP, MI355X)")
    p.add_argument("-c", "--config", required=True, help="yaml configuration file")
    p.add_argument("-s", "--seed", dest="seed", type=int, default=1024, help="accepted; inference draws nothing")
    p.add_argument("--datadir", required=True, help="folder of the DMS assay CSVs")
    p.add_argument("--ProteinGym_reference_file", required=True, help="the DMS reference file")
    p.add_argument("--structdir", required=True, help="folder of the PDB files")
    p.add_argument("--surfdir", default="", help="surface point clouds (S3F): not computed on this path")
    p.add_argument("--ckpt", required=True, help="the task checkpoint (torch.save({'model': state dict}))")
    p.add_argument("--output_scores_folder", required=True)
    p.add_argument("--DMS_index", type=int, default=None, help="index of the assay in the reference file (default: all)")
    p.add_argument("--MSA_retrieval_location", default=None, help="folder of EVE score files: adds the _MSA column")
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--precision", choices=sorted(_lib.PRECISIONS), default="f16x3", help="ESM2's GEMM operand precision")
    p.add_argument("--max_rows", type=int, default=0)
    p.add_argument("--esm_dims", default=None, help="layers,embed_dim,heads,ffn_dim of the checkpoint's ESM2 (test hook)")
    return p


def msa_average(pred: np.ndarray, mutants, eve: pd.DataFrame):
    """compute_fitness.py:152-199: (rows kept, (standardised pred + standardised EVE) / 2) over the mutants of the EVE file that
    were scored, in the EVE file's order (a repeated mutant keeps its last score); float32 like the reference's tensors."""
    index = {m: i for i, m in enumerate(mutants)}
    eve_dict = {row["mutant"]: row["EVE_ensemble"] for _, row in eve.iterrows()}
    keep = [index[m] for m in eve_dict if m in index]
    e = np.array([s for m, s in eve_dict.items() if m in index], dtype=np.float32)
    if len(keep) < len(mutants):
        print(f"Warning: Only {len(keep)} out of {len(mutants)} mutations were matched with EVE scores", file=sys.stderr)
    p = pred[keep].astype(np.float32)
    z = lambda a: (a - a.mean(dtype=np.float32)) / a.std(ddof=1, dtype=np.float32)
    return keep, ((z(p) + z(e)) / np.float32(2.0)).astype(np.float32)


def write_scores(path: str, model_name: str, rows, pred, pred_msa=None):
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        f.write(f",mutant,mutated_sequence,DMS_score,{model_name}_score" + (f",{model_name}_MSA_score" if pred_msa is not None else "") + "\n")
        for i, (_, muts, target) in enumerate(rows):
            line = f",{':'.join(muts)},,{np.float32(target):.6f},{pred[i]:.6f}"
            if pred_msa is not None:
                line += f",{pred_msa[i]:.6f}"
            f.write(line + "\n")


def main(argv=None):
    args = parser().parse_args(argv)
    cfg = s2f.load_yaml(args.config, dict(datadir=args.datadir, structdir=args.structdir, surfdir=args.surfdir, ckpt=args.ckpt))
    esm_cfg = dict(synthetic.ESM2_650M)
    if args.esm_dims:
        layers, D, H, F = (int(x) for x in args.esm_dims.split(","))
        esm_cfg.update(layers=layers, embed_dim=D, heads=H, ffn_dim=F)
    want = s2f.check_yaml(cfg, esm_cfg["embed_dim"], None if args.esm_dims else "ESM-2-650M")
    model_name = os.path.splitext(os.path.basename(args.config))[0]
    mapping = pd.read_csv(args.ProteinGym_reference_file)
    ids = list(cfg.get("id_list") or mapping["DMS_id"])
    if args.DMS_index is not None:
        ids = [ids[args.DMS_index]]
        print(f"Scoring {ids[0]} with model {model_name}")
    ids = [i for i in ids if i not in set(cfg.get("exclude_id_list") or [])]
    model = s2f.from_state_dict(s2f.load_checkpoint(os.path.expanduser(cfg.get("model_checkpoint") or args.ckpt)), esm_cfg,
                                layers=want["layers"], device=args.device, precision=args.precision, max_rows=args.max_rows,
                                radius=want["radius"], max_neighbors=want["max_neighbors"], plddt_threshold=want["plddt_threshold"])
    try:
        for dms_id in ids:
            row = mapping[mapping["DMS_id"] == dms_id].iloc[0]
            out_path = os.path.join(args.output_scores_folder, row["DMS_filename"])
            if os.path.exists(out_path):
                print(f"Assay {row['DMS_filename']} already computed. Skipping.")
                continue
            assay = pd.read_csv(os.path.join(args.datadir, row["DMS_filename"]), low_memory=False)
            rows = s2f.sort_mutants(assay["mutant"], assay["DMS_score"])
            pos, plddt, s_start, s_end = s2f.load_structure(os.path.expanduser(cfg.get("structure_path") or args.structdir), row["pdb_file"],
                                                            row["pdb_range"], dms_id)
            pred = model.score_assay(dms_id, row["target_seq"], rows, pos, plddt, s_start, s_end)
            pred_msa = None
            if args.MSA_retrieval_location:
                eve = pd.read_csv(os.path.join(args.MSA_retrieval_location, row["DMS_filename"]))
                keep, pred_msa = msa_average(pred, [":".join(r[1]) for r in rows], eve)
                rows, pred = [rows[i] for i in keep], pred[keep]
            write_scores(out_path, model_name, rows, pred, pred_msa)
    finally:
        model.close()
        model.esm.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
