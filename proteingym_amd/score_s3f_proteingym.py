"""Drop-in for ``proteingym/baselines/S3F/compute_fitness.py`` on MI355X, for the S3F configuration (config/evaluate/s3f.yaml).

Same flags.  The yaml is read as score_s2f_proteingym reads it and checked by proteingym_amd.s3f.check_yaml: a ``SurfGVP`` structure
model with the released surface dimensions and a ``surface_path``; its ``batch_size`` decides which masked sequences share a pooled
surface row.  Per assay: the C-alpha atoms of ``pdb_file`` over ``pdb_range``, the surface pickles ``<pdb stem>.pkl``
under --surfdir (made beforehand with the reference's script/process_surface.py; reading one unpickles it), the mutants in the
reference's sorted order, one forward per masked sequence of the reference's list, and the reference's CSV with ``<config name>_score``
and, with --MSA_retrieval_location, ``<config name>_MSA_score``.  An existing output file is skipped.

Divergences, deliberate: score_s2f_proteingym's (--DMS_index 0 scores assay 0; no results_*.csv), and an assay whose loader batch
would hold masked sequences of two sequence windows is refused unless batch_size is 1.  Additive flags: --device, --precision,
--max_rows, --esm_dims (a test hook: the ESM2 dimensions of a checkpoint that is not ESM-2-650M).
"""
from __future__ import annotations

import argparse
import os
import sys

import pandas as pd

from . import _lib, s2f, s3f, synthetic
from .score_s2f_proteingym import msa_average, write_scores


def parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="S3F scoring (HIP, MI355X)")
    p.add_argument("-c", "--config", required=True, help="yaml configuration file")
    p.add_argument("-s", "--seed", dest="seed", type=int, default=1024, help="accepted; inference draws nothing")
    p.add_argument("--datadir", required=True, help="folder of the DMS assay CSVs")
    p.add_argument("--ProteinGym_reference_file", required=True, help="the DMS reference file")
    p.add_argument("--structdir", required=True, help="folder of the PDB files")
    p.add_argument("--surfdir", required=True, help="folder of the surface files, <pdb stem>.pkl")
    p.add_argument("--ckpt", required=True, help="the task checkpoint (torch.save({'model': state dict}))")
    p.add_argument("--output_scores_folder", required=True)
    p.add_argument("--DMS_index", type=int, default=None, help="index of the assay in the reference file (default: all)")
    p.add_argument("--MSA_retrieval_location", default=None, help="folder of EVE score files: adds the _MSA column")
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--precision", choices=sorted(_lib.PRECISIONS), default="f16x3", help="ESM2's GEMM operand precision")
    p.add_argument("--max_rows", type=int, default=0)
    p.add_argument("--esm_dims", default=None, help="layers,embed_dim,heads,ffn_dim of the checkpoint's ESM2 (test hook)")
    return p


def main(argv=None):
    args = parser().parse_args(argv)
    cfg = s2f.load_yaml(args.config, dict(datadir=args.datadir, structdir=args.structdir, surfdir=args.surfdir, ckpt=args.ckpt))
    esm_cfg = dict(synthetic.ESM2_650M)
    if args.esm_dims:
        layers, D, H, F = (int(x) for x in args.esm_dims.split(","))
        esm_cfg.update(layers=layers, embed_dim=D, heads=H, ffn_dim=F)
    want = s3f.check_yaml(cfg, esm_cfg["embed_dim"], None if args.esm_dims else "ESM-2-650M")
    model_name = os.path.splitext(os.path.basename(args.config))[0]
    mapping = pd.read_csv(args.ProteinGym_reference_file)
    ids = list(cfg.get("id_list") or mapping["DMS_id"])
    if args.DMS_index is not None:
        ids = [ids[args.DMS_index]]
        print(f"Scoring {ids[0]} with model {model_name}")
    ids = [i for i in ids if i not in set(cfg.get("exclude_id_list") or [])]
    model = s3f.from_state_dict(s3f.load_checkpoint(os.path.expanduser(cfg.get("model_checkpoint") or args.ckpt)), esm_cfg,
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
            surface = s3f.load_surface(os.path.expanduser(cfg.get("surface_path") or args.surfdir), row["pdb_file"])
            pred = model.score_assay(dms_id, row["target_seq"], rows, pos, plddt, s_start, s_end, surface, want["batch_size"])
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
