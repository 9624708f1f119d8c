"""Drop-in for ``proteingym/baselines/protssn/compute_fitness.py`` on MI355X.

Same flags.  ``--mutant_dataset_dir`` holds ``DATASET/<name>/<name>.pdb`` and ``<name>.tsv`` (or ``.csv``); the assays are the sorted
folder names.  Per assay: the structure's N, CA and C atoms and its own sequence, one unmasked ESM2 forward, then every checkpoint of
``--gnn_model_name`` (``k{10,20,30}_h{512,768,1280}``, read from ``<gnn_model_dir>/protssn_k{k}_h{h}.pt``) on that structure's k-nearest
graph; ``<output_scores_folder>/<name>.csv`` is written, or extended, with one ``ProtSSN_k{k}_h{h}`` column per checkpoint and, with
``--use_ensemble``, ``ProtSSN_ensemble``.  The normalisation files come from ``<repo_path>/proteingym/baselines/protssn/norm`` or
``--norm_dir``.  ``--plm`` is a local fair-esm ESM2 ``.pt`` or a local HF ``EsmModel`` directory; nothing is downloaded.

Refused: ``--gnn`` other than egnn, k or h outside the released sets, a yaml whose embedding / residual / mlp_num / dropout /
edge_attr_dim / output_dim differ from the released checkpoints'.  A failing assay (a non-standard residue, a wild-type mismatch, a
missing file) is reported on stderr and skipped; the exit status is then 1.

Divergences, deliberate: ``ProtSSN_ensemble`` is the mean of the single-model columns only (the reference averages every column that
starts with ``ProtSSN``, so its second run averages the old ensemble into the new one), and it is written for the assays of this call,
not for every file of the output folder.  Additive flags: --DMS_index, --precision, --device, --norm_dir, --edge_chunk, --test_widths (a
test hook: accepts any h, for the checkpoints of a smaller seeded model).
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import pandas as pd

from . import protssn


def parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="ProtSSN scoring (HIP, MI355X)")
    p.add_argument("--gnn", type=str, default="egnn", help="egnn (gat and gcn are not computed on this path)")
    p.add_argument("--gnn_config", type=str, default="src/config/egnn.yaml", help="gnn config")
    p.add_argument("--gnn_model_dir", type=str, default="model/", help="folder of protssn_k{k}_h{h}.pt")
    p.add_argument("--gnn_model_name", type=str, default=None, nargs="+", help="k{k}_h{h}, several allowed")
    p.add_argument("--plm", type=str, default="facebook/esm2_t33_650M_UR50D", help="local ESM2 .pt or HF EsmModel directory")
    p.add_argument("--use_ensemble", action="store_true", help="write ProtSSN_ensemble")
    p.add_argument("--mutant_dataset_dir", type=str, default="data/evaluation", help="folder that holds DATASET/")
    p.add_argument("--mutant_name", type=str, default=None, help="accepted; the graphs are not cached on disk")
    p.add_argument("--mutant_pos_col", type=str, default="mutant", help="mutation column name")
    p.add_argument("--mutant_score_col", type=str, default="DMS_score", help="the assay's score column name")
    p.add_argument("--score_info", type=str, default=None, help="per-assay spearman file")
    p.add_argument("--output_scores_folder", type=str, default="result/", help="the result output path")
    p.add_argument("--repo_path", type=str, default=None, help="Path to ProteinGym repo")
    p.add_argument("--norm_dir", type=str, default=None, help="folder of cath_k{k}_mean_attr.pt (default: under --repo_path)")
    p.add_argument("--DMS_index", type=int, default=None, help="index of the assay among the sorted folder names (default: all)")
    p.add_argument("--precision", choices=("f16x3", "fp32"), default="f16x3")
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--edge_chunk", type=int, default=0, help="edges per chunk of the per-edge stages (0: the library's default)")
    p.add_argument("--test_widths", action="store_true", help="test hook: accept any h")
    return p


def read_mutants(folder: str, name: str) -> pd.DataFrame:
    tsv, csv = os.path.join(folder, f"{name}.tsv"), os.path.join(folder, f"{name}.csv")
    if os.path.exists(tsv):
        return pd.read_table(tsv)
    if os.path.exists(csv):
        return pd.read_csv(csv)
    raise ValueError(f"Invalid file: {tsv} or {csv}")


def check_args(args) -> list:
    """The refusals that need no file but the yaml: [(column name, k, h)] of the requested checkpoints."""
    import yaml
    if args.gnn != "egnn":
        raise ValueError(f"--gnn {args.gnn}: this path runs the released egnn checkpoints only")
    if not args.gnn_model_name:
        raise ValueError("--gnn_model_name is required (k{k}_h{h}, several allowed)")
    with open(args.gnn_config) as f:
        cfg = yaml.safe_load(f)[args.gnn]
    args.layers = protssn.check_yaml(cfg)
    out = []
    for name in args.gnn_model_name:
        if args.test_widths:
            k, h = (int(x[1:]) for x in name.split("_"))
            if k not in protssn.KS:
                raise ValueError(f"Invalid k: {k}")
        else:
            k, h = protssn.parse_model_name(name)
        out.append((f"ProtSSN_k{k}_h{h}", k, h))
    return out


def write_columns(path: str, mutant_df: pd.DataFrame, columns: dict, use_ensemble: bool) -> pd.DataFrame:
    """compute_fitness.py predict / ensemble on one result file: created from the assay's table when missing, else extended."""
    if not os.path.exists(path):
        mutant_df.to_csv(path, index=False)
    result = pd.read_csv(path)
    for col, values in columns.items():
        result[col] = values
    if use_ensemble:
        result["ProtSSN_ensemble"] = protssn.ensemble_mean({c: result[c] for c in result.columns})
    result.to_csv(path, index=False)
    return result


def main(argv=None):
    args = parser().parse_args(argv)
    wanted = check_args(args)
    if args.repo_path is None:
        args.repo_path = os.path.dirname(os.path.dirname(os.getcwd()))
    norms = {k: protssn.load_norm(k, args.repo_path, args.norm_dir) for k in sorted({k for _, k, _ in wanted})}
    dataset = os.path.join(args.mutant_dataset_dir, "DATASET")
    names = sorted(os.listdir(dataset))
    if args.DMS_index is not None:
        names = [names[args.DMS_index]]
    os.makedirs(args.output_scores_folder, exist_ok=True)
    esm = protssn.load_plm(args.plm, device=args.device, precision=args.precision)
    node_in = esm.cfg["embed_dim"]
    models, failed, info = {}, [], {"name": [], "count": []}
    try:
        for col, k, h in wanted:
            print(f"--------------- ProtSSN k{k}_h{h} ---------------")
            sd = protssn.load_checkpoint(args.gnn_model_dir, k, h)
            models[col] = (k, protssn.from_state_dict(sd, node_in, h, args.layers, device=args.device, precision=args.precision,
                                                      edge_chunk=args.edge_chunk))
        for name in names:
            try:
                n, ca, c, seq = protssn.read_pdb(os.path.join(dataset, name, f"{name}.pdb"))
                mutant_df = read_mutants(os.path.join(dataset, name), name)
                lps = protssn.score_structure(models, protssn.residue_rows(esm, seq), n, ca, c, norms)
                offset = protssn.OFFSETS.get(name, 1)
                columns = {col: mutant_df[args.mutant_pos_col].apply(lambda x: protssn.label_row(x, seq, lps[col], offset)) for col in lps}
                result = write_columns(os.path.join(args.output_scores_folder, name + ".csv"), mutant_df, columns, args.use_ensemble)
            except Exception as e:                                  # the reference's wrong_proteins list: report, go on
                print(f">>> {name}: skipped: {type(e).__name__}: {e}", file=sys.stderr)
                failed.append(name)
                continue
            info["name"].append(name)
            info["count"].append(len(result))
            if args.mutant_score_col in result.columns:
                from scipy.stats import spearmanr
                for col in columns:
                    rho = spearmanr(result[args.mutant_score_col], result[col]).correlation
                    info.setdefault(col, []).append(0 if np.isnan(rho) else rho)
                    print(f">>> {name} {col}: {info[col][-1]}; mutant_num: {len(result)}")
    finally:
        for _, m in models.values():
            m.close()
        esm.close()
    if args.score_info is not None and info["name"]:
        new = pd.DataFrame({k: v for k, v in info.items() if len(v) == len(info["name"])})
        if os.path.exists(args.score_info):
            old = pd.read_csv(args.score_info)
            if list(old.get("name", [])) == info["name"]:
                for col in new.columns:
                    old[col] = new[col]
                new = old
        new.to_csv(args.score_info, index=False)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
