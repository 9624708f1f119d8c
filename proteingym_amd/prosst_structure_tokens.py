"""Drop-in for ``venusrem/data/get_struc_seq.py`` (proteingym/baselines/venusrem; ProSST's tokens are the same) on MI355X.

    python -m proteingym_amd.prosst_structure_tokens --pdb_dir structures/ --vocab_size 2048 20 --out_dir structure_sequence \
        --model_path AE.pt --cluster_dir static/

The reference's flags (--pdb_dir, --pdb_file, --vocab_size, --overwrite, --out_dir) plus --model_path (AE.pt) and --cluster_dir (the folder
of ``<K>.joblib`` or ``<K>.npy``), which the reference takes from its package folder, and --device.  Writes
``<out_dir>/<K>/<name>.fasta`` = ``>{name}`` and the comma-joined tokens on one line, byte for byte what the reference writes and what
``compute_fitness.py`` reads as ``<base_dir>/structure_sequence/<K>/`` (ProSST) or ``<struc_seq_dir>/<K>/`` (VenusREM: ``--struc_seq_dir`` is
``<out_dir>`` itself, the K folder is appended there).  Every requested K comes from one
encoder pass per structure (the reference re-creates and re-runs the model per K).  A structure that fails is reported and skipped.
With --pdb_file the output takes the file's base name without its extension (the reference splits the whole path at the first dot).
"""
from __future__ import annotations

import argparse
import os
import sys
from typing import List, Optional

from . import prosst


def parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="ProSST / VenusREM structure tokens (HIP, MI355X)")
    p.add_argument("--pdb_dir", type=str, default=None, help="Directory containing PDB files")
    p.add_argument("--pdb_file", type=str, default=None, help="PDB file")
    p.add_argument("--vocab_size", type=int, default=[2048], nargs="+", help="Vocabulary size")
    p.add_argument("--overwrite", action="store_true", help="Overwrite existing files")
    p.add_argument("--out_dir", type=str, default=None, help="Output directory")
    p.add_argument("--model_path", type=str, default=None, help="AE.pt (the structure encoder's checkpoint)")
    p.add_argument("--cluster_dir", type=str, default=None, help="folder of <K>.joblib / <K>.npy k-means codebooks")
    p.add_argument("--device", type=int, default=0)
    return p


def run(args, quantizer: Optional[prosst.PdbQuantizer] = None) -> int:
    """Returns the number of structures that failed."""
    if args.out_dir is None or (args.pdb_dir is None and args.pdb_file is None):
        raise SystemExit("--out_dir and one of --pdb_dir / --pdb_file are required")
    for v in args.vocab_size:
        if v not in prosst.VOCAB_SIZES:
            raise SystemExit(f"--vocab_size {v}: one of {list(prosst.VOCAB_SIZES)}")
    sizes = list(dict.fromkeys(args.vocab_size))
    if args.pdb_dir is not None:
        jobs = [(f[:-4], os.path.join(args.pdb_dir, f)) for f in sorted(os.listdir(args.pdb_dir)) if f.endswith(".pdb")]
    else:
        jobs = [(os.path.splitext(os.path.basename(args.pdb_file))[0], args.pdb_file)]
    os.makedirs(args.out_dir, exist_ok=True)
    for v in sizes:
        os.makedirs(os.path.join(args.out_dir, str(v)), exist_ok=True)
    q = quantizer or prosst.PdbQuantizer(sizes, model_path=args.model_path, cluster_dir=args.cluster_dir, device=args.device)
    failed: List[str] = []
    try:
        for name, path in jobs:
            out = {v: os.path.join(args.out_dir, str(v), name + ".fasta") for v in sizes}
            todo = [v for v in sizes if args.overwrite or args.pdb_dir is None or not os.path.exists(out[v])]
            if not todo:
                continue
            try:
                _, tokens = q.tokens_for(path)
            except Exception as e:               # the reference's process_pdb_file: report the file and go on
                print(f"Error in processing {path}: {e}", file=sys.stderr)
                failed.append(name)
                continue
            for v in todo:
                with open(out[v], "w") as f:
                    f.write(prosst.fasta_text(name, tokens[v]))
    finally:
        if quantizer is None:
            q.close()
    if failed:
        print("Error proteins: ", failed, file=sys.stderr)
    return len(failed)


def main(argv=None) -> int:
    return 1 if run(parser().parse_args(argv)) else 0


if __name__ == "__main__":
    sys.exit(main())
