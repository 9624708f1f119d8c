"""Drop-in for ``python -m vespag predict`` and ``python -m vespag eval proteingym`` (proteingym/baselines/vespag) on MI355X.

    python -m proteingym_amd.score_vespag_proteingym predict -i proteins.fasta -o out --checkpoint-file state_dict_v2.pt --plm esm2_t36_3B_UR50D.pt
    python -m proteingym_amd.score_vespag_proteingym eval-proteingym --reference-file DMS_substitutions.csv --dms-directory DMS/ -o out \
        --checkpoint-file state_dict_v2.pt -e embeddings.npz

``predict`` has the reference's flags (runner/predict.py): every single-residue variant of every protein of the FASTA, or the mutants of
``--mutation-file`` (a CSV with a header line: protein id, ``:``-joined mutant); ``<id>.csv`` with the header ``mutant,VespaG`` per protein,
or ``vespag_scores_all.csv`` with ``DMS_id,mutant,VespaG``.  ``eval-proteingym`` has eval/eval.py's: one ``<DMS_id>.csv`` per assay of the
reference file, which merge.py reads under config.json's ``VespaG`` entry (key ``mutant``), and ``VespaG_Spearman_per_DMS.csv`` for the
assays that carry ``DMS_score`` (the reference's closing step reads a file its own call never writes; here the correlation is computed
from the per-assay frames).

Without ``-e`` the embeddings are computed here: ``--plm`` is a local fair-esm ESM2 ``.pt`` or a local HF ``EsmModel`` directory (ESM2-3B for
the released head; nothing is downloaded), the whole FASTA goes through pgmi_vespag_landscapes, and ``--save-embeddings out.npz`` keeps the
rows for re-use as the reference keeps its ``esm2_embeddings.h5``.  ``-e`` takes an ``.npz`` (id -> [L, 2560]), or the reference's ``.h5`` where
h5py is installed.  A forward that leaves the fp16 range is repeated in precision fp32.  Additive flags: --plm, --device, --precision,
--max_rows, --save-embeddings.  ``--h5-output`` is refused without h5py.
"""
from __future__ import annotations

import argparse
import os
import sys
from typing import Dict, List, Optional

import numpy as np

from . import _lib, vespag


def _pair(p, on: str, off: str, dest: str, default: bool, help: str):
    p.add_argument(on, dest=dest, action="store_true", default=default, help=help)
    p.add_argument(off, dest=dest, action="store_false", help=argparse.SUPPRESS)


def _common(p):
    p.add_argument("-o", "--output", dest="output_path", default=None, help="output folder (default: ./output)")
    p.add_argument("-e", "--embeddings", dest="embedding_file", default=None, help="pre-computed ESM2 embeddings (.npz; .h5 with h5py)")
    p.add_argument("--checkpoint-file", dest="checkpoint_file", default=None, help="state_dict_v2.pt (default: ./model_weights/state_dict_v2.pt)")
    p.add_argument("--id-map", dest="id_map_file", default=None, help="CSV mapping embedding ids to FASTA ids")
    _pair(p, "--normalize", "--dont-normalize", "normalize_scores", True, "scores through 1 / (1 + exp(-s)) (default)")
    p.add_argument("--plm", default=None, help="local ESM2 .pt or HF EsmModel directory; required unless -e is given")
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--precision", choices=("f16x3", "fp32"), default="f16x3")
    p.add_argument("--max_rows", type=int, default=0, help="workspace rows per device call (0 = library default)")
    p.add_argument("--save-embeddings", dest="save_embeddings", default=None, help="write the residue rows computed here to this .npz (refused with -e)")


def parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="VespaG scoring (HIP, MI355X)")
    sub = p.add_subparsers(dest="command", required=True)
    a = sub.add_parser("predict", help="vespag predict")
    a.add_argument("-i", "--input", dest="fasta_file", required=True, help="FASTA file of protein sequences")
    a.add_argument("--mutation-file", dest="mutation_file", default=None, help="CSV (with a header line) of protein id, mutant")
    _pair(a, "--single-csv", "--multi-csv", "single_csv", False, "one vespag_scores_all.csv instead of one CSV per protein")
    _pair(a, "--no-csv", "--csv", "no_csv", False, "write no CSV")
    _pair(a, "--h5-output", "--no-h5-output", "h5_output", False, "write vespag_scores_all.h5 (needs h5py)")
    _pair(a, "--zero-idx", "--one-idx", "zero_based_mutations", False, "positions start at 0")
    _common(a)
    b = sub.add_parser("eval-proteingym", help="vespag eval proteingym")
    b.add_argument("--reference-file", dest="dms_reference_file", required=True, help="DMS reference file")
    b.add_argument("--dms-directory", dest="dms_directory", required=True, help="folder of the per-DMS score files")
    _common(b)
    return p


class Scorer:
    """The head of the run, with the ESM2 model when embeddings are computed here; a forward that leaves the fp16 range (PGMI_EOVERFLOW)
    is repeated on an fp32 pair, built once."""

    def __init__(self, sd, plm: Optional[str], device: int, precision: str, max_rows: int):
        self.sd, self.plm, self.device, self.max_rows = sd, plm, device, max_rows
        self.pair = self._build(precision)
        self.fp32 = None

    def _build(self, precision: str):
        esm = None
        if self.plm:
            from . import protssn
            esm = protssn.load_plm(self.plm, device=self.device, precision=precision, max_rows=self.max_rows)
        try:
            return esm, vespag.from_state_dict(self.sd, esm=esm, device=self.device, precision=precision)
        except Exception:
            if esm is not None:
                esm.close()
            raise

    def landscapes(self, seqs, want_rows: bool):
        def run(pair):
            r = pair[1].landscapes(seqs, want_rows=want_rows)
            return r if want_rows else (r, None)
        try:
            return run(self.pair)
        except _lib.PgmiError as e:
            if e.code != _lib.EOVERFLOW:
                raise
        print("[proteingym_amd] an activation left the fp16 range: embedding these proteins in precision fp32", file=sys.stderr)
        if self.fp32 is None:
            self.fp32 = self._build("fp32")
        return run(self.fp32)

    def head(self, rows, wt_cols):
        try:
            return self.pair[1].head(rows, wt_cols)
        except _lib.PgmiError as e:
            if e.code != _lib.EOVERFLOW or self.pair[1].config.precision == _lib.PREC_FP32:
                raise
        print("[proteingym_amd] a row left the fp16 range: running the head on these rows in precision fp32", file=sys.stderr)
        if self.fp32 is None:
            self.fp32 = self._build("fp32")
        return self.fp32[1].head(rows, wt_cols)

    def close(self):
        for pair in (self.pair, self.fp32):
            if pair:
                pair[1].close()
                if pair[0] is not None:
                    pair[0].close()


def check_outputs(args):
    """The refusals that need no model."""
    if getattr(args, "h5_output", False):
        try:
            import h5py  # noqa: F401
        except ImportError:
            raise RuntimeError("--h5-output needs h5py, which is not installed; the CSV output holds the same scores") from None
    if args.embedding_file and args.save_embeddings:
        raise ValueError("--save-embeddings writes the rows computed here; with -e/--embeddings none are computed")
    if not args.embedding_file and not args.plm:
        raise ValueError("--plm is required unless -e/--embeddings is given (a local ESM2 .pt or HF EsmModel directory; nothing is downloaded)")


def score_proteins(args, sequences: Dict[str, str], mutations_per_protein: Optional[Dict[str, list]]):
    """runner/predict.py from the loaded sequences on: ({id: {mutant: score}}, {id: y [L, 20]})."""
    check_outputs(args)
    sd = vespag.load_checkpoint(args.checkpoint_file or os.path.join(os.getcwd(), "model_weights", "state_dict_v2.pt"))
    input_dim, _ = vespag.check_state_dict(sd)
    one_indexed = not getattr(args, "zero_based_mutations", False)
    ids = list(sequences)
    scorer = None
    try:
        if args.embedding_file:
            emb = vespag.load_embeddings(args.embedding_file)
            if args.id_map_file:
                emb = vespag.apply_id_map(emb, args.id_map_file)
            for pid in ids:
                if pid not in emb:
                    raise KeyError(f"{args.embedding_file}: no embedding for {pid!r}")
                vespag.check_embedding(pid, sequences[pid], emb[pid], input_dim)
            scorer = Scorer(sd, None, args.device, args.precision, args.max_rows)
            ys = {pid: scorer.head(emb[pid], vespag.wt_columns(sequences[pid])) for pid in ids}
        else:
            scorer = Scorer(sd, args.plm, args.device, args.precision, args.max_rows)
            y, rows = scorer.landscapes([sequences[pid] for pid in ids], want_rows=bool(args.save_embeddings))
            ys = dict(zip(ids, y))
            if args.save_embeddings:
                np.savez(args.save_embeddings, **dict(zip(ids, rows)))
    finally:
        if scorer is not None:
            scorer.close()
    if mutations_per_protein is None:
        mutations_per_protein = {pid: vespag.landscape(seq, one_indexed) for pid, seq in sequences.items()}
    scores = {pid: vespag.score_mutations(ys[pid], mutations_per_protein.get(pid, []), args.normalize_scores) for pid in ids}
    return scores, ys


def write_csvs(output_path: str, scores: Dict[str, Dict[str, float]], single_csv: bool):
    """runner/predict.py:206-232."""
    if not single_csv:
        for pid, muts in scores.items():
            with open(os.path.join(output_path, pid + ".csv"), "w") as f:
                f.write("mutant,VespaG\n")
                f.writelines(f"{sav},{score}\n" for sav, score in muts.items())
    else:
        with open(os.path.join(output_path, "vespag_scores_all.csv"), "w") as f:
            f.write("DMS_id,mutant,VespaG\n")
            f.writelines(f"{pid},{sav},{score}\n" for pid, muts in scores.items() for sav, score in muts.items())


def predict(args) -> int:
    out = args.output_path or os.path.join(os.getcwd(), "output")
    os.makedirs(out, exist_ok=True)
    sequences = vespag.read_fasta(args.fasta_file)
    muts = vespag.read_mutation_file(args.mutation_file, not args.zero_based_mutations) if args.mutation_file else None
    scores, ys = score_proteins(args, sequences, muts)
    if args.h5_output:
        import h5py
        with h5py.File(os.path.join(out, "vespag_scores_all.h5"), "w") as f:
            for pid, y in ys.items():
                f.create_dataset(pid, data=y)
    if not args.no_csv:
        write_csvs(out, scores, args.single_csv)
    return 0


def eval_proteingym(args) -> int:
    import pandas as pd
    out = args.output_path or os.path.join(os.getcwd(), "output", "proteingym217")
    os.makedirs(out, exist_ok=True)
    ref = pd.read_csv(args.dms_reference_file)
    sequences = {row["DMS_id"]: row["target_seq"] for _, row in ref.iterrows()}
    frames = {row["DMS_id"]: pd.read_csv(os.path.join(args.dms_directory, row["DMS_filename"])) for _, row in ref.iterrows()}
    muts = {pid: [vespag.Mutation.from_mutation_string(m, one_indexed=True) for m in df["mutant"].astype(str)] for pid, df in frames.items()}
    scores, _ = score_proteins(args, sequences, muts)
    write_csvs(out, scores, single_csv=False)
    records: List[dict] = []
    for pid, df in frames.items():
        if "DMS_score" not in df.columns:
            continue
        from scipy.stats import spearmanr
        pred = df["mutant"].astype(str).map(scores[pid])
        records.append({"DMS_id": pid, "spearman": spearmanr(df["DMS_score"], pred).correlation})
    if records:
        res = pd.DataFrame.from_records(records)
        res.to_csv(os.path.join(out, "VespaG_Spearman_per_DMS.csv"), index=False)
        print(f"Mean Spearman r: {res['spearman'].mean():.3f}")
    return 0


def main(argv=None) -> int:
    args = parser().parse_args(argv)
    return predict(args) if args.command == "predict" else eval_proteingym(args)


if __name__ == "__main__":
    sys.exit(main())
