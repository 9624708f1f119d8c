"""Drop-in for ``proteingym/baselines/progen2/compute_fitness.py`` on MI355X.

Same flags, same assay resolution (row --DMS_index of the reference file), same output file ``<output_scores_folder>/<DMS_id>.csv``
with the columns the reference writes (mutant, Progen2_score, DMS_score).  Scores are compute_fitness.py:35-82's calc_fitness
(proteingym_amd/progen2.py), the terminals '1' ... '2' added only when the assay has no mutated_sequence column and --indel_mode is
off (:143-144).  Additive flags: --device, --max_rows.
"""
from __future__ import annotations

import argparse
import json
import os

import numpy as np

from . import causal_lm as clm, progen2 as pg

# compute_fitness.py --test (:146-159): the reference's own check of a checkpoint -- one sequence and the log-likelihood each released
# checkpoint must give it (reduction 'sum', tolerance 0.1).  These constants are part of the reference CLI's behaviour that --test
# reproduces, so they live with the CLI.
X_UNIREF90BFD30 = ("2GFLPFRGADEGLAAREAATLAARGTAARAYREDSWAVPVPRGLLGDLTARVAALGAASPPPADPLAVTLDLHHVTAEVALTTVLDAATLVHGQTRVLSAEDAAEAATAAAAATEAY"
                   "LERLQDFVLFMSASVRVWRRGNAAGATGPEWDQWYTVADRDALGSAPTHLAVLGRQADALCHFVLDRVAWGTCGTPLWSGDEDLGNVVATFAGYADRLATAPRDLIM1")
CHECKPOINT_X_LL = {"progen2-small": (X_UNIREF90BFD30, -2.4), "progen2-medium": (X_UNIREF90BFD30, -1.9),
                   "progen2-base": (X_UNIREF90BFD30, -1.9), "progen2-large": (X_UNIREF90BFD30, -1.8),
                   "progen2-xlarge": (X_UNIREF90BFD30, -1.0)}


def parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="ProGen2 scoring (HIP, MI355X)")
    p.add_argument("--Progen2_model_name_or_path", type=str, required=True, help="ProGen2 checkpoint directory (config.json + pytorch_model.bin)")
    p.add_argument("--DMS_reference_file_path", type=str, help="reference CSV listing the assays (DMS_id, DMS_filename, target_seq)")
    p.add_argument("--DMS_data_folder", type=str, help="folder holding the assay CSVs")
    p.add_argument("--DMS_index", type=int, help="row of the reference CSV to score")
    p.add_argument("--output_scores_folder", type=str, default=None, help="where <DMS_id>.csv is written")
    p.add_argument("--indel_mode", action="store_true", help="score the mutated_sequence column as it is (insertions / deletions)")
    p.add_argument("--fp16", action="store_true", help="accepted; scoring always runs in f16x3 (split-fp16 operands, fp32-class results)")
    p.add_argument("--test", action="store_true", help="the reference's check of the checkpoint on one known sequence first")
    p.add_argument("--device", type=int, default=0, help="HIP device")
    p.add_argument("--max_rows", type=int, default=0, help="workspace rows per device call (0 = library default)")
    return p


def main(argv=None):
    args = parser().parse_args(argv)
    if args.fp16:
        print("--fp16: scoring runs in f16x3 (split-fp16 GEMM and attention operands, fp32 accumulation)")
    config = json.load(open(os.path.join(args.Progen2_model_name_or_path, "config.json")))
    print("Maximum context length: {}".format(config["n_positions"]))
    model = pg.from_pretrained(args.Progen2_model_name_or_path, device=args.device, max_rows=args.max_rows)
    DMS_id, target_seq, DMS_data = clm.load_assay(args, "Progen2", args.Progen2_model_name_or_path)
    if args.test:
        model_size = args.Progen2_model_name_or_path.rstrip("/").split("/")[-1]
        seq, expected = CHECKPOINT_X_LL[model_size]
        score = model.calc_fitness(np.array([seq]), model_context_len=1024, reduction="sum")     # the reference's default (:35)
        print(score, expected, abs(score - expected))
        assert abs(score - expected) < 0.1
    prots = pg.sequences_to_score(DMS_data, target_seq, args.indel_mode)
    DMS_data["Progen2_score"] = model.calc_fitness(prots, model_context_len=int(config["n_positions"]))
    out = clm.write_scores(args, DMS_id, DMS_data, ["mutant", "Progen2_score", "DMS_score"])
    model.close()
    return out


if __name__ == "__main__":
    main()
