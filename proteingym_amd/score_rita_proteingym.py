"""Drop-in for ``proteingym/baselines/rita/compute_fitness.py`` on MI355X.

Same flags, same assay resolution (row --DMS_index of the reference file), same output file ``<output_scores_folder>/<DMS_id>.csv``
with the columns the reference writes (mutant, RITA_score, DMS_score).  Scores are the reference's calc_fitness: the sum over
(chunk, direction) of -mean CE (proteingym_amd/causal_lm.py).  Additive flags: --tokenizer_path (the reference hard-codes its
tokenizer directory; default here: the model directory), --device, --max_rows.
"""
from __future__ import annotations

import argparse

from . import causal_lm as clm


def parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="RITA scoring (HIP, MI355X)")
    clm.add_common_flags(p, "--RITA_model_name_or_path", "RITA checkpoint directory (config.json + pytorch_model.bin / model.safetensors)")
    return p


def main(argv=None):
    args = parser().parse_args(argv)
    return clm.score_assay(args, args.RITA_model_name_or_path, "RITA", "RITA_score", ["mutant", "RITA_score", "DMS_score"])


if __name__ == "__main__":
    main()
