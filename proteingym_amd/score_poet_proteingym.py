"""Drop-in for ``proteingym/baselines/PoET/scripts/score.py`` on MI355X.

Same flags and the same file: ``<output_scores_folder>/<DMS_filename>`` with the columns ``mutated_sequence`` and ``PoET_score`` -- the
mean over 15 ensemble members (3 context lengths x 5 similarity cut-offs) of (forward + backward) / 2 of log p(variant | prompt).  The
homology weights are computed once per MSA and every prompt is encoded once per direction; a variant costs its own rows against the
cached prompt.  --batch_size is accepted and has no effect on the arithmetic: the library packs variants itself.

A DMS file without a ``mutated_sequence`` column is refused: the reference would encode its mutant strings ("A25G") as sequences.
The MSA is ``<MSA_folder>/<DMS_filename stem>.a3m.zst`` (needs a zstd module) or, failing that, ``<stem>.a3m`` in the same folder.
Additive flags: --device, --max_rows."""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import pandas as pd

from . import poet


def parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="PoET log-likelihood scores (HIP, MI355X)", formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("--checkpoint", type=str, default="proteingym/baselines/PoET/scripts/data/poet.ckpt")
    p.add_argument("--DMS_reference_file_path", type=str, default="reference_files/DMS_substitutions.csv")
    p.add_argument("--DMS_data_folder", type=str, default="data/DMS_ProteinGym_substitutions")
    p.add_argument("--DMS_index", type=int, default=1, help="zero-based row (iloc) of the reference file")
    p.add_argument("--output_scores_folder", type=str, default="data/zero_shot_substitutions_scores/PoET")
    p.add_argument("--MSA_folder", type=str, default="proteingym/baselines/PoET/scripts/data/msas/DMS_substitutions")
    p.add_argument("--context_lengths", type=int, nargs="+", default=list(poet.CONTEXT_LENGTHS))
    p.add_argument("--relative_to_wt", action="store_true")
    p.add_argument("--batch_size", type=int, default=8, help="accepted; no effect on the scores (the library packs variants itself)")
    p.add_argument("--seed", type=int, default=poet.SEED)
    p.add_argument("--device", type=int, default=0, help="HIP device")
    p.add_argument("--max_rows", type=int, default=0, help="workspace rows (0: sized from the largest prompt)")
    return p


def main(argv=None) -> str:
    """Scores one assay and returns the path of the CSV."""
    args = parser().parse_args(argv)
    os.makedirs(args.output_scores_folder, exist_ok=True)
    ref = pd.read_csv(args.DMS_reference_file_path).iloc[args.DMS_index]
    msa_start, msa_end = int(ref["MSA_start"]), int(ref["MSA_end"])
    wt_sequence = ref["target_seq"][msa_start - 1:msa_end]
    filename = ref["DMS_filename"]
    df = pd.read_csv(os.path.join(args.DMS_data_folder, filename))
    if "mutated_sequence" not in df.columns:
        raise SystemExit(f"{filename}: no mutated_sequence column (the reference would score the mutant strings themselves as sequences)")
    variant_sequences = df["mutated_sequence"].values
    variants = [poet.frame(v) for v in variant_sequences]
    if args.relative_to_wt:
        variants.append(poet.frame(wt_sequence))
    for i, v in enumerate(variants):
        if (v == poet.GAP).any():
            raise SystemExit(f"variant {i} holds a gap character")

    try:
        msa_sequences = poet.read_msa(args.MSA_folder, filename)
    except (FileNotFoundError, RuntimeError) as e:
        raise SystemExit(str(e)) from None
    if not msa_sequences or msa_sequences[0].decode() != wt_sequence:
        raise SystemExit(f"{filename}: the first MSA row is not target_seq[MSA_start-1:MSA_end]")
    msa = poet.encoded_msa(msa_sequences)
    weights = poet.homology_weights(poet.neighbor_counts(msa, poet.THETA, args.device))
    prompts = poet.member_prompts(msa_sequences, msa, weights, args.context_lengths, args.seed)

    longest = poet.max_prompt_tokens(prompts)
    padded = max((sum((s.size + 31) // 32 * 32 for s in p) for _, p in prompts), default=0)
    max_rows = args.max_rows or max(padded + 32, 16384)
    model = poet.from_checkpoint(args.checkpoint, device=args.device, max_rows=max_rows, max_prompt=longest)
    try:
        logps = poet.ensemble_scores(model, prompts, variants, args.relative_to_wt)
    finally:
        model.close()
    out_path = os.path.join(args.output_scores_folder, filename)
    pd.DataFrame(data={"mutated_sequence": variant_sequences, "PoET_score": logps}).to_csv(out_path, index=False)
    return out_path


if __name__ == "__main__":
    main(sys.argv[1:])
