"""TranceptEVE on the HIP path (``proteingym/baselines/trancepteve``): Tranception with two inference-time priors, the retrieved
alignment's (MSA) and the EVE Bayesian VAE's.

Device work: ``pgmi_eve_log_prior`` (the EVE log-prior of the wild type, eve.EveModel.log_prior) and the three-way fusion inside the
sequence log-likelihood (``pgmi_tr_sequence_loglik_eve`` / ``_shared_eve``, through tranception.TranceptionModel).  Host work, here: the
alignments and depths (trancepteve/utils/msa_utils.py:63-139, model_pytorch.py:907-938), the log-prior table and its cache
(:940-1001), the aggregation weights (:722-763), the two recalibrations (:822-905; fusion, means and the temperature iteration in
torch fp32 on the device's token log-probabilities) and the retrieval state ``TranceptionModel.score_mutants`` scores with.
DESIGN.md 4.6g has the estimator and what differs from the reference on purpose.
"""
from __future__ import annotations

import json
import os
import pickle
from typing import List, Optional, Sequence

import numpy as np

from . import alignment, eve, tranception as ptr

ALPHABET = alignment.AMINO_ACIDS


# ---- aggregation weights (model_pytorch.py:722-763) ---------------------------------------------------------------------------------
def aggregation_weights(retrieval_type: str, aggregation_mode: str, msa_depth: int, eve_depth: int, manual: bool = False,
                        manual_msa_weight: float = 0.5, manual_eve_weight: float = 0.5):
    """(alpha, beta): the MSA and EVE weights of the fusion."""
    if manual:
        return manual_msa_weight, manual_eve_weight
    if retrieval_type == "Tranception":
        return 0.6, 0.0
    if retrieval_type != "TranceptEVE":
        raise ValueError(f"inference_time_retrieval_type {retrieval_type!r}: Tranception or TranceptEVE")
    if aggregation_mode == "aggregate_indel":
        return (0.0, 0.0) if msa_depth < 10 else (0.5, 0.1)

    def table(depth, values):
        for power, v in zip(range(1, 6), values):
            if depth < 10 ** power:
                return v
        return values[5]
    return table(msa_depth, (0.0, 0.1, 0.3, 0.4, 0.4, 0.5)), table(eve_depth, (0.0, 0.3, 0.6, 0.7, 0.7, 0.8))


# ---- EVE alignment, checkpoints, log-prior ---------------------------------------------------------------------------------------------
class EveMSA:
    """What TranceptEVE reads off EVE's ``MSA_processing`` (model_pytorch.py:912-919): focus columns under
    ``threshold_focus_cols_frac_gaps``, the focus sequence over them and the number of sequences kept (``EVE_processed_depth``)."""

    def __init__(self, MSA_location: str, threshold_sequence_frac_gaps=0.5, threshold_focus_cols_frac_gaps=1.0):
        fa = alignment.FocusAlignment(MSA_location, True, threshold_sequence_frac_gaps, threshold_focus_cols_frac_gaps, True)
        self.focus_seq = fa.focus_seq
        self.focus_cols = [int(c) for c in fa.focus_cols]
        self.focus_seq_trimmed = "".join(self.focus_seq[c] for c in self.focus_cols)
        self.depth = len(fa.names)


def eve_model_paths(EVE_model_folder: str, MSA_data_file: str, UniProt_ID: Optional[str], seeds: Sequence) -> List[str]:
    """score_trancepteve.py:128-142: <folder>/<MSA stem>_seed_<s>, else <folder>/<UniProt_ID>_seed_<s>."""
    out = []
    stem = os.path.basename(MSA_data_file.split(".a2m")[0])
    for seed in seeds:
        for name in (f"{stem}_seed_{seed}", f"{UniProt_ID}_seed_{seed}"):
            if os.path.exists(f"{EVE_model_folder}/{name}"):
                out.append(EVE_model_folder + os.sep + name)
                break
        else:
            raise FileNotFoundError(f"No EVE Model available for {MSA_data_file} with random seed {seed} in {EVE_model_folder}")
    return out


def log_prior_table(logp: np.ndarray, focus_cols: Sequence[int], MSA_start: int, full_sequence_len: int) -> np.ndarray:
    """model_pytorch.py:996-998: float32 [full_sequence_len, 25], -inf except [MSA_start + focus columns, 5:]."""
    table = np.full((full_sequence_len, 25), -np.inf, dtype=np.float32)
    table[[MSA_start + c for c in focus_cols], 5:] = np.asarray(logp, dtype=np.float32)
    return table


def cache_location(EVE_model_path: str, num_samples: int) -> str:
    parts = EVE_model_path.split("/")
    return "/".join(parts[:-1]) + os.sep + "log_prior" + os.sep + "_".join([parts[-1], str(num_samples), "log_space"])


def eve_log_prior(model_paths: Sequence[str], params_location: str, msa: EveMSA, full_sequence_len: int, MSA_start: int,
                  num_samples: int = 10, use_cache: bool = True, device: int = 0) -> np.ndarray:
    """get_EVE_models_and_log_prior (model_pytorch.py:940-973): the mean over the seeds' checkpoints of each one's log-prior table.  A
    table is read from ``<folder>/log_prior/<name>_<num_samples>_log_space`` when that file exists (the reference's format: a pickled
    torch tensor; its files are read, ours are readable by it) and written there otherwise; ``use_cache=False`` neither reads nor writes.
    The generator's seed is the checkpoint's seed number (the digits after ``_seed_``)."""
    import torch
    with open(params_location) as f:
        params = json.load(f)
    residues = eve.encode_residues([msa.focus_seq_trimmed])
    total = 0
    for path in model_paths:
        where = cache_location(path, num_samples)
        if use_cache and os.path.exists(where):
            print("Loading EVE log prior from disk")
            with open(where, "rb") as f:
                single = pickle.load(f)
            single = torch.as_tensor(single).detach().cpu().float()
        else:
            print("Computing EVE log prior")
            d, blob = eve.load_checkpoint(path, params, len(msa.focus_cols))
            model = eve.EveModel(d, blob, device=device)
            tail = os.path.basename(path).rsplit("_seed_", 1)[-1]
            try:
                mean, _ = model.log_prior(residues[0], num_samples, seed=int(tail) if tail.isdigit() else 0)
            finally:
                model.close()
            single = torch.from_numpy(log_prior_table(mean, msa.focus_cols, MSA_start, full_sequence_len))
            if use_cache:
                os.makedirs(os.path.dirname(where), exist_ok=True)
                with open(where, "wb") as f:
                    pickle.dump(single, f)
        total = total + single
    return (total / len(model_paths)).numpy()


# ---- recalibration (model_pytorch.py:822-905) --------------------------------------------------------------------------------------
def fuse_host(shift_log_probas, start_slice, end_slice, state, retrieval_type):
    """The forward's fusion (model_pytorch.py:1087-1133) for unflipped substitution windows, in torch fp32: shift_log_probas
    [B, T - 1, V]; ``state``: MSA_log_prior / EVE_log_prior tensors, MSA_start, MSA_end, alpha, beta, eve_fallback."""
    fused = shift_log_probas.clone()
    if retrieval_type is None:
        return fused
    a, b = state["alpha"], state["beta"]
    for i in range(fused.shape[0]):
        if not (state["MSA_start"] < end_slice[i] and state["MSA_end"] > start_slice[i]):
            continue
        lo, hi = max(start_slice[i], state["MSA_start"]), min(end_slice[i], state["MSA_end"])
        if hi <= lo:
            continue
        msa = state["MSA_log_prior"][lo:hi, :]
        r0 = max(0, state["MSA_start"] - start_slice[i])
        r1 = r0 + (hi - lo)
        two = (1 - a) * shift_log_probas[i, r0:r1, 5:] + a * msa[..., 5:]
        if retrieval_type == "Tranception":
            fused[i, r0:r1, 5:] = two
        else:
            fused[i, r0:r1, 5:] = (1 - b) * two + b * state["EVE_log_prior"][lo:hi, 5:]
            if state["eve_fallback"]:
                rows = [ix for ix in range(fused.shape[1]) if fused[i, ix, 5:].min() == -np.inf]
                inside = [ix for ix in rows if state["MSA_start"] <= ix + start_slice[i] < state["MSA_end"]]
                outside = [ix for ix in rows if ix not in inside]
                fused[i, inside, 5:] = (1 - a) * shift_log_probas[i, inside, 5:] + a * msa[[ix + start_slice[i] - lo for ix in inside], 5:]
                fused[i, outside, 5:] = (1 - a) * shift_log_probas[i, outside, 5:]
    return fused


def transformer_log_softmax(model: ptr.TranceptionModel, sequence: str, state, retrieval_type="Tranception"):
    """get_transformer_log_softmax (model_pytorch.py:822-874): the (fused) log-probabilities [len(sequence) + 1, V] of the wild type
    over consecutive windows of n_ctx - 2 residues, the token log-probabilities from the device."""
    import torch
    ctx = model.n_ctx - 2
    num_windows = 1 + int(len(sequence) / ctx)
    starts = [w * ctx for w in range(num_windows)]
    windows = [sequence[s:s + ctx] for s in starts]
    ends = [min(len(sequence), s + ctx) for s in starts]
    ids, _ = model.encode_batch(windows)
    logp = torch.from_numpy(model.token_logprobs(ids))[:, :-1, :].contiguous()
    fused = fuse_host(logp, starts, ends, state, retrieval_type)
    V = fused.shape[-1]
    if num_windows > 1:
        trimmed = torch.zeros((len(sequence) + 1, V))
        at = 0
        for w in range(num_windows):
            if w < num_windows - 1:
                trimmed[at:at + ctx] = fused[w, :ctx]
            else:
                trimmed[at:] = fused[w, :len(sequence) + 1 - at]
            at += ctx
        fused = trimmed
    return fused.view(-1, V)[:len(sequence) + 1]


def iterative_recalibrations(log_proba_to_calibrate, avg_log_proba_target, distance_stop_criterion=0.001, max_steps=1000):
    """model_pytorch.py:876-886, as written."""
    import torch
    loss = abs(log_proba_to_calibrate.mean() - avg_log_proba_target)
    step = 0
    while loss > distance_stop_criterion:
        T = log_proba_to_calibrate.mean() / avg_log_proba_target
        log_proba_to_calibrate = torch.log_softmax(log_proba_to_calibrate / T, dim=-1)
        loss = abs(log_proba_to_calibrate.mean() - avg_log_proba_target)
        step += 1
        if step > max_steps:
            break
    return log_proba_to_calibrate


def recalibrate_MSA_probas(model, target_seq, state):
    """model_pytorch.py:888-895.  The reference asks get_transformer_log_softmax for retrieval type None, which its forward replaces by
    the model's own type (:1035): the rows are the fully fused ones, in both directions, the reversed pass with the unflipped priors and
    indexed by the same rows -- reproduced as it runs."""
    lr = transformer_log_softmax(model, target_seq, state, state["type"])
    rl = transformer_log_softmax(model, target_seq[::-1], state, state["type"])
    s, e = state["MSA_start"], state["MSA_end"]
    target = (lr[s:e, 5:].mean() + rl[s:e, 5:].mean()) / 2.0
    print("Optimal temperature for MSA proba recalibration: {}".format(state["MSA_log_prior"][s:e, 5:].mean() / target))
    state["MSA_log_prior"][s:e, 5:] = iterative_recalibrations(state["MSA_log_prior"][s:e, 5:], avg_log_proba_target=target)


def recalibrate_EVE_probas(model, target_seq, state, focus_cols):
    """model_pytorch.py:897-905: the transformer fused with the MSA prior (the default retrieval type ``"Tranception"`` of
    get_transformer_log_softmax) in both directions, the reversed pass with the unflipped prior -- both as the reference runs them."""
    lr = transformer_log_softmax(model, target_seq, state)
    rl = transformer_log_softmax(model, target_seq[::-1], state)
    cols = [state["MSA_start"] + c for c in focus_cols]
    target = (lr[cols, 5:].mean() + rl[cols, 5:].mean()) / 2.0
    print("Optimal temperature for EVE proba recalibration: {}".format(state["EVE_log_prior"][cols, 5:].mean() / target))
    state["EVE_log_prior"][cols, 5:] = iterative_recalibrations(state["EVE_log_prior"][cols, 5:], avg_log_proba_target=target)


# ---- the retrieval state of one assay ---------------------------------------------------------------------------------------------
def build_state(model: ptr.TranceptionModel, target_seq: str, MSA_filename: str, MSA_weight_file_name: Optional[str], MSA_start: int,
                MSA_end: int, indel_mode: bool = False, threshold_sequence_frac_gaps=0.5, threshold_focus_cols_frac_gaps=1.0,
                retrieval_type: str = "TranceptEVE", eve_table: Optional[np.ndarray] = None, eve_msa: Optional[EveMSA] = None,
                manual_weights: bool = False, manual_msa_weight: float = 0.5, manual_eve_weight: float = 0.5,
                MSA_recalibrate: bool = False, EVE_recalibrate: bool = False, clustal_omega_location: Optional[str] = None,
                seq_name_to_weight=None) -> dict:
    """The dict ``TranceptionModel.retrieval`` of a TranceptEVE (or Tranception) run, built as the reference's constructor and
    ``score_mutants`` build theirs (model_pytorch.py:684-763, :1190-1191): MSA prior and depth, EVE table and depth, weights,
    recalibrations.  ``eve_table`` [len(target_seq), 25] is ``eve_log_prior``'s result (or a recorded one)."""
    import torch
    mode = "aggregate_indel" if indel_mode else "aggregate_substitution"
    prior, msa_depth = ptr.get_msa_prior(MSA_filename, MSA_weight_file_name, MSA_start, MSA_end, len(target_seq),
                                         retrieval_aggregation_mode=mode, seq_name_to_weight=seq_name_to_weight,
                                         threshold_sequence_frac_gaps=threshold_sequence_frac_gaps, return_depth=True)
    eve_on = retrieval_type == "TranceptEVE"
    if eve_on and (eve_table is None or eve_msa is None):
        raise ValueError("TranceptEVE needs the EVE log-prior table and its alignment")
    eve_depth = eve_msa.depth if eve_on else 0
    alpha, beta = aggregation_weights(retrieval_type, mode, msa_depth, eve_depth, manual_weights, manual_msa_weight, manual_eve_weight)
    print("Aggregation weights of retrieved MSA & EVE model are based on processed MSA depth: MSA({}) and EVE({})".format(alpha, beta))
    fallback = bool(eve_on and threshold_focus_cols_frac_gaps < 1.0 and not indel_mode)
    # the recalibrations always run the forward in aggregate_substitution mode (model_pytorch.py:853): their fallback (:1121) does not
    # look at the run's own mode
    recal_fallback = bool(eve_on and threshold_focus_cols_frac_gaps < 1.0)
    state = dict(type=retrieval_type, MSA_log_prior=torch.log(torch.tensor(prior).float()), MSA_start=int(MSA_start), MSA_end=int(MSA_end), alpha=alpha,
                 beta=beta, eve_fallback=recal_fallback,
                 EVE_log_prior=torch.tensor(np.asarray(eve_table, dtype=np.float32)) if eve_on else None)
    saved, model.retrieval = model.retrieval, None                  # the recalibrations read the bare transformer's rows
    try:
        if MSA_recalibrate:
            recalibrate_MSA_probas(model, target_seq, state)
        if EVE_recalibrate and eve_on:
            recalibrate_EVE_probas(model, target_seq, state, eve_msa.focus_cols)
    finally:
        model.retrieval = saved
    out = dict(log_prior=state["MSA_log_prior"].numpy(), MSA_start=int(MSA_start), MSA_end=int(MSA_end), weight=float(alpha),
               MSA_processed_depth=int(msa_depth), EVE_processed_depth=int(eve_depth), eve_weight=float(beta))
    if eve_on:
        out.update(eve_log_prior=state["EVE_log_prior"].numpy(), eve_fallback=fallback)
    if indel_mode:
        out["aligner"] = ptr.SequenceAligner(MSA_filename, clustal_omega_location)
    return out
