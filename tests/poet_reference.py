"""TEST INFRASTRUCTURE ONLY -- drives the unmodified reference PoET code (proteingym/baselines/PoET) on the CPU, where the reference
tree exists (oracle.ref_harness.REF_ROOT): the pins of tests/test_poet_host.py and tests/golden/make_golden_poet.py.

The reference's modules import each other as the package ``poet``; they are imported with its folder on sys.path for the duration of
the load only and then moved to private names, so nothing called ``poet`` stays importable.  poet/msa/sampling.py imports numba, which
need not be installed: for that load only, and only when no real numba is importable, a stand-in whose njit / prange are the identity
is registered (and what was registered under the name before is put back).  The reference's embed() / logits() need flash-attn on a GPU; its LAYERS run unmodified on the CPU when the packed
sequences are built paddable, which is what tiered_forward does."""
import importlib
import importlib.util
import os
import sys
import types

import numpy as np

from oracle.ref_harness import REF_ROOT

POET_DIR = os.path.join(REF_ROOT, "proteingym", "baselines", "PoET")
_mods = {}


def reference_available() -> bool:
    return os.path.isfile(os.path.join(POET_DIR, "poet", "models", "poet.py"))


def _numba_stand_in():
    m = types.ModuleType("numba")

    def njit(*args, **kwargs):
        if len(args) == 1 and callable(args[0]) and not kwargs:
            return args[0]
        return lambda f: f
    m.njit, m.prange, m.uint16 = njit, range, int
    return m


def _real_numba() -> bool:
    """A numba that came from an installation (another test module may have left a file-less stub under the name)."""
    m = sys.modules.get("numba")
    if m is not None:
        return getattr(m, "__file__", None) is not None
    try:
        return importlib.util.find_spec("numba") is not None
    except ValueError:
        return False


def _load():
    if _mods:
        return _mods
    if not reference_available():
        raise RuntimeError(f"reference PoET code not found under {POET_DIR}")
    mods = {}
    saved = {k: sys.modules.get(k) for k in ("numba", "pyzstd")}
    if not _real_numba():                                        # for the duration of this load only; a real one is never shadowed
        sys.modules["numba"] = _numba_stand_in()
    if saved["pyzstd"] is None and importlib.util.find_spec("pyzstd") is None:
        sys.modules["pyzstd"] = types.ModuleType("pyzstd")       # score.py imports it at the top; only .zst inputs call it
    sys.path.insert(0, POET_DIR)
    try:
        for name in ("poet.alphabets", "poet.fasta", "poet.models.poet", "poet.models.modules.packed_sequence", "poet.msa.sampling"):
            mods[name] = importlib.import_module(name)
        spec = importlib.util.spec_from_file_location("_ref_poet_score", os.path.join(POET_DIR, "scripts", "score.py"))
        mods["score"] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mods["score"])
    finally:
        sys.path.remove(POET_DIR)
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
        for k in [k for k in sys.modules if k == "poet" or k.startswith("poet.")]:
            sys.modules["_ref_" + k] = sys.modules.pop(k)
    _mods.update(mods)
    return _mods


def alphabet():
    return _load()["poet.alphabets"].Uniprot21(include_gap=True, include_startstop=True, distinct_startstop=True)


def score_module():
    return _load()["score"]


def sampling():
    return _load()["poet.msa.sampling"]


def build_model(init_args, sd, dtype=None):
    """The reference PoET in eval mode with ``sd`` (names without their leading component) loaded, on the CPU."""
    import torch
    model = _load()["poet.models.poet"].PoET(**init_args)
    model.load_state_dict({k: torch.as_tensor(np.asarray(v, dtype=np.float32)) for k, v in sd.items()}, strict=False)
    model = model.eval()
    return model.to(dtype) if dtype is not None else model


def tiered_forward(model, sequences):
    """log_softmax of PoET.forward over the sequence-of-sequences ``sequences`` (token arrays): [total, V].  The reference's layers
    are called unmodified, one after the other, on a PackedTensorSequences built paddable (indices from compute_indices, batch_size =
    the number of sequences), with the whole concatenation as ONE sequence-of-sequences."""
    import torch
    PTS = _load()["poet.models.modules.packed_sequence"].PackedTensorSequences
    sizes = torch.tensor([len(s) for s in sequences], dtype=torch.int32)
    xs = torch.cat([torch.from_numpy(np.asarray(s)).long() for s in sequences])
    cu = torch.nn.functional.pad(sizes.cumsum(dim=0, dtype=torch.int32), (1, 0))
    total = torch.tensor([0, int(sizes.sum())], dtype=torch.int32)
    with torch.no_grad():
        h = PTS(packed_tensor=model.token_embed(xs), positions=torch.cat([torch.arange(int(n)) for n in sizes]),
                indices=PTS.compute_indices(sizes), cu_seqlens=cu, cu_seqlens_cpu=cu, max_s=int(sizes.max()),
                batch_size=len(sequences), to_paddedable=True)
        for layer in model.decoder.layers:
            h, _, _ = layer.forward(h, seqs_cu_seqlens=total, seqs_cu_seqlens_cpu=total, return_memory=True)
            # the second attention re-labelled the packing as one sequence; the next layer's first attention needs the sequences back
            h.cu_seqlens, h.cu_seqlens_cpu, h.max_s = cu, cu, int(sizes.max())
            h.indices, h.batch_size = PTS.compute_indices(sizes), len(sequences)
        logits = model.linear(model.norm(h.x))
    return torch.log_softmax(logits, dim=-1).numpy()


def variant_logprobs(model, prompt, variant_tokens):
    """log p(. | prompt, variant[<= t]) [len, V]: what logits() computes with cached memory, read from the tiered forward of
    prompt + [variant_tokens] (the model is causal: the prompt's rows do not see the variant)."""
    lp = tiered_forward(model, list(prompt) + [np.asarray(variant_tokens)])
    return lp[-len(variant_tokens):]


def score(model, prompt, variant):
    lp = variant_logprobs(model, prompt, variant[:-1])
    tgt = np.asarray(variant[1:])
    keep = tgt != 23
    return float(lp[np.arange(len(tgt))[keep], tgt[keep]].astype(np.float64).sum())
