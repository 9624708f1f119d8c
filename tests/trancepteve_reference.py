"""TEST INFRASTRUCTURE ONLY -- loads the unmodified reference TranceptEVE package (proteingym/baselines/trancepteve) on the CPU, where
the reference tree exists: the pins of tests/test_trancepteve_host.py and tests/golden/make_golden_trancepteve.py.

Shims: those of oracle.ref_harness.load_reference_tranception (transformers names the reference imports, the Clustal Omega stand-in)
and tests/eve_reference.py's numba / Bio stubs; ``proteingym/baselines/trancepteve`` goes on sys.path only while the package is
imported, with the module isolation of tests/eve_reference.py for the top-level names ``utils`` and ``EVE``.
"""
import os
import sys
import types

import numpy as np

import eve_reference
from oracle.ref_harness import REF_ROOT, load_reference_tranception

TTE_DIR = os.path.join(REF_ROOT, "proteingym", "baselines", "trancepteve")
_loaded = None


def reference_available() -> bool:
    return os.path.isfile(os.path.join(TTE_DIR, "score_trancepteve.py"))


def load_reference():
    """(trancepteve package with model_pytorch, utils.msa_utils and EVE.VAE_model imported, tokenizer)."""
    global _loaded
    if _loaded is None:
        if not reference_available():
            raise RuntimeError(f"reference TranceptEVE code not found under {TTE_DIR}")
        _, tok = load_reference_tranception()
        eve_reference._stubs()
        for n in ("sklearn", "sklearn.model_selection"):
            if n not in sys.modules:
                try:
                    __import__(n)
                except ImportError:
                    sys.modules[n] = types.ModuleType(n)
                    sys.modules[n].train_test_split = None
        saved = {k: sys.modules.pop(k) for k in list(sys.modules) if eve_reference._ours(k)}
        sys.path.insert(0, TTE_DIR)
        try:
            import importlib
            pkg = importlib.import_module("trancepteve")
            importlib.import_module("trancepteve.model_pytorch")
            importlib.import_module("trancepteve.utils.msa_utils")
            importlib.import_module("trancepteve.EVE.VAE_model")
        finally:
            sys.path.remove(TTE_DIR)
            for k in [k for k in sys.modules if eve_reference._ours(k)]:
                sys.modules.pop(k)
            sys.modules.update(saved)
        _loaded = (pkg, tok)
    return _loaded


def build_vae(params, state, seq_len):
    """The reference's VAE_model (trancepteve/EVE) with ``state`` loaded, on the CPU, in eval() as get_EVE_log_prior_single puts it."""
    import copy
    import torch
    pkg, _ = load_reference()
    data = types.SimpleNamespace(seq_len=seq_len, alphabet_size=20, Neff=1.0)
    p = copy.deepcopy(params)
    model = pkg.EVE.VAE_model.VAE_model(model_name="toy", data=data, encoder_parameters=p["encoder_parameters"],
                                        decoder_parameters=p["decoder_parameters"], random_seed=42)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v, dtype=np.float32)) for k, v in state.items()})
    return model


class DrawRecorder:
    """Records every ``torch.randn_like`` draw while the reference runs, in order."""

    def __enter__(self):
        import torch
        self._randn, self.draws = torch.randn_like, []

        def randn_like(t, *a, **k):
            eps = self._randn(t, *a, **k)
            self.draws.append(eps.detach().numpy().copy())
            return eps
        torch.randn_like = randn_like
        return self

    def __exit__(self, *exc):
        import torch
        torch.randn_like = self._randn
        return False

    def per_sample(self, names):
        """The draws as one dict per sample, named in the order tests/eve_ref.py documents (without the dropout masks)."""
        assert len(self.draws) % len(names) == 0, (len(self.draws), len(names))
        return [dict(zip(names, self.draws[i:i + len(names)])) for i in range(0, len(self.draws), len(names))]


def log_prior_single(vae, focus_seq_trimmed, num_samples, full_len=None, MSA_start=0, focus_cols=None):
    """get_EVE_log_prior_single of the unmodified reference on one sequence; returns the [full_len, 25] float32 table."""
    pkg, _ = load_reference()
    L = len(focus_seq_trimmed)
    me = types.SimpleNamespace()
    msa = types.SimpleNamespace(focus_cols=list(range(L)) if focus_cols is None else list(focus_cols))
    full_len = L if full_len is None else full_len
    out = pkg.model_pytorch.TrancepteveLMHeadModel.get_EVE_log_prior_single(
        me, EVE_model=vae, sequences_to_score=[focus_seq_trimmed], full_sequence_len=full_len, MSA_start=MSA_start,
        MSA_end=MSA_start + L, EVE_MSA=msa, EVE_num_samples_log_proba=num_samples)
    return out.detach().numpy()
