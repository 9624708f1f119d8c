"""TEST INFRASTRUCTURE ONLY -- drives the unmodified reference EVE code (proteingym/baselines/EVE) on the CPU, where the reference
tree exists (oracle.ref_harness.REF_ROOT): the restatement pin of tests/test_eve_host.py and tests/golden/make_golden_eve.py.

Shims: stub ``numba`` / ``numba_progress`` / ``Bio`` modules (utils/weights.py imports them at module level; the scoring path never
calls them), and the EVE directory on sys.path only while its ``EVE`` and ``utils`` packages are imported -- the reference tree has
another top-level ``utils`` (proteingym/utils) that oracle/ref_harness.py imports under the same name, so the module table is put
back afterwards and the EVE modules are reached through the objects returned here.
"""
import contextlib
import os
import sys
import types

import numpy as np

from oracle.ref_harness import REF_ROOT

EVE_DIR = os.path.join(REF_ROOT, "proteingym", "baselines", "EVE")
_loaded = None


def reference_available() -> bool:
    return os.path.isfile(os.path.join(EVE_DIR, "compute_evol_indices_DMS.py"))


def _stubs():
    if "numba" not in sys.modules:
        nb = types.ModuleType("numba")
        _dec = lambda *a, **k: a[0] if (len(a) == 1 and callable(a[0]) and not k) else (lambda f: f)
        nb.jit = nb.njit = _dec
        nb.prange = lambda n: range(int(n))
        sys.modules["numba"] = nb
    if "numba_progress" not in sys.modules:
        npg = types.ModuleType("numba_progress")
        npg.ProgressBar = contextlib.nullcontext
        sys.modules["numba_progress"] = npg
    for n in ["Bio", "Bio.SeqIO", "Bio.SeqRecord", "Bio.Seq"]:
        if n not in sys.modules:
            sys.modules[n] = types.ModuleType(n)


def _ours(name):
    return name in ("utils", "EVE") or name.startswith(("utils.", "EVE."))


@contextlib.contextmanager
def eve_imports():
    """sys.path / sys.modules as ``python compute_evol_indices_DMS.py`` run from the EVE directory sees them."""
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if _ours(k)}
    if _loaded is not None:
        sys.modules.update(_loaded[2])
    sys.path.insert(0, EVE_DIR)
    try:
        yield
    finally:
        sys.path.remove(EVE_DIR)
        mine = {k: sys.modules.pop(k) for k in list(sys.modules) if _ours(k)}
        if _loaded is not None:
            _loaded[2].update(mine)
        sys.modules.update(saved)


def load_reference():
    """(EVE.VAE_model module, utils.data_utils module) of the reference."""
    global _loaded
    if _loaded is None:
        if not reference_available():
            raise RuntimeError(f"reference EVE code not found under {EVE_DIR}")
        _stubs()
        _loaded = (None, None, {})
        with eve_imports():
            import importlib
            vm = importlib.import_module("EVE.VAE_model")
            du = importlib.import_module("utils.data_utils")
        _loaded = (vm, du, _loaded[2])
    return _loaded[0], _loaded[1]


def build_model(params, state, seq_len):
    """The reference VAE_model with ``state`` (name -> array) loaded, on the CPU, in the mode the scoring script leaves it in (train)."""
    import copy
    import torch
    vm, _ = load_reference()
    data = types.SimpleNamespace(seq_len=seq_len, alphabet_size=20, Neff=1.0)
    p = copy.deepcopy(params)
    model = vm.VAE_model(model_name="toy", data=data, encoder_parameters=p["encoder_parameters"],
                         decoder_parameters=p["decoder_parameters"], random_seed=42)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v, dtype=np.float32)) for k, v in state.items()})
    return model


class NoiseRecorder:
    """Wraps ``torch.randn_like`` and the decoder's dropout layer while a reference forward runs and names the draws in the order
    tests/eve_ref.py documents."""

    def __init__(self, model, names):
        self.model, self.names, self.noise = model, list(names), {}

    def _next(self, kind):
        name = self.names[len(self.noise)]
        assert name.startswith("keep") == (kind == "keep"), (name, kind)
        return name

    def __enter__(self):
        import torch
        self._randn = torch.randn_like
        self._drop = self.model.decoder.dropout_layer if self.model.decoder.dropout_proba > 0 else None
        rec = self

        def randn_like(t, *a, **k):
            eps = rec._randn(t, *a, **k)
            rec.noise[rec._next("eps")] = eps.detach().numpy().copy()
            return eps

        class Drop(torch.nn.Module):
            def forward(self, x):
                y = rec._drop(x)
                # a kept element is x / (1 - p); a kept zero cannot be told from a dropped one and does not need to be
                rec.noise[rec._next("keep")] = ((y != 0) | (x == 0)).numpy().astype(np.uint8)
                return y

        torch.randn_like = randn_like
        if self._drop is not None:
            self.model.decoder.dropout_layer = Drop()
        return self

    def __exit__(self, *exc):
        import torch
        torch.randn_like = self._randn
        if self._drop is not None:
            self.model.decoder.dropout_layer = self._drop
        return False
