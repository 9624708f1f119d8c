"""TEST INFRASTRUCTURE ONLY -- drives the unmodified reference ProteinMPNN code (proteingym/baselines/protein_mpnn) on the CPU, where
the reference tree exists (oracle.ref_harness.REF_ROOT): the pins of tests/test_mpnn_host.py and tests/golden/make_golden_mpnn.py.
The two files import only torch and numpy; they are loaded by path under private module names, without touching sys.path for good."""
import importlib.util
import os
import sys

import numpy as np

from oracle.ref_harness import REF_ROOT

MPNN_DIR = os.path.join(REF_ROOT, "proteingym", "baselines", "protein_mpnn")
_mods = {}


def reference_available() -> bool:
    return os.path.isfile(os.path.join(MPNN_DIR, "protein_mpnn_utils.py"))


def _load(name):
    if name not in _mods:
        if not reference_available():
            raise RuntimeError(f"reference ProteinMPNN code not found under {MPNN_DIR}")
        spec = importlib.util.spec_from_file_location(f"_ref_mpnn_{name}", os.path.join(MPNN_DIR, name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        _mods[name] = mod
    return _mods[name]


def utils():
    """the reference's protein_mpnn_utils module"""
    return _load("protein_mpnn_utils")


def script():
    """the reference's compute_fitness module (its main() imports protein_mpnn_utils by name: see run_script)"""
    return _load("compute_fitness")


def build_model(sd, num_edges):
    """The reference ProteinMPNN in eval mode with ``sd`` (name -> array) loaded, on the CPU, as compute_fitness.py builds it."""
    import torch
    u = utils()
    model = u.ProteinMPNN(ca_only=False, num_letters=21, node_features=128, edge_features=128, hidden_dim=128, num_encoder_layers=3,
                          num_decoder_layers=3, augment_eps=0.0, k_neighbors=num_edges)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v, dtype=np.float32)) for k, v in sd.items()})
    return model.eval()


def forward(model, X, S, mask, chain_M, residue_idx, chain_encoding, randn, dtype=None):
    """log-probabilities [B, L, 21] of the reference forward; dtype torch.float64 runs the same module in double."""
    import torch
    dtype = dtype or torch.float32
    t = lambda a, d: torch.as_tensor(np.asarray(a), dtype=d)
    args = lambda: (t(X, dtype), t(S, torch.long), t(mask, dtype), t(chain_M, dtype), t(residue_idx, torch.long),
                    t(chain_encoding, torch.long), t(randn, dtype))
    if dtype == torch.float32:
        with torch.no_grad():
            return model(*args()).numpy()
    # the module in double: its weights converted, torch's default dtype switched (the forward's torch.zeros / torch.ones) and its
    # explicit .float() casts (one-hot matrices) widened for the duration of the call
    import copy
    model = copy.deepcopy(model).to(dtype)
    saved_default, saved_float = torch.get_default_dtype(), torch.Tensor.float
    torch.set_default_dtype(dtype)
    torch.Tensor.float = lambda self, *a, **k: self.to(dtype)
    try:
        with torch.no_grad():
            out = model(*args())
    finally:
        torch.Tensor.float = saved_float
        torch.set_default_dtype(saved_default)
    # a cast that the two switches above do not reach would narrow the result on the way: refuse that run
    if out.dtype != dtype:
        raise RuntimeError(f"the reference forward returned {out.dtype}, not {dtype}")
    return out.numpy()


def run_script(argv, record=None):
    """compute_fitness.py's own command line, in process.  ``record`` (a list) receives every torch.randn draw of the scoring loop."""
    import torch
    sc = script()
    sys.modules["protein_mpnn_utils"] = utils()
    real = torch.randn

    def randn(*a, **k):
        r = real(*a, **k)
        if record is not None:
            record.append(r.detach().cpu().numpy().copy())
        return r

    saved_argv = sys.argv
    torch.randn = randn
    try:
        sys.argv = ["compute_fitness.py"] + list(argv)
        ap = _script_parser(sc)
        sc.main(ap.parse_args())
    finally:
        torch.randn = real
        sys.argv = saved_argv
        sys.modules.pop("protein_mpnn_utils", None)


def _script_parser(sc):
    """The reference builds its parser under ``if __name__ == "__main__"`` only.  That block is taken from the file's syntax tree, not
    from its text: the statements before the first parse_args() call are compiled as they stand, so the layout of the file does not
    matter, and a block of another shape (no guard, no parser named argparser, other statements among them) is an error here."""
    import argparse
    import ast
    path = os.path.join(MPNN_DIR, "compute_fitness.py")
    tree = ast.parse(open(path).read(), path)
    guards = [n for n in tree.body if isinstance(n, ast.If) and isinstance(n.test, ast.Compare)
              and isinstance(n.test.left, ast.Name) and n.test.left.id == "__name__"]
    if len(guards) != 1:
        raise RuntimeError(f"{path}: expected one `if __name__ == ...` block, found {len(guards)}")
    body = []
    for stmt in guards[0].body:
        if any(isinstance(n, ast.Attribute) and n.attr == "parse_args" for n in ast.walk(stmt)):
            break
        body.append(stmt)
    build, adds = body[:1], body[1:]
    ok = (build and isinstance(build[0], ast.Assign) and [getattr(t, "id", None) for t in build[0].targets] == ["argparser"] and adds
          and all(isinstance(x, ast.Expr) and isinstance(x.value, ast.Call) and isinstance(x.value.func, ast.Attribute)
                  and x.value.func.attr == "add_argument" and getattr(x.value.func.value, "id", None) == "argparser" for x in adds))
    if not ok:
        raise RuntimeError(f"{path}: the block before parse_args() is not `argparser = ...` followed by argparser.add_argument calls")
    ns = {"argparse": argparse}
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
    return ns["argparser"]


def option_names():
    return sorted(a.option_strings[0] for a in _script_parser(script())._actions if a.option_strings and a.option_strings[0] != "-h")
