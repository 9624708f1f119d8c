"""TEST INFRASTRUCTURE ONLY -- drives the unmodified reference ProGen3 code (proteingym/baselines/progen3) on the CPU in fp32 with
``moe_implementation="eager"``, where the reference tree exists (oracle.ref_harness.REF_ROOT): the pins of tests/test_progen3_host.py
and tests/golden/make_golden_progen3.py.

The reference imports packages that need not be installed; for the duration of the load only, and only for names that nothing real
provides, stand-ins are registered (what was registered under a name before is put back):
  megablocks.*                              empty modules with a placeholder dMoE / Arguments (the eager block never touches them)
  flash_attn.ops.triton.layer_norm          rms_norm_fn written out as x * rsqrt(mean(x^2) + eps) * w in fp32
  Bio                                       empty (scorer.py reads FASTA files with it; nobody here does)
  transformers.modeling_utils.GenerationMixin   aliased to transformers.generation.GenerationMixin where a newer transformers moved it
The reference's modules import each other as the package ``progen3``; they are loaded with its folder on sys.path and then moved to
private names, so nothing called ``progen3`` stays importable (the product's own module is proteingym_amd.progen3)."""
import importlib
import importlib.util
import os
import sys
import types

import numpy as np

from oracle.ref_harness import REF_ROOT

PG3_DIR = os.path.join(REF_ROOT, "proteingym", "baselines", "progen3")
_mods = {}


def reference_available() -> bool:
    return os.path.isfile(os.path.join(PG3_DIR, "progen3", "modeling.py"))


def _missing(name: str) -> bool:
    if name in sys.modules:
        return False
    try:
        return importlib.util.find_spec(name) is None
    except (ImportError, ValueError):
        return True


def _stand_ins():
    import torch
    out = {}
    if _missing("megablocks"):
        names = ["megablocks", "megablocks.layers", "megablocks.layers.moe", "megablocks.layers.dmoe", "megablocks.layers.arguments",
                 "megablocks.layers.common"]
        for n in names:
            out[n] = types.ModuleType(n)
        for n in names[1:]:
            setattr(out[n.rsplit(".", 1)[0]], n.rsplit(".", 1)[1], out[n])
        out["megablocks.layers.dmoe"].dMoE = type("dMoE", (torch.nn.Module,), {})
        out["megablocks.layers.arguments"].Arguments = type("Arguments", (), {"__init__": lambda self, **kw: self.__dict__.update(kw)})
        out["megablocks.layers.moe"].clear_load_balancing_loss = lambda: None
    if _missing("flash_attn"):
        names = ["flash_attn", "flash_attn.ops", "flash_attn.ops.triton", "flash_attn.ops.triton.layer_norm"]
        for n in names:
            out[n] = types.ModuleType(n)
        for n in names[1:]:
            setattr(out[n.rsplit(".", 1)[0]], n.rsplit(".", 1)[1], out[n])

        def rms_norm_fn(x, weight, bias, residual=None, eps=1e-6, dropout_p=0.0, prenorm=False, residual_in_fp32=False):
            assert bias is None and residual is None and dropout_p == 0.0 and not prenorm
            xf = x.float()
            return (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps) * weight.float()).to(x.dtype)
        out["flash_attn.ops.triton.layer_norm"].rms_norm_fn = rms_norm_fn
    if _missing("Bio"):
        out["Bio"] = types.ModuleType("Bio")
        out["Bio"].SeqIO = types.ModuleType("Bio.SeqIO")
        out["Bio.SeqIO"] = out["Bio"].SeqIO
    return out


def _load():
    if _mods:
        return _mods
    if not reference_available():
        raise RuntimeError(f"reference ProGen3 code not found under {PG3_DIR}")
    import transformers.modeling_utils as tmu
    added_mixin = not hasattr(tmu, "GenerationMixin")
    if added_mixin:
        from transformers.generation import GenerationMixin
        tmu.GenerationMixin = GenerationMixin
    stand = _stand_ins()
    saved = {k: sys.modules.get(k) for k in stand}
    sys.modules.update(stand)
    before = {k for k in sys.modules if k == "progen3" or k.startswith("progen3.")}
    sys.path.insert(0, PG3_DIR)
    try:
        mods = {n: importlib.import_module("progen3." + n) for n in ("config", "modeling", "scorer", "batch_preparer", "tokenizer")}
        mods["moe"] = importlib.import_module("progen3.model.moe")
        mods["attention"] = importlib.import_module("progen3.model.attention")
    finally:
        sys.path.remove(PG3_DIR)
        for k in [k for k in sys.modules if (k == "progen3" or k.startswith("progen3.")) and k not in before]:
            sys.modules["_ref_" + k] = sys.modules.pop(k)
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
        if added_mixin:
            del tmu.GenerationMixin
    _mods.update(mods)
    return _mods


def make_config(**kw):
    """A ProGen3Config for the CPU: eager experts, fp32, no cache."""
    base = dict(moe_implementation="eager", torch_dtype="float32", use_cache=False)
    base.update(kw)
    return _load()["config"].ProGen3Config(**base)


def build_model(config, seed: int):
    """ProGen3ForCausalLM(config) with seeded weights (the reference's own initialiser at config.initializer_range; the RMSNorm weights
    moved off 1 so that they take part)."""
    import torch
    torch.manual_seed(seed)
    model = _load()["modeling"].ProGen3ForCausalLM(config).float().eval()
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith("norm.weight") or name.endswith("layernorm.weight"):
                p.add_(torch.randn_like(p) * 0.1)
    return model


def encode(sequences, reverse: bool):
    """batch_preparer.get_batch_kwargs: the padded input_ids / labels / position_ids / sequence_ids tensors."""
    import torch
    return _load()["batch_preparer"].ProGen3BatchPreparer().get_batch_kwargs(list(sequences), device=torch.device("cpu"), reverse=reverse)


def score(model, sequences, max_batch_tokens: int = 65536):
    """ProGen3Scorer.evaluate -> (log_likelihood, perplexity) float arrays in the order of `sequences`."""
    out = _load()["scorer"].ProGen3Scorer(model, max_batch_tokens=max_batch_tokens).evaluate(list(sequences))
    return out["log_likelihood"].double().numpy(), out["perplexity"].double().numpy()


def forward_details(model, kwargs):
    """One forward of the padded batch `kwargs`: (log_softmax(logits) [B,T,V] fp32, per-layer router probabilities [layers][B*T, E]
    fp32 -- empty for one expert)."""
    import torch
    with torch.no_grad():
        out = model(input_ids=kwargs["input_ids"], sequence_ids=kwargs["sequence_ids"], position_ids=kwargs["position_ids"],
                    output_router_weights=model.config.num_experts > 1, return_dict=True)
    lp = torch.log_softmax(out.logits.float(), dim=-1).numpy()
    routers = [r.float().numpy() for r in (out.router_weights or ())] if model.config.num_experts > 1 else []
    return lp, routers


def to_megablocks(sd, config):
    """The eager state dict re-saved under the megablocks names: per layer experts.mlp.w1 / v1 [E F, D] (the experts' w1 / w3 stacked),
    experts.mlp.w2 [E F, D] (every expert's w2 transposed to [F, D], stacked) and router.layer.weight."""
    import torch
    E, gated = config.num_experts, config.gated_mlp
    out = {k: v for k, v in sd.items() if ".block_sparse_moe." not in k}
    for i in range(config.num_hidden_layers):
        p = f"model.layers.{i}.block_sparse_moe."
        out[p + "experts.mlp.w1"] = torch.cat([sd[p + f"experts.{e}.w1.weight"] for e in range(E)])
        if gated:
            out[p + "experts.mlp.v1"] = torch.cat([sd[p + f"experts.{e}.w3.weight"] for e in range(E)])
        out[p + "experts.mlp.w2"] = torch.cat([sd[p + f"experts.{e}.w2.weight"].T for e in range(E)]).contiguous()
        if E > 1:
            out[p + "router.layer.weight"] = sd[p + "gate.weight"]
    return out
