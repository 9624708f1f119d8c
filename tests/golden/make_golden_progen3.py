"""Writes tests/golden/ProGen3_toy/ from the LIVE reference (proteingym/baselines/progen3, driven by tests/progen3_reference.py on the
CPU in fp32 with the eager expert block):

  A/, B/                   two seeded toy checkpoints in the eager layout (config.json + model.safetensors, or Hugging Face shards with
                           model.safetensors.index.json where one file would pass the repository's size limit; tensors stored as
                           float16: every value is then exactly what any loader reads):
                           A = hidden 128, ffn 192, gated, 2 layers, 2 heads on 1 K/V head, 4 experts top-2;
                           B = hidden 128, ffn 64, not gated, 2 layers, 2 heads on 2 K/V heads, 8 experts top-2
  A_megablocks/, B_megablocks/   the same weights re-saved under the megablocks names
  TOY_PG3_SUB.csv          mutant / DMS_score: substitutions of the target sequence (singles and multiples)
  TOY_PG3_INDEL.csv        mutant / mutated_sequence / DMS_score: sequences of unequal lengths
  TOY_PG3_REFERENCE.csv    the mapping file (row 0: substitutions, row 1: indels)
  scores_{A,B}_{sub,indel}.csv   the reference's scores (ProGen3Scorer.evaluate): mutant, log_likelihood, perplexity, DMS_score
  golden_progen3.npz       for the indel sequences: token ids of both directions (right-padded), and per config the final token
                           log-probs, the per-layer router probabilities and the chosen experts

initializer_range is 0.1, so routing is far from uniform.  The maker asserts that the k-th and the (k+1)-th router probability are at
least 1e-3 apart for every layer, token and direction of every fixture sequence, and tries seeds until they are: no test leaves a case
out.

    python tests/golden/make_golden_progen3.py [out_dir]
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]

COMMON = dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, num_experts_per_tok=2, initializer_range=0.1,
              max_num_sequences=4, max_position_embeddings=256, rope_theta=100000.0, rms_norm_eps=1e-5, hidden_act="silu", vocab_size=134)
CONFIGS = {"A": dict(COMMON, intermediate_size=192, gated_mlp=True, num_key_value_heads=1, num_experts=4),
           "B": dict(COMMON, intermediate_size=64, gated_mlp=False, num_key_value_heads=2, num_experts=8)}
GAP = 1e-3
AA = "ACDEFGHIKLMNPQRSTVWY"
TARGET = "MKTAYIAKQRQISFVKSHFSRQLE"


def toy_assays():
    rng = np.random.default_rng(5)
    muts = []
    for n in (1, 1, 1, 1, 1, 2, 2, 3):
        parts = []
        for p in sorted(rng.choice(len(TARGET), n, replace=False)):
            parts.append(f"{TARGET[p]}{p + 1}{rng.choice([a for a in AA if a != TARGET[p]])}")
        muts.append(":".join(parts))
    sub = [(m, float(np.round(rng.standard_normal(), 3))) for m in muts]
    seqs = [TARGET, TARGET[:9] + TARGET[12:], TARGET[:5] + "GW" + TARGET[5:], TARGET[3:], TARGET + "KLV", TARGET[:15] + "P" + TARGET[15:20]]
    indel = [(f"indel_{i}", s, float(np.round(rng.standard_normal(), 3))) for i, s in enumerate(seqs)]
    return sub, indel


def apply(mutant):
    s = list(TARGET)
    for m in mutant.split(":"):
        assert s[int(m[1:-1]) - 1] == m[0]
        s[int(m[1:-1]) - 1] = m[-1]
    return "".join(s)


def gaps_ok(pr, model, sequences, k):
    for rev in (False, True):
        kw = pr.encode(sequences, rev)
        _, routers = pr.forward_details(model, kw)
        real = (kw["input_ids"].numpy() != 0).reshape(-1)
        for r in routers:
            s = -np.sort(-r.astype(np.float64), axis=-1)
            if (s[real, k - 1] - s[real, k]).min() < GAP:
                return False
    return True


def save_sharded(state, d, max_bytes=900_000):
    """model.safetensors when it fits a committed file, else Hugging Face shards (model-0000i-of-0000n.safetensors and
    model.safetensors.index.json), as the larger published checkpoints are stored."""
    from safetensors.torch import save_file
    shards, size = [{}], 0
    for k, v in state.items():
        n = v.numel() * v.element_size()
        if shards[-1] and size + n > max_bytes:
            shards.append({})
            size = 0
        shards[-1][k] = v
        size += n
    for fn in os.listdir(d):
        if fn.endswith(".safetensors") or fn.endswith(".index.json"):
            os.remove(os.path.join(d, fn))
    if len(shards) == 1:
        save_file(shards[0], os.path.join(d, "model.safetensors"))
        return
    weight_map = {}
    for i, sh in enumerate(shards):
        fn = f"model-{i + 1:05d}-of-{len(shards):05d}.safetensors"
        save_file(sh, os.path.join(d, fn))
        weight_map.update({k: fn for k in sh})
    json.dump(dict(metadata={}, weight_map=weight_map), open(os.path.join(d, "model.safetensors.index.json"), "w"), indent=1)


def main(out_dir):
    import torch
    import progen3_reference as pr
    os.makedirs(out_dir, exist_ok=True)
    sub, indel = toy_assays()
    sub_seqs, indel_seqs = [apply(m) for m, _ in sub], [s for _, s, _ in indel]
    with open(os.path.join(out_dir, "TOY_PG3_SUB.csv"), "w") as f:
        f.write("mutant,DMS_score\n" + "".join(f"{m},{y}\n" for m, y in sub))
    with open(os.path.join(out_dir, "TOY_PG3_INDEL.csv"), "w") as f:
        f.write("mutant,mutated_sequence,DMS_score\n" + "".join(f"{m},{s},{y}\n" for m, s, y in indel))
    with open(os.path.join(out_dir, "TOY_PG3_REFERENCE.csv"), "w") as f:
        f.write("DMS_id,DMS_filename,target_seq\n" + f"TOY_PG3_SUB,TOY_PG3_SUB.csv,{TARGET}\n" + f"TOY_PG3_INDEL,TOY_PG3_INDEL.csv,{TARGET}\n")
    ids = {rev: pr.encode(indel_seqs, rev)["input_ids"].numpy().astype(np.int32) for rev in (False, True)}
    golden = dict(sequences=np.array(indel_seqs), ids_fwd=ids[False], ids_rev=ids[True])
    for name, kw in CONFIGS.items():
        config = pr.make_config(**kw)
        for seed in range(100):
            model = pr.build_model(config, 20250000 + seed)
            with torch.no_grad():
                for p in model.parameters():
                    p.copy_(p.half().float())                          # the stored values
            if gaps_ok(pr, model, sub_seqs + indel_seqs, config.num_experts_per_tok):
                break
        else:
            raise RuntimeError(f"config {name}: no seed keeps the router probabilities {GAP} apart")
        print(f"config {name}: seed {seed}")
        sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
        for suffix, state, impl in (("", sd, "eager"), ("_megablocks", pr.to_megablocks(sd, config), "megablocks")):
            d = os.path.join(out_dir, name + suffix)
            os.makedirs(d, exist_ok=True)
            save_sharded({k: v.half().contiguous() for k, v in state.items()}, d)
            json.dump(dict(kw, model_type="progen3", moe_implementation=impl, torch_dtype="float16"), open(os.path.join(d, "config.json"), "w"), indent=1)
        for tag, seqs, rows in (("sub", sub_seqs, [(m, y) for m, y in sub]), ("indel", indel_seqs, [(m, y) for m, _, y in indel])):
            ll, ppl = pr.score(model, seqs)
            with open(os.path.join(out_dir, f"scores_{name}_{tag}.csv"), "w") as f:
                f.write("mutant,log_likelihood,perplexity,DMS_score\n")
                f.write("".join(f"{m},{float(a)!r},{float(b)!r},{y}\n" for (m, y), a, b in zip(rows, ll, ppl)))
        for rev, tag in ((False, "fwd"), (True, "rev")):
            lp, routers = pr.forward_details(model, pr.encode(indel_seqs, rev))
            golden[f"{name}_logprobs_{tag}"] = lp.astype(np.float32)
            golden[f"{name}_router_{tag}"] = np.stack(routers).astype(np.float32)                      # [layers, B*T, E]
            golden[f"{name}_experts_{tag}"] = np.stack([np.argsort(-r.astype(np.float64), axis=-1, kind="stable")[:, :config.num_experts_per_tok]
                                                        for r in routers]).astype(np.int32)
    np.savez_compressed(os.path.join(out_dir, "golden_progen3.npz"), **golden)
    # the tokenizer's table as data, for the id-pinning test
    import shutil
    shutil.copyfile(os.path.join(pr.PG3_DIR, "progen3", "tokenizer.json"), os.path.join(out_dir, "tokenizer.json"))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "ProGen3_toy"))
