"""Secondary measurement: MULAN scoring throughput on a BLAT_ECOLX-shaped structure chunk (L = 286, T = 288), seeded weights at
MULAN-small's shape (6 layers, D = 320, 20 heads of 16; proteingym_amd.synthetic.mulan_config).  Two legs:

  singles  every single mutant of the assay's size (4 996): at most 286 position sets, one kept row each
  multi    about 5 000 distinct position sets of 2-4 positions (one multi-mutant each)

Per leg one JSON line: position-set forwards per second, mutants per second, the per-class HIP-event breakdown (the adapter's layer is
counted in the same classes as the six main layers).  The adapter's share of the call is taken against a yardstick: ESM2's
pgmi_masked_logprobs at the same B and T on the SAME main-stack weights, timed in interleaved rounds -- MULAN, yardstick, yardstick --
so that the share and the A/A spread of the yardstick come from one session.  --torch adds the comparison: batch-1 fp32 forwards per
second of the restatement assembled from the installed transformers' ESM modules (HF's own initialisation: it is timed, not compared)
on the same GPU, in a child process that ends before this one opens the device.

    python scripts/bench_mulan.py [--layers 6] [--rounds 3] [--precision f16x3] [--torch]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.getcwd())
from proteingym_amd import _lib, mulan, saprot, synthetic  # noqa: E402
from proteingym_amd import esm as pesm  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--layers", type=int, default=6)
ap.add_argument("--embed-dim", type=int, default=320)
ap.add_argument("--heads", type=int, default=20)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--multi-sets", type=int, default=5000)
ap.add_argument("--precision", default="f16x3", choices=sorted(_lib.PRECISIONS))
ap.add_argument("--torch", action="store_true", help="also time the fp32 torch restatement at batch 1")
ap.add_argument("--torch-only", action="store_true", help="(internal) run the torch baseline alone and print its JSON")
args = ap.parse_args()
AA = "ACDEFGHIKLMNPQRSTVWY"
L, N_SINGLES = 286, 4996
rng = np.random.default_rng(29)
seq = "".join(rng.choice(list(AA), L))
wt_ids = mulan.tokenize(seq, False)
T = wt_ids.size
rows = np.full((L, mulan.ROW_WIDTH), mulan.PAD_VALUE)
rows[:, 0] = rng.uniform(40.0, 99.0, L)                     # about a quarter of the residues under pLDDT 70
for i, a in enumerate(seq):
    rows[i, 4:6 + mulan.ROT_LEN[a]] = rng.uniform(-np.pi, np.pi, 2 + mulan.ROT_LEN[a])
angles, plddt = mulan.chunk_features(rows)

every = [f"{seq[p]}{p + 1}{a}" for p in range(L) for a in AA if a != seq[p]]
singles = [every[i] for i in sorted(rng.choice(len(every), N_SINGLES, replace=False))]
multi, seen = [], set()
while len(multi) < args.multi_sets:
    ps = tuple(sorted(int(p) for p in rng.choice(L, int(rng.integers(2, 5)), replace=False)))
    if ps not in seen:
        seen.add(ps)
        multi.append(":".join(f"{seq[p]}{p + 1}{rng.choice([a for a in AA if a != seq[p]])}" for p in ps))

cfg = synthetic.mulan_config(args.embed_dim, args.heads, args.layers)


def torch_leg():
    import torch
    from transformers import EsmConfig
    from transformers.models.esm import modeling_esm as M
    D = cfg["embed_dim"]
    main = EsmConfig(vocab_size=33, hidden_size=D, num_hidden_layers=cfg["layers"], num_attention_heads=cfg["heads"], intermediate_size=4 * D,
                     position_embedding_type="rotary", layer_norm_eps=1e-5, token_dropout=True, emb_layer_norm_before=False, pad_token_id=1,
                     mask_token_id=32, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    adapter = EsmConfig(hidden_size=D, num_hidden_layers=1, num_attention_heads=cfg["heads"], intermediate_size=4 * D, hidden_dropout_prob=0.0,
                        attention_probs_dropout_prob=0.0, layer_norm_eps=1e-5, emb_layer_norm_before=False, token_dropout=True,
                        esmfold_config=None, vocab_list=None)
    for c in (main, adapter):
        c._attn_implementation = "eager"
    dev = torch.device("cuda")
    torch.manual_seed(0)
    enc, ad_enc, head, rope = (m.to(dev).eval() for m in (M.EsmEncoder(main), M.EsmEncoder(adapter), M.EsmLMHead(main), M.EsmRotaryEmbedding(config=main)))
    E, mlp = torch.nn.Embedding(33, D).to(dev), torch.nn.Linear(7, D).to(dev)
    ids = torch.from_numpy(wt_ids.astype(np.int64)).to(dev)[None]
    raw, pl = torch.from_numpy(angles).to(dev), torch.from_numpy(plddt).to(dev)
    arange = torch.arange(T, device=dev)[None]

    def forward(p):
        with torch.no_grad():
            tok, st = ids.clone(), raw.clone()
            st[pl <= 70.0] = 4.0
            tok[0, p], st[p] = 32, -4.0
            emb = E(tok) + ad_enc(mlp(st)[None], attention_mask=None).last_hidden_state
            emb = emb.masked_fill((tok == 32).unsqueeze(-1), 0.0) * 0.88 / (1 - (tok == 32).sum(-1).float() / T)[:, None, None]
            hidden = enc(emb, attention_mask=None, position_embeddings=rope(emb, arange)).last_hidden_state
            return torch.log_softmax(head(hidden)[0, p], -1).cpu()
    for p in range(1, 21):
        forward(p)
    torch.cuda.synchronize()
    n, t0 = 200, time.perf_counter()
    for i in range(n):
        forward(1 + i % L)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(json.dumps(dict(leg="torch_fp32_batch1", layers=cfg["layers"], embed_dim=D, T=int(T), forwards=n, seconds=round(dt, 4),
                          forwards_per_s=round(n / dt, 1))), flush=True)


if args.torch_only:
    torch_leg()
    sys.exit(0)
if args.torch:                                              # a child process of its own, before this one opens the GPU: torch brings its own HIP runtime
    import subprocess
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--torch-only", "--layers", str(args.layers), "--embed-dim", str(args.embed_dim),
                            "--heads", str(args.heads)], capture_output=True, text=True)
    torch_line = child.stdout.strip().splitlines()[-1] if child.returncode == 0 and child.stdout.strip() else None
    if torch_line is None:
        raise SystemExit("the torch baseline failed:\n" + child.stderr[-2000:])

sd = synthetic.mulan_state_dict(cfg, seed=5)
model = mulan.from_state_dict(cfg, sd, precision=args.precision)
model.set_structure(angles, plddt)
# the yardstick: the same main stack as a plain ESM2 model
esm_cfg = dict(cfg, arch=_lib.ARCH_ESM2)
yard = pesm.EsmModel(esm_cfg, saprot.pack(esm_cfg, {k: v for k, v in sd.items() if not k.startswith(mulan.ADAPTER)}), precision=args.precision)


def run_yard(B):
    tokens = np.tile(wt_ids, (B, 1))
    mask = 1 + np.arange(B) % L
    t0 = time.perf_counter()
    yard.masked_logprobs(tokens, mask)
    return time.perf_counter() - t0


def profile_of(m):
    return {k: dict(ms=round(v["ms"], 2), calls=v["launches"]) for k, v in m.profile().items() if v["launches"]}


for leg, muts in (("singles", singles), ("multi", multi)):
    pos, wt, mt, off = mulan.parse_chunk(muts, seq, 1, L, False)
    set_off, set_pos, entry = saprot.position_sets(pos, off)
    n_sets = len(set_off) - 1

    def score():
        t0 = time.perf_counter()
        table = model.set_logprobs(wt_ids, set_off, set_pos)
        pesm.score_parsed(table, entry, wt, mt, off)
        return time.perf_counter() - t0
    score(), run_yard(n_sets)                                # warm-up: first launches, rotary tables, clocks
    rounds = [(score(), run_yard(n_sets), run_yard(n_sets)) for _ in range(args.rounds)]
    s, a, b = (float(np.median([r[i] for r in rounds])) for i in range(3))
    model.profile_reset(), model.profile_enable(True)
    score()
    model.profile_enable(False)
    prof = profile_of(model)
    yard.profile_reset(), yard.profile_enable(True)
    run_yard(n_sets)
    yard.profile_enable(False)
    print(json.dumps(dict(leg=leg, precision=args.precision, layers=cfg["layers"], embed_dim=cfg["embed_dim"], T=int(T), mutants=len(muts),
                          position_sets=n_sets, kept_rows=int(set_off[-1]), seconds=round(s, 4), sets_per_s=round(n_sets / s, 1),
                          mutants_per_s=round(len(muts) / s, 1), yardstick_seconds=[round(a, 4), round(b, 4)],
                          adapter_share=round(1.0 - 0.5 * (a + b) / s, 4), yardstick_aa_spread=round(abs(a - b) / (0.5 * (a + b)), 4),
                          rounds=[[round(x, 4) for x in r] for r in rounds], kernels_profiled=prof, yardstick_profiled=profile_of(yard))),
          flush=True)
model.close()
yard.close()
if args.torch:
    print(torch_line, flush=True)
