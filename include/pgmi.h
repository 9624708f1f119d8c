/*
 * pgmi.h -- C ABI of libpgmi.so, the MI355X (gfx950) masked-LM scorer behind ProteinGym's
 * ESM zero-shot path.
 *
 * The reference (OATML-Markslab/ProteinGym, /root/reference) has no FFI: a "baseline" plugs in
 * through (1) the per-baseline CLI + per-assay CSV and (2) the in-process seam
 *     model, alphabet = pretrained.load_model_and_alphabet(path)
 *                         (proteingym/baselines/esm/compute_fitness.py:349, esm/pretrained.py:24-28)
 *     model(tokens_int64[B,T])["logits"] -> f32 [B,T,33]
 *                         (compute_fitness.py:502; esm/model/esm1.py:116,177; esm/model/esm2.py:76,130)
 * Every entry point below names the reference code it replaces.  The Python host
 * (proteingym_amd/) binds these with ctypes; INTEGRATION.md shows the stub a ProteinGym
 * maintainer would add.
 *
 * Conventions: plain C types only; return 0 on success, negative PGMI_E* otherwise (never
 * throws); the caller owns every host buffer; the library owns device memory and one HIP
 * stream per model handle.  A handle is not thread-safe; distinct handles are independent.
 * pgmi_last_error() returns a thread-local message for the last failing call.
 */
#ifndef PGMI_H
#define PGMI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PGMI_ABI_VERSION 7

/* error codes */
#define PGMI_OK 0
#define PGMI_EINVAL (-1)   /* bad argument / unsupported shape */
#define PGMI_ENOMEM (-2)   /* device allocation failed */
#define PGMI_EHIP (-3)     /* HIP runtime error (message in pgmi_last_error) */
#define PGMI_ENODEV (-4)   /* no usable GPU */
#define PGMI_EPARSE (-5)   /* malformed mutant string / wild-type mismatch */
#define PGMI_EOVERFLOW (-6) /* 16-bit modes: an activation left the fp16/bf16 range (re-run in fp32) */

/* architectures: esm/model/esm1.py (arch "roberta_large": ESM-1b, ESM-1v) and esm/model/esm2.py */
#define PGMI_ARCH_ESM1B 1
#define PGMI_ARCH_ESM2 2
/* Tranception: GPT2-style causal LM with grouped ALiBi, depth-wise conv on q/k/v, squared ReLU
 * (proteingym/baselines/tranception/tranception/model_pytorch.py) */
#define PGMI_ARCH_TRANCEPTION 3
#define PGMI_ARCH_MSA 4          /* MSA Transformer (esm_msa1b): axial attention, esm/model/msa_transformer.py */
/* ProGen2: GPT-J-style causal LM, parallel residual, partial interleaved rotary, tanh-GELU
 * (proteingym/baselines/progen2/models/progen/modeling_progen.py); created with pgmi_pg2_model_create */
#define PGMI_ARCH_PROGEN2 5
/* Pre-LN causal decoder with a sequential residual: RITA (rotary) and ProtGPT2 = GPT-2 (learned positions); created with
 * pgmi_gpt_model_create */
#define PGMI_ARCH_GPT 6
#define PGMI_GPT_POS_ROTARY 0   /* RITA (proteingym/baselines/rita/rita_modeling.py): rotate-half rotary, untied lm_head */
#define PGMI_GPT_POS_LEARNED 1  /* GPT-2 (transformers GPT2LMHeadModel): wpe added to wte, lm_head tied to wte */
/* ESM C (ESM Cambrian, proteingym/baselines/evoscale/esm/models/esmc.py): pre-LN encoder with q/k LayerNorm, SwiGLU, scaled residual;
 * created with pgmi_model_create, scored with pgmi_token_logprobs / pgmi_masked_logprobs (see the ESM C section below) */
#define PGMI_ARCH_ESMC 7
/* SaProt (proteingym/baselines/saprot/compute_fitness.py, HF EsmForMaskedLM): ESM2 over a 446-token structure-aware vocabulary;
 * created with pgmi_saprot_model_create, scored with pgmi_saprot_* (see the SaProt section below) */
#define PGMI_ARCH_SAPROT 8
/* PoET (proteingym/baselines/PoET/poet/models/poet.py): tiered causal decoder over a sequence-of-sequences, scored against a cached
 * prompt; created with pgmi_poet_model_create, scored with pgmi_poet_* (see the PoET section below) */
#define PGMI_ARCH_POET 9
/* ProGen3 (proteingym/baselines/progen3/progen3/modeling.py): pre-RMSNorm causal decoder with grouped-query attention, rotate-half
 * rotary and a routed mixture-of-experts feed-forward block; created with pgmi_pg3_model_create, scored with pgmi_pg3_* (see the
 * ProGen3 section below) */
#define PGMI_ARCH_PROGEN3 10
/* ESM3 (proteingym/baselines/evoscale/esm/models/esm3.py): ESM C's blocks under a multi-track input embedding, block 0 with the
 * geometric attention branch over per-token backbone frames; created with pgmi_esm3_model_create, a window's structure bound with
 * pgmi_esm3_set_structure, scored with pgmi_token_logprobs / pgmi_masked_logprobs (see the ESM3 section below) */
#define PGMI_ARCH_ESM3 11
/* ESM-IF1 (proteingym/baselines/esm/esm/inverse_folding/gvp_transformer.py): the autoregressive decoder of the GVP-Transformer, every
 * layer cross-attending to one encoded backbone; created with pgmi_esmif1_model_create, the backbone's encoder output bound with
 * pgmi_esmif1_set_memory, scored with pgmi_esmif1_* (see the ESM-IF1 section below) */
#define PGMI_ARCH_ESMIF1 12
/* MULAN (proteingym/baselines/mulan/mulan/model.py): ESM2's or SaProt's encoder with a structure adapter over per-residue angle rows
 * added to the word embeddings; created with pgmi_mulan_model_create, a chunk's angles bound with pgmi_mulan_set_structure, scored
 * with pgmi_mulan_* (see the MULAN section below) */
#define PGMI_ARCH_MULAN 13

/* GEMM operand precision.  Residual stream, LayerNorm statistics, softmax and every
 * accumulator are fp32 in all modes. */
#define PGMI_PREC_FP32 0  /* v_mfma_f32_32x32x2_f32: exact fp32 products (parity-gated mode) */
#define PGMI_PREC_BF16 1  /* bf16 operands, fp32 accumulate (throughput mode; error is measured, not assumed) */
#define PGMI_PREC_F16X3 2 /* split-fp16 3-pass error-compensated GEMM (fp32-class accuracy on the f16 MFMA pipe) */

/* token ids of the 33-symbol ESM alphabet (esm/data.py:151-157, esm/constants.py:8) */
#define PGMI_TOK_CLS 0
#define PGMI_TOK_PAD 1
#define PGMI_TOK_EOS 2
#define PGMI_TOK_UNK 3
#define PGMI_TOK_MASK 32
#define PGMI_VOCAB 33
#define PGMI_PG2_VOCAB 32  /* ProGen2 (progen2/tokenizer.json) */
#define PGMI_ESMC_VOCAB 64 /* ESM C: the ESM token ids above, 64 logits columns (33..63 untrained, inside the log-softmax) */
#define PGMI_SAPROT_VOCAB 446 /* SaProt: 5 specials + 21 amino-acid letters x 21 structure letters */
#define PGMI_SAPROT_GROUPS 21 /* amino-acid letters ACDEFGHIKLMNPQRSTVWY# = columns of the group table */

typedef struct pgmi_config {
    int32_t abi_version;          /* = PGMI_ABI_VERSION */
    int32_t arch;                 /* PGMI_ARCH_* */
    int32_t layers;               /* encoder_layers */
    int32_t embed_dim;            /* D  (encoder_embed_dim) */
    int32_t heads;                /* H  (encoder_attention_heads); head_dim D/H: 64, an even value below 64 (ESM2 8M/35M/150M: 16/24/32), or 128 (ESM2-15B) */
    int32_t ffn_dim;              /* F  (encoder_ffn_embed_dim; 4*D for ESM2, esm2.py:52) */
    int32_t vocab;                /* = 33 (other families: their section below) */
    int32_t max_positions;        /* ESM-1b learned positions (table has max_positions+2 rows, modules.py:246-251); 0 for ESM2 */
    int32_t token_dropout;        /* esm1.py:125-131 / esm2.py:85-91 */
    int32_t emb_layer_norm_before;/* pretrained.py:80-82,98 */
    int32_t precision;            /* PGMI_PREC_* */
    int32_t max_rows;             /* workspace rows (B*T per internal chunk); 0 = default */
    float ln_eps;                 /* LayerNorm epsilon; 0 = 1e-5 (ESM: modules.py:80-81; Tranception: config.layer_norm_epsilon) */
} pgmi_config;

typedef struct pgmi_model pgmi_model;
typedef struct pgmi_assay pgmi_assay;
typedef struct pgmi_pppl pgmi_pppl;

/* ---- library ---------------------------------------------------------------------------- */
int pgmi_abi_version(void);
int pgmi_device_count(void);
const char* pgmi_last_error(void);

/* Number of fp32 elements of the flat weight blob for cfg, in this order (all row-major,
 * nn.Linear layout y = x W^T + b, esm/modules.py; names as in SURVEY.md Appendix A):
 *   embed_tokens[V,D]; (ESM1B) embed_positions[max_positions+2,D];
 *   (emb_layer_norm_before) w[D],b[D];
 *   per layer: self_attn_layer_norm w,b; q_proj W[D,D],b; k_proj W,b; v_proj W,b; out_proj W,b;
 *              final_layer_norm w,b; fc1 W[F,D],b[F]; fc2 W[D,F],b[D];
 *   emb_layer_norm_after w,b; lm_head.dense W[D,D],b; lm_head.layer_norm w,b; lm_head.bias[V].
 * (lm_head.weight is tied to embed_tokens, esm1.py:101-105.)  Returns <0 on a bad cfg. */
int64_t pgmi_weight_count(const pgmi_config* cfg);

/* Replaces pretrained.load_model_and_alphabet + model.cuda() (compute_fitness.py:349-353):
 * uploads the blob to `device`, packs it for the selected precision, allocates workspace.
 * embed_tokens must be the value load_state_dict leaves in the tied embed_tokens/lm_head.weight
 * parameter, i.e. after the host applied pretrained.py:97 (<mask> row zeroing for v1 files). */
int pgmi_model_create(const pgmi_config* cfg, const float* weights, int64_t n_weights,
                      int device, pgmi_model** out);
void pgmi_model_destroy(pgmi_model* m);
int pgmi_model_device(const pgmi_model* m);

/* ---- forward ---------------------------------------------------------------------------- */
/* Replaces `torch.log_softmax(model(tokens)["logits"], -1)` (compute_fitness.py:476,502):
 * tokens int32 [B,T] row-major (host), out f32 [B,T,V] (host).  <pad> tokens are honoured as
 * the reference does (embedding rows zeroed, keys masked).  Chunked internally. */
int pgmi_token_logprobs(pgmi_model* m, const int32_t* tokens, int B, int T, float* out);

/* The masked-marginals inner loop (compute_fitness.py:489-503) for B ready-made rows:
 * row b is forwarded with tokens[b, mask_pos[b]] replaced by <mask>; out[b,:] =
 * log_softmax(logits[b, mask_pos[b], :]).  tokens/mask_pos host int32, out host f32 [B,V]. */
int pgmi_masked_logprobs(pgmi_model* m, const int32_t* tokens, const int32_t* mask_pos,
                         int B, int T, float* out);

/* ---- per-assay pipeline, inputs resident in HBM --------------------------------------------
 * pgmi_assay_create uploads everything one DMS assay needs:
 *   wt_tokens  int32 [n_tok]   cls + residues + eos   (BatchConverter, esm/data.py:262-297)
 *   positions  int32 [P]       token positions to mask (any subset of [0,n_tok); the reference
 *                              runs all n_tok, compute_fitness.py:489 -- rows no mutant reads
 *                              may be skipped without changing any output)
 *   window                     model window (1024): for n_tok > window each position gets
 *                              get_optimal_window(i, n_tok, window) (utils/scoring_utils.py:43-52,
 *                              compute_fitness.py:492-495)
 *   sub_pos/sub_wt/sub_mt int32 [n_sub], mut_off int64 [n_mut+1]
 *                              flattened substitutions of every mutant: token position (1+idx),
 *                              wild-type and mutant token ids (label_row, compute_fitness.py:240-250)
 * pgmi_assay_run then executes the whole hot path on the device: masked windows -> forward ->
 * head on masked rows -> log-softmax table [n_tok,V] (NaN rows where not computed) ->
 * per-mutant score = sum_subs (f32(lp[mt]-lp[wt])) accumulated in double.
 * scores_host / table_host may be NULL; scores_dev (device pointer, double[n_mut]) may be NULL. */
int pgmi_assay_create(pgmi_model* m, const int32_t* wt_tokens, int n_tok,
                      const int32_t* positions, int P, int window,
                      const int32_t* sub_pos, const int32_t* sub_wt, const int32_t* sub_mt,
                      const int64_t* mut_off, int64_t n_mut, pgmi_assay** out);
int pgmi_assay_run(pgmi_model* m, pgmi_assay* a, double* scores_host, float* table_host,
                   double* scores_dev);
void pgmi_assay_destroy(pgmi_assay* a);

/* ---- pseudo-perplexity over variable-length sequences, library resident in HBM (BASELINE config 5) ----
 * Replaces the `--scoring-strategy pseudo-ppl` driver (compute_fitness.py:515-529: one compute_pppl call per
 * row of the `mutated_sequence` column) and compute_pppl itself (:258-279).
 * pgmi_pppl_create uploads a whole library ONCE:
 *   tokens   uint8 [seq_off[n_seq]]  every sequence as BatchConverter writes it: <cls> + residues + <eos>
 *                                    (esm/data.py:286-295), concatenated; no <pad>
 *   seq_off  int64 [n_seq+1]         seq_off[0] = 0
 * pgmi_pppl_run scores the sequences [first, first+count) (a shard of the library: ranks take disjoint
 * ranges).  For a sequence of L residues the reference loops i in range(1, L-1), masks TOKEN i and reads
 * log p(sequence[i]) = log-prob of token i+1's identity at position i (its off-by-one; residues 0 and L-1
 * are never scored, residue L-2's identity is scored at residue L-3's position, L <= 2 gives 0.0): all of it
 * is reproduced.  The (sequence, i) rows are enumerated on the device from the resident tokens; sequences of
 * DIFFERENT lengths share a batch: the run is ordered by length, a batch's T is its longest member, shorter
 * members are <pad>-filled and masked per sequence (key mask, position count and token-dropout ratio over the
 * non-pad tokens, exactly what the reference computes for a sequence alone).  No windowing, like the
 * reference: ESM-1b/1v fail above max_positions tokens ("Sequence length ... above maximum sequence length").
 *   scores_host double [count]  sum(log_probs): left-to-right double sum of the f32 terms (python's sum)
 *   terms_host  float  [pgmi_pppl_rows(first,count)]  optional: the terms, sequence by sequence in library order
 *   scores_dev  device double [count], optional
 * pgmi_pppl_rows: number of masked forwards (rows) the range needs.  pgmi_pppl_stats: rows, batches, real and
 * padded token counts of the last run (packing efficiency = tokens / padded_tokens). */
int pgmi_pppl_create(pgmi_model* m, const uint8_t* tokens, const int64_t* seq_off, int64_t n_seq, pgmi_pppl** out);
int pgmi_pppl_run(pgmi_model* m, pgmi_pppl* lib, int64_t first, int64_t count, double* scores_host,
                  float* terms_host, double* scores_dev);
int64_t pgmi_pppl_rows(const pgmi_pppl* lib, int64_t first, int64_t count);
int pgmi_pppl_stats(const pgmi_pppl* lib, int64_t* rows, int64_t* batches, int64_t* tokens, int64_t* padded_tokens);
void pgmi_pppl_destroy(pgmi_pppl* lib);

/* ---- host-side mutant parsing (label_row's string handling, compute_fitness.py:240-250) -----
 * text: n_mut NUL-free mutant strings ("A25G:L30P") concatenated, str_off int64 [n_mut+1].
 * sequence: wild type (len seq_len); offset_idx as --offset-idx.  Two-pass: call with
 * sub_* == NULL to get the substitution count in *n_sub, then with buffers of that size.
 * Fails with PGMI_EPARSE on a wild-type mismatch ("The listed wildtype does not match the
 * provided sequence") or a malformed token.  Letters map through the ESM alphabet
 * (unknown -> <unk>, esm/data.py:125-128). */
int pgmi_parse_mutants(const char* text, const int64_t* str_off, int64_t n_mut,
                       const char* sequence, int seq_len, int offset_idx,
                       int32_t* sub_pos, int32_t* sub_wt, int32_t* sub_mt,
                       int64_t* mut_off, int64_t* n_sub);

/* ---- host-side scoring from a log-prob table (label_row's arithmetic, compute_fitness.py:240-250) -----
 * table: float32 [n_rows][vocab] log-probabilities (row = token position, <cls> = 0), e.g. a table merged from position shards
 * or returned by pgmi_assay_run; sub_* / mut_off as pgmi_parse_mutants returns them.  scores[i] = sum over the substitutions of
 * mutant i, in the order of its string, of the float32 difference table[pos][mt] - table[pos][wt], accumulated in double -- the
 * reference's `.item()` sum and the device's score_mutants_kernel, bit for bit.  Host code, no GPU needed; rows that were never
 * computed (NaN) give NaN scores.  PGMI_EINVAL on a position or token outside the table. */
int pgmi_score_mutants(const float* table, int n_rows, int vocab, const int32_t* sub_pos, const int32_t* sub_wt,
                       const int32_t* sub_mt, const int64_t* mut_off, int64_t n_mut, double* scores);

/* get_optimal_window (proteingym/utils/scoring_utils.py:43-52) */
void pgmi_optimal_window(int position, int seq_len_with_special, int model_window,
                         int* start, int* end);

/* ---- profiling (HIP events on the model's stream) ----------------------------------------- */
#define PGMI_K_EMBED 0
#define PGMI_K_LAYERNORM 1
#define PGMI_K_GEMM_QKV 2
#define PGMI_K_ATTENTION 3
#define PGMI_K_GEMM_OUT 4
#define PGMI_K_GEMM_FC1 5
#define PGMI_K_GEMM_FC2 6
#define PGMI_K_HEAD 7
#define PGMI_K_SCORE 8
#define PGMI_K_KEPT_ROWS 9   /* last layer after attention, on the kept (masked) rows only: gathers + out-projection + LN + FFN */
#define PGMI_K_MOE_ROUTE 10  /* ProGen3: permutation, gather and weighted combine around the expert GEMMs (the router rides in PGMI_K_LAYERNORM) */
#define PGMI_K_GEOM 11       /* ESM3: block 0's geometric attention kernel (its LayerNorm and two GEMMs ride in their own classes) */
#define PGMI_K_CROSS_ATTENTION 12 /* ESM-IF1: the cross-attention over the encoder memory (its q prep and kernel; in set_memory the plane prep) */
#define PGMI_K_COUNT 13
/* on != 0: every launch of the classes above is bracketed by hipEventRecord on the stream. */
int pgmi_profile_enable(pgmi_model* m, int on);
/* Sum of event-measured milliseconds, launch count and algorithmic FLOPs / bytes for a class
 * since the last reset. */
int pgmi_profile_get(pgmi_model* m, int kernel_class, double* ms, int64_t* launches,
                     double* flops, double* bytes);
int pgmi_profile_reset(pgmi_model* m);
int pgmi_synchronize(pgmi_model* m);

/* Test hooks of the GEMM launchers (bit-neutral: they only change how a launch is cut into work items / row chunks):
 * "gemm_half_tail" (0: no half-height tail items; default 1), "gemm_max_rows" (> 0: cut every launch into row chunks of at most
 * that many rows), "att_xcd_local" (1: the dense attention launches walk their blocks in the XCD-local order; 0: the (query block,
 * head, sequence) grid; -1, default: by shape -- same bits, for interleaved timing), "att_v3" (dense head_dim-64 attention: -1, default:
 * the software-pipelined kernel from seven query tiles per sequence on; 0: the round-3 kernel everywhere; 1: the pipelined kernel
 * wherever it is defined -- same bits).  The library reads PGMI_GEMM_HALF_TAIL / PGMI_GEMM_MAX_ROWS when a model is created (and at the
 * model-less pgmi_op_* / pgmi_bench_* entries) for the options nobody has set through this call: an explicit value stays in force until
 * -1 hands "gemm_half_tail" / "gemm_max_rows" back to the environment.  Process-wide; returns PGMI_EINVAL for another name. */
int pgmi_set_option(const char* name, int64_t value);

/* ---- single ops (numerics tests compare each against the torch op it replaces) -------------
 * All pointers are host; each call uploads, runs the production kernel, downloads. */
int pgmi_op_layernorm(int device, const float* x, const float* w, const float* b,
                      int rows, int D, float eps, float* y);               /* modules.py:80-81 */
int pgmi_op_gemm(int device, int precision, const float* A, const float* W, const float* bias,
                 const float* residual, int M, int N, int K, int epilogue /*0 none,1 gelu,2 squared relu,3 tanh-gelu,4 SwiGLU,5 relu (f16x3 only);
                 +256 (f16x3): the split-fp16-plane output epilogue, its planes returned rebuilt as fp32*/,
                 float* C);          /* C = epi(A W^T + bias) + residual; modules.py:134-140.
                                      * SwiGLU (4 + 256 only, f16x3, N % 64 == 0): W and bias in blocks of 64 rows = 32 gate rows then
                                      * 32 up rows; C [M, N/2] with C[:, 32 b + i] = silu(gate row 64 b + i) * (up row 64 b + 32 + i) */
/* ESM C's QK-LayerNorm prep pass on qkv [B*T, 3D] (D = 64 H <= 2048): qk [B*T, 2D] = the attention's q | k operands rebuilt as fp32:
 * LayerNorm(q) * q_w (no bias, eps 1e-5) rotated by rotate-half rotary (head_dim 64) and times log2(e), then the same for k without
 * the factor; v [B*T, D] = the v operand.  Either output may be NULL.  iters > 0: *ms = mean time of that many further launches. */
int pgmi_op_qkln_prep(int device, const float* qkv, const float* q_w, const float* k_w, int B, int T, int H, int iters, float* qk,
                      float* v, double* ms);
int pgmi_op_attention(int device, int precision, const float* qkv, const int32_t* kv_len,
                      int B, int T, int H, int rotary, float* ctx);
                                     /* multihead_attention.py:354-395; qkv [B*T,3*H*64], q pre-scaled */
/* The causal attention of one decoder layer in SLOT SPACE, through the launchers the decoders use.  heads of `lanes` (64 / 128 / 256) lanes,
 * Da = heads * lanes, every head lanes / 64 slot groups of 64; slopes [heads] (ALiBi, zeros for none) selects the causal kernels.
 * Fused form (RITA, ProtGPT2, ProGen2): X [B*T, K] (K % 32 == 0), W [3 Da, K] (rows q | k | v), bias [3 Da]; qkv = conv = NULL.  The fused
 *   QKV projection forms X W^T + bias and rotates the pair (i, i + 32) of every slot group g of a q / k head at position t (restarting
 *   per sequence) by rot_cos / rot_sin [T][lanes / 64][64] at [t][g][i] (both NULL: no rotary; entries i and i + 32 hold the same angle).
 * Conv form (Tranception; lanes 64, heads % 4 == 0): qkv fp32 [B*T, 3 Da] and conv [3][4][64][8] -- per (q | k | v, head group
 *   h / (heads / 4), lane) 7 right-aligned causal taps, tap j on token t - 6 + j (zero before the sequence), entry 7 the bias; X, W, bias,
 *   rot_cos, rot_sin = NULL.
 * q is taken as given (pre-scaled).  ctx [B*T, Da]: the split-plane context the out-projection consumes, rebuilt as fp32.  What a launcher
 * refuses is PGMI_EINVAL with its message. */
int pgmi_op_causal_attention(int device, int lanes, const float* X, const float* W, const float* bias, int K, const float* qkv,
                             const float* conv, const float* rot_cos, const float* rot_sin, const float* slopes, int B, int T,
                             int heads, float* ctx);
/* The dense (bidirectional) attention of one encoder layer in SLOT SPACE, through the launchers and the argument pattern of run_encoder.
 * heads of `lanes` (64, or 128: ESM2-15B) lanes, Da = heads * lanes, every head lanes / 64 slot groups of 64.  X [B*T, K] (K % 32 == 0),
 * W [3 Da, K] (rows q | k | v), bias [3 Da]: the fused QKV projection forms X W^T + bias, multiplies q by log2(e) and rotates the pair
 * (i, i + 32) of every slot group g of a q / k head at position t (restarting per sequence) by rot_cos / rot_sin [T][lanes / 64][64] at
 * [t][g][i] (both NULL: no rotary; entries i and i + 32 hold the same angle).  The projection is f16x3 whatever `out` is: the bf16-operand
 * GEMM that the bf16 mode runs in front of this epilogue is not reached from here.  kv_len int32 [B] (NULL: T everywhere): sequence b's
 * queries see its keys 0 .. kv_len[b] - 1.  q is taken as given (pre-scaled).  The V^T planes are zeroed before the projection (pad keys
 * must be finite); the q | k planes and the context start as 0xFF bytes (NaN).  Honours the "att_v3" and "att_xcd_local" options.
 * ctx [B*T, Da]: the context rebuilt as fp32 -- out 0: the kernel's fp32 rows; 1: the split planes the f16x3 out-projection consumes
 * (hi + lo 2^-11); 2: the bf16 plane of the bf16 mode (bits << 16).  qk (nullable) [B*T, 2 Da]: the q | k operand planes rebuilt as fp32,
 * q with its log2(e) factor; v (nullable) [B*T, Da]: the v operand read back out of the transposed, key-permuted V^T planes.
 * PGMI_EINVAL, before the device is touched: a NULL X / W / bias / ctx, K % 32 != 0, lanes other than 64 / 128, only one of rot_cos /
 * rot_sin, a kv_len[b] outside [1, T].  What a launcher refuses (out outside 0 .. 2) is PGMI_EINVAL with its message. */
int pgmi_op_dense_attention(int device, int lanes, const float* X, const float* W, const float* bias, int K, const float* rot_cos,
                            const float* rot_sin, const int32_t* kv_len, int B, int T, int heads, int out, float* ctx, float* qk, float* v);
/* The MSA Transformer's two axial attentions (axial_attention.py:108-168, :232-275), through the launchers and the argument pattern of the
 * model's forward.  Heads of 64 lanes, D = 64 H; q is taken as given (pre-scaled by 1/8).
 * pgmi_op_tied_row_attention: qkv [R*C, 3 D] (q | k | v), token order (r, c).  s[h,i,j] = sum_{r,d} q[r,i,h,d] k[r,j,h,d] / sqrt(R) is ONE
 *   score matrix per head, P = softmax_j, ctx[r,i,h,:] = sum_j P[h,i,j] v[r,j,h,:].  splits: the K splits S of the scores GEMM (0: the
 *   forward's rule, pgmi_op_tied_row_splits; else S must divide R, 1 .. 16).  ctx [R*C, D]: the split-plane context the out-projection
 *   consumes, rebuilt as fp32; probs (nullable) [H, C, Kp], Kp = C rounded up to 64: the P planes of the update GEMM rebuilt as fp32,
 *   padding columns included (exact zeros).  The q planes and the context planes are one buffer, as in the forward; the partial scores,
 *   P, V^T and that buffer start as 0xFF bytes (NaN): a score, probability or V^T element the kernels neither write nor ignore shows as
 *   NaN.  (Not so a context row: the q operand overwrites the shared buffer first, so an unwritten context row holds finite q values
 *   and only the comparison of values finds it.)  PGMI_EINVAL with the launcher's message, before anything is allocated, for a bad
 *   `splits`, C > 1024 and operands beyond the 32-bit offset range.
 * pgmi_op_tied_row_splits: a test-only entry beside the two ops, so that a test reads the S the forward's rule picks for (R, C, H)
 *   instead of trusting its own copy of the rule.  Host only.  Returns S (1 .. 16), or PGMI_EINVAL (negative) for a non-positive argument.
 * pgmi_op_column_attention: X [C*R, K] (K % 32 == 0), token order (c, r), W [3 D, K] (rows q | k | v), bias [3 D]: the fused QKV
 *   projection (no rotary) forms X W^T + bias, then every column is one sequence of R rows of the dense attention (B = C, T = R, kv_len = R,
 *   pad keys zeroed); honours the "att_v3" option.  ctx [C*R, D], order (c, r): the split-plane context (0xFF bytes before the launch)
 *   rebuilt as fp32. */
/* PoET's segment-causal attention over a shared prefix (attention_prefix.hip) in SLOT SPACE, through the prep pass and the launcher the
 * model uses; heads of 64 lanes, Da = 64 heads, no rotary, q taken as given (pre-scaled).  qkv fp32 [seg_off[n_seg]][3 Da]: the packed
 * rows of n_seg segments (segment b = rows seg_off[b] .. seg_off[b+1]-1, every segment non-empty); prefix_kv fp32 [P][2 Da] (k | v; NULL
 * when P = 0).  A query at position t of its segment sees the P prefix keys and the keys 0 .. t of its segment.  ctx [rows][Da]:
 * split != 0: the split-plane context the out-projection consumes, rebuilt as fp32; 0: the kernel's fp32 rows. */
int pgmi_op_prefix_attention(int device, const float* qkv, const int32_t* seg_off, int n_seg, const float* prefix_kv, int P, int heads,
                             int split, float* ctx);
/* ESM-IF1's cross-attention (attention_prefix.hip, the prefix-only instantiation) in SLOT SPACE, through the prep passes and the launcher
 * the model uses; heads of 64 lanes, Da = 64 heads, q taken as given (pre-scaled).  q fp32 [seg_off[n_seg]][Da]: the packed query rows
 * of n_seg non-empty segments; mem_kv fp32 [S][2 Da] (k | v), S >= 1.  Every query row sees the S memory keys, unmasked, and nothing
 * else; the memory planes are written once by the prep pass over one segment of S rows (as pgmi_esmif1_set_memory fills a layer's
 * planes) and start as 0xFF bytes (NaN), as does the context.  ctx [rows][Da]: split != 0: the split-plane context the out-projection
 * consumes, rebuilt as fp32; 0: the kernel's fp32 rows.  S <= 0, an empty segment or a NULL pointer is PGMI_EINVAL. */
int pgmi_op_cross_attention(int device, const float* q, const int32_t* seg_off, int n_seg, const float* mem_kv, int S, int heads,
                            int split, float* ctx);
/* A test-only entry beside them, host only: how the PoET / ESM-IF1 entries cut a call of B sequences of lens[b] tokens into packed
 * chunks for a workspace of max_rows rows, so that a test reads the rule the entries run.  drop_last != 0: the model reads
 * lens[b] - 1 tokens (a log-likelihood); same_length != 0: a chunk is a run of sequences of one length (ESM-IF1).  A chunk takes
 * sequences while its packed rows stay within max_rows and its key rows, every sequence padded to a multiple of 32, within
 * max_rows rounded down to a multiple of 32.  out_b1 [B]: the end b1 of each successive chunk [b0, b1); *out_n: their number.
 * PGMI_EINVAL with the entries' own message at the first sequence that fits no chunk alone; a length below 1 (2 with drop_last), a
 * NULL pointer or a non-positive size is PGMI_EINVAL too. */
int pgmi_op_packed_chunks(const int32_t* lens, int B, int drop_last, int same_length, int max_rows, int32_t* out_b1, int32_t* out_n);
/* ProGen3's pieces (elementwise.hip rmsnorm16_kernel, moe.hip, api_progen3.hip moe_ffn) on their own buffers.
 * pgmi_op_rmsnorm: y [rows][D] = the split operand launch_rmsnorm16 writes, rebuilt as fp32 (hi + lo 2^-11); D % 32 == 0, D <= 5120.
 * pgmi_op_moe: the routed block on fp32 rows h [M][D] taken as they are (no norm): gate [E][D] (ignored when E == 1); w1 [E][F][D],
 *   w3 [E][F][D] (gated != 0, else ignored), w2 [E][D][F].  out [M][D] = sum_k weight_k * expert_k(h) (fp32); ids int32 [M][top_k] and
 *   weights f32 [M][top_k] (nullable; E == 1: not written).  The experts run through the model's own path: router, permutation,
 *   gather, one launch_gemm16 pair per non-empty expert, combine. */
int pgmi_op_rmsnorm(int device, const float* x, const float* w, int rows, int D, float eps, float* y);
/* ESM3's geometric attention (geom_attention.hip; geom_attention.py forward between its proj and out_proj), fp32 in and out.
 * proj [B*S][15 H]: per token q_rot | k_rot | v | q_dist | k_dist, H x 3 each.  rot [n][S][9], trans [n][S][3], frame_mask int32 [n][S]
 * with n = B (per_row_frames != 0) or 1 (every row shares the frames).  w_rot / w_dist [H]: softplus of rotation_scale_per_head /
 * distance_scale_per_head.  For head h: score(i,j) = (R_i q_rot_i . R_j k_rot_j) / sqrt(3) w_rot[h] - |T_i q_dist_i - T_j k_dist_j| /
 * sqrt(3) w_dist[h]; softmax over the framed keys j; out[i] = R_i^T sum_j p_ij R_j v_j; rows of frameless queries are zero.
 * out [B*S][3 H].  pgmi_op_geom_key_tile: the keys per LDS tile the launch uses for S (16, 64 or 256). */
int pgmi_op_geom_attention(int device, const float* proj, const float* rot, const float* trans, const int32_t* frame_mask,
                           int per_row_frames, const float* w_rot, const float* w_dist, int B, int S, int H, float* out);
int pgmi_op_geom_key_tile(int S);
int pgmi_op_moe(int device, const float* h, const float* gate, const float* w1, const float* w3, const float* w2, int M, int D, int F,
                int E, int top_k, int gated, float* out, int32_t* ids, float* weights);
int pgmi_op_tied_row_attention(int device, const float* qkv, int R, int C, int H, int splits, float* ctx, float* probs);
int pgmi_op_tied_row_splits(int R, int C, int H);
int pgmi_op_column_attention(int device, const float* X, const float* W, const float* bias, int K, int R, int C, int H, float* ctx);
/* The scoring tail (elementwise.hip) through the production launchers, on the entry's own buffers: host pointers in and out.  Every output
 * buffer starts as 0xFF bytes (an element the kernel skips comes back as NaN) and carries 64 guard values behind it; a guard value the
 * kernel touched fails the call with PGMI_EHIP.  *nonfinite: the device flag after the launch (zero before it).  Every refusal below is
 * PGMI_EINVAL with a message, made before the device is looked for or anything is allocated, as is a NULL pointer or a non-positive size.
 * pgmi_op_vocab_logsoftmax: h [rows][D], E [V][D], bias [V]; out [rows][V] = log_softmax(h E^T + bias).  One lane per logit: V outside
 *   1 .. 64 is refused.
 * pgmi_op_wide_logsoftmax: logits [rows][ldl], ldl % 4 == 0, ldl >= V; the columns V .. ldl-1 are padding whose values must not matter.
 *   tgt NULL: out [rows][V]; else out [rows] = log p(column tgt[r]), every tgt[r] in [0, V).
 * pgmi_op_group_logsoftmax: the grouped head; full [rows][V] and group [rows][groups] (either may be NULL, not both), groups of `width`
 *   columns from column `first`.  What launch_group_logsoftmax refuses (D % 4, D > 2560, V > 512, more than 64 groups or columns per
 *   group, groups past column V) comes back with its message.
 * pgmi_op_seq_loglik: out [B] = sum over the targets of a sequence of the fused log-probability.  Dense form (lens != NULL): lp [B*T][V],
 *   tokens [B*T], n_lp_rows = B T, lens[b] in [0, T]; target t of sequence b is tokens[b T + t + 1], read from row b T + t, t < lens[b] - 1.
 *   Ragged form (lens == NULL): sequence b owns the T - seq_p[b] packed rows from seq_off[b] on (its tokens seq_p[b] .. T-1) and takes
 *   the rows of the tokens before seq_p[b] from sequence seq_root[b], which must own all its T rows (seq_p == 0); every sequence sums
 *   T - 1 targets.  prior (nullable) [n_prior_rows][V] with the windows a0 / row0 / n / flip [B]: target t in [a0, a0 + n) takes prior row
 *   row0 + (t - a0), or row0 + n - 1 - (t - a0) when flip, as (1 - alpha) lp + alpha prior; eve (nullable, needs prior; same rows):
 *   (1 - beta) that + beta eve, or `that` alone where eve is -inf and eve_fallback != 0.  Refused: a token outside [0, V), a window
 *   with a0 + n > T - 1 or row0 + n > n_prior_rows, ragged rows outside [0, n_lp_rows). */
int pgmi_op_vocab_logsoftmax(int device, const float* h, const float* E, const float* bias, int rows, int D, int V, float* out,
                             int32_t* nonfinite);
int pgmi_op_wide_logsoftmax(int device, const float* logits, int ldl, int rows, int V, const int32_t* tgt, float* out, int32_t* nonfinite);
int pgmi_op_group_logsoftmax(int device, const float* h, const float* E, const float* bias, int rows, int D, int V, int first, int groups,
                             int width, float* full, float* group, int32_t* nonfinite);
int pgmi_op_seq_loglik(int device, const float* lp, const int32_t* tokens, int B, int T, int V, const int32_t* lens, const int32_t* seq_off,
                       const int32_t* seq_p, const int32_t* seq_root, int n_lp_rows, const float* prior, int n_prior_rows,
                       const int32_t* a0, const int32_t* row0, const int32_t* n, const int32_t* flip, float alpha, const float* eve,
                       float beta, int eve_fallback, float* out);

/* ---- Tranception (arch PGMI_ARCH_TRANCEPTION; vocab 25, max_positions = n_ctx, precision f16x3) ------
 * Weight blob order (fp32, names as in the HF state dict, Conv1D weights as stored = [in,out]):
 *   transformer.wte.weight [V,D];
 *   per layer h.{i}: ln_1 w,b; attn.c_attn W[D,3D], b[3D];
 *        attn.{query,key,value}_depthwiseconv.{0,1,2}.conv weight [64,k] (k = 3,5,7), bias [64]  (in that order);
 *        attn.c_proj W[D,D], b; ln_2 w,b; mlp.c_fc W[D,F], b[F]; mlp.c_proj W[F,D], b[D];
 *   transformer.ln_f w,b; lm_head.weight [V,D].
 *
 * pgmi_tr_token_logprobs: replaces log_softmax(model(input_ids, attention_mask).logits)
 *   (model_pytorch.py:731-783); tokens int32 [B,T] right-padded with [PAD]=3; out f32 [B,T,V].
 * pgmi_tr_sequence_loglik: the scoring reduction of tranception/utils/scoring_utils.py:97-128 --
 *   out[b] = sum_{t < lens[b]-1} log p(tokens[b,t+1] | tokens[b,<=t]) -- with the inference-time
 *   retrieval fusion of model_pytorch.py:806-830 when log_prior != NULL: for sequence b, logit rows
 *   [prior_a0[b], prior_a0[b]+prior_n[b]) are replaced by (1-alpha)*logp + alpha*log_prior[row],
 *   row = prior_row0[b] + i (or prior_row0[b] + n-1-i when prior_flip[b] != 0: right-to-left scoring).
 *   lens[b] counts [CLS] and [SEP].  log_prior is f32 [P,V] (host). */
int pgmi_tr_token_logprobs(pgmi_model* m, const int32_t* tokens, int B, int T, float* out);
int pgmi_tr_sequence_loglik(pgmi_model* m, const int32_t* tokens, const int32_t* lens, int B, int T,
                            const float* log_prior, int P, const int32_t* prior_a0, const int32_t* prior_row0,
                            const int32_t* prior_n, const int32_t* prior_flip, float alpha, float* out);
/* pgmi_tr_sequence_loglik_shared: the same quantity for B sequences of EXACTLY T tokens each (no padding), computed with the work
 *   the reference's loop repeats shared: the reference forwards every mutated sequence in full, once per reading direction
 *   (tranception/utils/scoring_utils.py:97-128 inside :77-150; model_pytorch.py:878-928), although the model is causal (attention
 *   model_pytorch.py:155-183, depth-wise convolution :73-88) and a mutated sequence equals the wild type up to its first mutated token.
 *   ref[b] names the sequence of this call whose prefix sequence b shares (its "root": the wild type cut to the same window); a root
 *   has ref[b] == b and is forwarded in full.  For every other sequence only the rows from its first difference from its root on go
 *   through LayerNorm, the GEMMs and the head (the depth-wise convolution and the attention also recompute the head of that token's
 *   32-token tile from the root's rows, so that tiles stay whole); keys, values, convolution history and log-probability rows before
 *   that are the root's.  Every row
 *   goes through the same kernels with the same inputs in the same order as in pgmi_tr_sequence_loglik: out[b] has the same bits.
 *   token_logprobs (optional, f32 [B,T,V]): the rows pgmi_tr_token_logprobs would return.  rows_forwarded (optional): token rows that
 *   went through the network (B*T for the unshared call). */
int pgmi_tr_sequence_loglik_shared(pgmi_model* m, const int32_t* tokens, const int32_t* ref, int B, int T,
                                   const float* log_prior, int P, const int32_t* prior_a0, const int32_t* prior_row0,
                                   const int32_t* prior_n, const int32_t* prior_flip, float alpha, float* out,
                                   float* token_logprobs, int64_t* rows_forwarded);
/* pgmi_tr_sequence_loglik_eve / pgmi_tr_sequence_loglik_shared_eve: the two calls above with TranceptEVE's second prior
 *   (trancepteve/model_pytorch.py:1113-1133).  eve_log_prior f32 [P,V] (host, nullable; needs log_prior) is indexed and flipped exactly
 *   like log_prior (prior_row0, prior_n, prior_flip).  For a fused position with network log-probability lp, retrieval row m and EVE
 *   row e at the target token, in fp32 and in this order: (1-beta)*((1-alpha)*lp + alpha*m) + beta*e; where e is -inf (a column outside
 *   EVE's focus columns) and eve_fallback != 0: (1-alpha)*lp + alpha*m; with eve_fallback == 0 the -inf goes through the arithmetic as
 *   in the reference.  eve_log_prior == NULL: the two calls above, bit for bit (they are these calls with NULL); the _shared_eve
 *   output has the bits of the _eve output. */
int pgmi_tr_sequence_loglik_eve(pgmi_model* m, const int32_t* tokens, const int32_t* lens, int B, int T,
                                const float* log_prior, int P, const int32_t* prior_a0, const int32_t* prior_row0,
                                const int32_t* prior_n, const int32_t* prior_flip, float alpha, const float* eve_log_prior, float beta,
                                int eve_fallback, float* out);
int pgmi_tr_sequence_loglik_shared_eve(pgmi_model* m, const int32_t* tokens, const int32_t* ref, int B, int T,
                                       const float* log_prior, int P, const int32_t* prior_a0, const int32_t* prior_row0,
                                       const int32_t* prior_n, const int32_t* prior_flip, float alpha, const float* eve_log_prior,
                                       float beta, int eve_fallback, float* out, float* token_logprobs, int64_t* rows_forwarded);

/* Tuning utility: times `iters` launches of the production GEMM (device-resident random operands,
 * HIP events) for one shape; variant selects the launch parameters (negative or below 1000 = library default;
 * 1000 + t: see gemm_f16.hip gemm_group_m).  split_out: 0 fp32 output, 1 split fp16 planes (the next GEMM's operand),
 * 2 fp32 output with the in-place residual of the out-projection / FC2, 3 the fused QKV epilogue (N = 3 D).
 * Writes the mean milliseconds per launch. */
int pgmi_bench_gemm(int device, int precision, int M, int N, int K, int epilogue, int split_out,
                    int variant, int iters, double* ms_per_launch);
/* The same for several variants on ONE set of operands, timed in `rounds` interleaved rounds of `iters` launches
 * each (within-process A/B); ms_out[v] = median over the rounds of the mean milliseconds per launch. */
int pgmi_bench_gemm_ab(int device, int precision, int M, int N, int K, int epilogue, int split_out,
                       const int* variants, int n_variants, int rounds, int iters, double* ms_out);

/* ---- ProGen2 (arch PGMI_ARCH_PROGEN2; vocab 32, max_positions = n_positions, heads % 8 == 0, precision f16x3) ----
 * Tokens (progen2/tokenizer.json): <|pad|> 0, <|bos|> 1, <|eos|> 2, '1' 3, '2' 4, 'A'..'Z' 5..29.  head_dim = D / heads: any even
 * value up to 256 (80 and 96 run zero-padded in the 128-lane layout, 256 = progen2-xlarge in four 64-lane slot groups).
 * Weight blob order (fp32, nn.Linear layout [out,in], names as in the HF state dict):
 *   transformer.wte.weight [V,D];
 *   per layer h.{i}: ln_1 w,b; attn.qkv_proj.weight with its rows REORDERED to q | k | v, [3D,D] (row h*dh + j of each block = dim j
 *        of head h: the mp_num = 8 interleave of q, v, k blocks of modeling_progen.py:157-168 undone by the host,
 *        proteingym_amd/progen2.py); attn.out_proj.weight [D,D]; mlp.fc_in W[F,D], b[F]; mlp.fc_out W[D,F], b[D];
 *   transformer.ln_f w,b; lm_head W[V,D], b[V].
 * (qkv_proj and out_proj carry no bias; ln_2 does not exist: both branches read ln_1's output, modeling_progen.py:252-283.)
 *
 * pgmi_pg2_model_create: as pgmi_model_create, with the config's rotary_dim (2 .. head_dim, even; head_dim when the config has
 *   none): the first rotary_dim dims of every q / k head rotate in interleaved pairs (2i, 2i+1), inv_freq = 10000^(-2i/rotary_dim),
 *   angle = fp32(t) * fp32(inv_freq) (modeling_progen.py:38-58).  Returns an ordinary model: destroy, profile, synchronize as usual.
 * pgmi_pg2_token_logprobs: log_softmax(model(input_ids).logits) over all 32 columns; tokens int32 [B,T] (no padding, T <=
 *   n_positions), out f32 [B,T,32].
 * pgmi_pg2_sequence_loglik: the reduction of progen2/compute_fitness.py:53-74 for B rows of L tokens each: the model reads
 *   tokens[b, :L-1], the targets are tokens[b, 1:], the last target is dropped when it is '1' (3) or '2' (4), and out[b] = sum over
 *   the kept targets of the log-softmax over logits columns 5..29 at the target's column.  n_kept (optional, int32 [B]) receives the
 *   number of kept targets (the reference's score is -CE = out[b] / n_kept[b]; 0 kept targets: its mean is NaN).  Every kept target
 *   must be an amino-acid id 5..29.  Equal-length rows only: reading direction and chunking are the host's. */
int pgmi_pg2_model_create(const pgmi_config* cfg, int rotary_dim, const float* weights, int64_t n_weights, int device, pgmi_model** out);
int pgmi_pg2_token_logprobs(pgmi_model* m, const int32_t* tokens, int B, int T, float* out);
int pgmi_pg2_sequence_loglik(pgmi_model* m, const int32_t* tokens, int B, int L, float* out, int32_t* n_kept);

/* ---- Causal decoder (arch PGMI_ARCH_GPT; any vocab, max_positions = n_positions / max_seq_len, precision f16x3) ----------------
 * Per layer: x += out_proj(causal_attention(ln_1(x))); x += fc_out(gelu_tanh(fc_in(ln_2(x)))); then ln_f and the bias-free head.
 * Scores are scaled by head_dim^-1/2; gelu_tanh(u) = 0.5 u (1 + tanh(0.79788456 (u + 0.044715 u^3))) (RITA_gelu, gelu_new).
 * head_dim = D / heads: an even value up to 64 (zero-padded to 64 lanes) or 128 (RITA XL).  Token ids are the tokenizer's own.
 * Weight blob order (fp32, nn.Linear layout [out,in]; GPT-2's Conv1D weights are transposed and c_attn split by the host,
 * proteingym_amd/causal_lm.py):
 *   wte [V,D]; (LEARNED) wpe [max_positions,D];
 *   per layer: ln_1 w,b; Wq [D,D], bq; Wk, bk; Wv, bv; Wo [D,D], bo; ln_2 w,b; fc_in W[F,D], b[F]; fc_out W[D,F], b[D];
 *   ln_f w,b; (ROTARY) lm_head [V,D].
 * pos_kind ROTARY (RITA): q and k rotate by rotate-half over the whole head, pairs (j, j + head_dim/2),
 *   inv_freq = 10000^(-2j/head_dim), angle = fp32(t) * fp32(inv_freq) (rita_modeling.py:36-62).
 * pos_kind LEARNED (GPT-2): x = wte[id] + wpe[t]; the head is wte itself.
 *
 * pgmi_gpt_weight_count: the blob size for (cfg, pos_kind); <0 on a bad cfg.  (pgmi_weight_count returns -1 for this arch.)
 * pgmi_gpt_model_create: as pgmi_model_create, with pos_kind.  Returns an ordinary model: destroy, profile, synchronize as usual.
 * pgmi_gpt_token_logprobs: log_softmax(model(input_ids).logits) over all V columns; tokens int32 [B,T] (no padding,
 *   T <= max_positions), out f32 [B,T,V].
 * pgmi_gpt_sequence_loglik: B rows right-padded to T tokens (pad ids must lie in [0, V)), row b holding lens[b] >= 2 real tokens.
 *   sum[b] = sum over t < lens[b]-1 of log p(tokens[b,t+1] | tokens[b,<=t]) and n_targets[b] = lens[b]-1 (optional); the
 *   reference's -CE of the row is sum[b] / n_targets[b].  Pad positions are never scored and need no key mask (a causal row reads
 *   no key to its right).  A row's result has the same bits whatever else is in the batch.
 * Heads with V <= 64 (RITA: 26) run on one wave per row; wider ones (ProtGPT2: 50257) on the f16x3 GEMM into fp32 logits followed
 * by a 256-thread log-softmax per row, over the target rows only when scoring. */
int64_t pgmi_gpt_weight_count(const pgmi_config* cfg, int pos_kind);
int pgmi_gpt_model_create(const pgmi_config* cfg, int pos_kind, const float* weights, int64_t n_weights, int device, pgmi_model** out);
int pgmi_gpt_token_logprobs(pgmi_model* m, const int32_t* tokens, int B, int T, float* out);
int pgmi_gpt_sequence_loglik(pgmi_model* m, const int32_t* tokens, const int32_t* lens, int B, int T, double* sum, int32_t* n_targets);

/* ---- ProGen3 (arch PGMI_ARCH_PROGEN3; vocab > 64, max_positions = rotary table rows, precision f16x3) ----------------------------
 * Tokens (progen3/tokenizer.json): <pad> 0, <bos> 1, <eos> 2, "1" 6, "2" 7, letters A 8 .. Y 32; a sequence is <bos> 1 SEQ 2 <eos>.
 * Embedding: embed_tokens[id] + embed_seq_id[0] (one sequence per row: sequence_ids are all zero), folded into one table at creation.
 * Per layer: x += o_proj(attn(rmsnorm(x))); x += moe(rmsnorm(x)); no bias anywhere; rmsnorm(x) = x * rsqrt(mean(x^2) + ln_eps) * w.
 * Attention: heads query heads on kv_heads key / value heads (heads % kv_heads == 0; query head h reads K/V head h / (heads / kv_heads)),
 *   rotate-half rotary over the whole head, inv_freq = rope_theta^(-2j/head_dim), angle = fp32(t) * fp32(inv_freq), causal, scores
 *   scaled by head_dim^-1/2.  head_dim = D / heads in {64, 80, 96, 128, 256}.  The K/V projection rows are replicated to their query heads
 *   when the fused QKV weight is packed, so the attention kernels see heads full heads.  clip_qkv must be 0 (unset): the clamp sits
 *   between the projection and the rotary, inside the fused epilogue.
 * MoE (model/moe.py SparseMoeBlock): p = softmax_fp32(gate h); the top_k largest p (ties: lower index), divided by their sum, weigh
 *   w2(silu(w1 h) * w3 h) (gated) or w2(silu(w1 h)) of the chosen experts.  n_experts == 1: the plain MLP, no gate.  2 <= n_experts <= 64
 *   otherwise.  Rows whose token is <pad> are not routed.
 * Then the final rmsnorm and the untied lm_head [V,D]; log-softmax over all V columns.
 * Weight blob order (fp32, nn.Linear layout [out,in]):
 *   model.embed_tokens [V,D]; model.embed_seq_id row 0 [D];
 *   per layer: input_layernorm w [D]; q_proj [D,D]; k_proj [kv_heads * head_dim, D]; v_proj (same); o_proj [D,D];
 *        post_attention_layernorm w [D]; (n_experts > 1) gate [E,D]; per expert: w1 [F,D]; (gated) w3 [F,D]; w2 [D,F];
 *   model.norm w [D]; lm_head [V,D].
 *
 * pgmi_pg3_weight_count: the blob size for (cfg, params); <0 on a bad cfg.  (pgmi_weight_count returns -1 for this arch.)
 * pgmi_pg3_model_create: as pgmi_model_create, with params.  Returns an ordinary model: destroy, profile, synchronize as usual.
 * pgmi_pg3_token_logprobs: tokens int32 [B,T] right-padded with <pad> (0), T <= max_positions; out f32 [B,T,V] = log_softmax(logits);
 *   rows of <pad> tokens hold values nobody should read.
 * pgmi_pg3_sequence_loglik: the signature and meaning of pgmi_gpt_sequence_loglik: B rows right-padded to T, row b holding lens[b] >= 2
 *   real tokens (none of them <pad>); sum[b] = sum over t < lens[b]-1 of log p(tokens[b,t+1] | tokens[b,<=t]), fp32 terms summed in
 *   double left to right; n_targets[b] = lens[b]-1.  A row's result has the same bits whatever else is in the batch.
 * pgmi_pg3_routing: the experts and weights the last forward chose in `layer` for its first `rows` token rows (row = b * T_in + t of
 *   the last device chunk; T_in = T - 1 after pgmi_pg3_sequence_loglik): ids int32 [rows][top_k] (-1: a <pad> row), weights f32. */
typedef struct pgmi_pg3_params {
    int32_t kv_heads;             /* num_key_value_heads */
    int32_t n_experts;            /* num_experts */
    int32_t top_k;                /* num_experts_per_tok (<= n_experts) */
    int32_t gated;                /* gated_mlp */
    float rope_theta;
    float clip_qkv;               /* 0 = unset; anything else is refused */
} pgmi_pg3_params;
int64_t pgmi_pg3_weight_count(const pgmi_config* cfg, const pgmi_pg3_params* params);
int pgmi_pg3_model_create(const pgmi_config* cfg, const pgmi_pg3_params* params, const float* weights, int64_t n_weights, int device,
                          pgmi_model** out);
int pgmi_pg3_token_logprobs(pgmi_model* m, const int32_t* tokens, int B, int T, float* out);
int pgmi_pg3_sequence_loglik(pgmi_model* m, const int32_t* tokens, const int32_t* lens, int B, int T, double* sum, int32_t* n_targets);
int pgmi_pg3_routing(pgmi_model* m, int layer, int rows, int32_t* ids, float* weights);

/* ---- ESM C (arch PGMI_ARCH_ESMC; vocab 64, head_dim 64, embed_dim <= 2048, ffn_dim = the SwiGLU hidden width F, precision f16x3) --
 * Per block: x += out_proj(attn(x)) / s; x += ffn(x) / s with s = sqrt(layers / 36) (transformer_stack.py:50, blocks.py:150-162).
 * attn: LayerNorm (with bias) -> QKV without bias -> q, k each LayerNorm-ed over the whole width D without bias (before the head
 * split) -> rotate-half rotary per 64-dim head (base 1e4) -> softmax(q k^T / 8) v -> out_proj without bias.  ffn: LayerNorm (with
 * bias) -> W1 -> silu(gate) * up -> W2, both bias-free.  Then a LayerNorm without bias and the head Linear(D,D) + erf-GELU +
 * LayerNorm + Linear(D,64); log-softmax over all 64 columns.  Token ids are ESM's (PGMI_TOK_*); <pad> keys are masked.
 * Weight blob order (fp32, nn.Linear layout [out,in], names as in ESMC.state_dict()):
 *   embed.weight [64,D];
 *   per block i (transformer.blocks.i.): attn.layernorm_qkv.0.{weight,bias} [D]; attn.layernorm_qkv.1.weight [3D,D] (q | k | v rows);
 *     attn.q_ln.weight [D]; attn.k_ln.weight [D]; attn.out_proj.weight [D,D]; ffn.0.{weight,bias} [D];
 *     ffn.1.weight [2F,D] with its rows in SwiGLU block order: for b < F/32, the gate rows 32b .. 32b+31 (the first F rows of the
 *     checkpoint) then the up rows F+32b .. F+32b+31 (the pgmi_op_gemm SwiGLU layout); ffn.3.weight [D,F];
 *   transformer.norm.weight [D]; sequence_head.0.{weight [D,D], bias}; sequence_head.2.{weight,bias}; sequence_head.3.{weight [64,D], bias [64]}.
 * pgmi_weight_count gives its size.  pgmi_masked_logprobs serves this arch (out [B,64]); ready-made rows carry their own window (ESM C's
 * window rule differs from pgmi_optimal_window, so pgmi_assay_create refuses this arch). */

/* ---- ESM3 (arch PGMI_ARCH_ESM3; vocab 64, head_dim 64, embed_dim <= 2048, ffn_dim = the SwiGLU hidden width F, precision f16x3) ----
 * The blocks are ESM C's (above), with the same scaled residual, final LayerNorm and 64-column sequence head.  What differs:
 * Input embedding (esm3.py EncodeInputs with the defaults of ESM3.forward / ESM3.logits): x = sequence_embed[id] +
 *   structure_tokens_embed[structure token] + c[p], where c[p] = plddt_projection(rbf16(1)) + structure_per_res_plddt_projection(
 *   rbf16(p)) + ss8_embed[0] + sasa_embed[0] is folded at creation in fp32 (rbf16: 16 centres on [0,1], width 1/16) and p = 1 where
 *   the token has finite coordinates, else 0.  The function and residue-annotation tracks are at their padding rows: zero.
 * Block 0 (blocks.py:150-162): x += attn(x) / s; x += geom_attn(x) / s; x += ffn(x) / s.  geom_attn (geom_attention.py, v_heads = Hv):
 *   LayerNorm without bias -> Linear(D, 15 Hv) -> the geometric attention of pgmi_op_geom_attention over the bound frames ->
 *   Linear(3 Hv, D), both bias-free.  When no token of the bound window has a frame the branch is exactly zero and is not launched.
 * Limits: Hv % 4 == 0, 15 Hv <= 3 D, roundup(3 Hv, 32) <= min(D, F).
 * Weight blob order (fp32, nn.Linear layout [out,in], names as in ESM3.state_dict()):
 *   encoder.sequence_embed.weight [64,D]; encoder.plddt_projection.{weight [D,16], bias [D]};
 *   encoder.structure_per_res_plddt_projection.{weight [D,16], bias [D]}; encoder.structure_tokens_embed.weight [4101,D];
 *   encoder.ss8_embed.weight [11,D]; encoder.sasa_embed.weight [19,D];
 *   per block i (transformer.blocks.i.): ESM C's ten tensors in ESM C's order; block 0 has, between attn.out_proj.weight and ffn.0.weight,
 *     geom_attn.distance_scale_per_head [Hv]; geom_attn.rotation_scale_per_head [Hv]; geom_attn.s_norm.weight [D];
 *     geom_attn.proj.weight [15 Hv, D]; geom_attn.out_proj.weight [D, 3 Hv];
 *   transformer.norm.weight [D]; output_heads.sequence_head.{0.weight [D,D], 0.bias, 2.weight, 2.bias, 3.weight [64,D], 3.bias [64]}.
 * The other five output heads are not part of the blob.
 *
 * pgmi_esm3_weight_count: the blob size for (cfg, v_heads); <0 on a bad cfg.  (pgmi_weight_count returns -1 for this arch.)
 * pgmi_esm3_model_create: as pgmi_model_create, with v_heads.  Returns an ordinary model: destroy, profile, synchronize as usual.
 * pgmi_esm3_set_structure: binds one window of T tokens (<cls> + residues + <eos>); every later pgmi_token_logprobs /
 *   pgmi_masked_logprobs call must have this T, and all its rows share the structure (masking changes the sequence id only).
 *   structure_tokens int32 [T] in [0, 4101) (4096 mask, 4097 eos, 4098 bos); plddt int32 [T]: p above; rot f32 [T][9] row-major
 *   3x3 and trans f32 [T][3]: the frames of build_affine3d_from_coordinates (Gram-Schmidt on (C, CA, N); frameless tokens carry the
 *   frame of the window's mean N / CA / C, or the identity); frame_mask int32 [T]: non-zero = the token has a frame.
 *   Without a bound window the forward entries return PGMI_EINVAL. */
int64_t pgmi_esm3_weight_count(const pgmi_config* cfg, int v_heads);
int pgmi_esm3_model_create(const pgmi_config* cfg, int v_heads, const float* weights, int64_t n_weights, int device, pgmi_model** out);
int pgmi_esm3_set_structure(pgmi_model* m, const int32_t* structure_tokens, const int32_t* plddt, const float* rot, const float* trans,
                            const int32_t* frame_mask, int T);

/* ---- SaProt (arch PGMI_ARCH_SAPROT; vocab 446, max_positions 0, every precision) ---------------------------------------------
 * The model is ESM2 (rotary, erf-GELU, tied LM head; head dims as for ESM2) and its weight blob is ESM2's in pgmi_weight_count's order
 * with V = 446 (HF names -> ESM names: proteingym_amd/saprot.py).  Token ids are the tokenizer's: <cls> 0, <pad> 1, <eos> 2, <unk> 3,
 * <mask> 4, then for a in "ACDEFGHIKLMNPQRSTVWY#" and s in "pynwrqhgdlvtmfsaeikc#" the token a+s at 5 + 21 index(a) + index(s).
 * Id 32 is an ordinary residue token here: the <mask> id is the model's own (mask_id, the config's mask_token_id = 4), and with
 * token_dropout the embedding is scaled by 0.88 / (1 - #mask / #tokens) as in ESM2.  <pad> is honoured as in pgmi_token_logprobs.
 *
 * pgmi_saprot_model_create: as pgmi_model_create, with mask_id.  Returns an ordinary model: destroy, profile, synchronize as usual.
 * pgmi_saprot_token_logprobs: log_softmax(model(input_ids).logits) over all 446 columns; tokens int32 [B,T], out f32 [B,T,446].
 * pgmi_saprot_group_logprobs: the forwards of compute_fitness.py:17-55 for one structure chunk, one per DISTINCT set of mutated
 *   positions (the masked input depends on nothing else).  wt_tokens int32 [T]: <cls> + the chunk's tokens + <eos>; position set s is
 *   set_pos[set_off[s] .. set_off[s+1]) (CSR; token positions, <cls> = 0, ascending, on residue tokens).  The forward of set s
 *   replaces every token of the set by '#' + its structure letter (the amino-acid half masked).  out f32 [set_off[n_sets]][21]:
 *   for entry e = (set, position), out[e][a] = log sum_s p(a+s) = logsumexp(logits[5 + 21 a .. + 21)) - logsumexp(logits[0 .. 446))
 *   at that position; the reference's per-sub-mutation term log(sum probs[mt] / sum probs[wt]) is out[e][mt] - out[e][wt], so
 *   pgmi_score_mutants(out, n_entries, 21, sub_pos = e, sub_wt, sub_mt, ...) gives its scores.  An entry's bits do not depend on
 *   the other sets of the call.  T + 31 > max_rows is PGMI_EINVAL: the reference does not window, neither does this path. */
int pgmi_saprot_model_create(const pgmi_config* cfg, int mask_id, const float* weights, int64_t n_weights, int device, pgmi_model** out);
int pgmi_saprot_token_logprobs(pgmi_model* m, const int32_t* tokens, int B, int T, float* out);
int pgmi_saprot_group_logprobs(pgmi_model* m, const int32_t* wt_tokens, int T, const int32_t* set_off, const int32_t* set_pos,
                               int n_sets, float* out);

/* ---- MULAN (arch PGMI_ARCH_MULAN; vocab 33 or 446, max_positions 0, every precision) ----------------------------------------------
 * The main stack is ESM2 (groups = 0: the 33-token ESM alphabet, <mask> = 32) or SaProt's encoder (groups = 21: the 446-token layout
 * of the SaProt section, <mask> = 4).  In front of it sits the structure adapter (mulan/model_utils.py:59-97): per token a row of
 * seven angles (phi, psi, chi1..chi5, radians) goes through Linear(7 -> D), one full ESM layer of width D WITHOUT rotary (and without
 * a position table), and a final LayerNorm; the result is added to the word embedding before token dropout:
 *   x = (E[token] + adapter(row)), zero at <mask>, times 0.88 / (1 - #mask / #tokens) with token_dropout.
 * The angle row of token t is chosen per forward: 4.0 (seven times) for the first and last token and where plddt[t] <= 70, -4.0 where
 * t is one of the forward's masked positions (this wins), else the bound angles (dataset.py:306-314, compute_fitness.py:117-126).
 * Weight blob: ESM2's in pgmi_weight_count's order with V = vocab, then MLP.weight [D][7], MLP.bias [D], one layer in the same
 * per-layer order with fc1 [4D,D] and fc2 [D,4D], and the adapter's final LayerNorm w, b (HF names: proteingym_amd/mulan.py).
 *
 * pgmi_mulan_model_create: groups must fit cfg->vocab (0: 33, 21: 446); mask_id is the tokenizer's <mask> id.
 * pgmi_mulan_set_structure: binds the chunk -- angles f32 [T][7], plddt f32 [T] (the values of the two end tokens are not read) -- for
 *   the T tokens <cls> + residues + <eos>.  The forward entries refuse another T, and PGMI_EINVAL without a bound chunk.
 * pgmi_mulan_token_logprobs: B explicit rows tokens int32 [B][T] (no <pad>); row b's masked positions are
 *   row_pos[row_off[b] .. row_off[b+1]) (ascending, possibly none): they choose the -4 angle rows, the tokens are taken as given.
 *   out f32 [B][T][V]: log_softmax over all V columns.
 * pgmi_mulan_set_logprobs: one forward per position set (CSR as in pgmi_saprot_group_logprobs, on residue tokens) of the wild type
 *   wt_tokens [T], the set's tokens replaced by <mask> and its angle rows by -4.  out f32 [set_off[n_sets]][V] (groups = 0: the
 *   log-softmax row at every (set, position)) or [..][21] (groups = 21: SaProt's group table).  An entry's bits do not depend on the
 *   other sets of the call.  T + 31 > max_rows is PGMI_EINVAL: sequences are not windowed. */
int64_t pgmi_mulan_weight_count(const pgmi_config* cfg);
int pgmi_mulan_model_create(const pgmi_config* cfg, int mask_id, int groups, const float* weights, int64_t n_weights, int device,
                            pgmi_model** out);
int pgmi_mulan_set_structure(pgmi_model* m, const float* angles, const float* plddt, int T);
int pgmi_mulan_token_logprobs(pgmi_model* m, const int32_t* tokens, int B, int T, const int32_t* row_off, const int32_t* row_pos, float* out);
int pgmi_mulan_set_logprobs(pgmi_model* m, const int32_t* wt_tokens, int T, const int32_t* set_off, const int32_t* set_pos, int n_sets,
                            float* out);

/* ---- PoET (arch PGMI_ARCH_POET; vocab 24 .. 64, head_dim an even value up to 64, precision f16x3) ------------------------------
 * Tokens (poet/alphabets.py Uniprot21 with gap and distinct start / stop): "ARNDCQEGHILKMFPSTWYV" 0..19, gap 20, start 21, stop 22,
 * mask 23 (also X, B, Z; O = 11, U = 4).  No position table: both attentions of a layer rotate q and k by the position inside the
 * sequence (interleaved pairs (2i, 2i+1), inv_freq = 10000^(-2i/head_dim), angle = fp32(t) * fp32(inv_freq)), q scaled by head_dim^-1/2.
 * Per layer: x += out_proj(self_attn(norm1(x))) within each sequence; x += out_proj(multihead_attn(norm2(x))) causally over the
 * sequence-of-sequences; x += linear2(gelu_erf(linear1(norm3(x)))).  Then `norm` (final_norm != 0) and linear [V,D] + bias.
 * Config: max_positions = the largest prompt in tokens the caller will set (the per-layer prefix cache is allocated for it; 0: none);
 * max_rows >= the prompt's tokens with every prompt sequence rounded up to 32.
 * Weight blob order (fp32, nn.Linear layout [out,in], state-dict names without their leading component):
 *   token_embed.weight [V,D];
 *   per layer decoder.layers.{i}: norm1 w,b; self_attn.{q_proj, k_proj, v_proj}.weight [D,D] each; self_attn.out_proj W[D,D], b;
 *        norm2 w,b; multihead_attn.{q_proj, k_proj, v_proj}.weight; multihead_attn.out_proj W, b; norm3 w,b;
 *        linear1 W[F,D], b[F]; linear2 W[D,F], b[D];
 *   (final_norm) norm w,b; linear W[V,D], b[V].
 *
 * pgmi_poet_weight_count: the blob size for (cfg, final_norm); <0 on a bad cfg.  (pgmi_weight_count returns -1 for this arch.)
 * pgmi_poet_model_create: as pgmi_model_create, with final_norm.  Returns an ordinary model: destroy, profile, synchronize as usual.
 * pgmi_poet_set_prompt: the tiered forward (PoET.embed) over a prompt of n_seg sequences, tokens int32 [sum seg_len] concatenated, each
 *   with its start and stop token; fills the per-layer prefix cache with the tier-2 keys (rotated) and values.  n_seg = 0 clears the
 *   cache (the reference's memory=None).  A prompt of more than max_positions tokens is PGMI_EINVAL (the cache never grows mid-assay);
 *   after any failure no prompt is set.
 * pgmi_poet_prompt_logprobs: out f32 [sum seg_len][V] = log_softmax(PoET.forward(prompt)) of the prompt last set.
 * pgmi_poet_token_logprobs: variants int32 [B,T] right-padded with the mask token, lens[b] >= 1 real tokens (start / stop counted);
 *   out f32 [B,T,V], row (b,t) = log p(. | prompt, tokens[b, <= t]) for t < lens[b]; rows beyond lens[b] are NaN.
 * pgmi_poet_sequence_loglik: out f64 [B], out[b] = sum over t < lens[b]-1 of log p(tokens[b,t+1] | prompt, tokens[b, <= t]), targets
 *   equal to the mask token skipped (scripts/score.py: CrossEntropyLoss(ignore_index=mask_token)); fp32 terms summed left to right in
 *   fp64.  Only rows that have a target reach the head.  A variant's result has the same bits whatever else is in the call and however
 *   the call is chunked. */
#define PGMI_POET_TOK_GAP 20
#define PGMI_POET_TOK_START 21
#define PGMI_POET_TOK_STOP 22
#define PGMI_POET_TOK_MASK 23
int64_t pgmi_poet_weight_count(const pgmi_config* cfg, int final_norm);
int pgmi_poet_model_create(const pgmi_config* cfg, int final_norm, const float* weights, int64_t n_weights, int device, pgmi_model** out);
int pgmi_poet_set_prompt(pgmi_model* m, const int32_t* tokens, const int32_t* seg_len, int n_seg);
int pgmi_poet_prompt_logprobs(pgmi_model* m, float* out);
int pgmi_poet_token_logprobs(pgmi_model* m, const int32_t* tokens, const int32_t* lens, int B, int T, float* out);
int pgmi_poet_sequence_loglik(pgmi_model* m, const int32_t* tokens, const int32_t* lens, int B, int T, double* out);

/* ---- ESM-IF1 (arch PGMI_ARCH_ESMIF1; the decoder; vocab <= 64, head_dim 64, precision f16x3) -------------------------------------
 * Tokens (esm/data.py Alphabet.from_architecture("invariant_gvp"), 35 ids): <pad> 1, "LAGVSERTIDPKQNFYMHWCXBUZO.-" 4..30, <mask> 32,
 * <cath> 33.  A sequence of L residues is <cath> + its L ids (no eos): the model reads the first L tokens and predicts the L residues.
 * x = sqrt(D) embed_tokens[tok] + sinusoidal(2 + t) (esm/modules.py SinusoidalPositionalEmbedding, sin | cos halves; the table is built
 * at creation for min(16384, max_rows) positions); per layer, pre-LN: causal self-attention, cross-attention over the S rows of the
 * encoder output (q from the decoder row; k / v from the memory; all with biases, q scaled by head_dim^-1/2), fc2(relu(fc1 x)); then
 * layer_norm and output_projection [V,D] without bias.  The encoder runs outside the library, once per structure.
 * Config: layers / embed_dim / heads / ffn_dim = decoder_*; max_positions = the largest memory in rows (residues + 2) the caller will
 * set (the per-layer K / V^T planes are allocated for it).  Decoder length and memory length are independent.
 * Weight blob order (fp32, nn.Linear layout [out,in], names under `decoder.`):
 *   embed_tokens.weight [V,D];
 *   per layer layers.{i}: self_attn_layer_norm w,b; self_attn.{q,k,v}_proj W[D,D],b each; self_attn.out_proj W,b;
 *        encoder_attn_layer_norm w,b; encoder_attn.q_proj W[D,D],b; encoder_attn.{k,v}_proj W[D,E],b each (E = enc_dim);
 *        encoder_attn.out_proj W,b; final_layer_norm w,b; fc1 W[F,D],b[F]; fc2 W[D,F],b[D];
 *   layer_norm w,b; output_projection.weight [V,D].
 *
 * pgmi_esmif1_weight_count: the blob size for (cfg, enc_dim); <0 on a bad cfg.  (pgmi_weight_count returns -1 for this arch.)
 * pgmi_esmif1_model_create: as pgmi_model_create, with enc_dim = encoder_embed_dim (a multiple of 32).  A head_dim other than 64 is
 *   PGMI_EINVAL.  Returns an ordinary model: destroy, profile, synchronize as usual.
 * pgmi_esmif1_set_memory: enc_out f32 [S][enc_dim], the encoder's output rows of one backbone (the two end rows the reference pads with
 *   included).  Every layer's k_proj / v_proj (with bias) of it goes into that layer's planes; scoring never re-packs them.
 *   S > max_positions (or the workspace rows), S <= 0 and a non-finite value are PGMI_EINVAL; after any failure no memory is set.
 * pgmi_esmif1_token_logprobs: sequences int32 [B,T] right-padded (pad values are not read), lens[b] >= 1 tokens; out f32 [B,T,V],
 *   row (b,t) = log p(. | memory, tokens[b, <= t]) for t < lens[b]; rows beyond lens[b] are NaN.
 * pgmi_esmif1_sequence_loglik: lens[b] >= 2; out f64 [B], out[b] = mean over t < lens[b]-1 of log p(tokens[b,t+1] | memory,
 *   tokens[b, <= t]) = the reference's -mean(cross_entropy): fp32 terms summed left to right in fp64 on the device, divided by the
 *   count.  A sequence's result has the same bits whatever else is in the call and however the call is chunked. */
int64_t pgmi_esmif1_weight_count(const pgmi_config* cfg, int enc_dim);
int pgmi_esmif1_model_create(const pgmi_config* cfg, int enc_dim, const float* weights, int64_t n_weights, int device, pgmi_model** out);
int pgmi_esmif1_set_memory(pgmi_model* m, const float* enc_out, int S);
int pgmi_esmif1_token_logprobs(pgmi_model* m, const int32_t* tokens, const int32_t* lens, int B, int T, float* out);
int pgmi_esmif1_sequence_loglik(pgmi_model* m, const int32_t* tokens, const int32_t* lens, int B, int T, double* out);

/* ---- EVE / DeepSequence (Bayesian alignment VAE; its own handle and config, precision fp32) ------------------------------------
 * Replaces VAE_model.all_likelihood_components and the sampling loop of compute_evol_indices_chunk
 * (proteingym/baselines/EVE/EVE/VAE_model.py:165-181, :466-481; VAE_encoder.py:69-88; VAE_decoder.py:112-167) as
 * compute_evol_indices_DMS.py runs them: the model is never put in eval mode, so the decoder's dropout is part of the estimator.
 * ELBO[m, j] = -(BCE + KLD) of row m under noise sample j; DESIGN.md 4.6f has the estimator, the generator and the divergences
 * (one set of decoder weights per sample, shared by all rows of the assay).
 *
 * Weight blob: fp32, the tensors of VAE_model.state_dict() in its own order, each flattened row-major:
 *   encoder.hidden_layers.{i}.weight [E_i, in_i], .bias [E_i]   i = 0 .. n_enc-1 (in_0 = 20 L)
 *   encoder.fc_mean.weight [z, E_last], .bias [z]; encoder.fc_log_var.weight [z, E_last], .bias [z]
 *   decoder.sparsity_weight_mean, decoder.sparsity_weight_log_var [H / tiles, L]          (sparsity_tiles > 0 only)
 *   decoder.last_hidden_layer_weight_mean, _log_var [C L, H]     (C = conv_depth, or 20 without the convolution; H = D_last)
 *   decoder.last_hidden_layer_bias_mean, _log_var [20 L]
 *   decoder.temperature_scaler_mean, _log_var [1]                                        (temperature != 0 only)
 *   decoder.hidden_layers_mean.{i}.weight [D_i, in_i], .bias [D_i]   i = 0 .. n_dec-1 (in_0 = z), then the same of
 *   decoder.hidden_layers_log_var.{i}
 *   decoder.output_convolution_mean.weight, decoder.output_convolution_log_var.weight [20, C, 1]     (conv_depth > 0 only)
 * Residues: uint8 [M][L], the letter's index in "ACDEFGHIKLMNPQRSTVWY"; 255 (any value >= 20) = no letter: an all-zero one-hot row,
 * which adds nothing to the encoder's first layer and has no target term in the BCE.
 * Limits: alphabet 20; encoder without dropout and input convolution (both parameter files); conv_depth % 4 == 0;
 * H % sparsity_tiles == 0; at most PGMI_EVE_MAX_LAYERS layers per stack. */
#define PGMI_EVE_MAX_LAYERS 8
#define PGMI_EVE_ACT_RELU 0
#define PGMI_EVE_ACT_TANH 1
#define PGMI_EVE_ACT_SIGMOID 2
#define PGMI_EVE_ACT_ELU 3
#define PGMI_EVE_ACT_LINEAR 4
typedef struct pgmi_eve_config {
    int32_t abi_version;                          /* = PGMI_ABI_VERSION */
    int32_t seq_len;                              /* L: focus columns */
    int32_t alphabet;                             /* = 20 */
    int32_t z_dim;
    int32_t n_enc, enc_sizes[PGMI_EVE_MAX_LAYERS];   /* encoder_parameters.hidden_layers_sizes */
    int32_t n_dec, dec_sizes[PGMI_EVE_MAX_LAYERS];   /* decoder_parameters.hidden_layers_sizes */
    int32_t conv_depth;                           /* convolution_output_depth when convolve_output, else 0 */
    int32_t temperature;                          /* include_temperature_scaler */
    int32_t sparsity_tiles;                       /* num_tiles_sparsity when include_sparsity, else 0 */
    int32_t enc_act, dec_first_act, dec_last_act; /* PGMI_EVE_ACT_* */
    int32_t precision;                            /* PGMI_PREC_FP32 (the only mode so far) */
    float dropout_p;                              /* decoder_parameters.dropout_proba */
} pgmi_eve_config;
typedef struct pgmi_eve pgmi_eve;
/* One sample's noise, host buffers, in the order the reference draws it (VAE_model.py:170, VAE_decoder.py:120-161): eps tensors are
 * the randn_like draws, keep tensors the dropout layer's Bernoulli(1 - p) masks (1 = kept; read only when dropout_p > 0). */
typedef struct pgmi_eve_noise {
    float* z_eps;                                 /* [M][z] */
    uint8_t* keep[PGMI_EVE_MAX_LAYERS + 1];       /* keep[0] [M][z] on z; keep[i + 1] [M][D_i] after hidden layer i */
    float* w_eps[PGMI_EVE_MAX_LAYERS];            /* [D_i][in_i] */
    float* b_eps[PGMI_EVE_MAX_LAYERS];            /* [D_i] */
    float* wout_eps;                              /* [C L][H] */
    float* bout_eps;                              /* [20 L] */
    float* conv_eps;                              /* [20][C]; conv_depth > 0 */
    float* sparsity_eps;                          /* [H / tiles][L]; sparsity_tiles > 0 */
    float* temp_eps;                              /* [1]; temperature != 0 */
} pgmi_eve_noise;
/* pgmi_eve_weight_count: size of the blob above; -1 for a config the library refuses (pgmi_last_error).
 * pgmi_eve_create / pgmi_eve_destroy: the device-resident model (one HIP stream).
 * pgmi_eve_profile_model: the handle's profiling view for pgmi_profile_enable / _get / _reset / pgmi_synchronize (owned by the handle,
 *   never destroyed by the caller).  Classes: PGMI_K_EMBED = the weight sampler, PGMI_K_GEMM_FC1 = latent + hidden layers,
 *   PGMI_K_GEMM_FC2 = the final GEMM, PGMI_K_SCORE = the ELBO reduction, PGMI_K_HEAD = the encoder.
 * pgmi_eve_encode: mu, log_var f32 [M][z] of the (deterministic) encoder.
 * pgmi_eve_elbo: one sample.  Row i of the call is row row_base + i of the assay (what the generator's per-row noise is indexed by).
 *   injected != NULL: every noise tensor comes from the caller (seed and sample are not read); NULL: from the device generator
 *   (Philox4x32-10 keyed by seed, counter = (element / 4, sample, tensor)).  elbo / bce / kld: f32 [M], each nullable.  A row's
 *   values depend on its residues, its global index, seed and sample only -- not on M, the other rows or the row chunking.
 * pgmi_eve_noise_fill: writes the generator's noise of (seed, sample, rows row_base .. row_base + M) into out's non-NULL buffers.
 * pgmi_eve_evol_indices: the production loop: samples 0 .. num_samples-1, per-row sum and sum of squares (of the ELBO minus the
 *   row's first sample) in fp64 on the device.  mean_elbo, std_elbo: f64 [M], std with the n - 1 denominator (torch.std); row 0 is
 *   the wild type, so evol_index[m] = -(mean_elbo[m] - mean_elbo[0]).
 * pgmi_set_option("eve_max_rows", n): rows per chunk of the hidden layers / logits (0: what fits 256 MB of logits; test hook,
 *   bit-neutral).  pgmi_set_option("eve_fixed_sample", j): pgmi_eve_evol_indices draws every sample with index j (-1: off; test hook
 *   of the accumulators). */
int64_t pgmi_eve_weight_count(const pgmi_eve_config* cfg);
int pgmi_eve_create(const pgmi_eve_config* cfg, const float* weights, int64_t n_weights, int device, pgmi_eve** out);
void pgmi_eve_destroy(pgmi_eve* m);
pgmi_model* pgmi_eve_profile_model(pgmi_eve* m);
int pgmi_eve_encode(pgmi_eve* m, const uint8_t* residues, int M, float* mu, float* log_var);
int pgmi_eve_elbo(pgmi_eve* m, const uint8_t* residues, int M, int64_t row_base, uint64_t seed, int sample,
                  const pgmi_eve_noise* injected, float* elbo, float* bce, float* kld);
int pgmi_eve_noise_fill(pgmi_eve* m, uint64_t seed, int sample, int64_t row_base, int M, pgmi_eve_noise* out);
int pgmi_eve_evol_indices(pgmi_eve* m, const uint8_t* residues, int M, int num_samples, uint64_t seed, double* mean_elbo,
                          double* std_elbo);
/* pgmi_eve_log_prior: TranceptEVE's EVE log-prior of ONE row (get_EVE_log_prior_single, trancepteve/model_pytorch.py:975-1001; decoder
 *   trancepteve/EVE/VAE_decoder.py): the mean over num_samples Monte-Carlo samples of log_softmax(decoder(z)) over the 20 letters of
 *   every position, each sample with freshly drawn decoder weights and latent.  The reference's model is in eval(): cfg.dropout_p is
 *   ignored here and the keep masks of an injected struct are not read.  residues uint8 [L].  Sample j draws with the counters of
 *   pgmi_eve_elbo(row_base = 0, sample = j): pgmi_eve_noise_fill(seed, j, 0, 1, ..) hands out its noise, and num_samples such structs
 *   as `injected` (seed is then not read) give the generator path's bits.  The final layer is fused with its sampler (the sampled
 *   [20 L][H] matrix never exists in memory) and a launch serves several samples from one read of the means and standard deviations.
 *   Per (position, letter): fp64 sum and sum of squares of (logp - the first sample's logp), added in sample order on the device;
 *   mean_logp, std_logp (nullable): f64 [L][20], std with the n - 1 denominator.  Limits: last hidden size >= 20, conv_depth <= 612.
 * pgmi_set_option("eve_prior_batch", n): samples per batch of that call (0: default; a batch runs in launches of at most 4 samples).
 *   Bit-neutral: no sum's order depends on it. */
int pgmi_eve_log_prior(pgmi_eve* m, const uint8_t* residues, int num_samples, uint64_t seed, const pgmi_eve_noise* injected,
                       double* mean_logp, double* std_logp);

/* ---- ProteinMPNN (message passing on a k-nearest-neighbour backbone graph; its own handle and config, precision fp32) ------------
 * Replaces ProteinMPNN.forward and _scores (proteingym/baselines/protein_mpnn/protein_mpnn_utils.py:920-1100, :39-47) as
 * compute_fitness.py runs them: one forward per mutant under a random decoding order, pmpnn_ll = -(masked mean NLL).  Everything that
 * depends only on the structure (graph, edge features, the three encoder layers, the mutant-independent part of every decoder
 * layer's first Linear) is computed once by pgmi_mpnn_set_structure; a mutant costs the decoder only.  DESIGN.md 4.6h has the
 * restatement, the factorisation and the kernels.
 *
 * Weight blob: fp32, the tensors of ProteinMPNN(ca_only=False).state_dict() in its own order, each flattened row-major:
 *   features.embeddings.linear.weight [16, 66], .bias [16]; features.edge_embedding.weight [128, 416];
 *   features.norm_edges.weight, .bias [128]; W_e.weight [128, 128], .bias [128]; W_s.weight [21, 128];
 *   encoder_layers.{i}: norm1, norm2, norm3 (.weight, .bias [128] each); W1 [128, 384], W2 [128, 128], W3 [128, 128], W11 [128, 384],
 *     W12 [128, 128], W13 [128, 128], dense.W_in [512, 128], dense.W_out [128, 512] (.weight then .bias each)
 *   decoder_layers.{i}: norm1, norm2; W1 [128, 512], W2 [128, 128], W3 [128, 128], dense.W_in [512, 128], dense.W_out [128, 512]
 *   W_out.weight [21, 128], .bias [21]
 * Letters: the index in "ACDEFGHIKLMNPQRSTVWYX" (0 .. 20).
 * Limits: hidden width 128; num_edges 1 .. 48 (the v_48_* checkpoints' value); L <= 8192; at most PGMI_MPNN_MAX_LAYERS layers per stack; backbone_noise 0. */
#define PGMI_MPNN_MAX_LAYERS 8
typedef struct pgmi_mpnn_config {
    int32_t abi_version;                          /* = PGMI_ABI_VERSION */
    int32_t hidden;                               /* = 128 */
    int32_t num_edges;                            /* the checkpoint's num_edges (48); K = min(num_edges, L) */
    int32_t enc_layers, dec_layers;               /* 3, 3 */
    int32_t precision;                            /* PGMI_PREC_FP32 (the only mode) */
} pgmi_mpnn_config;
typedef struct pgmi_mpnn pgmi_mpnn;
/* pgmi_mpnn_weight_count: size of the blob above; -1 for a config the library refuses (pgmi_last_error).
 * pgmi_mpnn_create / pgmi_mpnn_destroy: the device-resident model (one HIP stream).
 * pgmi_mpnn_profile_model: the handle's profiling view for pgmi_profile_enable / _get / _reset / pgmi_synchronize (owned by the handle).
 *   Classes: PGMI_K_EMBED = the whole structure pass (one launch per pgmi_mpnn_set_structure; its GEMMs and LayerNorms are counted
 *   here and under no other class); of the decoder: PGMI_K_ATTENTION = the edge kernel, PGMI_K_GEMM_OUT = W3, PGMI_K_LAYERNORM = the
 *   two LayerNorm stages, PGMI_K_GEMM_FC1 / _FC2 = the FFN, PGMI_K_GEMM_QKV = the next layer's [A | P] projection, PGMI_K_HEAD =
 *   W_out + log-softmax, PGMI_K_SCORE = the per-mutant mean.
 * pgmi_mpnn_set_structure: X f32 [L][4][3] (N, CA, C, O; missing atoms 0), mask f32 [L] (0 where any of the four is missing, else 1),
 *   residue_idx i32 [L] (+100 per chain), chain_label i32 [L].  Neighbours: the K = min(num_edges, L) smallest adjusted CA distances
 *   of a row, ties broken by ascending distance, then ascending index (torch.topk leaves the order of ties open; the edges of a node
 *   are summed, so only the set matters).  Replaces the previous structure of the handle.
 * pgmi_mpnn_graph (test view): E_idx i32 [L][K], E f32 [L][K][128] (ProteinFeatures' output, after norm_edges); each nullable.
 * pgmi_mpnn_encoder (test view): h_V f32 [L][128], h_E f32 [L][K][128] after the last encoder layer; each nullable.
 * pgmi_mpnn_log_probs: S u8 [B][L], rank i32 [B][L] (rank[b][i] = position of residue i in mutant b's decoding order; edge (i, j) sees
 *   the sequence at j iff mask_i and rank_i > rank_j), out f32 [B][L][21].
 * pgmi_mpnn_scores: the production call: out f64 [B], out[b] = -(sum_i mask_i (-log p_i[S_i])) / sum_i mask_i, summed in fp64 in a
 *   fixed order; no log-probability leaves the device.  A mutant's result has the same bits whatever else is in the call.
 * pgmi_set_option("mpnn_max_rows", n): (mutant, residue) rows per chunk (0: 32768; clamped to 1 << 20; test hook, bit-neutral). */
int64_t pgmi_mpnn_weight_count(const pgmi_mpnn_config* cfg);
int pgmi_mpnn_create(const pgmi_mpnn_config* cfg, const float* weights, int64_t n_weights, int device, pgmi_mpnn** out);
void pgmi_mpnn_destroy(pgmi_mpnn* m);
pgmi_model* pgmi_mpnn_profile_model(pgmi_mpnn* m);
int pgmi_mpnn_set_structure(pgmi_mpnn* m, const float* X, const float* mask, const int32_t* residue_idx, const int32_t* chain_label,
                            int L);
int pgmi_mpnn_graph(pgmi_mpnn* m, int32_t* E_idx, float* E);
int pgmi_mpnn_encoder(pgmi_mpnn* m, float* h_V, float* h_E);
int pgmi_mpnn_log_probs(pgmi_mpnn* m, const uint8_t* S, const int32_t* rank, int B, float* out);
int pgmi_mpnn_scores(pgmi_mpnn* m, const uint8_t* S, const int32_t* rank, int B, double* out);

/* ---- S2F (ESM2 residue rows through a GVP-GNN on the C-alpha radius graph; its own handle and config, fp32) -----------------------
 * Replaces FusionNetwork / GVPGNN.forward and ResidueTypePrediction.inference (proteingym/baselines/S3F/s3f/{model,gvp,gvp_layer,
 * task}.py) as script/evaluate.py runs them: one forward per distinct set of masked positions.  The graph and W_e depend on the
 * structure only and are computed once by pgmi_s2f_set_structure, with every layer's edge share of the first message GVP.  DESIGN.md
 * 4.6n has the restatement and the factorisation.  S3F's surface branch is not computed.
 *
 * Weight blob: fp32, each tensor flattened row-major; a GVP is wh.weight, ws.weight, ws.bias, then (with vector outputs) wv.weight,
 * wsv.weight, wsv.bias:
 *   residue_embdding.weight [D, D]; W_v.0.scalar_norm.{weight, bias} [D]; W_v.1.ws.{weight [256, D], bias};
 *   W_e.0.scalar_norm.{weight, bias} [16]; W_e.1 = GVP (16, 1) -> (64, 1), h = 1;
 *   layers.{l}: conv.message_func.0 = GVP (576, 33) -> (256, 16), h = 33; .1, .2 = GVP (256, 16) -> (256, 16), h = 16;
 *     norm.0.scalar_norm.{weight, bias}, norm.1.scalar_norm.{weight, bias} [256];
 *     ff_func.0 = GVP (256, 16) -> (1024, 32), h = 32; ff_func.1 = GVP (1024, 32) -> (256, 16), h = 32;
 *   W_out.0.scalar_norm.{weight, bias} [256]; W_out.1 = GVP (256, 16) -> (256, 0), h = 16; linear.{weight [20, 256], bias [20]}
 * The 20 letters are in the order "GASPVTCILNDQKEMHFRYW".
 * Limits: node (256, 16), edge (64, 1), 16 RBFs, vector gate, activations (relu, none); node_in a multiple of 32; at most 8 layers;
 * L <= 8192 (pgmi_s2f_set_logprobs: L + 2 tokens inside the ESM2 model's workspace, no windows: the caller cuts the window). */
typedef struct pgmi_s2f_config {
    int32_t abi_version;                          /* = PGMI_ABI_VERSION */
    int32_t node_in;                              /* D: 1280 for ESM-2-650M */
    int32_t node_s, node_v, edge_s, edge_v, rbf;  /* = 256, 16, 64, 1, 16 */
    int32_t layers;                               /* 5 */
    int32_t max_neighbors;                        /* radius_graph's max_num_neighbors (32) */
    float radius;                                 /* 10.0 */
    float plddt_threshold;                        /* 70.0: rows with a smaller pLDDT take the ESM logits */
} pgmi_s2f_config;
typedef struct pgmi_s2f pgmi_s2f;
/* pgmi_s2f_weight_count: size of the blob above; -1 for a config the library refuses (pgmi_last_error).
 * pgmi_s2f_create: esm (nullable) is an ESM2 model of width node_in; the handle borrows it and its stream (destroy the handle first)
 *   and runs on its device.  Without one the handle has its own stream on `device` and serves pgmi_s2f_gvp_forward only.
 * pgmi_s2f_profile_model: the handle's profiling view (owned by the handle).  Classes: PGMI_K_EMBED = the structure pass,
 *   PGMI_K_GEMM_QKV = the input Linears and the per-node tables of the first message GVP, PGMI_K_ATTENTION = the per-edge row
 *   kernels (gather + norms, the GVPs' vector halves), PGMI_K_GEMM_OUT = the two per-edge ws GEMMs, PGMI_K_LAYERNORM = aggregation +
 *   tuple LayerNorm, PGMI_K_GEMM_FC1 / _FC2 = the feed-forward ws GEMMs, PGMI_K_KEPT_ROWS = the feed-forward GVPs' vector halves,
 *   PGMI_K_HEAD = W_out, the 20-way Linear and the log-softmax.  The ESM2 forward of pgmi_s2f_set_logprobs is timed on the ESM2
 *   model's own view.
 * pgmi_s2f_set_structure: pos f32 [L][3] (C-alpha), plddt f32 [L].  Edges (j -> i): per centre i the j in ascending index with
 *   squared distance < radius^2, self included, the first max_neighbors + 1 kept, then the self edge dropped; sorted by (i, j).
 * pgmi_s2f_graph (test view): n_edges; src, dst i32 [E]; e_s f32 [E][64], e_v f32 [E][3] (W_e's output); each nullable; E <= 33 L.
 * pgmi_s2f_gvp_forward: node_feat f32 [B][L][D], seq_logits f32 [B][L][20] -> lp f32 [B][L][20] (the 20-way log-softmax; low-pLDDT
 *   rows from seq_logits); node_s f32 [B][L][256] and node_v f32 [B][L][16][3] (nullable): the node state after the last layer.
 * pgmi_s2f_set_logprobs: the hot path.  wt_tokens i32 [T = L + 2] (<cls>, residues, <eos>), aa_cols i32 [20] (the token id of each
 *   of the 20 letters), position sets as CSR (set_off [n_sets + 1], set_pos: residue indices 0 .. L - 1, ascending inside a set).
 *   One ESM2 forward per set with the set's residues at <mask>, its emb_layer_norm_after rows through the GNN;
 *   out f32 [n_entries][20] = the row of (set, position); full (nullable) f32 [n_sets][L][20].  A set's bits do not depend on the
 *   other sets of the call or on the chunking.
 * pgmi_set_option("s2f_max_rows", n): rows per chunk, a masked copy costing max(E, L + 2) (0: 262144; test hook, bit-neutral). */
int64_t pgmi_s2f_weight_count(const pgmi_s2f_config* cfg);
int pgmi_s2f_create(const pgmi_s2f_config* cfg, const float* weights, int64_t n_weights, pgmi_model* esm, int device, pgmi_s2f** out);
void pgmi_s2f_destroy(pgmi_s2f* m);
pgmi_model* pgmi_s2f_profile_model(pgmi_s2f* m);
int pgmi_s2f_set_structure(pgmi_s2f* m, const float* pos, const float* plddt, int L);
int pgmi_s2f_graph(pgmi_s2f* m, int32_t* n_edges, int32_t* src, int32_t* dst, float* e_s, float* e_v);
int pgmi_s2f_gvp_forward(pgmi_s2f* m, const float* node_feat, const float* seq_logits, int B, float* lp, float* node_s, float* node_v);
int pgmi_s2f_set_logprobs(pgmi_s2f* m, const int32_t* wt_tokens, int T, const int32_t* aa_cols, const int32_t* set_off,
                          const int32_t* set_pos, int n_sets, float* out, float* full);

/* ---- S3F (S2F plus SurfGVP's surface half: a second GVP-GNN over the 16-NN graph of a surface point cloud; its own handle, fp32) ----
 * Replaces SurfGVP.forward (proteingym/baselines/S3F/s3f/gvp.py) under FusionNetwork / ResidueTypePrediction.inference as
 * script/evaluate.py runs them with config/evaluate/s3f.yaml.  The residue half is the S2F handle's code unchanged.  The surface half:
 * every surface point takes the ESM2 rows of its 3 nearest C-alpha atoms (surf_in_linear on [row | distance], mean), surf_in_mlp on
 * [mean | 42 features], surf_W_v, five surf_layers over the 16-NN graph (source = neighbour, target = centre, edge vector
 * p_source - p_centre), surf_W_out.  SurfGVP.residue2surface returns nothing, so the readout is the mean of surf_W_out's rows over ALL
 * surface points of the loader's batch, one [256] row added to every residue's W_out row; a pool group is that batch.  DESIGN.md 4.6p
 * has the restatement and the factorisation.  Producing the surface (points, HKS, curvatures) is the caller's.
 *
 * Weight blob: fp32, row-major, three parts:
 *   1. the S2F blob of the residue half (above), linear.{weight, bias} included;
 *   2. the surface MLP, folded on the host (H = 2 D): Wz [H, D] = W_1h W_x; Wsf [H, surf_feat + 1] = [W_1f | W_1h w_d]; b_1 [H];
 *      surf_in_mlp.2.{weight, bias} [H] (the LayerNorm); surf_in_mlp.4.{weight [D, H], bias [D]} -- where surf_in_linear.weight =
 *      [W_x | w_d] and surf_in_mlp.0.weight = [W_1h | W_1f];
 *   3. the surface GNN in the S2F blob's order with surf_W_v, surf_W_e, surf_layers, surf_W_out for W_v, W_e, layers, W_out, without
 *      residue_embdding and without linear.
 * Limits: S2F's; node_in <= 4096; surf_feat = 42, surf_res_neighbors = 3, surf_neighbors = 16; L >= 3; 17 <= Ns <= 1048576.
 * Workspace per masked copy of a chunk, in bytes: 4 Ns (2 D + 3670 + D) for the surface (the Ns x 2 D hidden of the MLP, the D-wide
 * rows and the GNN's stages; 30 KB per point at D = 1280) + 4 L (2 D + 2 D + 3670) for the residue half and Z. */
typedef struct pgmi_s3f_config {
    pgmi_s2f_config s2f;                          /* the residue half, and the dimensions both halves share */
    int32_t surf_feat;                            /* 42: HKS (32) | curvatures (10) */
    int32_t surf_res_neighbors;                   /* 3 */
    int32_t surf_neighbors;                       /* 16 */
} pgmi_s3f_config;
typedef struct pgmi_s3f pgmi_s3f;
/* pgmi_s3f_weight_count / _create / _destroy: as S2F's.
 * pgmi_s3f_profile_model(m, part): part 0 = the residue half's view (S2F's classes; PGMI_K_HEAD also holds the pooled row's add),
 *   part 1 = the surface half's view (owned by the handle).  Surface classes: PGMI_K_EMBED = the structure pass (both k-NN searches,
 *   surf_W_e, the structure term of the MLP, every layer's edge share), PGMI_K_GEMM_OUT = the surface MLP (Z, the row kernel, its
 *   second Linear, surf_W_v), PGMI_K_GEMM_QKV = the per-point tables of the first message GVP, PGMI_K_ATTENTION = the surface message
 *   kernel, PGMI_K_LAYERNORM, PGMI_K_GEMM_FC1 / _FC2, PGMI_K_KEPT_ROWS as S2F's, PGMI_K_HEAD = surf_W_out and the column sum.
 * pgmi_s3f_set_structure: pos, plddt as S2F's; surf_pos f32 [Ns][3], surf_feat f32 [Ns][42].  On the device, in fp32 squared
 *   distances with ties to the lower index: every point's 16 nearest other points (stored per centre in ascending source index) and its
 *   3 nearest C-alpha atoms (nearest first).
 * pgmi_s3f_graph (test view): the residue edges as pgmi_s2f_graph; src i32 [Ns][16]; res i32 [Ns][3]; res_dist f32 [Ns][3];
 *   e_s f32 [16 Ns][64], e_v f32 [16 Ns][3] (surf_W_e's output); each nullable.
 * pgmi_s3f_gvp_forward: node_feat, seq_logits, lp as S2F's for B copies; pool_off i32 [n_pools + 1]: consecutive copies
 *   [pool_off[g], pool_off[g + 1]) share one pooled row; surf_s f32 [B][Ns][256], surf_v f32 [B][Ns][16][3] (nullable): the surface
 *   node state after the last layer; pool_sum f32 [B][256] (nullable): per copy the column sum of surf_W_out's rows, in a fixed order
 *   (its count is Ns).  A copy's sum and everything before it have the same bits alone, in a batch and under any row cap.
 * pgmi_s3f_set_logprobs: as S2F's, with the pool groups over the sets.
 * pgmi_set_option("s2f_max_rows", n): a masked copy costs max(E, 16 Ns, L + 2) rows here. */
int64_t pgmi_s3f_weight_count(const pgmi_s3f_config* cfg);
int pgmi_s3f_create(const pgmi_s3f_config* cfg, const float* weights, int64_t n_weights, pgmi_model* esm, int device, pgmi_s3f** out);
void pgmi_s3f_destroy(pgmi_s3f* m);
pgmi_model* pgmi_s3f_profile_model(pgmi_s3f* m, int part);
int pgmi_s3f_set_structure(pgmi_s3f* m, const float* pos, const float* plddt, int L, const float* surf_pos, const float* surf_feat, int Ns);
int pgmi_s3f_graph(pgmi_s3f* m, int32_t* n_edges, int32_t* src, int32_t* dst, float* e_s, float* e_v, int32_t* surf_src, int32_t* surf_res,
                   float* surf_res_dist, float* surf_e_s, float* surf_e_v);
int pgmi_s3f_gvp_forward(pgmi_s3f* m, const float* node_feat, const float* seq_logits, int B, const int32_t* pool_off, int n_pools, float* lp,
                         float* surf_s, float* surf_v, float* pool_sum);
int pgmi_s3f_set_logprobs(pgmi_s3f* m, const int32_t* wt_tokens, int T, const int32_t* aa_cols, const int32_t* set_off,
                          const int32_t* set_pos, int n_sets, const int32_t* pool_off, int n_pools, float* out, float* full);

/* ---- UniRep (the 1900-unit multiplicative LSTM; its own handle and config, precision f16x3 or fp32) ---------------------------------
 * Replaces babbler1900's graph (proteingym/baselines/unirep/unirep.py:318-408: embedding, mLSTMCell1900.call :81-132 under
 * tf.nn.dynamic_rnn, Dense(25), tfa.seq2seq.sequence_loss) as unirep_inference.py:48-57 runs it.  DESIGN.md 4.6m has the restatement,
 * the folding and the step's structure.
 * Tokens (utils/data_utils.py:16-45): pad 0, M 1 .. L 21, O 22, X/Z/B/J 23, start 24, stop 25.  A formatted sequence is start + its
 * residues (format_seq(stop=False)): n + 1 tokens for n residues; the model reads the first n and predicts the last n (classes
 * target - 1; a target of 0 is masked out of the mean).
 * Weight blob: fp32, what the host folds from the checkpoint's arrays in float64 (proteingym_amd/unirep.py fold): with w' = w *
 * rsqrt(max(sum over rows of w^2, 1e-12)) * g per column (tf.nn.l2_normalize(axis=0) * g, unirep.py:119-122) and E the embedding,
 *   Tmx [26][H] = E wmx';  Tx [26][4 H] = E wx' + b;  wmh' [H][H];  wh' [H][4 H] (columns i | f | o | u);  Dense kernel [H][25];
 *   Dense bias [25].
 * H is padded to a multiple of 32 inside the library (zero weights and table entries: the padded units stay at c = h = 0).
 *
 * pgmi_unirep_weight_count: size of the blob above; -1 for a config the library refuses (pgmi_last_error): bf16 is refused.
 * pgmi_unirep_model_create / pgmi_unirep_destroy: the device-resident model (one HIP stream).
 * pgmi_unirep_profile_model: the handle's profiling view (owned by the handle).  Classes: PGMI_K_GEMM_FC1 = h_prev wmh, PGMI_K_LAYERNORM
 *   = the multiply by Tmx[token], PGMI_K_GEMM_FC2 = m wh, PGMI_K_ATTENTION = the gates, PGMI_K_HEAD = Dense + log-softmax, PGMI_K_EMBED
 *   = the rows' initial state, PGMI_K_SCORE = the per-sequence mean.
 * pgmi_unirep_set_target: tokens int32 [L + 1], the formatted target sequence.  Runs its L steps once and keeps, on the device, the
 *   state (c, h) after every step and the [L][25] log-probability rows.  L = 0 clears the target; after a failure no target is set.
 * pgmi_unirep_sequence_nll: n formatted sequences packed in tokens, sequence i = tokens[offsets[i] .. offsets[i+1]) (at least 2
 *   tokens).  out f64 [n]: the mean negative log-likelihood sum(xent * mask) / (sum(mask) + 1e-12), fp32 terms added in double, left to
 *   right.  With a target set and from_scratch == 0, a sequence's join step is the number of residues it shares with the target from
 *   the left (0 when its first token differs): it runs the steps join .. n_i - 1 from the target's state after `join` steps, and its
 *   terms before the join are read from the target's rows.  from_scratch != 0, or no target: every sequence runs from the zero state.
 *   Both give the same bits.  Internally the sequences are grouped by length, ordered by join step and cut into chunks of at most
 *   max_rows rows.  out_rowsteps (nullable): the (row, step) cell evaluations executed = sum of n_i - join_i.
 * pgmi_unirep_token_logprobs: tokens int32 [L] = the inputs; out f32 [L][25], row t = log_softmax(Dense(h_t)) after tokens[0 .. t].
 * pgmi_op_mlstm_step: one cell step of `rows` rows on caller-supplied state: h_prev, c_prev f32 [rows][H], tokens int32 [rows];
 *   h, c f32 [rows][Hp] and the pre-activations z f32 [rows][4][Hp] (i, f, o, u), Hp = H rounded up to 32, padding included.
 * pgmi_set_option("unirep_max_rows", n): rows per chunk (0: the config's max_rows, or 8192; test hook, bit-neutral). */
typedef struct pgmi_unirep_config {
    int32_t abi_version;                          /* = PGMI_ABI_VERSION */
    int32_t hidden;                               /* H: 1900 for the released model */
    int32_t vocab;                                /* = 26 */
    int32_t precision;                            /* PGMI_PREC_F16X3 or PGMI_PREC_FP32 */
    int32_t max_rows;                             /* rows per chunk; 0 = 8192 */
} pgmi_unirep_config;
typedef struct pgmi_unirep pgmi_unirep;
int64_t pgmi_unirep_weight_count(const pgmi_unirep_config* cfg);
int pgmi_unirep_model_create(const pgmi_unirep_config* cfg, const float* weights, int64_t n_weights, int device, pgmi_unirep** out);
void pgmi_unirep_destroy(pgmi_unirep* m);
pgmi_model* pgmi_unirep_profile_model(pgmi_unirep* m);
int pgmi_unirep_set_target(pgmi_unirep* m, const int32_t* tokens, int L);
int pgmi_unirep_sequence_nll(pgmi_unirep* m, const int32_t* tokens, const int64_t* offsets, int64_t n, int from_scratch, double* out,
                             int64_t* out_rowsteps);
int pgmi_unirep_token_logprobs(pgmi_unirep* m, const int32_t* tokens, int L, float* out);
int pgmi_op_mlstm_step(pgmi_unirep* m, const float* h_prev, const float* c_prev, const int32_t* tokens, int rows, float* h, float* c,
                       float* z);

/* ---- CARP (the dilated-convolution ByteNet masked LM; its own handle and config, precision f16x3 or fp32) ----------------------------
 * Replaces the ByteNetLM forward of sequence_models (microsoft/protein-sequence-models) as proteingym/baselines/carp_mif/
 * compute_fitness.py runs it at batch 1.  DESIGN.md 4.6o has the restatement and the list of readings made without that library.
 * Tokens: indices into the checkpoint's alphabet (proteingym_amd/carp.py PROTEIN_ALPHABET), no start or stop token.
 * Block n (dilation 2^(n mod (log2 r + 1))): x + PFF2(GELU(LN3(Conv(GELU(LN2(PFF1(GELU(LN1(x))))))))), LN eps ln_eps, erf-GELU; the
 * convolution is zero-padded at both ends of every sequence.  Head: last_norm, decoder, log-softmax over all vocab columns.
 * Weight blob (fp32, what proteingym_amd/carp.py blob_from_state folds and permutes):
 *   token table [vocab][d_model] = embedding rows through the 1x1 up-embedder, bias included;
 *   per block: LN1 w, b [d_model]; PFF1 [d_hidden][d_model], bias [d_hidden]; LN2 w, b [d_hidden];
 *              conv [d_hidden out][kernel_size][d_hidden in], bias [d_hidden]; LN3 w, b [d_hidden]; PFF2 [d_model][d_hidden], bias [d_model];
 *   last_norm w, b [d_model]; decoder [vocab][d_model], bias [vocab].
 *
 * pgmi_carp_weight_count: size of the blob; -1 for a config the library refuses (pgmi_last_error).
 * pgmi_carp_create / pgmi_carp_destroy: the device-resident model (one HIP stream).
 * pgmi_carp_profile_model: the handle's profiling view (owned by the handle).  Classes: PGMI_K_EMBED = the token table gather,
 *   PGMI_K_LAYERNORM = the three LayerNorm + GELU row kernels, PGMI_K_GEMM_FC1 = PFF1, PGMI_K_ATTENTION = the dilated convolution,
 *   PGMI_K_GEMM_FC2 = PFF2, PGMI_K_HEAD = row gather + last_norm + decoder + log-softmax, PGMI_K_SCORE = the per-sequence sum.
 * pgmi_carp_token_logprobs: B sequences packed in tokens (lens int32 [B], each >= 1); out f32 [sum lens][vocab].
 * pgmi_carp_masked_logprobs: one copy of wt_tokens [L] per listed position with that token replaced by mask_id; out f32
 *   [n_pos][vocab] = row positions[i] of copy i.  The row is gathered before last_norm: the head runs on n_pos rows.
 * pgmi_carp_sequence_loglik: out f64 [B] = the sum over a sequence's tokens of log p(x_t) from one unmasked forward, fp32 terms
 *   added in double, left to right.
 * All three cut their rows into chunks of at most max_rows rows between sequences (a longer sequence runs alone); a sequence's
 *   bits do not depend on the call's other sequences or on the chunking.  PGMI_EOVERFLOW: an activation left the fp16 range
 *   (precision f16x3); run in fp32.
 * pgmi_op_dilated_conv: the block's convolution alone, fp32 in and out (the split of x and W happens inside): x [M][C], W
 *   [C][taps][C] (the blob's permuted form), bias [C], seg_off int32 [n_seg + 1] ascending from 0 to M; precision f16x3 = the
 *   implicit-GEMM kernel, fp32 = im2col + the fp32 GEMM.
 * pgmi_op_ln_gelu: gelu_erf(LayerNorm(x)) per row, x [rows][D]; precision f16x3 = the split operand rebuilt as hi + lo 2^-11. */
typedef struct pgmi_carp_config {
    int32_t abi_version;                          /* = PGMI_ABI_VERSION */
    int32_t d_model, d_hidden, n_layers;          /* D; d_h = D / 2 (slim) or D; blocks */
    int32_t kernel_size;                          /* 5 */
    int32_t r;                                    /* the dilation cycle's last value, a power of two (128) */
    int32_t vocab, mask_id;                       /* rows of the token table; the index of '#' */
    int32_t precision;                            /* PGMI_PREC_F16X3 or PGMI_PREC_FP32 */
    int32_t max_rows;                             /* rows per chunk; 0 = 16384 */
    float ln_eps;                                 /* 1e-5 */
} pgmi_carp_config;
typedef struct pgmi_carp pgmi_carp;
int64_t pgmi_carp_weight_count(const pgmi_carp_config* cfg);
int pgmi_carp_create(const pgmi_carp_config* cfg, const float* weights, int64_t n_weights, int device, pgmi_carp** out);
void pgmi_carp_destroy(pgmi_carp* m);
pgmi_model* pgmi_carp_profile_model(pgmi_carp* m);
int pgmi_carp_token_logprobs(pgmi_carp* m, const int32_t* tokens, const int32_t* lens, int B, float* out);
int pgmi_carp_masked_logprobs(pgmi_carp* m, const int32_t* wt_tokens, int L, const int32_t* positions, int n_pos, float* out);
int pgmi_carp_sequence_loglik(pgmi_carp* m, const int32_t* tokens, const int32_t* lens, int B, double* out);
int pgmi_op_dilated_conv(int device, int precision, const float* x, const float* W, const float* bias, const int32_t* seg_off, int n_seg,
                         int C, int taps, int dilation, float* out);
int pgmi_op_ln_gelu(int device, int precision, const float* x, const float* w, const float* b, int rows, int D, float eps, float* y);
/* Times the f16x3 convolution kernel alone: seeded operands on the device, n_seg equal segments (M % n_seg == 0), two warm-up launches,
 * then the mean milliseconds of `iters` launches between two events. */
int pgmi_bench_dilated_conv(int device, int M, int n_seg, int C, int taps, int dilation, int iters, double* ms_per_launch);

/* ---- ProtSSN (an EGNN over the k-nearest C-alpha graph on ESM2's residue rows; its own handle and config; additions only, the ABI
 * version is unchanged) ------------------------------------------------------------------------------------------------------------
 * Replaces the GNN_model forward of proteingym/baselines/protssn (src/module/egnn/network.py EGNN, egnn_pytorch_geometric.py
 * EGNN_Sparse with mlp_num 2, dropout 0, no coordinate update, no norms, no soft edge) and the ESM2 rows PLM_model feeds it.  The
 * graph, its 93 edge attributes and the normalisation are built on the host (proteingym_amd/protssn.py); DESIGN.md 4.6q.
 * Dimensions: D = node_in, h = hidden (m_dim), A = edge_attr_dim; the first edge Linear is Hh = 2 (2 D + A + 1) wide.  Padded:
 *   Hp = roundup(Hh, 32), hp = roundup(h, 32), Ap = roundup(A + 1, 32); every pad row, column and bias is zero.
 * Weight blob (fp32, what proteingym_amd/protssn.py pack writes; nn.Linear [out, in]), per layer n of mpnn_layes:
 *   Wij [2 Hp][D]      edge_mlp.0.weight's columns 0 .. D (rows 0 .. Hp: they meet x[edge_index[1]], the neighbour) and D .. 2 D
 *                      (rows Hp .. 2 Hp: they meet x[edge_index[0]], the centre)
 *   We  [Hp][Ap]       its columns 2 D .. 2 D + A + 1: the edge attributes, then the squared distance of the normalised positions
 *   b1  [Hp]           edge_mlp.0.bias
 *   W2  [hp][Hp], b2 [hp]           edge_mlp.3
 *   W3  [2 D][D + hp], b3 [2 D]     node_mlp.0 (input columns x | m_i)
 *   W4  [D][2 D], b4 [D]            node_mlp.3
 *   then lin.weight [20][D], lin.bias [20].
 * pgmi_protssn_weight_count: size of that blob; -1 for a config the library refuses (pgmi_last_error).
 * pgmi_protssn_create / pgmi_protssn_destroy: the device-resident checkpoint (one HIP stream).
 * pgmi_protssn_profile_model: the handle's profiling view (owned by the handle).  Classes: PGMI_K_EMBED = the graph's upload
 *   (pgmi_protssn_set_graph) and the edge share e We^T + b1, PGMI_K_GEMM_QKV = the per-node tables x [Wi; Wj]^T,
 *   PGMI_K_ATTENTION = the edge-row kernel, PGMI_K_GEMM_OUT = the W2 product, PGMI_K_LAYERNORM = the aggregation (and the split of
 *   x), PGMI_K_GEMM_FC1 = W3, PGMI_K_KEPT_ROWS = the SiLU between W3 and W4, PGMI_K_GEMM_FC2 = W4 + residual, PGMI_K_HEAD = the
 *   20-way Linear and log(softmax + 1e-9).
 * pgmi_protssn_set_graph: the host-built, already normalised graph: pos f32 [L][3], n_edges edges (centre[e], neighbour[e]) =
 *   (edge_index[0], edge_index[1]), edge_attr f32 [n_edges][A].  The squared distance |pos[centre] - pos[neighbour]|^2 (fp32) and
 *   the CSR by neighbour (stable: ascending edge order per node) are formed here.  The arrays are free to go on return.
 * pgmi_protssn_forward: esm_rep f32 [L][D] -> lp f32 [L][20] = log(softmax(lin(x_6)) + 1e-9); hidden (nullable) f32 [L][D] = x_6.
 *   Edges are processed in chunks of edge_chunk; a row's bits do not depend on the chunk size.
 * pgmi_esm_residue_rows: one unmasked forward of tokens int32 [T] (<cls> + residues + <eos>) through an ESM2 model; rows f32
 *   [T - 2][D] = the residue rows after emb_layer_norm_after (HF EsmModel's last_hidden_state[1 : T - 1]).
 * pgmi_op_egnn_message: one layer's message and aggregation alone on host pointers: weights = a one-layer blob as above, the graph as
 *   pgmi_protssn_set_graph takes it, x f32 [L][D]; out f32 [L][h] = m_i (precision f16x3: the split operand rebuilt as hi + lo 2^-11).
 * PGMI_EINVAL before any device work: node_in not a multiple of 32 in 32 .. 8192, hidden outside 1 .. 4096, L < 2, an edge index
 *   outside 0 .. L - 1, a self edge, a non-finite value. */
typedef struct pgmi_protssn_config {
    int32_t abi_version;                          /* = PGMI_ABI_VERSION */
    int32_t node_in, hidden, layers;              /* 1280; 512, 768 or 1280; 6 */
    int32_t edge_attr_dim;                        /* 93 */
    int32_t precision;                            /* PGMI_PREC_F16X3 or PGMI_PREC_FP32 */
    int32_t edge_chunk;                           /* edges per chunk of the per-edge stages; 0 = 8192 */
} pgmi_protssn_config;
typedef struct pgmi_protssn pgmi_protssn;
int64_t pgmi_protssn_weight_count(const pgmi_protssn_config* cfg);
int pgmi_protssn_create(const pgmi_protssn_config* cfg, const float* weights, int64_t n_weights, int device, pgmi_protssn** out);
void pgmi_protssn_destroy(pgmi_protssn* m);
pgmi_model* pgmi_protssn_profile_model(pgmi_protssn* m);
int pgmi_protssn_set_graph(pgmi_protssn* m, const float* pos, int L, int n_edges, const int32_t* centre, const int32_t* neighbour,
                           const float* edge_attr);
int pgmi_protssn_forward(pgmi_protssn* m, const float* esm_rep, float* lp, float* hidden);
int pgmi_esm_residue_rows(pgmi_model* esm, const int32_t* tokens, int T, float* rows);
int pgmi_op_egnn_message(int device, const pgmi_protssn_config* cfg, const float* weights, int64_t n_weights, const float* pos, int L,
                         int n_edges, const int32_t* centre, const int32_t* neighbour, const float* edge_attr, const float* x, float* out);

/* ---- VespaG (a two-Linear head over ESM2-3B's residue rows, every protein of a FASTA; its own handle and config; additions only, the
 * ABI version is unchanged) ---------------------------------------------------------------------------------------------------------
 * Replaces the model side of proteingym/baselines/vespag/vespag: the embedder (data/embeddings.py: last_hidden_state[1 : L + 1] of one
 * unmasked forward per protein) and FNN([256], 2560, 20) (models/fnn.py, models/utils.py construct_fnn: Linear, Dropout -- identity in
 * eval --, LeakyReLU(0.01), Linear) with mask_non_mutations (utils/utils.py).  Tokenisation, mutations and the score are host work
 * (proteingym_amd/vespag.py); DESIGN.md 4.6s.
 * A library is what pgmi_pppl_create takes: tokens u8, concatenated, and seq_off i64 [n_seq + 1] with seq_off[0] = 0; every sequence
 *   <cls> + L_i >= 1 residues + <eos>.  Packed rows: [sum L_i][D] in the caller's order, sequence n at row seq_off[n] - 2 n.
 * pgmi_esm_packed_rows: emb_layer_norm_after of every residue row of the library through an ESM2 model.  Sequences run in descending
 *   length (stable), in chunks of max(1, cap / roundup(T, 32)) sequences, T = the chunk's longest, shorter ones <pad>-filled; cap =
 *   row_cap when 0 < row_cap < the workspace rows, else the workspace rows.  The last layer's row-local stages run on the residue rows
 *   only.  rows_host (nullable) f32 [sum L_i][D].  stats (nullable) i64 [3] = chunks, residue tokens + 2 per sequence, tokens with pads.
 *   The fp16 range flag is read on the device after every chunk (PGMI_EOVERFLOW).
 * pgmi_op_packed_rows_plan: that plan alone, on the host (no device is touched): order i32 [n_seq] = the sequences as they run,
 *   chunk_end i32 [n_seq] = the end (in `order`) of chunk i, *n_chunks, packed_off i64 [n_seq + 1] = the packed row of sequence n.
 * Weight blob (fp32, nn.Linear [out, in]): net.0.weight [hidden][input_dim], net.0.bias [hidden], net.3.weight [20][hidden],
 *   net.3.bias [20].
 * pgmi_vespag_create: esm (nullable) is an ESM2 model of width input_dim and the config's precision; the handle borrows it and its
 *   stream (destroy the handle first).  Without it the handle has a stream of its own and runs pgmi_vespag_head only.
 * pgmi_vespag_profile_model: the handle's profiling view (owned by the handle).  Classes: PGMI_K_LAYERNORM = the split of the rows
 *   (f16x3), PGMI_K_GEMM_FC1 = the first Linear, PGMI_K_HEAD = the row kernel.  The encoder is timed on the ESM2 model's own profile,
 *   where PGMI_K_SCORE = the scatter of a chunk's rows to their packed place.
 * wt_cols i32 [rows]: the column (0 .. 19, AMINO_ACIDS = "ACDEFGHIKLMNPQRSTVWY") of each row's wild type, which gets exact 0.0
 *   (mask_non_mutations); -1 leaves the row as it is.
 * pgmi_vespag_landscapes: packed rows of the library, then the head, without leaving the device: y_host f32 [sum L_i][20];
 *   rows_host (nullable) f32 [sum L_i][input_dim].
 * pgmi_vespag_head: the head on pre-computed rows_host f32 [R][input_dim] -> y_host f32 [R][20]; bit-equal to pgmi_vespag_landscapes
 *   on the same rows.  The rows come from a file, so every one of the R x input_dim values is read on the host before the upload (one
 *   serial pass) and a non-finite one is PGMI_EINVAL; the packed route checks its rows on the device instead and refuses one the same way
 *   in precision fp32 (f16x3: PGMI_EOVERFLOW).  Both entries read the [R][20] result on the host: a non-finite value is PGMI_EOVERFLOW.
 * pgmi_op_vespag_head: the head alone on host pointers (W1 [hidden][input_dim], b1, W2 [20][hidden], b2).
 * PGMI_EINVAL before any device work: input_dim or hidden not a multiple of 32 (32 .. 8192, 32 .. 768), out != 20, a non-ESM2 model,
 *   a width or precision that differs, a sequence below 3 tokens, a token id outside the alphabet or <pad>, the longest sequence + 31
 *   above the workspace rows, a wt_cols value outside -1 .. 19, a non-finite row. */
typedef struct pgmi_vespag_config {
    int32_t abi_version;                          /* = PGMI_ABI_VERSION */
    int32_t input_dim, hidden, out;               /* 2560, 256, 20 */
    int32_t precision;                            /* PGMI_PREC_F16X3 or PGMI_PREC_FP32 */
    float negative_slope;                         /* 0.01 */
} pgmi_vespag_config;
typedef struct pgmi_vespag pgmi_vespag;
int pgmi_esm_packed_rows(pgmi_model* esm, const uint8_t* tokens, const int64_t* seq_off, int64_t n_seq, int row_cap, float* rows_host,
                         int64_t* stats);
int pgmi_op_packed_rows_plan(const int64_t* seq_off, int64_t n_seq, int row_cap, int32_t* order, int32_t* chunk_end, int32_t* n_chunks,
                             int64_t* packed_off);
int64_t pgmi_vespag_weight_count(const pgmi_vespag_config* cfg);
int pgmi_vespag_create(const pgmi_vespag_config* cfg, const float* weights, int64_t n_weights, pgmi_model* esm, int device, pgmi_vespag** out);
void pgmi_vespag_destroy(pgmi_vespag* m);
pgmi_model* pgmi_vespag_profile_model(pgmi_vespag* m);
int pgmi_vespag_landscapes(pgmi_vespag* m, const uint8_t* tokens, const int64_t* seq_off, int64_t n_seq, const int32_t* wt_cols, float* y_host,
                           float* rows_host);
int pgmi_vespag_head(pgmi_vespag* m, const float* rows_host, const int32_t* wt_cols, int64_t R, float* y_host);
int pgmi_op_vespag_head(int device, int precision, const float* rows, const float* W1, const float* b1, const float* W2, const float* b2,
                        const int32_t* wt_cols, int R, int input_dim, int hidden, float slope, float* y);

/* ---- ProSST structure quantizer (one local subgraph per residue through a GVP-GNN, k-means tokens; its own handle, fp32) -----------
 * Replaces PdbQuantizer's model side (proteingym/baselines/prosst/prosst/structure/{quantizer.py, encoder/gvp.py, encoder/layer.py};
 * venusrem/structure is the same code): generate_graph's features, generate_pos_subgraph(pure_subgraph = True, interval 1),
 * AutoGraphEncoder.get_embedding in eval mode, scatter_mean, F.normalize and KMeans.predict.  DESIGN.md 4.6t has the restatement, the
 * stand-ins and the sharing.  The ProSST transformer itself is not computed: its code is not in the reference tree.
 *
 * Weight blob: fp32, each tensor flattened row-major; a GVP is wh.weight, ws.weight, ws.bias, then (with vector outputs) wv.weight
 * (vector_gate = False: no wsv):
 *   W_v.0.scalar_norm.{weight, bias} [20]; W_v.1 = GVP (20, 3) -> (256, 32), h = 32;
 *   W_e.0.scalar_norm.{weight, bias} [32]; W_e.1 = GVP (32, 1) -> (64, 2), h = 2;
 *   layers.{l}: conv.message_func.0 = GVP (576, 66) -> (256, 32), h = 66; .1, .2 = GVP (256, 32) -> (256, 32), h = 32;
 *     norm.0.scalar_norm.{weight, bias}, norm.1.scalar_norm.{weight, bias} [256];
 *     ff_func.0 = GVP (256, 32) -> (1024, 64), h = 64; ff_func.1 = GVP (1024, 64) -> (256, 32), h = 64;
 *   W_out.0.scalar_norm.{weight, bias} [256]; W_out.1 = GVP (256, 32) -> (256, 0), h = 32.
 * Limits: node (256, 32), edge (64, 2), at most 8 layers, max_nodes <= 40, 1 <= L <= 8192 and L != 3 (the reference's torch.cross
 * without dim runs over the residue axis there), K <= 8192 centres of width 256. */
typedef struct pgmi_prosst_config {
    int32_t abi_version;                          /* = PGMI_ABI_VERSION */
    int32_t node_s, node_v, edge_s, edge_v;       /* = 256, 32, 64, 2 */
    int32_t layers;                               /* 6 */
    int32_t max_nodes;                            /* 40: nodes kept of a subgraph with more than `threshold` candidates */
    int32_t threshold;                            /* 30 */
    float radius;                                 /* 10.0 */
} pgmi_prosst_config;
typedef struct pgmi_prosst pgmi_prosst;
/* pgmi_prosst_weight_count: size of the blob above; -1 for a config the library refuses (pgmi_last_error).
 * pgmi_prosst_create / _destroy: a handle with a stream of its own on `device`.
 * pgmi_prosst_profile_model: the handle's profiling view (owned by the handle).  Classes: PGMI_K_EMBED = the structure pass on the
 *   device (every layer's edge tables, layer 0's messages over the global edges), PGMI_K_GEMM_QKV = the per-node tables of the first
 *   message GVP, PGMI_K_ATTENTION = the message kernel, PGMI_K_LAYERNORM = aggregation, tuple LayerNorms and the feed-forward operand
 *   rows, PGMI_K_GEMM_FC1 / _FC2 = the feed-forward ws GEMMs, PGMI_K_KEPT_ROWS = the feed-forward GVPs' vector halves, PGMI_K_HEAD =
 *   W_out, the mean per subgraph and the normalisation, PGMI_K_SCORE = the codebook assignment.
 * pgmi_prosst_set_structure: X f32 [L][4][3] = N, CA, C, O.  On the host, in double on these float32 values: CA-CA distances; the
 *   global edges (a -> b), a != b, d < radius, in row-major order of (a, b), a the source and b the target; per anchor i the
 *   subgraph's nodes = row i of the distances sorted ascending (ties: lower index first), the first 50, those with d < radius, the
 *   first max_nodes of them when more than `threshold` remain, sorted by index; a subgraph's edges = the global edges between its
 *   nodes, with the global edge's features.  W_v (once per residue) and W_e (once per global edge) run there too.
 * pgmi_prosst_subgraphs (test view; every pointer nullable): counts i64 [3] = E global edges, N node copies, ES subgraph edges;
 *   edges i32 [2][E] = a then b; e_s f32 [E][64], e_v f32 [E][2][3] = W_e's output; node_off i32 [L + 1], nodes i32 [N] = the node
 *   CSR; edge_off i32 [L + 1], edge_gid i32 [ES] = per subgraph the global edge of each of its edges, ascending (the reference's
 *   row-major order over the sorted node set).
 * pgmi_op_prosst_subgraphs: the same host graph pass without a handle or a device (cfg's radius, max_nodes and threshold; no weights):
 *   the view above without W_e's output, and the arrays the kernels read: in_off i32 [N + 1], in_gid i32 [ES], in_src i32 [ES] = per
 *   node copy (node q of anchor i, in CSR order) its incoming subgraph edges p -> q in ascending p, as (global edge, copy of p).
 * pgmi_prosst_embed: the encoder on every subgraph; out f32 [L][256] = the L2-normalised mean of W_out's rows, pooled (nullable)
 *   f32 [L][256] the mean before the normalisation; node_s f32 [n][256] / node_v f32 [n][32][3] (nullable): the node state after the
 *   last layer of the n nodes of subgraph `sub`.  Layer 0's messages are computed once per global edge (every copy of a residue
 *   enters it with the same state); from layer 1 on the work is per node copy.  A subgraph's bits do not depend on the chunking.
 * pgmi_prosst_assign: tokens i32 [L] = argmin_k |c_k|^2 - 2 x.c_k over centres f32 [K][256] in fp32, the lowest index on a tie, for
 *   the embeddings of the last pgmi_prosst_embed (kept on the device): any number of codebooks per encoder pass.
 * pgmi_op_prosst_assign: the same assignment on host embeddings emb f32 [n][256]; bit-equal to pgmi_prosst_assign on the same rows.
 *   At most 2^20 rows and 2^28 products n K per call (the [n][K] table is one allocation); more is refused: call it in slices.
 * pgmi_set_option("prosst_max_rows", n): node copies per chunk (0: 32768; test hook, bit-neutral).
 * pgmi_set_option("prosst_share_layer0", 0 / 1): 0 runs layer 0 per node copy like the others (measurement only). */
int64_t pgmi_prosst_weight_count(const pgmi_prosst_config* cfg);
int pgmi_prosst_create(const pgmi_prosst_config* cfg, const float* weights, int64_t n_weights, int device, pgmi_prosst** out);
void pgmi_prosst_destroy(pgmi_prosst* m);
pgmi_model* pgmi_prosst_profile_model(pgmi_prosst* m);
int pgmi_prosst_set_structure(pgmi_prosst* m, const float* X, int L);
int pgmi_prosst_subgraphs(pgmi_prosst* m, int64_t* counts, int32_t* edges, float* e_s, float* e_v, int32_t* node_off, int32_t* nodes,
                          int32_t* edge_off, int32_t* edge_gid);
int pgmi_op_prosst_subgraphs(const pgmi_prosst_config* cfg, const float* X, int L, int64_t* counts, int32_t* edges, int32_t* node_off,
                             int32_t* nodes, int32_t* edge_off, int32_t* edge_gid, int32_t* in_off, int32_t* in_gid, int32_t* in_src);
int pgmi_prosst_embed(pgmi_prosst* m, float* out, float* pooled, int sub, float* node_s, float* node_v);
int pgmi_prosst_assign(pgmi_prosst* m, const float* centres, int K, int32_t* tokens);
int pgmi_op_prosst_assign(int device, const float* emb, int64_t n, const float* centres, int K, int32_t* tokens);

/* ---- MSA Transformer (arch PGMI_ARCH_MSA; vocab 33, head_dim 64, precision f16x3) --------------------
 * Replaces MSATransformer.forward (proteingym/baselines/esm/esm/model/msa_transformer.py:146-205; tied
 * row attention esm/axial_attention.py:33-168, column attention :171-297) and the masked-marginals loop
 * of compute_fitness.py:380-394.
 * Config: max_positions = args.max_positions (1024), emb_layer_norm_before = 1, token_dropout = 0,
 * max_rows >= roundup(R,32) * roundup(T,32) for the largest token grid.
 * Weight blob (fp32, nn.Linear [out,in]), state-dict names after the loader's row/column swap
 * (pretrained.py:110-116):
 *   embed_tokens.weight [33,D] (the tied lm_head.weight), embed_positions.weight [max_positions+2, D],
 *   msa_position_embedding [1024, D] (a [1024,1] parameter is broadcast by the host),
 *   emb_layer_norm_before.{weight,bias};
 *   per layer: row_self_attention.{layer_norm.{weight,bias}, layer.q_proj.{weight,bias}, k_proj, v_proj,
 *              out_proj}, column_self_attention.{same}, feed_forward_layer.{layer_norm.{weight,bias},
 *              layer.fc1.{weight,bias}, layer.fc2.{weight,bias}};
 *   emb_layer_norm_after.{weight,bias}; lm_head.dense.{weight,bias}; lm_head.layer_norm.{weight,bias};
 *   lm_head.bias [33].
 *
 * pgmi_msa_token_logprobs: log_softmax(model(tokens[None])["logits"])[0] for one alignment.
 *   tokens int32 [R][T] (<cls> first in every row, no <pad>), out float32 [R][T][33].
 * pgmi_msa_masked_logprobs: for i < n, mask column positions[i] of the FIRST row, run the columns
 *   [starts[i], min(T, starts[i] + window)) of all rows, keep log-probabilities of that cell:
 *   out float32 [n][33].  (window = T when T <= 1024; else 1024 with starts from pgmi_optimal_window,
 *   exactly as compute_fitness.py:383-388 crops.)  The alignment stays resident in HBM across the n forwards. */
int pgmi_msa_token_logprobs(pgmi_model* m, const int32_t* tokens, int R, int T, float* out);
int pgmi_msa_masked_logprobs(pgmi_model* m, const int32_t* tokens, int R, int T, int window,
                             const int32_t* positions, const int32_t* starts, int n, float* out);

/* ---- alignment pre-processing ---------------------------------------------
 * Cluster sizes (inverse sequence weights) of an alignment: replaces the numba kernel
 * calc_num_cluster_members_nogaps_parallel (proteingym/utils/weights.py:164-216, called by
 * calc_weights_fast :13-53) and MSA_processing.compute_weight
 * (baselines/tranception/tranception/utils/msa_utils.py:341-352).
 *   matrix  int8 [N][L]  symbols mapped to 0..29; invalid_value marks gaps / lower-case columns
 *   counts_out int32 [N] #{j : matches(i,j) / nongap(i) > identity_threshold}, self included;
 *                        0 for a sequence with no valid symbol (the reference gives it weight 0)
 *   kernel_ms  optional: duration of the pair-count kernel (HIP events on its stream)
 * The double-precision predicate of the reference is evaluated exactly (per non-gap length on the
 * host, integer compares on the device): results are bit-identical to the reference's counts. */
int pgmi_msa_cluster_counts(int device, const int8_t* matrix, int64_t N, int64_t L, int invalid_value,
                            double identity_threshold, int32_t* counts_out, double* kernel_ms);
/* Neighbour counts of PoET's homology weights (proteingym/baselines/PoET/poet/msa/sampling.py _compute_homology_weights, numpy path):
 * the same pair kernel with the predicate
 *   counts_out[i] = #{j : 1 - matches(i,j) / nongap(i) <= theta}, self included, in the reference's float64 arithmetic
 * (evaluated on the host once per non-gap length, integer compares on the device: counts equal the reference's exactly).  A gap never
 * matches anything.  A row with no non-gap symbol is PGMI_EINVAL (the reference divides by zero there).  theta in [0, 1]. */
int pgmi_msa_neighbor_counts(int device, const int8_t* matrix, int64_t N, int64_t L, int invalid_value,
                             double theta, int32_t* counts_out, double* kernel_ms);

#ifdef __cplusplus
}
#endif
#endif /* PGMI_H */
