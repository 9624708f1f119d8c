// Internal header of the C ABI's translation units (api_*.hip): the device-resident model / assay / library state behind the opaque
// handles of include/pgmi.h and the host-side helpers they share.  Nothing here is part of the ABI.
//   api_model.hip        errors, configuration and token checks, weight split, linear() / qkv_launch() (a model's GEMMs as a
//                        GemmLaunch), prefix_launch() / alloc_prefix_cache(), model create (validation, per-arch dispatch, workspace) /
//                        destroy, options, profiling
//   api_esm.hip          ESM-1b / ESM-1v / ESM2 weights (create_esm), the encoder forward of the ESM family and ESM C (run_encoder,
//                        run_head), masked-marginals assays, pseudo-ppl libraries
//   api_tranception.hip  Tranception weights, prefix-shared chunks; token log-probs and sequence log-likelihoods (on run_decoder)
//   api_progen2.hip      ProGen2 weights (GPT-J rotary, bias-free projections), its 25-column amino-acid head and sequence
//                        log-likelihoods
//   api_gpt.hip          causal decoder: RITA / ProtGPT2 weights, the decoder body of RITA / ProtGPT2 / ProGen2 / Tranception (sequential
//                        or ProGen2's parallel residual; dense or Tranception's ragged prefix-shared rows) and the sublayers it shares
//                        with the packed decoders (self_attention, out_proj, ffn), narrow and wide LM heads, the log-likelihood tail
//                        (loglik_tail), the checks and token log-probs of RITA / ProtGPT2 / ProGen2; RITA / ProtGPT2 log-likelihoods
//   api_poet.hip         PoET: tiered (within-sequence, then sequence-of-sequences) causal decoder on attention_prefix.hip over the
//                        prefix cache of a prompt; score_packed, the driver of its and ESM-IF1's token log-prob / log-likelihood
//                        entries (chunks cut by packed_chunks.h pack_chunk)
//   api_esmif1.hip       ESM-IF1's decoder: self_attention, then cross-attention over the prefix cache of one encoded backbone
//                        (attention_prefix.hip); its entries run on score_packed
//   api_progen3.hip      ProGen3 weights (RMSNorm, grouped-query attention as replicated K/V projection rows, per-expert FC1 / FC2), its
//                        feed-forward block on moe.hip (pg3_ffn, moe_ffn), the C entries; it runs on run_decoder
//   api_esmc.hip         ESM C weights (QK-LayerNorm, SwiGLU, scaled residual, untied 64-column head); it runs on run_encoder
//   api_esm3.hip         ESM3 weights (ESM C's blocks, the folded multi-track embedding, block 0's geometric attention branch), the
//                        bound window structure, geom_branch (run_encoder calls it after block 0's attention); it runs on run_encoder
//   api_saprot.hip       SaProt: ESM2's weights and encoder with a 446-token vocabulary; position-set rows and the grouped log-softmax head
//   api_mulan.hip        MULAN: ESM2's (or SaProt's) weights and encoder behind a structure adapter -- Linear(7 -> D) over per-residue
//                        angle rows, one encoder layer without rotary, LayerNorm -- added to the word embeddings; position-set rows
//   api_eve.hip          EVE / DeepSequence: its own handle (pgmi_eve), blob walk, encoder, one ELBO sample, noise seam, the sampling loop
//   api_mpnn.hip         ProteinMPNN: its own handle (pgmi_mpnn), blob walk, the per-structure pass (graph, features, encoder, hoisted
//                        decoder tables), the per-batch decoder and head
//   api_carp.hip         CARP: its own handle (pgmi_carp), blob walk, the ByteNet forward over packed sequences (conv_f16.hip), masked
//                        rows / token log-probs / sequence log-likelihoods, the convolution's and the row kernel's op entries
//   api_protssn.hip      ProtSSN: its own handle (pgmi_protssn), blob walk, the graph of one structure, the EGNN forward in edge chunks
//                        (egnn.hip around the existing GEMMs), the ESM2 residue rows that feed it, the message op entry
//   api_vespag.hip       VespaG: the packed residue rows of a library of sequences through an ESM2 model (length-sorted chunks, the residue
//                        rows as run_encoder's keep list, the scatter to the caller's order), its own handle (pgmi_vespag), blob walk,
//                        the head on packed rows (vespag.hip after one GEMM), the head's op entry
//   side handles         what the handles outside pgmi_model (pgmi_eve, pgmi_mpnn, pgmi_unirep, pgmi_s2f, pgmi_carp, pgmi_protssn, pgmi_vespag; pgmi_s3f
//                        holds two pgmi_s2f) share, in api_model.hip and below: side_open (blob, device and stream of a create),
//                        BlobCursor, linear(), DevBuf / reserve_all (grow-only workspace), side_sync, overflow_error, side_release
//   api_msa.hip          MSA Transformer weights and forward (tied row attention, column attention)
//   api_host.hip         host-only entries: mutant parser, table -> scores, optimal window
//   api_ops.hip          single-op and timing entries for the numerics tests and the A/B scripts
#pragma once
#include <math.h>
#include <stdlib.h>
#include <cmath>
#include <algorithm>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "common.h"
#include "gemm16x_kernel.h"          // XMap (the tied row attention's operand maps); no kernel is instantiated here
#include "packed_chunks.h"           // SegPlan, pack_chunk

namespace pgmi {

// 16-bit operand of one Linear weight [N,K]: f16x3 = fp16 (hi, lo) of W*2^s in the K-interleaved layout (common.h
// ki_off: per row, groups of 32 hi halfs + 32 lo halfs), bf16 = one plane; out_scale = 2^-s is applied in the GEMM epilogue.
// They are GemmLaunch's W and out_scale (common.h).
struct W16 {
    unsigned short* p = nullptr;
    float out_scale = 1.0f;
};

struct Layer {
    float *ln1_w, *ln1_b, *wqkv, *bqkv, *wo, *bo, *ln2_w, *ln2_b, *w1, *b1, *w2, *b2;
    W16 wqkv16, wo16, w116, w216;
    int ffn = 0;                  // the layer's own FC1 / FC2 width where it is not cfg.ffn_dim (MULAN's adapter: 4 D); 0: cfg.ffn_dim
    float* conv = nullptr;        // Tranception: [3][4][64][8] right-aligned 7-tap filters + bias (attention_f16.hip)
    // MSA Transformer: ln1/wqkv/wo = tied row attention, c_* = column attention, ln2/w1/w2 = feed forward
    float *c_ln_w = nullptr, *c_ln_b = nullptr, *c_bqkv = nullptr, *c_bo = nullptr;
    W16 c_wqkv16, c_wo16;
    // ESM-IF1 decoder: ln1/wqkv/wo = causal self-attention, c_ln / c_wq16 + c_bq (q, from the decoder rows) / c_wqkv16 + c_bqkv (zero q
    // block | k | v, from the encoder rows: [3 Da, D_enc]) / c_wo16 = encoder_attn, ln2/w1/w2 = feed forward
    float* c_bq = nullptr;
    W16 c_wq16;
    float *q_ln = nullptr, *k_ln = nullptr;       // ESM C: q_ln (times 1/8) / k_ln weights
    // ProGen3 with more than one expert: the router's fp32 gate [E,D]; per expert FC1 (gated: w1 | w3 in EPI_SWIGLU's 32 gate | 32 up
    // row blocks, [2F,D]; else w1 [F,D]) and FC2 [D,F].  One expert: w116 / w216 as for every other model.
    float* gate = nullptr;
    std::vector<W16> ew1, ew2;
    // ESM3 block 0: the geometric attention branch -- s_norm's weight, proj [15 Hv, D], out_proj [D, Kp] (its 3 Hv input columns
    // zero-padded to Kp = roundup(3 Hv, 32); 1/s on its out_scale), softplus of the two per-head scales
    float *g_norm_w = nullptr, *g_wrot = nullptr, *g_wdist = nullptr;
    W16 g_proj16, g_out16;
};

struct ProfEvent {
    hipEvent_t start, stop;
    int cls;
};

// The shared prefix of attention_prefix.hip's launches, per layer, in their operand layout: planes [layers][K | V^T][2 planes][plane]
// halfs, plane = Da * pitch, for a prefix of at most pitch = roundup(max_positions, 32) rows (0: the model has no cache); `rows` of
// them are valid (0: no prefix is set).  meta, for a workspace of cap = max_rows rows: two SegPlan slots (upload_plan) of
// plan_ints(cap) = 3 cap + 2 ints -- seg_off [cap + 1] and a pad, ent_seg [cap], ent_tile [cap]: a plan has at most cap segments and
// cap tiles -- then the sequence offsets of a log-likelihood chunk, [cap + 1] and 3 of pad: meta_ints(cap) = 7 cap + 8.
struct PrefixCache {
    unsigned short* planes = nullptr;
    size_t pitch = 0, plane = 0, cap = 0;
    int rows = 0;
    int32_t* meta = nullptr;
    static size_t plan_ints(size_t cap) { return 3 * cap + 2; }
    static size_t meta_ints(size_t cap) { return 2 * plan_ints(cap) + cap + 4; }
    unsigned short* k(int l) const { return planes ? planes + (size_t)l * 4 * plane : nullptr; }
    unsigned short* vt(int l) const { return planes ? k(l) + 2 * plane : nullptr; }
    int32_t* plan(int slot) const { return meta + (size_t)slot * plan_ints(cap); }
    int32_t* seq_off() const { return plan(2); }
};

}  // namespace pgmi

using namespace pgmi;

struct pgmi_assay;
struct pgmi_pppl;

struct pgmi_model {
    pgmi_config cfg;
    int device = 0;
    hipStream_t stream = nullptr;
    std::vector<void*> allocs;          // everything to hipFree
    std::vector<pgmi_assay*> assays;    // live assays created on this model (orphaned on destroy)
    std::vector<pgmi_pppl*> pppls;      // live pseudo-ppl libraries (same rule)
    // weights
    float *embed_tokens = nullptr, *embed_positions = nullptr;
    float *lnb_w = nullptr, *lnb_b = nullptr, *lna_w = nullptr, *lna_b = nullptr;
    float *hd_w = nullptr, *hd_b = nullptr, *hln_w = nullptr, *hln_b = nullptr;
    // the log-softmax head [V,D] and its bias [V]: embed_tokens (ESM family, MSA Transformer: tied) or an untied matrix (ESM C, and the
    // narrow causal-decoder heads; RITA's and Tranception's bias is `zeros`)
    float *head_w = nullptr, *head_b = nullptr;
    std::vector<Layer> layers;
    W16 hd16;
    // what the shared layer loops (run_encoder, run_decoder) read per model: FC1's epilogue (common.h Epilogue) and output columns
    // (ffn_dim; 2 ffn_dim for ESM C's SwiGLU); the encoder's embedding as a plain table gather (ESM C: no token dropout, position
    // table or <pad> zeroing); the causal attention's ALiBi slopes (Tranception's grouped table; `zeros` for the others)
    int fc1_epi = EPI_GELU, fc1_cols = 0;
    bool embed_gather = false;
    // what the token checks and the embedding read per model: the <mask> id and the number of token ids (the ESM alphabet's 32 / 33;
    // SaProt's tokenizer has <mask> at 4, 446 ids, and an ordinary residue token at 32)
    int mask_id = PGMI_TOK_MASK, n_token_ids = PGMI_VOCAB;
    float* slopes = nullptr;
    float* tr_prior = nullptr;                          // device copy of the retrieval log-prior [P,V]
    size_t tr_prior_cap = 0;
    int32_t* tr_meta = nullptr;                         // prefix-shared scoring: the chunk's index arrays (TrChunk)
    size_t tr_meta_cap = 0;
    // ProGen2: rotary_dim and the amino-acid rows 5..29 of its head
    int pg2_rotary = 0;
    float *pg2_aa_w = nullptr, *pg2_aa_b = nullptr;
    // causal decoder (api_gpt.hip; ProGen2 and Tranception run on it too): the residual order, the wide head -- the f16x3 planes of wte
    // zero-padded to gpt_Vp = roundup(V, 64) rows and its fp32 logits [gpt_head_rows][gpt_Vp] (V <= 64: head_w / head_b) --;
    // per-sequence sums.  Rotary: rot_cos / rot_sin uploaded at creation (RITA, ProGen2); learned positions: embed_positions (ProtGPT2)
    int gpt_Vp = 0, gpt_head_rows = 0;
    bool parallel_residual = false;     // ProGen2: attention and MLP both read ln_1's output; else ln_2 follows the attention
    float* gpt_logits = nullptr;
    W16 gpt_head16;
    double* gpt_sum = nullptr;
    // ProGen3 (api_progen3.hip): RMSNorm in place of LayerNorm in the decoder loop and the head; the expert block's dimensions and
    // workspace (MoeWs: slots = max_rows * top_k + n_experts * the GEMM's row tile); the routing of the last forward per layer
    bool rms_norm = false;
    int pg3_E = 0, pg3_k = 0, pg3_gated = 0;
    struct MoeWs {
        int32_t *ids = nullptr, *slot = nullptr, *blk_cnt = nullptr, *blk_base = nullptr, *counts_seg = nullptr;   // ids: [layers][max_rows * top_k]
        float *wts = nullptr, *y = nullptr, *t32 = nullptr;       // wts: [layers][max_rows * top_k]; y [slots][D]; t32 [slots][F] (non-gated; one expert: [max_rows][F])
        unsigned short *a16 = nullptr, *g16 = nullptr;            // [slots][2 D], [slots][2 F] halfs
        int32_t* counts_host = nullptr;                           // pinned [2 E + 1]
        size_t layer_stride = 0;
    } moe;
    // MSA Transformer
    float* msa_pe = nullptr;                            // msa_position_embedding [1024, D]
    float* xt = nullptr;                                // residual stream in column-major token order
    int32_t *msa_full = nullptr, *msa_kv_len = nullptr; // device copy of the MSA token grid; [C] = R
    size_t msa_full_cap = 0;
    float *tied_part = nullptr, *tied_p = nullptr, *tied_vt = nullptr;   // split-K scores, probabilities, V^T
    size_t tied_part_cap = 0, tied_p_cap = 0, tied_vt_cap = 0;
    int msa_kv_R = 0, msa_kv_C = 0;
    float ln_eps = 1e-5f;
    // the narrow head (narrow_head) runs the model's last LayerNorm lna first: every causal decoder and ESM-IF1; PoET by its checkpoint
    bool final_norm = false;
    // PoET (the prompt's tier-2 K, rotated, and V^T of every layer) and ESM-IF1 (the encoded backbone's K / V^T of every layer's
    // encoder_attn): the prefix every packed launch shares, the launches' plans and the sequence offsets of a log-likelihood chunk
    PrefixCache pfx;
    std::vector<float> poet_prompt_lp;  // PoET: the log-probability rows of the prompt last set
    // ESM-IF1 (api_esmif1.hip): if1_enc = the encoder width, if1_mem / if1_mem16 the staging of one encoder output
    // [max_positions][if1_enc] (fp32, split), if1_pos the sinusoidal table [if1_pos_len][D] (row t = position padding_idx + 1 + t)
    int if1_enc = 0, if1_pos_len = 0;
    float *if1_mem = nullptr, *if1_pos = nullptr;
    unsigned short* if1_mem16 = nullptr;
    // ESM3 (api_esm3.hip): v_heads and the out-projection's padded K; the structure-token table and the two folded constant rows; the
    // bound window (pgmi_esm3_set_structure): structure tokens, plddt flags, frames and frame mask of e3_T tokens, e3_framed = any frame
    int e3_vheads = 0, e3_Kp = 0;
    float *e3_struct_embed = nullptr, *e3_const = nullptr;
    int32_t *e3_stok = nullptr, *e3_plddt = nullptr, *e3_mask = nullptr;
    float *e3_rot = nullptr, *e3_trans = nullptr;
    size_t e3_cap = 0;
    int e3_T = 0;
    bool e3_framed = false;
    // MULAN (api_mulan.hip): mu_groups = 0 (ESM2's 33 tokens) or 21 (SaProt's layout); the adapter -- MLP [D][7] and bias, one layer, its
    // final LayerNorm --; the bound chunk (pgmi_mulan_set_structure): raw angle rows [mu_T][7] and pLDDT [mu_T] (mu_T = 0: none bound)
    int mu_groups = 0;
    float *mu_w = nullptr, *mu_b = nullptr, *mu_lna_w = nullptr, *mu_lna_b = nullptr;
    Layer mu_layer;
    float *mu_angles = nullptr, *mu_plddt = nullptr;
    size_t mu_angles_cap = 0, mu_plddt_cap = 0;
    int mu_T = 0;
    // 16-bit activations: h16_plane = R*D and g16_plane = R*F elements (f16x3: K-interleaved hi | lo rows, 2 halfs per element; bf16: 1
    // half).  They are allocation sizes; no launcher takes them as a stride.
    unsigned short *h16 = nullptr, *g16 = nullptr;
    size_t h16_plane = 0, g16_plane = 0;
    unsigned short *qk16 = nullptr, *vt16 = nullptr;   // attention operands (f16x3): [2][R*2D], [2][R*D]
    size_t qk16_plane = 0, vt16_plane = 0;
    int32_t* nonfinite = nullptr;
    int gemm_variant = 0;
    int keep_rows = 1;                                 // last layer's row-local stages on the kept rows only (PGMI_KEEP_ROWS)
    int last_B = 0, last_T = 0;
    int dh = kHeadDim;    // true head dim; heads are laid out in 64-lane slot groups (pgmi_model_create)
    int rot_halves = 1;   // slot groups per head: 1, 2 for head_dim 128 (and ProGen2's 80 / 96), 4 for ProGen2's 256
    int Hs = 0;           // slot groups per token = heads * rot_halves
    int Da = 0;           // attention width = heads * 64 (== embed_dim when dh == 64)
    float *rot_cos = nullptr, *rot_sin = nullptr;
    int rot_len = 0;
    // max(3 Da, roundup(V, 64), D, V, heads) zeros: the bias of a bias-free QKV / out-projection / wide head GEMM / LayerNorm / head,
    // and all-zero ALiBi slopes (model_create)
    float* zeros = nullptr;
    // workspace
    int max_rows = 0;
    float *x = nullptr, *h = nullptr, *qkv = nullptr, *g = nullptr, *lp = nullptr, *denom = nullptr;
    int32_t *tokens = nullptr, *pos_idx = nullptr, *kv_len = nullptr, *row_idx = nullptr, *aux_i = nullptr;
    // profiling
    bool prof = false;
    std::vector<ProfEvent> events;
    size_t events_used = 0;
    double prof_ms[PGMI_K_COUNT] = {0};
    int64_t prof_n[PGMI_K_COUNT] = {0};
    double prof_flops[PGMI_K_COUNT] = {0};
    double prof_bytes[PGMI_K_COUNT] = {0};
};

struct pgmi_assay {
    pgmi_model* m = nullptr;
    int n_tok = 0, P = 0, T = 0;
    int64_t n_mut = 0, n_sub = 0;
    std::vector<void*> allocs;
    int32_t *wt = nullptr, *positions = nullptr, *win_start = nullptr, *mask_rel = nullptr;
    int32_t *sub_pos = nullptr, *sub_wt = nullptr, *sub_mt = nullptr;
    int64_t* mut_off = nullptr;
    float* table = nullptr;
    double* scores = nullptr;
};

// A library of variable-length sequences resident in HBM for pseudo-perplexity scoring (config 5).
struct pgmi_pppl {
    pgmi_model* m = nullptr;
    int64_t N = 0;
    std::vector<int64_t> off;           // host copy of seq_off [N+1]
    std::vector<void*> allocs;
    uint8_t* tok8 = nullptr;            // all tokens, one byte each
    int64_t* off_dev = nullptr;
    int64_t last_rows = 0, last_chunks = 0, last_tokens = 0, last_padded = 0;   // statistics of the last run
};

namespace pgmi {

template <typename T>
int dev_alloc(std::vector<void*>& pool, T** p, size_t n) {
    void* q = nullptr;
    if (n == 0) n = 1;
    hipError_t e = hipMalloc(&q, n * sizeof(T));
    if (e != hipSuccess) {
        set_error("hipMalloc(%zu bytes) failed: %s", n * sizeof(T), hipGetErrorString(e));
        return PGMI_ENOMEM;
    }
    pool.push_back(q);
    *p = static_cast<T*>(q);
    return PGMI_OK;
}

template <typename T>
int dev_upload(std::vector<void*>& pool, T** p, const T* host, size_t n) {
    int rc = dev_alloc(pool, p, n);
    if (rc) return rc;
    if (n) PGMI_HIP(hipMemcpy(*p, host, n * sizeof(T), hipMemcpyHostToDevice));
    return PGMI_OK;
}

// Scopes may nest (MULAN's adapter layer runs inside run_encoder's embed scope) and an inner scope may grow m->events: a scope keeps
// the INDEX of its event, never a pointer into the vector.
struct ProfScope {
    pgmi_model* m;
    bool on = false;
    size_t idx = 0;
    ProfScope(pgmi_model* m_, int cls, double flops, double bytes) : m(m_) {
        if (!m->prof) return;
        if (m->events_used == m->events.size()) {
            ProfEvent e;
            if (hipEventCreate(&e.start) != hipSuccess || hipEventCreate(&e.stop) != hipSuccess) return;
            m->events.push_back(e);
        }
        idx = m->events_used++;
        on = true;
        m->events[idx].cls = cls;
        m->prof_n[cls] += 1;
        m->prof_flops[cls] += flops;
        m->prof_bytes[cls] += bytes;
        hipEventRecord(m->events[idx].start, m->stream);
    }
    ProfScope(const ProfScope&) = delete;
    ~ProfScope() {
        if (on) hipEventRecord(m->events[idx].stop, m->stream);
    }
};

template <typename T>
int ensure_cap(pgmi_model* m, T** p, size_t* cap, size_t need) {
    if (need <= *cap) return PGMI_OK;
    // grown buffers are owned by the model's pool; the old one stays in the pool until destroy (shapes
    // change rarely: once per alignment)
    T* q = nullptr;
    int rc = dev_alloc(m->allocs, &q, need);
    if (rc) return rc;
    *p = q;
    *cap = need;
    return PGMI_OK;
}

template <typename T>
constexpr T roundup32(T v) { return (v + 31) / 32 * 32; }

// A grow-only device buffer of a side handle, owned by the pool of the model it is reserved on; it reads as its pointer.
template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;
    int reserve(pgmi_model* m, size_t n) { return ensure_cap(m, &p, &cap, n); }
    operator T*() const { return p; }
};

// reserve_all(m, buf, n, buf, n, ...): every buffer to at least its n elements; the first failure ends it
inline int reserve_all(pgmi_model*) { return PGMI_OK; }
template <typename T, typename... Rest>
int reserve_all(pgmi_model* m, DevBuf<T>& b, size_t n, Rest&&... rest) {
    const int rc = b.reserve(m, n);
    return rc ? rc : reserve_all(m, rest...);
}

// ---- shared helpers (api_model.hip unless noted) ----
int prof_drain(pgmi_model* m);
// The embedded model of a side handle (pgmi_s2f, pgmi_carp, ...).  side_open: the refusals of a create after its config check -- the
// blob against the `want` elements the config needs, its values when scan_finite, the device -- then the GEMM test hooks, pm's device
// and precision and its stream (`lend` when given, else a new one).  Nothing is held when it fails.  side_sync: the end of a call --
// waits for the stream; rc unless it is PGMI_OK and a launch or the stream failed ("<what> failed: ...").  overflow_error: a head
// saw a non-finite log-probability.  side_release: teardown -- device, sync, events, pool, and the stream if it is the handle's.
int side_open(pgmi_model* pm, const char* name, const float* w, int64_t n_weights, int64_t want, bool scan_finite, int device, int precision,
              hipStream_t lend);
int side_sync(pgmi_model* pm, int rc, const char* what);
int overflow_error(int precision);
void side_release(pgmi_model* pm, bool own_stream);
int check_cfg(const pgmi_config* c);
int check_tokens(const int32_t* tokens, int B, int T, int n_ids = PGMI_VOCAB);
int check_vocab(const int32_t* tokens, int B, int T, int V);
int env_int(const char* name, int dflt);
int make_w16(std::vector<void*>& pool, const float* host, size_t n, size_t K, int precision, hipStream_t s, W16* out);
int linear(pgmi_model* m, const float* in32, const unsigned short* in16, const float* W32, const W16& w16, const float* bias,
           const float* residual, float* out32, unsigned short* out16, int M, int N, int K, int epi);
GemmLaunch qkv_launch(pgmi_model* m, const W16& w16, const float* bias, int M, int Da, int K, int T, int H);
PrefixAttLaunch prefix_launch(pgmi_model* m, const SegPlan& pl);
int alloc_prefix_cache(pgmi_model* m);              // m->pfx for cfg.max_positions prefix rows (0: no planes), and m->gpt_sum
int check_nonfinite(pgmi_model* m);
int reset_pad_keys(pgmi_model* m, int B, int T);
int model_create(const pgmi_config* cfg, const float* w, int64_t n_weights, int device, pgmi_model** out, int arch_arg,
                 const pgmi_pg3_params* pg3 = nullptr);
// api_esm.hip
struct BlobCursor;
void walk_esm(BlobCursor& c);                       // the ESM-1b / ESM2 blob into m; the cursor stays at its end
void walk_esm_layer(BlobCursor& c, Layer* L, size_t F);   // one layer of it, FC1 / FC2 of width F
// one encoder layer on the B T rows of m->x (run_encoder's loop body; MULAN's adapter with rotary off)
int encoder_layer(pgmi_model* m, const Layer& L, int B, int T, bool rotary, const int32_t* keep = nullptr, int n_keep = 0,
                  bool* compacted = nullptr);
int create_esm(pgmi_model* m, const pgmi_config* cfg, const float* w, int64_t n_weights);
int ensure_rotary(pgmi_model* m, int T);            // ESM2 / ESM C: tables for at least T positions
int upload_rotate_half(pgmi_model* m, int n);       // ESM2's rotary tables for positions 0..n-1 (rotate_half_slot layout)
int run_encoder(pgmi_model* m, int B, int T, const int32_t* keep = nullptr, int n_keep = 0, bool* compacted = nullptr);
int head_hidden(pgmi_model* m, int R, const int32_t* row_idx);   // run_head up to the LM head's LayerNorm: m->g [R,D]
int run_head(pgmi_model* m, int R, const int32_t* row_idx);
int run_rows(pgmi_model* m, int B, int T, int R, const int32_t* row_idx);
// api_tranception.hip
int create_tranception(pgmi_model* m, const pgmi_config* cfg, const float* w, int64_t n_weights);
// api_progen2.hip
int create_progen2(pgmi_model* m, const pgmi_config* cfg, const float* w, int64_t n_weights, int rotary_dim);
// api_gpt.hip
int create_gpt(pgmi_model* m, const pgmi_config* cfg, const float* w, int64_t n_weights, int pos_kind);
int64_t gpt_weight_count(const pgmi_config* c, int pos_kind);
int decoder_check(pgmi_model* m, int arch, int T);
int run_decoder(pgmi_model* m, int B, int T, const AttRagged* rg = nullptr, int rows = 0, double att_flops = 0);
// the sublayers of the 16-bit decoder loops (run_decoder, poet_forward, if1_forward) on the M rows of m->x:
// x += out_proj(causal_attn(ln_1(x))), dense B x T or ragged as run_decoder takes it (ProGen2: its MLP branch too, before the attention)
int self_attention(pgmi_model* m, const Layer& L, int B, int T, const AttRagged* rg = nullptr, int rows = 0, double att_flops = 0);
int out_proj(pgmi_model* m, const W16& wo16, const float* bo, int M);    // x += W ctx + b on the context rows in m->h16
int ffn(pgmi_model* m, const Layer& L, int M);                           // x += fc2(act(fc1(ln_2(x)))), act = m->fc1_epi
int narrow_head(pgmi_model* m, const float* src, int n);                 // lna when m->final_norm, log-softmax (V <= 64): src [n,D] -> m->lp [n,V]
// The end of a log-likelihood chunk: the R rows of m->x that have a target (row_idx on the device; nullptr: the first R rows as they
// are) through the narrow or wide head, log p(m->aux_i[r]) of each, their sums over the bc sequences (d_off [bc + 1], on the device)
// into m->gpt_sum and, asynchronously, into sum [bc].  R == 0: every sum is 0.
int loglik_tail(pgmi_model* m, const int32_t* row_idx, int R, const int32_t* d_off, int bc, double* sum);
int decoder_token_logprobs(pgmi_model* m, int arch, const int32_t* tokens, int B, int T, float* out);
int decoder_sequence_loglik(pgmi_model* m, int arch, const int32_t* tokens, const int32_t* lens, int B, int T, double* sum, int32_t* n_targets);
// api_progen3.hip
int pg3_check(const pgmi_config* c, const pgmi_pg3_params* p);
int64_t pg3_weight_count(const pgmi_config* c, const pgmi_pg3_params* p);
int create_progen3(pgmi_model* m, const pgmi_config* cfg, const float* w, int64_t n_weights, const pgmi_pg3_params* p);
void pack_swiglu(const float* w1, const float* w3, size_t F, size_t D, float* dst);   // w1 | w3 -> EPI_SWIGLU's 32 gate | 32 up row blocks
int moe_ws_alloc(std::vector<void*>& pool, pgmi_model::MoeWs* ws, size_t rows, size_t layers, int D, int F, int E, int top_k, int gated);
// x += w2(act(w1 h16)) on the M rows themselves (one expert): g16 [M][2 F] halfs of scratch
int dense_ffn(pgmi_model* m, const pgmi_model::MoeWs& ws, const W16& w1, const W16& w2, const unsigned short* h16, unsigned short* g16,
              int M, int D, int F, int gated, float* x);
int pg3_ffn(pgmi_model* m, const Layer& L, int layer, int M);       // x += moe(h16) of one layer (run_decoder)
// The expert block on split rows h16 [M][D] whose routing (ids / wts [M][top_k]) is known: permutation, gather, per-expert GEMMs, combine
// into x.  m gives the stream, the GEMM variant and the profile; ws the workspace.
int moe_ffn(pgmi_model* m, const pgmi_model::MoeWs& ws, const std::vector<W16>& ew1, const std::vector<W16>& ew2,
            const unsigned short* h16, const int32_t* ids, const float* wts, int M, int D, int F, int E, int top_k, int gated, float* x);
// api_poet.hip
int64_t poet_weight_count(const pgmi_config* c, int final_norm);
int create_poet(pgmi_model* m, const pgmi_config* cfg, const float* w, int64_t n_weights, int final_norm);
// What differs between the packed-decoder entries of PoET and ESM-IF1 (score_packed).
struct PackedScorer {
    int (*forward)(pgmi_model* m, int bc, int R, const SegPlan& pl);    // the chunk's bc sequences, R packed rows, uploaded -> m->x
    int pos_len;                    // the longest sequence the position table takes, and its name in the refusal
    const char* pos_what;
    const char* not_ready;          // non-null: the entry cannot run yet, and why
    bool same_length;               // a chunk is a run of sequences of one length
    bool vocab_per_row;             // token ids are checked per row over its lens[b] tokens (the pad value is not read); else over [B,T]
    int skip_target;                // log-likelihood: a target equal to this token does not count (-1: every target counts)
    bool mean;                      // log-likelihood: the mean over the lens[b] - 1 targets instead of their sum
};
// Sequences [B][T] right-padded, lens[b] tokens each, cut into chunks by pack_chunk.  loglik: the model reads tokens[b, :lens[b] - 1]
// and sum[b] = the sum (mean) of log p(tokens[b, t + 1]) over the targets that count; else it reads all lens[b] tokens and every row's
// log-probabilities go to out [B][T][V] (rows beyond lens[b]: NaN).
int score_packed(pgmi_model* m, const PackedScorer& e, const int32_t* tokens, const int32_t* lens, int B, int T, bool loglik, float* out,
                 double* sum);
// api_esmif1.hip
int if1_check(const pgmi_config* c, int enc_dim);
int64_t if1_weight_count(const pgmi_config* c, int enc_dim);
int create_esmif1(pgmi_model* m, const pgmi_config* cfg, const float* w, int64_t n_weights, int enc_dim);
// api_esmc.hip
int64_t esmc_weight_count(const pgmi_config* c);
int create_esmc(pgmi_model* m, const pgmi_config* cfg, const float* w, int64_t n_weights);
// api_esm3.hip
int esm3_check(const pgmi_config* c, int v_heads);
int64_t esm3_weight_count(const pgmi_config* c, int v_heads);
int create_esm3(pgmi_model* m, const pgmi_config* cfg, const float* w, int64_t n_weights, int v_heads);
int esm3_embed(pgmi_model* m, int B, int T);                        // m->tokens [B,T] -> m->x, over the bound window
int geom_branch(pgmi_model* m, const Layer& L, int B, int T);       // x += out_proj(geom_attn(s_norm(x))) / s on the M = B T rows of m->x
// api_saprot.hip
int create_saprot(pgmi_model* m, const pgmi_config* cfg, const float* w, int64_t n_weights, int mask_id);
// api_mulan.hip
int64_t mulan_weight_count(const pgmi_config* c);
int create_mulan(pgmi_model* m, const pgmi_config* cfg, const float* w, int64_t n_weights, int mask_id);
int mulan_embed(pgmi_model* m, int B, int T);       // the adapter on its input rows in m->x, then m->x = the embedding of m->tokens
// api_msa.hip
int create_msa(pgmi_model* m, const pgmi_config* cfg, const float* w, int64_t n_weights);
int run_msa(pgmi_model* m, int R, int C, int keep_col = -1, bool* compacted = nullptr);

// ESM2's rotate-half rotary on q and k (SaProt is ESM2 with another vocabulary; MULAN's main stack is either)
inline bool esm2_rotary(int arch) { return arch == PGMI_ARCH_ESM2 || arch == PGMI_ARCH_SAPROT || arch == PGMI_ARCH_MULAN; }
// ESM C's blocks (q / k LayerNorm, SwiGLU, scaled residual, 64-column head): ESM C itself and ESM3
inline bool esmc_blocks(int arch) { return arch == PGMI_ARCH_ESMC || arch == PGMI_ARCH_ESM3; }

// Walks a weight blob in the order include/pgmi.h documents.  upload / w16 / linear put the next n floats on the device; their forms
// with a host pointer upload a host re-layout instead and do not advance.  take hands the next n floats to a host re-layout.  The
// first error sticks: every later call does nothing, and finish() returns it -- or a mismatch if the walk did not end exactly at
// the end of the blob.
struct BlobCursor {
    pgmi_model* m;
    const float *p, *end;
    int rc = PGMI_OK;
    BlobCursor(pgmi_model* m_, const float* w, int64_t n_weights) : m(m_), p(w), end(w + n_weights) {}
    const float* take(size_t n) { p += n; return p - n; }
    void upload(float** dst, const float* host, size_t n) { if (!rc) rc = dev_upload(m->allocs, dst, host, n); }
    void upload(float** dst, size_t n) { upload(dst, take(n), n); }
    void upload(float** dst, const std::vector<float>& host) { upload(dst, host.data(), host.size()); }
    void w16(W16* dst, const float* host, size_t n, size_t K) { if (!rc) rc = make_w16(m->allocs, host, n, K, m->cfg.precision, m->stream, dst); }
    void w16(W16* dst, size_t n, size_t K) { w16(dst, take(n), n, K); }
    // a Linear weight [n / K, K]: fp32 in precision fp32, 16-bit planes otherwise
    void linear(float** w32, W16* w16_, const float* host, size_t n, size_t K) {
        if (m->cfg.precision == PGMI_PREC_FP32) upload(w32, host, n); else w16(w16_, host, n, K);
    }
    void linear(float** w32, W16* w16_, size_t n, size_t K) { linear(w32, w16_, take(n), n, K); }
    void linear(float** w32, W16* w16_, const std::vector<float>& host, size_t K) { linear(w32, w16_, host.data(), host.size(), K); }
    int finish() {
        if (!rc && p != end) { set_error("internal: blob walk mismatch"); rc = PGMI_EINVAL; }
        return rc;
    }
};

// a value of the split fp16 planes (common.h split_act) back as fp32: hi + lo 2^-11
inline float rebuild_split(unsigned short h, unsigned short l) {
    _Float16 a, b;
    memcpy(&a, &h, 2); memcpy(&b, &l, 2);
    return (float)a + (float)b * (1.0f / kLoScale);
}

// The scope of one single-op or timing entry (pgmi_op_* / pgmi_bench_*: api_ops.hip, api_carp.hip), made after the entry's argument
// checks.  Making it refuses a machine without a device and selects `device`; it owns what the entry puts on the device -- the pool
// (tmp.allocs; tmp is the model-shaped argument of the helpers that want one), MoE's pinned counts, the timer's events -- and releases
// it when the entry returns, on every path.  The first error sticks (BlobCursor's idiom): every later call does nothing and hands
// back null, so an entry is a list of plain statements and one `if (s.rc) return s.rc;` before its first launch.  `what` names the
// entry in "<what> failed: ..." ("rmsnorm op", "bench").
struct OpScope {
    const char* what;
    int rc = PGMI_OK;
    pgmi_model tmp{};
    std::vector<void*>& pool = tmp.allocs;
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool opened = false;

    OpScope(const char* what_, int device) : what(what_) {
        rc = open(device);
        opened = rc == PGMI_OK;
        if (rc == PGMI_EHIP) (void)hipGetLastError();    // reported here: not left for the next entry's sync() to find
    }
    OpScope(const OpScope&) = delete;
    ~OpScope() {
        for (hipEvent_t e : ev)
            if (e) hipEventDestroy(e);
        if (tmp.moe.counts_host) hipHostFree(tmp.moe.counts_host);
        for (void* p : pool) hipFree(p);
    }
    // a HIP call of the entry itself: its failure is the entry's "<what> failed: ..."
    int hip(hipError_t e) {
        if (!rc && e != hipSuccess) { set_error("%s failed: %s", what, hipGetErrorString(e)); rc = PGMI_EHIP; }
        return rc;
    }
    // n elements; fill = 0x00 or 0xFF: every byte starts as that (0xFF: NaN in fp32 and fp16, so an element a kernel skips shows)
    template <typename T>
    T* alloc(size_t n, int fill = -1) {
        T* p = nullptr;
        if (!rc) rc = dev_alloc(pool, &p, n);
        if (!rc && fill >= 0) hip(hipMemset(p, fill, n * sizeof(T)));
        return rc ? nullptr : p;
    }
    template <typename T>
    T* up(const T* host, size_t n) {
        T* p = nullptr;
        if (!rc) rc = dev_upload(pool, &p, host, n);
        return rc ? nullptr : p;
    }
    template <typename T>
    T* up(const std::vector<T>& host) { return up(host.data(), host.size()); }
    W16 w16(const float* host, size_t n, size_t K, int precision = PGMI_PREC_F16X3) {
        W16 w;
        if (!rc) rc = make_w16(pool, host, n, K, precision, nullptr, &w);
        return w;
    }
    // the end of the launches: waits for the device whatever rc is, unless the scope never opened (nothing is released under a
    // running kernel), then reads the launch error
    int sync() {
        if (!opened) return rc;
        hipError_t e = hipDeviceSynchronize();
        if (e == hipSuccess) e = hipGetLastError();
        return hip(e);
    }
    template <typename T>
    void down(T* host, const T* dev, size_t n) {
        if (!rc) hip(hipMemcpy(host, dev, n * sizeof(T), hipMemcpyDeviceToHost));
    }
    // split fp16 planes in K-interleaved rows (ki_off) [rows][cols] back as fp32 = hi + lo 2^-11
    void planes(float* host, const unsigned short* dev16, size_t rows, size_t cols) {
        std::vector<unsigned short> h(rc ? 0 : rows * cols * 2);
        down(h.data(), dev16, h.size());
        for (size_t r = 0; r < rows && !rc; ++r)
            for (size_t c = 0; c < cols; ++c) {
                const size_t o = ki_off(r, (int)c, (int)cols);
                host[r * cols + c] = rebuild_split(h[o], h[o + 32]);
            }
    }
    // one bf16 plane, row-major, back as fp32
    void bf16_plane(float* host, const unsigned short* dev16, size_t n) {
        std::vector<unsigned short> h(rc ? 0 : n);
        down(h.data(), dev16, n);
        for (size_t i = 0; i < n && !rc; ++i) {
            const unsigned int u = (unsigned int)h[i] << 16;
            memcpy(&host[i], &u, 4);
        }
    }
    // ms per launch of `iters` launches on the null stream between two events; 0 once rc is set.  launch() returns a PGMI code.
    template <typename F>
    double time_ms(F launch, int iters) {
        for (hipEvent_t& e : ev)
            if (!rc && !e) hip(hipEventCreate(&e));
        if (!rc) hip(hipEventRecord(ev[0], nullptr));
        for (int i = 0; i < iters && !rc; ++i) rc = launch();
        if (!rc) hip(hipEventRecord(ev[1], nullptr));
        if (!rc) hip(hipEventSynchronize(ev[1]));
        float ms = 0.f;
        if (!rc) hip(hipEventElapsedTime(&ms, ev[0], ev[1]));
        return (double)ms / iters;
    }

private:
    int open(int device) {
        if (pgmi_device_count() <= 0) { set_error("no HIP device visible"); return PGMI_ENODEV; }
        PGMI_HIP(hipSetDevice(device));
        return PGMI_OK;
    }
};

// Attention slot of model dim `col` in the rotate-half layout (ESM2, RITA): every head owns 64 lanes of the attention kernels; dim j
// of a head sits in slot j (first half) or 32 + (j - dh/2) (second half) so that rotary pairs (j, j + dh/2) are the kernels' pairs
// (i, i + 32).  dh == 64 is the identity layout; smaller heads leave zero slots (zero weight rows -> q,k,v slots exactly 0 -> scores
// and context unchanged).  head_dim 128: a head is two slot groups; group g in {0,1} holds dims 32 g + i (slots i < 32) and
// 64 + 32 g + i (slots 32 + i), so the rotary partners (j, j + 64) are again the kernels' pairs (i, i + 32) inside ONE 64-column wave
// tile of the QKV epilogue.
inline size_t rotate_half_slot(size_t col, size_t dh) {
    const size_t h = col / dh, j = col % dh;
    if (dh > 64) return (2 * h + ((j >> 5) & 1)) * 64 + ((j >> 6) << 5) + (j & 31);
    return h * 64 + (j < dh / 2 ? j : 32 + (j - dh / 2));
}

// Fused [3 Da, D] QKV projection from the blob's q | k | v blocks (each a [D, D] weight, followed by a [D] bias when bq is
// given): row o of block k goes to row k Da + slot(o), the q rows pre-scaled by qscale.  Rows no model dim maps to keep their
// zeros (zero q / k / v lanes change no score and no context value).
template <typename Slot>
void pack_qkv_slots(const float* src, size_t D, size_t Da, Slot slot, float qscale, float* wq, float* bq = nullptr) {
    for (size_t k = 0; k < 3; ++k) {
        const float sc = (k == 0) ? qscale : 1.0f;
        for (size_t o = 0; o < D; ++o) {
            float* dst = &wq[(k * Da + slot(o)) * D];
            for (size_t i = 0; i < D; ++i) dst[i] = src[o * D + i] * sc;
        }
        src += D * D;
        if (!bq) continue;
        for (size_t o = 0; o < D; ++o) bq[k * Da + slot(o)] = src[o] * sc;
        src += D;
    }
}

// Out-projection [D, D] -> [D, Da]: its input columns follow the same slot layout.
template <typename Slot>
void pack_out_cols(const float* src, size_t D, size_t Da, Slot slot, float* wo) {
    for (size_t o = 0; o < D; ++o)
        for (size_t i = 0; i < D; ++i) wo[o * Da + slot(i)] = src[o * D + i];
}

// Rotary cos / sin tables [n][groups][64] in the fused QKV epilogue's layout: slots i and 32 + i of slot group g rotate by
// angle(t, g, i), an fp32 angle.  Angle 0 passes the pair through (cosf(0) = 1 and sinf(0) = 0 exactly).
template <typename Angle>
int upload_rotary(pgmi_model* m, int n, int groups, Angle angle) {
    std::vector<float> c((size_t)n * groups * 64), s((size_t)n * groups * 64);
    for (int t = 0; t < n; ++t)
        for (int g = 0; g < groups; ++g)
            for (int i = 0; i < 32; ++i) {
                const float f = angle(t, g, i);
                const size_t o = ((size_t)t * groups + g) * 64;
                c[o + i] = c[o + 32 + i] = cosf(f);
                s[o + i] = s[o + 32 + i] = sinf(f);
            }
    int rc = dev_upload(m->allocs, &m->rot_cos, c.data(), c.size());
    if (!rc) rc = dev_upload(m->allocs, &m->rot_sin, s.data(), s.size());
    if (!rc) m->rot_len = n;
    return rc;
}

// attention_prefix.hip's launches (PoET, ESM-IF1): upload_plan puts a launch's (segment, tile) lists into plan slot 0 / 1 of m->pfx.meta.
inline size_t own_pitch(const pgmi_model* m) { return own_pitch(m->max_rows); }

inline int upload_plan(pgmi_model* m, SegPlan& p, int slot) {
    p.d_seg_off = m->pfx.plan(slot);
    p.d_ent_seg = p.d_seg_off + m->pfx.cap + 2;
    p.d_ent_tile = p.d_ent_seg + m->pfx.cap;
    PGMI_HIP(hipMemcpyAsync(p.d_seg_off, p.seg_off.data(), p.seg_off.size() * 4, hipMemcpyHostToDevice, m->stream));
    PGMI_HIP(hipMemcpyAsync(p.d_ent_seg, p.ent_seg.data(), p.ent_seg.size() * 4, hipMemcpyHostToDevice, m->stream));
    PGMI_HIP(hipMemcpyAsync(p.d_ent_tile, p.ent_tile.data(), p.ent_tile.size() * 4, hipMemcpyHostToDevice, m->stream));
    return PGMI_OK;
}

// Sequences of T tokens per workspace chunk: B * roundup(T, 32) <= max_rows, at least one.
inline int rows_per_chunk(const pgmi_model* m, int T) { return std::max(1, m->max_rows / roundup32(T)); }

// Drives a fixed-T batch through the workspace: fn(b0, bc) copies chunk [b0, b0 + bc) in, runs it and copies its results out
// (asynchronously); the stream is synchronized after every chunk, so host buffers of the chunk outlive their copies.
template <typename Fn>
int for_each_chunk(pgmi_model* m, int B, int T, Fn fn) {
    const int per = rows_per_chunk(m, T);
    for (int b0 = 0; b0 < B; b0 += per) {
        int rc = fn(b0, std::min(per, B - b0));
        if (rc) return rc;
        PGMI_HIP(hipStreamSynchronize(m->stream));
    }
    return PGMI_OK;
}

}  // namespace pgmi
