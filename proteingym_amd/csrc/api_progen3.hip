// ProGen3 (proteingym/baselines/progen3/progen3/modeling.py, model/attention.py, model/moe.py): model creation, the feed-forward block
// of a layer and the C entries.  The forward is the causal decoder's (api_gpt.hip run_decoder) with the model's norm and feed-forward
// block chosen by data; the wide LM head and the scoring entry are the causal decoder's too.
//
// Per layer (modeling.py DecoderLayer): x += o_proj(attn(rmsnorm(x))); x += moe(rmsnorm(x)); no bias anywhere.
//   Attention (model/attention.py): heads query heads on kv_heads key / value heads, each repeated heads / kv_heads times (repeat_kv);
//   rotate-half rotary over the whole head; causal; scale head_dim^-1/2.  Here the K / V projection rows of a key / value head are
//   replicated to its query heads when the fused QKV weight is packed, so the fused QKV epilogue and attention_f16x3_v2 run unchanged on
//   `heads` full heads: heads / kv_heads times the K / V projection FLOPs, and nothing else -- scoring keeps no K/V cache to shrink.
//   MoE (model/moe.py SparseMoeBlock): the router rides in the layer's second RMSNorm (moe.hip rmsnorm_route_kernel); then moe_ffn:
//   permutation -> gather of the split rows into expert-contiguous segments -> per non-empty expert FC1 (EPI_SWIGLU on w1 | w3 packed in
//   32 gate | 32 up row blocks; non-gated: fp32 rows, then silu_split_kernel) and FC2 into fp32 slot rows, both launch_gemm16 ->
//   weighted combine into x.  One expert: the plain MLP on the rows themselves, no router, no permutation.
//
// A row's bits do not depend on the rest of the batch: the router, gather and combine are row-local; the order inside an expert's
// segment is stable ((row, k) ascending), and the GEMM computes every output element from its own A row and W row over K in a fixed
// order, whatever the row's place in its tile or the segment's length (gemm_f16.hip: half-height tail, row chunks).
#include "model.h"

namespace pgmi {

constexpr int kPg3PadId = 0;                // tokenizer.json: <pad>
constexpr int kPg3HeadRows = 2048;          // logits rows per head GEMM (api_gpt.hip kWideHeadRows)
constexpr int kMoeTile = 256;               // gemm16x_kernel.h XBM: an expert's segment starts on a row tile of the GEMM

int pg3_check(const pgmi_config* c, const pgmi_pg3_params* p) {
    if (!p) { set_error("ProGen3 needs pgmi_pg3_params"); return PGMI_EINVAL; }
    if (p->kv_heads <= 0 || c->heads % p->kv_heads) {
        set_error("ProGen3: num_key_value_heads %d must divide num_attention_heads %d", p->kv_heads, c->heads);
        return PGMI_EINVAL;
    }
    if (p->n_experts < 1 || p->n_experts > kWave || p->top_k < 1 || p->top_k > p->n_experts) {
        set_error("ProGen3: %d experts, top-%d: this build runs 1 .. 64 experts with 1 <= top_k <= experts", p->n_experts, p->top_k);
        return PGMI_EINVAL;
    }
    if (p->clip_qkv != 0.0f) {
        set_error("ProGen3: clip_qkv = %g is not supported: the clamp sits between the projection and the rotary, inside the fused QKV epilogue", p->clip_qkv);
        return PGMI_EINVAL;
    }
    if (!(p->rope_theta > 0.0f)) { set_error("ProGen3: rope_theta must be positive, got %g", p->rope_theta); return PGMI_EINVAL; }
    return PGMI_OK;
}

int64_t pg3_weight_count(const pgmi_config* c, const pgmi_pg3_params* p) {
    const int64_t D = c->embed_dim, F = c->ffn_dim, V = c->vocab, E = p->n_experts, KVD = (int64_t)p->kv_heads * (D / c->heads);
    const int64_t layer = D + D * D + 2 * KVD * D + D * D + D + (E > 1 ? E * D : 0) + E * ((p->gated ? 2 : 1) * F * D + D * F);
    return V * D + D + (int64_t)c->layers * layer + D + V * D;
}

// w1 [F,D] | w3 [F,D] -> EPI_SWIGLU's FC1 [2F,D]: per 32 hidden units their 32 gate rows (w1), then their 32 up rows (w3)
void pack_swiglu(const float* w1, const float* w3, size_t F, size_t D, float* dst) {
    for (size_t b = 0; b < F / 32; ++b) {
        memcpy(dst + (2 * b) * 32 * D, w1 + b * 32 * D, 32 * D * sizeof(float));
        memcpy(dst + (2 * b + 1) * 32 * D, w3 + b * 32 * D, 32 * D * sizeof(float));
    }
}

int moe_ws_alloc(std::vector<void*>& pool, pgmi_model::MoeWs* ws, size_t rows, size_t layers, int D, int F, int E, int top_k, int gated) {
    const size_t n = rows * top_k, slots = n + (size_t)E * kMoeTile, nblk = (size_t)moe_perm_blocks((int)n);
    int rc = PGMI_OK;
    auto alloc = [&](auto** p, size_t k) { if (!rc) rc = dev_alloc(pool, p, k); };
    if (E == 1) {
        if (!gated) alloc(&ws->t32, rows * F);
        return rc;
    }
    ws->layer_stride = n;
    alloc(&ws->ids, layers * n);
    alloc(&ws->wts, layers * n);
    alloc(&ws->slot, n);
    alloc(&ws->blk_cnt, nblk * E);
    alloc(&ws->blk_base, nblk * E);
    alloc(&ws->counts_seg, (size_t)2 * E + 1);
    alloc(&ws->a16, slots * 2 * D);
    alloc(&ws->g16, slots * 2 * F);
    alloc(&ws->y, slots * D);
    if (!gated) alloc(&ws->t32, slots * F);
    if (rc) return rc;
    PGMI_HIP(hipHostMalloc(reinterpret_cast<void**>(&ws->counts_host), ((size_t)2 * E + 1) * sizeof(int32_t)));
    return PGMI_OK;
}

// One MLP on cnt split rows a16 [cnt][D]: FC1 (gated: EPI_SWIGLU into g16; else fp32 rows t32, then silu + split into g16), FC2 into
// out32 (+ residual).  Profiled as the model's FC1 / FC2.
static int expert_mlp(pgmi_model* m, const W16& w1, const W16& w2, const unsigned short* a16, unsigned short* g16, float* t32,
                      const float* residual, float* out32, int cnt, int D, int F, int gated) {
    GemmLaunch g;
    g.variant = m->gemm_variant; g.stream = m->stream;
    { ProfScope p(m, PGMI_K_GEMM_FC1, 2.0 * cnt * (gated ? 2 : 1) * F * D, 0);
      GemmLaunch a = g;
      a.A = a16; a.W = w1.p; a.out_scale = w1.out_scale;
      a.M = cnt; a.N = gated ? 2 * F : F; a.K = D;
      if (gated) { a.out16 = g16; a.epilogue = EPI_SWIGLU; } else a.out32 = t32;
      int rc = launch_gemm16(a);
      if (rc) return rc;
      if (!gated) launch_silu_split(t32, cnt, F, g16, m->stream); }
    ProfScope p(m, PGMI_K_GEMM_FC2, 2.0 * cnt * F * D, 0);
    GemmLaunch b = g;
    b.A = g16; b.W = w2.p; b.out_scale = w2.out_scale;
    b.residual = residual; b.out32 = out32;
    b.M = cnt; b.N = D; b.K = F;
    return launch_gemm16(b);
}

int dense_ffn(pgmi_model* m, const pgmi_model::MoeWs& ws, const W16& w1, const W16& w2, const unsigned short* h16, unsigned short* g16,
              int M, int D, int F, int gated, float* x) {
    return expert_mlp(m, w1, w2, h16, g16, ws.t32, x, x, M, D, F, gated);
}

int moe_ffn(pgmi_model* m, const pgmi_model::MoeWs& ws, const std::vector<W16>& ew1, const std::vector<W16>& ew2,
            const unsigned short* h16, const int32_t* ids, const float* wts, int M, int D, int F, int E, int top_k, int gated, float* x) {
    hipStream_t s = m->stream;
    const int n = M * top_k;
    { ProfScope p(m, PGMI_K_MOE_ROUTE, 0, (double)n * (4.0 * D + 12));
      launch_moe_permute(ids, n, E, kMoeTile, ws.blk_cnt, ws.blk_base, ws.counts_seg, ws.slot, s);
      PGMI_HIP(hipMemcpyAsync(ws.counts_host, ws.counts_seg, ((size_t)2 * E + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, s));
      launch_moe_gather(h16, ws.slot, n, top_k, D, ws.a16, s); }
    PGMI_HIP(hipGetLastError());
    // the per-expert launches take their row counts on the host: one stream synchronisation per layer (profiles/progen3/README.md)
    PGMI_HIP(hipStreamSynchronize(s));
    int routed = 0;
    for (int e = 0; e < E; ++e) {
        const int cnt = ws.counts_host[e];
        const size_t off = (size_t)ws.counts_host[E + e];
        if (cnt < 0 || routed + cnt > n) { set_error("internal: expert %d has %d of %d routed rows", e, cnt, n); return PGMI_EINVAL; }
        routed += cnt;
        if (!cnt) continue;                                        // an expert nobody chose launches nothing
        int rc = expert_mlp(m, ew1[e], ew2[e], ws.a16 + off * 2 * D, ws.g16 + off * 2 * F, ws.t32 ? ws.t32 + off * F : nullptr, nullptr,
                            ws.y + off * D, cnt, D, F, gated);
        if (rc) return rc;
    }
    { ProfScope p(m, PGMI_K_MOE_ROUTE, 0, (double)n * 4.0 * D + 8.0 * M * D);
      launch_moe_combine(ws.y, ws.slot, wts, M, top_k, D, x, s); }
    PGMI_HIP(hipGetLastError());
    return PGMI_OK;
}

// x += moe(rmsnorm(x)) of layer `layer` on the M rows of m->x (run_decoder)
int pg3_ffn(pgmi_model* m, const Layer& L, int layer, int M) {
    const int D = m->cfg.embed_dim, F = m->cfg.ffn_dim, E = m->pg3_E, k = m->pg3_k;
    const double ln_bytes = 2.0 * M * D * 4;
    if (E == 1) {
        { ProfScope p(m, PGMI_K_LAYERNORM, 0, ln_bytes);
          int rc = launch_rmsnorm16(m->x, L.ln2_w, M, D, m->ln_eps, m->h16, m->stream);
          if (rc) return rc; }
        return dense_ffn(m, m->moe, L.w116, L.w216, m->h16, m->g16, M, D, F, m->pg3_gated, m->x);
    }
    int32_t* ids = m->moe.ids + (size_t)layer * m->moe.layer_stride;
    float* wts = m->moe.wts + (size_t)layer * m->moe.layer_stride;
    { ProfScope p(m, PGMI_K_LAYERNORM, 2.0 * M * E * D, ln_bytes);
      MoeRoute r;
      r.gate = L.gate; r.E = E; r.top_k = k;
      r.tokens = m->tokens; r.pad_id = kPg3PadId;
      r.ids = ids; r.wts = wts;
      int rc = launch_rmsnorm_route(m->x, L.ln2_w, M, D, m->ln_eps, m->h16, r, m->stream);
      if (rc) return rc; }
    return moe_ffn(m, m->moe, L.ew1, L.ew2, m->h16, ids, wts, M, D, F, E, k, m->pg3_gated, m->x);
}

// Attention slot of dim j of a head in the rotate-half layout: the rotary partners (j, j + dh/2) are pair p = j % (dh/2), which sits in
// slots (p % 32, 32 + p % 32) of the head's slot group p / 32 -- the fused QKV epilogue's pairs (i, i + 32).  dh 64 and 128 give
// rotate_half_slot's layout; 80, 96 and 256 leave the slots past the last pair of a group zero (ProGen2's padding).
static size_t pg3_slot(size_t j, size_t dh) {
    const size_t half = dh / 2, p = j % half;
    return (p / 32) * 64 + (p % 32) + (j >= half ? 32 : 0);
}

// Weight blob: include/pgmi.h (PGMI_ARCH_PROGEN3).
int create_progen3(pgmi_model* m, const pgmi_config* cfg, const float* w, int64_t n_weights, const pgmi_pg3_params* p) {
    const size_t D = cfg->embed_dim, F = cfg->ffn_dim, V = cfg->vocab, dh = m->dh, Da = m->Da, H = cfg->heads, KV = p->kv_heads;
    const size_t G = m->rot_halves, rep = H / KV, E = p->n_experts;
    m->rms_norm = true;
    m->pg3_E = (int)E; m->pg3_k = p->top_k; m->pg3_gated = p->gated != 0;
    m->slopes = m->zeros;
    m->final_norm = true;
    BlobCursor c(m, w, n_weights);
    {   // embed_tokens[id] + embed_seq_id[0]: the reference's own fp32 add, once per table element
        const float* tok = c.take(V * D);
        const float* sid = c.take(D);
        std::vector<float> emb(V * D);
        for (size_t v = 0; v < V; ++v)
            for (size_t i = 0; i < D; ++i) emb[v * D + i] = tok[v * D + i] + sid[i];
        c.upload(&m->embed_tokens, emb.data(), emb.size());
    }
    // SDPA's head_dim^-1/2 folded into the q rows: the rotary is linear, so scaling before it is the same map
    const float qscale = 1.0f / sqrtf((float)dh);
    m->layers.resize(cfg->layers);
    std::vector<float> wq(3 * Da * D), wo_r(D * Da), fc1(p->gated ? 2 * F * D : 0);
    for (int l = 0; l < cfg->layers; ++l) {
        Layer& L = m->layers[l];
        c.upload(&L.ln1_w, D);
        const float* q = c.take(D * D);
        const float* kv[2] = {c.take(KV * dh * D), nullptr};
        kv[1] = c.take(KV * dh * D);
        std::fill(wq.begin(), wq.end(), 0.0f);
        for (size_t h = 0; h < H; ++h)
            for (size_t j = 0; j < dh; ++j) {
                const size_t row = h * G * 64 + pg3_slot(j, dh);
                float* dq = &wq[row * D];
                for (size_t i = 0; i < D; ++i) dq[i] = q[(h * dh + j) * D + i] * qscale;
                for (int b = 0; b < 2; ++b)                       // query head h reads key / value head h / rep (repeat_kv)
                    memcpy(&wq[((b + 1) * Da + row) * D], kv[b] + ((h / rep) * dh + j) * D, D * sizeof(float));
            }
        c.w16(&L.wqkv16, wq.data(), wq.size(), D);
        std::fill(wo_r.begin(), wo_r.end(), 0.0f);
        const float* o = c.take(D * D);                            // o_proj [D, H dh]: its input columns follow the slot layout
        for (size_t r = 0; r < D; ++r)
            for (size_t col = 0; col < D; ++col) wo_r[r * Da + (col / dh) * G * 64 + pg3_slot(col % dh, dh)] = o[r * D + col];
        c.w16(&L.wo16, wo_r.data(), wo_r.size(), Da);
        L.bqkv = L.bo = m->zeros;
        c.upload(&L.ln2_w, D);
        if (E > 1) c.upload(&L.gate, E * D);
        L.ew1.resize(E); L.ew2.resize(E);
        for (size_t e = 0; e < E; ++e) {
            if (p->gated) {
                const float* w1 = c.take(F * D);
                const float* w3 = c.take(F * D);
                pack_swiglu(w1, w3, F, D, fc1.data());
                c.w16(&L.ew1[e], fc1.data(), fc1.size(), D);
            } else c.w16(&L.ew1[e], F * D, D);
            c.w16(&L.ew2[e], D * F, F);
        }
        if (E == 1) { L.w116 = L.ew1[0]; L.w216 = L.ew2[0]; }
    }
    c.upload(&m->lna_w, D);
    const float* head = c.take(V * D);
    const size_t Vp = (V + 63) / 64 * 64;
    m->gpt_Vp = (int)Vp;
    {   // zero rows V .. Vp-1: whole 64-column GEMM tiles; the log-softmax excludes those columns by index
        std::vector<float> padded(Vp * D, 0.0f);
        memcpy(padded.data(), head, V * D * sizeof(float));
        c.w16(&m->gpt_head16, padded.data(), padded.size(), D);
    }
    m->gpt_head_rows = std::min(m->max_rows, kPg3HeadRows);
    int rc = c.finish();
    if (!rc) rc = dev_alloc(m->allocs, &m->gpt_logits, (size_t)m->gpt_head_rows * Vp);
    if (!rc) rc = dev_alloc(m->allocs, &m->gpt_sum, (size_t)m->max_rows);
    if (!rc) rc = moe_ws_alloc(m->allocs, &m->moe, (size_t)m->max_rows, (size_t)cfg->layers, (int)D, (int)F, (int)E, p->top_k, m->pg3_gated);
    if (rc) return rc;
    // inv_freq = rope_theta ** -(arange(0, dh, 2) / dh) and angle = t * inv_freq in fp32 (attention.py RotaryPositionalEmbedding);
    // slots past the last pair of a group: angle 0 (cos 1, sin 0 on zero lanes)
    const int half = (int)dh / 2;
    std::vector<float> inv(half);
    for (int i = 0; i < half; ++i) inv[i] = powf(p->rope_theta, -((float)(2 * i) / (float)dh));
    return upload_rotary(m, cfg->max_positions, (int)G, [&](int t, int g, int i) {
        const int pr = 32 * g + i;
        return pr < half ? (float)t * inv[pr] : 0.0f;
    });
}

}  // namespace pgmi

extern "C" {

int64_t pgmi_pg3_weight_count(const pgmi_config* cfg, const pgmi_pg3_params* params) {
    if (!cfg || !params || cfg->layers <= 0 || cfg->embed_dim <= 0 || cfg->ffn_dim <= 0 || cfg->vocab <= 0 || cfg->heads <= 0 ||
        cfg->embed_dim % cfg->heads || pg3_check(cfg, params)) return -1;
    return pg3_weight_count(cfg, params);
}

int pgmi_pg3_model_create(const pgmi_config* cfg, const pgmi_pg3_params* params, const float* weights, int64_t n_weights, int device,
                          pgmi_model** out) {
    if (out) *out = nullptr;
    if (!cfg || cfg->arch != PGMI_ARCH_PROGEN3) { set_error("pgmi_pg3_model_create: arch must be PGMI_ARCH_PROGEN3"); return PGMI_EINVAL; }
    return model_create(cfg, weights, n_weights, device, out, 0, params);
}

int pgmi_pg3_token_logprobs(pgmi_model* m, const int32_t* tokens, int B, int T, float* out) {
    return decoder_token_logprobs(m, PGMI_ARCH_PROGEN3, tokens, B, T, out);
}

int pgmi_pg3_sequence_loglik(pgmi_model* m, const int32_t* tokens, const int32_t* lens, int B, int T, double* sum, int32_t* n_targets) {
    return decoder_sequence_loglik(m, PGMI_ARCH_PROGEN3, tokens, lens, B, T, sum, n_targets);
}

int pgmi_pg3_routing(pgmi_model* m, int layer, int rows, int32_t* ids, float* weights) {
    if (!m || m->cfg.arch != PGMI_ARCH_PROGEN3) { set_error("not a ProGen3 model"); return PGMI_EINVAL; }
    if (m->pg3_E < 2) { set_error("a model of one expert routes nothing"); return PGMI_EINVAL; }
    if (layer < 0 || layer >= m->cfg.layers || rows <= 0 || rows > m->max_rows || (!ids && !weights)) { set_error("bad argument"); return PGMI_EINVAL; }
    PGMI_HIP(hipSetDevice(m->device));
    PGMI_HIP(hipStreamSynchronize(m->stream));
    const size_t o = (size_t)layer * m->moe.layer_stride, n = (size_t)rows * m->pg3_k;
    if (ids) PGMI_HIP(hipMemcpy(ids, m->moe.ids + o, n * 4, hipMemcpyDeviceToHost));
    if (weights) PGMI_HIP(hipMemcpy(weights, m->moe.wts + o, n * 4, hipMemcpyDeviceToHost));
    return PGMI_OK;
}

}  // extern "C"
