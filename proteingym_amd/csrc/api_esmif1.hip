// ESM-IF1 (proteingym/baselines/esm/esm/inverse_folding: gvp_transformer.py GVPTransformerModel, transformer_decoder.py,
// transformer_layer.py TransformerDecoderLayer): the DECODER -- model creation, the per-layer K / V^T planes of one encoded backbone,
// token log-probabilities / per-sequence mean log-likelihoods given those planes, and the C entries.  The encoder (featuriser, k-NN
// graph, GVP-GNN, 8 transformer layers) is one forward of L + 2 rows per structure and runs on the host side (proteingym_amd/esmif1.py).
//
// Decoder: x = sqrt(D) embed_tokens[tok] + sinusoidal(padding_idx + 1 + t); per layer (pre-LN, no dropout at inference)
//   x += out_proj(self_attn(self_attn_layer_norm(x)))                       causal within the sequence, q / k / v / out with biases
//   x += out_proj(encoder_attn(encoder_attn_layer_norm(x), memory))         q from the decoder row, k / v from the S encoder rows, unmasked
//   x += fc2(relu(fc1(final_layer_norm(x))))
// then layer_norm and output_projection [V, D] (no bias).  q is scaled by head_dim^-1/2 in both attentions (multihead_attention.py).
// compute_fitness_esm_if1.py hands every batch of mutants the same coordinates and runs the whole model on them; here
// pgmi_esmif1_set_memory projects the encoder output through every layer's k_proj / v_proj once and writes the planes into the prefix
// cache in the operand layout of attention_prefix.hip; every decoder launch reads them as the shared prefix of its cross-attention
// (launch_cross_attention); its self-attention is the causal decoder's (fused QKV epilogue + attention_f16.hip with zero ALiBi slopes)
// over runs of sequences of one length.  Rows are packed (no pad rows): every stage is row-local or, in the attentions, local to (row,
// its sequence, the memory), so a sequence's numbers do not depend on what shares its launch.  Decoder length and memory length are
// independent.
#include "model.h"

namespace pgmi {

constexpr int kIf1PosLen = 16384;           // sinusoidal table rows = the longest sequence (tokens, <cath> included)
constexpr int kIf1PaddingIdx = 1;           // esm/data.py Alphabet: <pad>

int if1_check(const pgmi_config* c, int enc_dim) {
    if (c->layers <= 0 || c->embed_dim <= 0 || c->heads <= 0 || c->ffn_dim <= 0) { set_error("non-positive model dimension"); return PGMI_EINVAL; }
    if (c->embed_dim % c->heads || c->embed_dim / c->heads != kHeadDim) {
        set_error("unsupported decoder head_dim (embed_dim %d / heads %d): ESM-IF1's attention runs head_dim 64 only", c->embed_dim, c->heads);
        return PGMI_EINVAL;
    }
    if (c->ffn_dim % 32) { set_error("ESM-IF1: decoder_ffn_embed_dim %d must be a multiple of 32", c->ffn_dim); return PGMI_EINVAL; }
    if (enc_dim <= 0 || enc_dim % 32) { set_error("ESM-IF1: encoder_embed_dim %d must be a positive multiple of 32", enc_dim); return PGMI_EINVAL; }
    if (c->vocab <= 0 || c->vocab > kWave) { set_error("ESM-IF1 vocab must be in [1, 64], got %d", c->vocab); return PGMI_EINVAL; }
    if (c->precision != PGMI_PREC_F16X3) { set_error("ESM-IF1 is available in precision f16x3 only"); return PGMI_EINVAL; }
    if (c->max_positions <= 0) { set_error("ESM-IF1: max_positions is the largest encoder memory in rows (residues + 2)"); return PGMI_EINVAL; }
    return PGMI_OK;
}

int64_t if1_weight_count(const pgmi_config* c, int enc_dim) {
    const int64_t D = c->embed_dim, F = c->ffn_dim, V = c->vocab, E = enc_dim;
    const int64_t self_att = 2 * D + 4 * (D * D + D), cross = 2 * D + (D * D + D) + 2 * (D * E + D) + (D * D + D);
    return V * D + (int64_t)c->layers * (self_att + cross + 2 * D + (F * D + F) + (D * F + D)) + 2 * D + V * D;
}

int create_esmif1(pgmi_model* m, const pgmi_config* cfg, const float* w, int64_t n_weights, int enc_dim) {
    const size_t D = cfg->embed_dim, F = cfg->ffn_dim, V = cfg->vocab, Da = m->Da, E = enc_dim;
    m->if1_enc = enc_dim;
    m->final_norm = true;
    m->slopes = m->zeros;                                       // the causal self-attention's ALiBi term is exactly 0
    m->fc1_epi = EPI_RELU;
    BlobCursor c(m, w, n_weights);
    c.upload(&m->embed_tokens, V * D);
    auto slot = [](size_t col) { return col; };                 // head_dim 64: a head's dims are its 64 lanes
    const float qscale = 1.0f / sqrtf((float)m->dh);
    m->layers.resize(cfg->layers);
    std::vector<float> wq(3 * Da * D), bq(3 * Da), cq(Da * D), cqb(Da), ckv(3 * Da * E), ckvb(3 * Da);
    for (int l = 0; l < cfg->layers; ++l) {
        Layer& L = m->layers[l];
        c.upload(&L.ln1_w, D);
        c.upload(&L.ln1_b, D);
        pack_qkv_slots(c.take(3 * (D * D + D)), D, Da, slot, qscale, wq.data(), bq.data());
        c.w16(&L.wqkv16, wq.data(), wq.size(), D);
        c.upload(&L.bqkv, bq.data(), bq.size());
        c.w16(&L.wo16, D * D, Da);
        c.upload(&L.bo, D);
        c.upload(&L.c_ln_w, D);                                 // c_*: encoder_attn
        c.upload(&L.c_ln_b, D);
        const float* q = c.take(D * D + D);                     // q_proj [D, D], b: scaled, applied to the decoder rows
        for (size_t i = 0; i < D * D; ++i) cq[i] = q[i] * qscale;
        for (size_t i = 0; i < D; ++i) cqb[i] = q[D * D + i] * qscale;
        c.w16(&L.c_wq16, cq.data(), cq.size(), D);
        c.upload(&L.c_bq, cqb.data(), cqb.size());
        // k_proj, v_proj [D, E], b each: rows Da .. 3 Da of a fused projection whose q block is zero, so that the prep pass of
        // attention_prefix.hip (fp32 q | k | v rows -> planes, as PoET's prompt fills its cache) writes the memory planes; S rows per structure and layer
        std::fill(ckv.begin(), ckv.end(), 0.0f);
        std::fill(ckvb.begin(), ckvb.end(), 0.0f);
        for (size_t k = 1; k < 3; ++k) {
            const float* kv = c.take(D * E + D);
            memcpy(&ckv[k * Da * E], kv, D * E * sizeof(float));
            memcpy(&ckvb[k * Da], kv + D * E, D * sizeof(float));
        }
        c.w16(&L.c_wqkv16, ckv.data(), ckv.size(), E);
        c.upload(&L.c_bqkv, ckvb.data(), ckvb.size());
        c.w16(&L.c_wo16, D * D, Da);
        c.upload(&L.c_bo, D);
        c.upload(&L.ln2_w, D);                                  // final_layer_norm
        c.upload(&L.ln2_b, D);
        c.w16(&L.w116, F * D, D);
        c.upload(&L.b1, F);
        c.w16(&L.w216, D * F, F);
        c.upload(&L.b2, D);
    }
    c.upload(&m->lna_w, D);                                     // decoder.layer_norm
    c.upload(&m->lna_b, D);
    c.upload(&m->head_w, V * D);                                // output_projection (no bias)
    m->head_b = m->zeros;
    int rc = c.finish();
    if (rc) return rc;
    // esm/modules.py SinusoidalPositionalEmbedding.get_embedding: row p = sin(p f_i) | cos(p f_i), f_i = exp(-i ln(10000) / (D / 2 - 1)),
    // fp32 frequencies and angles as the reference forms them; table row t is position padding_idx + 1 + t (make_positions without <pad>)
    m->if1_pos_len = std::min(kIf1PosLen, m->max_rows);
    {
        const size_t half = D / 2;
        std::vector<float> tab((size_t)m->if1_pos_len * D, 0.0f), freq(half);
        const float step = half > 1 ? (float)(log(10000.0) / (double)(half - 1)) : 0.0f;
        for (size_t i = 0; i < half; ++i) freq[i] = expf((float)i * -step);
        for (int t = 0; t < m->if1_pos_len; ++t) {
            const float p = (float)(kIf1PaddingIdx + 1 + t);
            float* row = &tab[(size_t)t * D];
            for (size_t i = 0; i < half; ++i) { const float a = p * freq[i]; row[i] = (float)sin((double)a); row[half + i] = (float)cos((double)a); }
        }
        rc = dev_upload(m->allocs, &m->if1_pos, tab.data(), tab.size());
        if (rc) return rc;
    }
    rc = alloc_prefix_cache(m);
    if (!rc) rc = dev_alloc(m->allocs, &m->if1_mem, (size_t)cfg->max_positions * E);
    if (!rc) rc = dev_alloc(m->allocs, &m->if1_mem16, (size_t)cfg->max_positions * E * 2);
    return rc;
}

// The decoder over B sequences of T rows each, packed (tokens in m->tokens, positions in m->pos_idx, the segments again in pl for the
// cross-attention's query tiles); leaves the residual stream in m->x.
static int if1_forward(pgmi_model* m, int B, int T, const SegPlan& pl) {
    const pgmi_config& c = m->cfg;
    const int M = B * T, D = c.embed_dim, Da = m->Da, S = m->pfx.rows;
    hipStream_t s = m->stream;
    int rc = reset_pad_keys(m, B, T);
    if (rc) return rc;
    { ProfScope p(m, PGMI_K_EMBED, 0, 2.0 * M * D * 4);
      launch_embed_scaled_pos(m->tokens, m->pos_idx, m->embed_tokens, m->if1_pos, sqrtf((float)D), M, D, m->x, s); }
    PrefixAttLaunch ca = prefix_launch(m, pl);                   // cross-attention over a layer's memory planes
    ca.ppitch = m->pfx.pitch; ca.P = S;
    for (int l = 0; l < c.layers; ++l) {
        const Layer& L = m->layers[l];
        rc = self_attention(m, L, B, T);                         // the causal decoder's, with zero ALiBi slopes and no rotary
        if (rc) return rc;
        { ProfScope p(m, PGMI_K_LAYERNORM, 0, 2.0 * M * D * 4);
          launch_layernorm16(m->x, L.c_ln_w, L.c_ln_b, M, D, m->ln_eps, m->h16, 1, s); }
        { ProfScope p(m, PGMI_K_GEMM_QKV, 2.0 * M * Da * D, 0);
          rc = linear(m, nullptr, m->h16, nullptr, L.c_wq16, L.c_bq, nullptr, m->qkv, nullptr, M, Da, D, EPI_NONE);
          if (rc) return rc; }
        { ca.pk16 = m->pfx.k(l); ca.pvt16 = m->pfx.vt(l);
          ProfScope p(m, PGMI_K_CROSS_ATTENTION, 4.0 * (double)M * S * Da, 0);
          rc = launch_cross_q_prep(m->qkv, (size_t)M, ca.H, ca.q16, ca.q_plane, s);
          if (!rc) rc = launch_cross_attention(ca);
          if (rc) return rc; }
        rc = out_proj(m, L.c_wo16, L.c_bo, M);
        if (!rc) rc = ffn(m, L, M);
        if (rc) return rc;
    }
    PGMI_HIP(hipGetLastError());
    return PGMI_OK;
}

static int if1_model_check(pgmi_model* m) {
    if (!m) { set_error("null model"); return PGMI_EINVAL; }
    if (m->cfg.arch != PGMI_ARCH_ESMIF1) { set_error("not an ESM-IF1 decoder"); return PGMI_EINVAL; }
    return PGMI_OK;
}

// Sequences right-padded (the pad value is not read), the prepended <cath> counted in lens[b]; the log-likelihood is the mean over all
// lens[b] - 1 targets.  A chunk is a run of sequences of ONE length (the dense causal attention takes B x T): a sequence goes through
// the same kernels at the same T whatever surrounds it.
static int if1_sequences(pgmi_model* m, const int32_t* tokens, const int32_t* lens, int B, int T, bool loglik, float* out, double* mean) {
    int rc = if1_model_check(m);
    if (rc) return rc;
    PackedScorer e = {};
    e.forward = [](pgmi_model* m, int bc, int R, const SegPlan& pl) { return if1_forward(m, bc, R / bc, pl); };
    e.pos_len = m->if1_pos_len; e.pos_what = "positions";
    e.not_ready = m->pfx.rows > 0 ? nullptr : "no encoder memory is set (pgmi_esmif1_set_memory)";
    e.same_length = e.vocab_per_row = e.mean = true;
    e.skip_target = -1;
    return score_packed(m, e, tokens, lens, B, T, loglik, out, mean);
}

}  // namespace pgmi

extern "C" {

int64_t pgmi_esmif1_weight_count(const pgmi_config* cfg, int enc_dim) {
    if (!cfg || cfg->layers <= 0 || cfg->embed_dim <= 0 || cfg->ffn_dim <= 0 || cfg->vocab <= 0 || enc_dim <= 0) return -1;
    return if1_weight_count(cfg, enc_dim);
}

int pgmi_esmif1_model_create(const pgmi_config* cfg, int enc_dim, const float* weights, int64_t n_weights, int device, pgmi_model** out) {
    if (out) *out = nullptr;
    if (!cfg || cfg->arch != PGMI_ARCH_ESMIF1) { set_error("pgmi_esmif1_model_create: arch must be PGMI_ARCH_ESMIF1"); return PGMI_EINVAL; }
    return model_create(cfg, weights, n_weights, device, out, enc_dim);
}

int pgmi_esmif1_set_memory(pgmi_model* m, const float* enc_out, int S) {
    int rc = if1_model_check(m);
    if (rc) return rc;
    m->pfx.rows = 0;                                              // whatever happens below, stale planes are never read
    if (!enc_out || S <= 0) { set_error("bad argument"); return PGMI_EINVAL; }
    if (S > m->cfg.max_positions) {
        set_error("encoder memory of %d rows: the planes were created for max_positions = %d", S, m->cfg.max_positions);
        return PGMI_EINVAL;
    }
    if (S > m->max_rows) { set_error("encoder memory of %d rows exceeds the workspace of %d rows", S, m->max_rows); return PGMI_EINVAL; }
    const size_t E = m->if1_enc, Da = m->Da;
    for (size_t i = 0; i < (size_t)S * E; ++i)
        if (!std::isfinite(enc_out[i])) { set_error("encoder memory: non-finite value at row %zu", i / E); return PGMI_EINVAL; }
    SegPlan pl;
    pl.add(S);
    PGMI_HIP(hipSetDevice(m->device));
    hipStream_t s = m->stream;
    PGMI_HIP(hipMemcpyAsync(m->if1_mem, enc_out, (size_t)S * E * 4, hipMemcpyHostToDevice, s));
    launch_split16(m->if1_mem, (int64_t)S * (int64_t)E, 1.0f, 2, (int)E, m->if1_mem16, s);
    rc = upload_plan(m, pl, 1);
    if (rc) return rc;
    for (int l = 0; l < m->cfg.layers; ++l) {
        const Layer& L = m->layers[l];
        { ProfScope p(m, PGMI_K_GEMM_QKV, 2.0 * S * 3 * Da * E, 0);
          rc = linear(m, nullptr, m->if1_mem16, nullptr, L.c_wqkv16, L.c_bqkv, nullptr, m->qkv, nullptr, S, 3 * (int)Da, (int)E, EPI_NONE);
          if (rc) return rc; }
        PrefixAttLaunch a = prefix_launch(m, pl);                // the prep pass over one segment of S rows: its K / V^T planes ARE the layer's cache
        a.qkv = m->qkv;
        a.k16 = m->pfx.k(l); a.vt16 = m->pfx.vt(l); a.pitch = m->pfx.pitch;
        ProfScope p(m, PGMI_K_CROSS_ATTENTION, 0, 4.0 * S * Da * 4);
        rc = launch_prefix_prep(a);
        if (rc) return rc;
    }
    PGMI_HIP(hipStreamSynchronize(s));
    m->pfx.rows = S;
    return PGMI_OK;
}

int pgmi_esmif1_token_logprobs(pgmi_model* m, const int32_t* tokens, const int32_t* lens, int B, int T, float* out) {
    return if1_sequences(m, tokens, lens, B, T, false, out, nullptr);
}

int pgmi_esmif1_sequence_loglik(pgmi_model* m, const int32_t* tokens, const int32_t* lens, int B, int T, double* out) {
    return if1_sequences(m, tokens, lens, B, T, true, nullptr, out);
}

}  // extern "C"
