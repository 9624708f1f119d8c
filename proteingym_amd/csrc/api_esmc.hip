// ESM C (ESM Cambrian; proteingym/baselines/evoscale/esm/models/esmc.py, layers/{transformer_stack,blocks,attention,rotary,
// regression_head}.py): model creation and the forward behind pgmi_token_logprobs / pgmi_masked_logprobs (api_esm.hip dispatches here
// through run_rows).
//
// Per block (blocks.py:150-162), s = sqrt(n_layers / 36):
//   x += out_proj(attn(x)) / s     attn: LayerNorm(D) -> bias-free QKV -> q_ln / k_ln over the whole width -> rotate-half rotary ->
//                                  dense softmax attention with scale 1/8
//   x += ffn(x) / s                ffn: LayerNorm(D) -> Linear(D, 2F) -> silu(gate) * up -> Linear(F, D), all bias-free
// then the bias-free final LayerNorm and the head Linear(D, D) + erf-GELU + LayerNorm + Linear(D, 64) (untied), log-softmax over all
// 64 columns.  Device path (f16x3): the QKV GEMM writes fp32 rows, qkln_prep_kernel (attention_f16_prep.hip) normalises q and k and
// writes the attention operands, the dense head_dim-64 attention of ESM runs unchanged, FC1 runs the SwiGLU epilogue (gemm16x_kernel.h)
// and 1/s rides on the out-projection's and FC2's out_scale (1.0 for 36 layers: the same bits as no scaling).  The last layer runs
// its row-local stages on the kept (masked) rows only, as ESM's run_encoder does.
#include "model.h"

namespace pgmi {

int64_t esmc_weight_count(const pgmi_config* c) {
    const int64_t D = c->embed_dim, F = c->ffn_dim, V = c->vocab;
    const int64_t layer = 2 * D + 3 * D * D + 2 * D + D * D + 2 * D + 2 * F * D + D * F;
    return V * D + (int64_t)c->layers * layer + D + (D * D + D) + 2 * D + (V * D + V);
}

// Weight blob: include/pgmi.h (PGMI_ARCH_ESMC).
int create_esmc(pgmi_model* m, const pgmi_config* cfg, const float* w, int64_t n_weights) {
    const size_t D = cfg->embed_dim, F = cfg->ffn_dim, V = cfg->vocab;
    // transformer_stack.py:50: residual branches divided by sqrt(n_layers / 36); exactly 1 for 36 layers
    const float inv_s = 1.0f / sqrtf((float)cfg->layers / 36.0f);
    BlobCursor c(m, w, n_weights);
    c.upload(&m->embed_tokens, V * D);
    m->layers.resize(cfg->layers);
    std::vector<float> qw(D);
    for (int l = 0; l < cfg->layers; ++l) {
        Layer& L = m->layers[l];
        c.upload(&L.ln1_w, D);
        c.upload(&L.ln1_b, D);
        c.w16(&L.wqkv16, 3 * D * D, D);
        // F.scaled_dot_product_attention's 1/sqrt(64) = 2^-3 folded into q_ln's weight: exact
        const float* q = c.take(D);
        for (size_t i = 0; i < D; ++i) qw[i] = q[i] * 0.125f;
        c.upload(&L.q_ln, qw.data(), D);
        c.upload(&L.k_ln, D);
        c.w16(&L.wo16, D * D, D);
        c.upload(&L.ln2_w, D);
        c.upload(&L.ln2_b, D);
        c.w16(&L.w116, 2 * F * D, D);
        c.w16(&L.w216, D * F, F);
        L.wo16.out_scale *= inv_s;
        L.w216.out_scale *= inv_s;
    }
    c.upload(&m->lna_w, D);
    c.w16(&m->hd16, D * D, D);
    c.upload(&m->hd_b, D);
    c.upload(&m->hln_w, D);
    c.upload(&m->hln_b, D);
    c.upload(&m->esmc_head_w, V * D);
    c.upload(&m->h_bias, V);
    int rc = c.finish();
    if (!rc) rc = upload_rotate_half(m, 1026);
    return rc;
}

// Encoder + head on the tokens in m->tokens [B,T]; log-probabilities of the rows row_idx [R] (device) in m->lp [R,64], or of all
// R = B*T rows when row_idx == nullptr.
int run_esmc_rows(pgmi_model* m, int B, int T, int R, const int32_t* row_idx) {
    const pgmi_config& c = m->cfg;
    const int M = B * T, D = c.embed_dim, F = c.ffn_dim, H = c.heads;
    hipStream_t s = m->stream;
    int rc = PGMI_OK;
    if (T > m->rot_len) rc = upload_rotate_half(m, std::max(T, 1026));
    if (!rc) rc = reset_pad_keys(m, B, T);
    if (rc) return rc;
    { ProfScope p(m, PGMI_K_EMBED, 0, (double)M * D * 4);
      launch_seq_stats(m->tokens, B, T, 0, m->denom, m->pos_idx, m->kv_len, s);          // kv_len: keys before the first <pad>
      launch_gather_rows(m->embed_tokens, m->tokens, M, D, m->x, s); }                   // esmc.py: nn.Embedding(64, d), nothing else
    const double ln_bytes = 2.0 * M * D * 4;
    bool compacted = false;
    for (int l = 0; l < c.layers; ++l) {
        const Layer& L = m->layers[l];
        { ProfScope p(m, PGMI_K_LAYERNORM, 0, ln_bytes);
          launch_layernorm16(m->x, L.ln1_w, L.ln1_b, M, D, 1e-5f, m->h16, m->h16_plane, 1, s); }
        { ProfScope p(m, PGMI_K_GEMM_QKV, 2.0 * M * 3 * D * D, 0);
          rc = linear(m, nullptr, m->h16, m->h16_plane, nullptr, L.wqkv16, nullptr, nullptr, m->qkv, nullptr, 0, M, 3 * D, D, EPI_NONE);
          if (rc) return rc; }
        // the QK-LayerNorm prep pass is profiled as attention (it produces the attention's operands): PGMI_K_ATTENTION counts both
        { ProfScope p(m, PGMI_K_ATTENTION, 4.0 * M * T * D, (double)M * D * 20);
          rc = launch_qkln_prep(m->qkv, L.q_ln, L.k_ln, 1e-5f, m->rot_cos, m->rot_sin, B, T, H, m->qk16, m->qk16_plane, m->vt16,
                                m->vt16_plane, s);
          if (!rc) rc = launch_attention_f16x3_v2(nullptr, m->kv_len, m->rot_cos, m->rot_sin, 0, B, T, H, m->qk16, m->qk16_plane, m->vt16,
                                                  m->vt16_plane, nullptr, m->h16, m->h16_plane, 1, s, nullptr, nullptr, kHeadDim);
          if (rc) return rc; }
        if (row_idx && m->keep_rows && l == c.layers - 1) {
            // everything after the attention is row-local: the masked rows only (api_esm.hip run_encoder)
            ProfScope p(m, PGMI_K_KEPT_ROWS, 2.0 * R * D * (D + 3.0 * F), 0);
            launch_gather_rows(m->x, row_idx, R, D, m->qkv, s);                      // residual rows (qkv is free after the prep pass)
            launch_gather_rows(reinterpret_cast<const float*>(m->h16), row_idx, R, D, reinterpret_cast<float*>(m->g16), s);
            rc = linear(m, nullptr, m->g16, m->g16_plane, nullptr, L.wo16, nullptr, m->qkv, m->x, nullptr, 0, R, D, D, EPI_NONE);
            if (!rc) launch_layernorm16(m->x, L.ln2_w, L.ln2_b, R, D, 1e-5f, m->h16, m->h16_plane, 1, s);
            if (!rc) rc = linear(m, nullptr, m->h16, m->h16_plane, nullptr, L.w116, nullptr, nullptr, nullptr, m->g16, m->g16_plane, R, 2 * F, D, EPI_SWIGLU);
            if (!rc) rc = linear(m, nullptr, m->g16, m->g16_plane, nullptr, L.w216, nullptr, m->x, m->x, nullptr, 0, R, D, F, EPI_NONE);
            if (rc) return rc;
            compacted = true;
            break;
        }
        { ProfScope p(m, PGMI_K_GEMM_OUT, 2.0 * M * D * D, 0);
          rc = linear(m, nullptr, m->h16, m->h16_plane, nullptr, L.wo16, nullptr, m->x, m->x, nullptr, 0, M, D, D, EPI_NONE);
          if (rc) return rc; }
        { ProfScope p(m, PGMI_K_LAYERNORM, 0, ln_bytes);
          launch_layernorm16(m->x, L.ln2_w, L.ln2_b, M, D, 1e-5f, m->h16, m->h16_plane, 1, s); }
        { ProfScope p(m, PGMI_K_GEMM_FC1, 2.0 * M * 2 * F * D, 0);
          rc = linear(m, nullptr, m->h16, m->h16_plane, nullptr, L.w116, nullptr, nullptr, nullptr, m->g16, m->g16_plane, M, 2 * F, D, EPI_SWIGLU);
          if (rc) return rc; }
        { ProfScope p(m, PGMI_K_GEMM_FC2, 2.0 * M * F * D, 0);
          rc = linear(m, nullptr, m->g16, m->g16_plane, nullptr, L.w216, nullptr, m->x, m->x, nullptr, 0, M, D, F, EPI_NONE);
          if (rc) return rc; }
    }
    {
        ProfScope p(m, PGMI_K_HEAD, 2.0 * R * D * (D + c.vocab), 0);
        const float* src = m->x;
        if (row_idx && !compacted) {
            launch_gather_rows(m->x, row_idx, R, D, m->h, s);
            src = m->h;
        }
        // transformer_stack.py:62 (LayerNorm without bias), then regression_head.py
        launch_layernorm16(src, m->lna_w, m->zeros, R, D, 1e-5f, m->h16, m->h16_plane, 1, s);
        rc = linear(m, nullptr, m->h16, m->h16_plane, nullptr, m->hd16, m->hd_b, nullptr, m->g, nullptr, 0, R, D, D, EPI_GELU);
        if (rc) return rc;
        launch_layernorm(m->g, m->hln_w, m->hln_b, R, D, 1e-5f, m->g, s);
        launch_vocab_logsoftmax(m->g, m->esmc_head_w, m->h_bias, R, D, c.vocab, m->lp, m->nonfinite, s);
    }
    PGMI_HIP(hipGetLastError());
    return PGMI_OK;
}

}  // namespace pgmi
