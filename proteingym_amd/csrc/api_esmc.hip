// ESM C (ESM Cambrian; proteingym/baselines/evoscale/esm/models/esmc.py, layers/{transformer_stack,blocks,attention,rotary,
// regression_head}.py): model creation.  The forward behind pgmi_token_logprobs / pgmi_masked_logprobs is ESM's (api_esm.hip
// run_encoder, run_head), steered by what this file stores on the model and its layers.
//
// Per block (blocks.py:150-162), s = sqrt(n_layers / 36):
//   x += out_proj(attn(x)) / s     attn: LayerNorm(D) -> bias-free QKV -> q_ln / k_ln over the whole width -> rotate-half rotary ->
//                                  dense softmax attention with scale 1/8
//   x += ffn(x) / s                ffn: LayerNorm(D) -> Linear(D, 2F) -> silu(gate) * up -> Linear(F, D), all bias-free
// then the bias-free final LayerNorm and the head Linear(D, D) + erf-GELU + LayerNorm + Linear(D, 64) (untied), log-softmax over all
// 64 columns.  Device path (f16x3): the embedding is a plain table gather (embed_gather); a layer with q_ln runs the QKV GEMM into
// fp32 rows and qkln_prep_kernel (attention_f16_prep.hip) normalises q and k and writes the attention operands, the dense head_dim-64
// attention of ESM runs unchanged; FC1 runs the SwiGLU epilogue (gemm16x_kernel.h) with 2F columns; 1/s rides on the
// out-projection's and FC2's out_scale (1.0 for 36 layers: the same bits as no scaling); the bias-free projections have null
// biases, the final LayerNorm the model's zeros.  The last layer runs its row-local stages on the kept (masked) rows only.
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
    m->lna_b = m->zeros;                                           // transformer_stack.py:62: LayerNorm without bias
    c.w16(&m->hd16, D * D, D);
    c.upload(&m->hd_b, D);
    c.upload(&m->hln_w, D);
    c.upload(&m->hln_b, D);
    c.upload(&m->head_w, V * D);
    c.upload(&m->head_b, V);
    m->embed_gather = true;                                        // esmc.py: nn.Embedding(64, d), nothing else
    m->fc1_epi = EPI_SWIGLU;
    m->fc1_cols = 2 * (int)F;
    return c.finish();
}

}  // namespace pgmi
