// ProGen2 (proteingym/baselines/progen2/models/progen/modeling_progen.py): model creation, the 25-column amino-acid head of the
// scoring entry and the C entries.
//
// Per layer (ProGenBlock, :252-283): h = ln_1(x);  x = x + out_proj(attn(h)) + fc_out(gelu_new(fc_in(h))) -- one LayerNorm, two
// branches that read it, both residual-adding into x.  The attention (:109-145, :147-224) is causal, scores in fp32 scaled by
// head_dim^-1/2, with GPT-J rotary on the first rotary_dim dims of q and k.  The forward is the causal decoder's (api_gpt.hip) in its
// parallel-residual order: the fused QKV epilogue (rotary, split planes, V^T) and attention_f16x3_v2 with all-zero ALiBi slopes (the
// ALiBi term is then exactly 0); the bias-free projections pass the model's zero vector as their bias.
#include "model.h"

namespace pgmi {

// Slot layout of one head.  The fused QKV epilogue rotates the slot pairs (i, i + 32) of every 64-lane slot group with one angle per
// (group, i) from the rotary tables; GPT-J rotates the interleaved dim pairs (2p, 2p + 1) with inv_freq index p.  So pair p goes to
// slots (i, i + 32) of group p / 32, i = p % 32, and the pass-through dims rotary_dim .. dh-1 fill the pair positions after the last
// rotary pair, two at a time, with cos 1 / sin 0 (exact).  Slots no dim takes (dh < 64 G) stay zero: zero q / k / v lanes change no
// score and no context value.
static int pg2_slot(int j, int rd) {
    const int k = j < rd ? j : j - rd;                           // index inside the rotary run / the pass-through run
    const int p = (j < rd ? 0 : rd / 2) + k / 2;                 // pair position within the head
    return (p / 32) * 64 + (p % 32) + 32 * (k & 1);
}

int create_progen2(pgmi_model* m, const pgmi_config* cfg, const float* w, int64_t n_weights, int rotary_dim) {
    const size_t D = cfg->embed_dim, F = cfg->ffn_dim, V = cfg->vocab;
    const int dh = m->dh, G = m->rot_halves;
    const size_t Da = m->Da;
    if (rotary_dim < 2 || rotary_dim > dh || rotary_dim % 2) {
        set_error("ProGen2 rotary_dim %d: must be even and in [2, head_dim = %d]", rotary_dim, dh);
        return PGMI_EINVAL;
    }
    m->pg2_rotary = rotary_dim;
    m->parallel_residual = true;                                   // the decoder body: no positional table, q / k rotated by the tables
    m->slopes = m->zeros;
    m->final_norm = true;
    m->fc1_epi = EPI_GELU_TANH;
    BlobCursor c(m, w, n_weights);
    c.upload(&m->embed_tokens, V * D);
    auto slot = [&](size_t col) -> size_t {                        // attention column of model dim `col` (head-major)
        const size_t h = col / dh;
        return h * G * 64 + pg2_slot((int)(col % dh), rotary_dim);
    };
    // scale_attn = sqrt(head_dim) (:87, :121): folded into the q rows; rotary is linear, so scaling before it is the same map
    const float qscale = 1.0f / sqrtf((float)dh);
    m->layers.resize(cfg->layers);
    std::vector<float> wq(3 * Da * D, 0.0f), wo_r(D * Da, 0.0f);
    for (int l = 0; l < cfg->layers; ++l) {
        Layer& L = m->layers[l];
        c.upload(&L.ln1_w, D);
        c.upload(&L.ln1_b, D);
        pack_qkv_slots(c.take(3 * D * D), D, Da, slot, qscale, wq.data());   // q | k | v blocks of the host-reordered projection
        c.w16(&L.wqkv16, wq.data(), wq.size(), D);
        pack_out_cols(c.take(D * D), D, Da, slot, wo_r.data());
        c.w16(&L.wo16, wo_r.data(), wo_r.size(), Da);
        L.bqkv = L.bo = m->zeros;                                  // qkv_proj and out_proj have no bias
        c.w16(&L.w116, F * D, D);
        c.upload(&L.b1, F);
        c.w16(&L.w216, D * F, F);
        c.upload(&L.b2, D);
    }
    c.upload(&m->lna_w, D);
    c.upload(&m->lna_b, D);
    const float* head_w = c.take(V * D);
    c.upload(&m->head_w, head_w, V * D);
    c.upload(&m->pg2_aa_w, head_w + 5 * D, 25 * D);               // rows 5..29: the amino-acid columns (compute_fitness.py:67-70)
    const float* head_b = c.take(V);
    c.upload(&m->head_b, head_b, V);
    c.upload(&m->pg2_aa_b, head_b + 5, 25);
    int rc = c.finish();
    if (rc) return rc;
    // cos / sin tables: slot i and 32 + i of group g hold the angle of pair position 32 g + i.  The angle is fp32(t) * inv_freq in
    // fp32 as fixed_pos_embedding computes it (:38-43); an fp64 angle would drift by ~1e-4 rad at t ~ 1000.
    const int half = rotary_dim / 2;
    std::vector<float> inv(half);
    for (int i = 0; i < half; ++i) inv[i] = 1.0f / powf(10000.0f, (float)(2 * i) / (float)rotary_dim);
    return upload_rotary(m, cfg->max_positions, G, [&](int t, int g, int i) {
        const int p = 32 * g + i;
        return p < half ? (float)t * inv[p] : 0.0f;                // pass-through pairs: cos 1, sin 0
    });
}

}  // namespace pgmi

extern "C" {

int pgmi_pg2_model_create(const pgmi_config* cfg, int rotary_dim, const float* weights, int64_t n_weights, int device, pgmi_model** out) {
    if (out) *out = nullptr;
    if (!cfg || cfg->arch != PGMI_ARCH_PROGEN2) { set_error("pgmi_pg2_model_create: arch must be PGMI_ARCH_PROGEN2"); return PGMI_EINVAL; }
    return model_create(cfg, weights, n_weights, device, out, rotary_dim);
}

int pgmi_pg2_token_logprobs(pgmi_model* m, const int32_t* tokens, int B, int T, float* out) {
    return decoder_token_logprobs(m, PGMI_ARCH_PROGEN2, tokens, B, T, out);
}

int pgmi_pg2_sequence_loglik(pgmi_model* m, const int32_t* tokens, int B, int L, float* out, int32_t* n_kept) {
    if (!m || !tokens || !out || B <= 0) { set_error("bad argument"); return PGMI_EINVAL; }
    if (L < 2) { set_error("rows of %d tokens: the model needs at least one input and one target token", L); return PGMI_EINVAL; }
    const int T = L - 1;                                            // input = ids[:-1], targets = ids[1:]
    int rc = decoder_check(m, PGMI_ARCH_PROGEN2, T);
    if (!rc) rc = check_vocab(tokens, B, L, m->cfg.vocab);
    if (rc) return rc;
    std::vector<int32_t> in((size_t)B * T), col((size_t)B * T, 0), kept(B);
    for (int b = 0; b < B; ++b) {
        const int32_t* row = tokens + (size_t)b * L;
        int n = T;
        if (row[L - 1] == 3 || row[L - 1] == 4) --n;               // compute_fitness.py:59-62: drop a terminal last target
        for (int t = 0; t < n; ++t) {
            const int tg = row[t + 1];
            if (tg < 5 || tg > 29) { set_error("row %d of this call: target %d at position %d is not an amino-acid token (5..29)", b, tg, t + 1); return PGMI_EINVAL; }
            col[(size_t)b * T + t] = tg - 5;
        }
        memcpy(&in[(size_t)b * T], row, (size_t)T * 4);
        kept[b] = n;
    }
    PGMI_HIP(hipSetDevice(m->device));
    hipStream_t s = m->stream;
    rc = for_each_chunk(m, B, T, [&](int b0, int bc) {
        PGMI_HIP(hipMemcpyAsync(m->tokens, in.data() + (size_t)b0 * T, (size_t)bc * T * 4, hipMemcpyHostToDevice, s));
        PGMI_HIP(hipMemcpyAsync(m->aux_i, col.data() + (size_t)b0 * T, (size_t)bc * T * 4, hipMemcpyHostToDevice, s));
        PGMI_HIP(hipMemcpyAsync(m->kv_len, kept.data() + b0, (size_t)bc * 4, hipMemcpyHostToDevice, s));
        int rc = run_decoder(m, bc, T);
        if (rc) return rc;
        const int M = bc * T, D = m->cfg.embed_dim;
        { ProfScope p(m, PGMI_K_HEAD, 2.0 * M * D * 25, 0);           // ln_f, then the log-softmax over columns 5..29 only
          launch_layernorm(m->x, m->lna_w, m->lna_b, M, D, m->ln_eps, m->h, s);
          launch_vocab_logsoftmax(m->h, m->pg2_aa_w, m->pg2_aa_b, M, D, 25, m->lp, m->nonfinite, s); }
        PGMI_HIP(hipGetLastError());
        { ProfScope p(m, PGMI_K_SCORE, 0, (double)bc * T * 8);
          launch_pg2_seq_loglik(m->lp, m->aux_i, m->kv_len, bc, T, 25, m->denom, s); }
        PGMI_HIP(hipMemcpyAsync(out + b0, m->denom, (size_t)bc * 4, hipMemcpyDeviceToHost, s));
        return PGMI_OK;
    });
    if (rc) return rc;
    if (n_kept) memcpy(n_kept, kept.data(), (size_t)B * 4);
    return check_nonfinite(m);
}

}  // extern "C"
