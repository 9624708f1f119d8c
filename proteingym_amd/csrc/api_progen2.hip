// ProGen2 (proteingym/baselines/progen2/models/progen/modeling_progen.py): model creation, the forward and its C entries.
//
// Per layer (ProGenBlock, :252-283): h = ln_1(x);  x = x + out_proj(attn(h)) + fc_out(gelu_new(fc_in(h))) -- one LayerNorm, two
// branches that read it, both residual-adding into x.  The attention (:109-145, :147-224) is causal, scores in fp32 scaled by
// head_dim^-1/2, with GPT-J rotary on the first rotary_dim dims of q and k.  It runs on the kernels the other causal LM uses: the fused
// QKV epilogue (rotary, split planes, V^T) and attention_f16x3_v2 with all-zero ALiBi slopes (the ALiBi term is then exactly 0).
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
    const size_t D = cfg->embed_dim, F = cfg->ffn_dim, V = cfg->vocab, H = cfg->heads;
    const int dh = m->dh, G = m->rot_halves;
    const size_t Da = m->Da;
    if (rotary_dim < 2 || rotary_dim > dh || rotary_dim % 2) {
        set_error("ProGen2 rotary_dim %d: must be even and in [2, head_dim = %d]", rotary_dim, dh);
        return PGMI_EINVAL;
    }
    m->pg2_rotary = rotary_dim;
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
        c.w16(&L.w116, F * D, D);
        c.upload(&L.b1, F);
        c.w16(&L.w216, D * F, F);
        c.upload(&L.b2, D);
    }
    c.upload(&m->lna_w, D);
    c.upload(&m->lna_b, D);
    const float* head_w = c.take(V * D);
    c.upload(&m->pg2_head_w, head_w, V * D);
    c.upload(&m->pg2_aa_w, head_w + 5 * D, 25 * D);               // rows 5..29: the amino-acid columns (compute_fitness.py:67-70)
    const float* head_b = c.take(V);
    c.upload(&m->pg2_head_b, head_b, V);
    c.upload(&m->pg2_aa_b, head_b + 5, 25);
    const std::vector<float> zeros(std::max(3 * Da, D), 0.0f), zs(H, 0.0f);
    c.upload(&m->pg2_zero, zeros.data(), zeros.size());
    c.upload(&m->pg2_slopes, zs.data(), zs.size());
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

// ProGen2 forward on tokens in m->tokens [B,T]; leaves log-probabilities in m->lp: [B*T, 32] (aa_only = false) or the log-softmax over
// columns 5..29 only, [B*T, 25] (aa_only = true).
static int run_progen2(pgmi_model* m, int B, int T, bool aa_only) {
    const pgmi_config& c = m->cfg;
    const int M = B * T, D = c.embed_dim, F = c.ffn_dim, H = c.heads, Da = m->Da;
    hipStream_t s = m->stream;
    if (T > c.max_positions) { set_error("sequence of %d tokens exceeds the model context n_positions=%d", T, c.max_positions); return PGMI_EINVAL; }
    int rc = reset_pad_keys(m, B, T);
    if (rc) return rc;
    { ProfScope p(m, PGMI_K_EMBED, 0, (double)M * D * 4);
      launch_gather_rows(m->embed_tokens, m->tokens, M, D, m->x, s); }       // wte[input_ids]: no positional table, no embedding LayerNorm
    const double ln_bytes = 2.0 * M * D * 4;
    for (int l = 0; l < c.layers; ++l) {
        const Layer& L = m->layers[l];
        { ProfScope p(m, PGMI_K_LAYERNORM, 0, ln_bytes);
          launch_layernorm16(m->x, L.ln1_w, L.ln1_b, M, D, m->ln_eps, m->h16, m->h16_plane, 1, s); }
        { ProfScope p(m, PGMI_K_GEMM_QKV, 2.0 * M * 3 * Da * D, 0);
          rc = launch_gemm16_qkv(m->h16, m->h16_plane, L.wqkv16.p, L.wqkv16.plane, m->pg2_zero, M, Da, D, L.wqkv16.out_scale,
                                 m->qk16, m->qk16_plane, m->vt16, m->vt16_plane, m->rot_cos, m->rot_sin, 1, T, m->Hs,
                                 m->gemm_variant, s, m->rot_halves, false);
          if (rc) return rc; }
        // the MLP branch first: it reads ln_1's output, which the attention's context rows then overwrite in h16
        { ProfScope p(m, PGMI_K_GEMM_FC1, 2.0 * M * F * D, 0);
          rc = linear(m, nullptr, m->h16, m->h16_plane, nullptr, L.w116, L.b1, nullptr, nullptr, m->g16, m->g16_plane, M, F, D, EPI_GELU_TANH);
          if (rc) return rc; }
        { ProfScope p(m, PGMI_K_GEMM_FC2, 2.0 * M * F * D, 0);
          rc = linear(m, nullptr, m->g16, m->g16_plane, nullptr, L.w216, L.b2, m->x, m->x, nullptr, 0, M, D, F, EPI_NONE);
          if (rc) return rc; }
        { ProfScope p(m, PGMI_K_ATTENTION, 2.0 * M * T * Da, 0);             // causal: half of the 4 M T Da of a dense pass
          rc = launch_attention_f16x3_v2(nullptr, nullptr, m->rot_cos, m->rot_sin, 1, B, T, H, m->qk16, m->qk16_plane, m->vt16,
                                         m->vt16_plane, nullptr, m->h16, m->h16_plane, 1, s, nullptr, m->pg2_slopes, m->rot_halves * kHeadDim);
          if (rc) return rc; }
        { ProfScope p(m, PGMI_K_GEMM_OUT, 2.0 * M * D * Da, 0);
          rc = linear(m, nullptr, m->h16, m->h16_plane, nullptr, L.wo16, m->pg2_zero, m->x, m->x, nullptr, 0, M, D, Da, EPI_NONE);
          if (rc) return rc; }
    }
    const int Vh = aa_only ? 25 : c.vocab;
    { ProfScope p(m, PGMI_K_HEAD, 2.0 * M * D * Vh, 0);
      launch_layernorm(m->x, m->lna_w, m->lna_b, M, D, m->ln_eps, m->h, s);
      launch_vocab_logsoftmax(m->h, aa_only ? m->pg2_aa_w : m->pg2_head_w, aa_only ? m->pg2_aa_b : m->pg2_head_b, M, D, Vh, m->lp,
                              m->nonfinite, s); }
    PGMI_HIP(hipGetLastError());
    return PGMI_OK;
}

static int pg2_check(pgmi_model* m, int T) {
    if (m->cfg.arch != PGMI_ARCH_PROGEN2) { set_error("not a ProGen2 model"); return PGMI_EINVAL; }
    if (T > m->cfg.max_positions) { set_error("sequence of %d tokens exceeds the model context n_positions=%d", T, m->cfg.max_positions); return PGMI_EINVAL; }
    if (T + 31 > m->max_rows) { set_error("T=%d exceeds workspace rows %d", T, m->max_rows); return PGMI_EINVAL; }
    return PGMI_OK;
}

}  // namespace pgmi

extern "C" {

int pgmi_pg2_model_create(const pgmi_config* cfg, int rotary_dim, const float* weights, int64_t n_weights, int device, pgmi_model** out) {
    if (out) *out = nullptr;
    if (!cfg || cfg->arch != PGMI_ARCH_PROGEN2) { set_error("pgmi_pg2_model_create: arch must be PGMI_ARCH_PROGEN2"); return PGMI_EINVAL; }
    return model_create(cfg, weights, n_weights, device, out, rotary_dim);
}

int pgmi_pg2_token_logprobs(pgmi_model* m, const int32_t* tokens, int B, int T, float* out) {
    if (!m || !tokens || !out || B <= 0 || T <= 0) { set_error("bad argument"); return PGMI_EINVAL; }
    int rc = pg2_check(m, T);
    if (rc) return rc;
    const int V = m->cfg.vocab;
    rc = check_vocab(tokens, B, T, V);
    if (rc) return rc;
    PGMI_HIP(hipSetDevice(m->device));
    rc = for_each_chunk(m, B, T, [&](int b0, int bc) {
        PGMI_HIP(hipMemcpyAsync(m->tokens, tokens + (size_t)b0 * T, (size_t)bc * T * 4, hipMemcpyHostToDevice, m->stream));
        int rc = run_progen2(m, bc, T, false);
        if (rc) return rc;
        PGMI_HIP(hipMemcpyAsync(out + (size_t)b0 * T * V, m->lp, (size_t)bc * T * V * 4, hipMemcpyDeviceToHost, m->stream));
        return PGMI_OK;
    });
    return rc ? rc : check_nonfinite(m);
}

int pgmi_pg2_sequence_loglik(pgmi_model* m, const int32_t* tokens, int B, int L, float* out, int32_t* n_kept) {
    if (!m || !tokens || !out || B <= 0) { set_error("bad argument"); return PGMI_EINVAL; }
    if (L < 2) { set_error("rows of %d tokens: the model needs at least one input and one target token", L); return PGMI_EINVAL; }
    const int T = L - 1;                                            // input = ids[:-1], targets = ids[1:]
    int rc = pg2_check(m, T);
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
        int rc = run_progen2(m, bc, T, true);
        if (rc) return rc;
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
