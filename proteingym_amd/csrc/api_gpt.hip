// Causal decoder: RITA (proteingym/baselines/rita/rita_modeling.py) and ProtGPT2, a GPT-2 (transformers GPT2LMHeadModel;
// proteingym/baselines/protgpt2/compute_fitness.py), and the bodies of ProGen2 (api_progen2.hip) and Tranception (api_tranception.hip).
// Model creation of RITA / ProtGPT2, the forward, the LM heads and the C entries.
//
// Per layer, sequential pre-LN residual (rita_modeling.py:208-219; GPT2Block): x += out_proj(attn(ln_1(x)));
// x += fc_out(gelu_tanh(fc_in(ln_2(x)))).  Parallel residual (ProGen2, modeling_progen.py:252-283): h = ln_1(x);
// x += out_proj(attn(h)) + fc_out(gelu_new(fc_in(h))).  The attention runs on the fused QKV epilogue (RITA: ESM2's rotate-half rotary
// tables; ProGen2: GPT-J's, in the same layout) and attention_f16x3_v2 with all-zero ALiBi slopes (the ALiBi term is then exactly 0);
// Tranception's layers (L.conv) project into fp32 rows whose depth-wise convolution runs in the attention's prep pass, with its grouped
// ALiBi slopes, and FC1 ends in its squared ReLU.  Heads: V <= 64 (RITA: 26, ProGen2: 32) on one wave per row (vocab_logsoftmax_kernel);
// wider ones (ProtGPT2: 50 257, tied to wte) on the f16x3 GEMM into fp32 logits, then one workgroup per row (wide_logsoftmax_kernel).
// When scoring, only the rows that have a target reach the head.  ProGen3 (api_progen3.hip) runs on the same body with RMSNorm in place
// of LayerNorm and its routed expert block in place of the dense MLP, and on the wide head.
#include "model.h"

namespace pgmi {

static bool wide_head(const pgmi_config& c) { return c.vocab > kWave; }
constexpr int kWideHeadRows = 2048;        // logits rows per head GEMM: 2048 x 50 304 x 4 B = 412 MB at ProtGPT2's vocabulary

int64_t gpt_weight_count(const pgmi_config* c, int pos_kind) {
    if (pos_kind != PGMI_GPT_POS_ROTARY && pos_kind != PGMI_GPT_POS_LEARNED) return -1;
    const int64_t D = c->embed_dim, F = c->ffn_dim, V = c->vocab, P = c->max_positions;
    const int64_t layer = 2 * D + 3 * (D * D + D) + (D * D + D) + 2 * D + (F * D + F) + (D * F + D);
    return V * D + (pos_kind == PGMI_GPT_POS_LEARNED ? P * D : 0) + (int64_t)c->layers * layer + 2 * D +
           (pos_kind == PGMI_GPT_POS_ROTARY ? V * D : 0);
}

int create_gpt(pgmi_model* m, const pgmi_config* cfg, const float* w, int64_t n_weights, int pos_kind) {
    const size_t D = cfg->embed_dim, F = cfg->ffn_dim, V = cfg->vocab, dh = m->dh, Da = m->Da;
    const bool rotary = pos_kind == PGMI_GPT_POS_ROTARY;
    BlobCursor c(m, w, n_weights);
    const float* wte = c.take(V * D);
    c.upload(&m->embed_tokens, wte, V * D);
    if (!rotary) c.upload(&m->embed_positions, (size_t)cfg->max_positions * D);
    auto slot = [&](size_t col) -> size_t { return rotate_half_slot(col, dh); };
    // scores * head_dim^-1/2 (rita_modeling.py:153, after the rotary; GPT2Attention): rotary is linear, so the scale folds into q
    const float qscale = 1.0f / sqrtf((float)dh);
    m->layers.resize(cfg->layers);
    std::vector<float> wq(3 * Da * D, 0.0f), bq(3 * Da, 0.0f), wo_r(D * Da, 0.0f);
    for (int l = 0; l < cfg->layers; ++l) {
        Layer& L = m->layers[l];
        c.upload(&L.ln1_w, D);
        c.upload(&L.ln1_b, D);
        pack_qkv_slots(c.take(3 * (D * D + D)), D, Da, slot, qscale, wq.data(), bq.data());
        c.w16(&L.wqkv16, wq.data(), wq.size(), D);
        c.upload(&L.bqkv, bq.data(), bq.size());
        pack_out_cols(c.take(D * D), D, Da, slot, wo_r.data());
        c.w16(&L.wo16, wo_r.data(), wo_r.size(), Da);
        c.upload(&L.bo, D);
        c.upload(&L.ln2_w, D);
        c.upload(&L.ln2_b, D);
        c.w16(&L.w116, F * D, D);
        c.upload(&L.b1, F);
        c.w16(&L.w216, D * F, F);
        c.upload(&L.b2, D);
    }
    c.upload(&m->lna_w, D);
    c.upload(&m->lna_b, D);
    const float* head = rotary ? c.take(V * D) : wte;                // GPT-2: lm_head.weight is wte itself
    const size_t Vp = (V + 63) / 64 * 64;
    m->gpt_Vp = (int)Vp;
    m->slopes = m->zeros;
    m->final_norm = true;
    m->fc1_epi = EPI_GELU_TANH;
    if (!wide_head(*cfg)) {
        c.upload(&m->head_w, head, V * D);
        m->head_b = m->zeros;
    } else {
        // zero rows V .. Vp-1: whole 64-column GEMM tiles; the log-softmax excludes those columns by index
        std::vector<float> padded(Vp * D, 0.0f);
        memcpy(padded.data(), head, V * D * sizeof(float));
        c.w16(&m->gpt_head16, padded.data(), padded.size(), D);
        m->gpt_head_rows = std::min(m->max_rows, kWideHeadRows);
    }
    int rc = c.finish();
    if (!rc && m->gpt_head_rows) rc = dev_alloc(m->allocs, &m->gpt_logits, (size_t)m->gpt_head_rows * Vp);
    if (!rc) rc = dev_alloc(m->allocs, &m->gpt_sum, (size_t)m->max_rows);
    if (!rc && rotary) rc = upload_rotate_half(m, cfg->max_positions);
    return rc;
}

// A layer's or the head's norm of fp32 rows into the f16x3 split operand: LayerNorm, or ProGen3's weight-only RMSNorm (m->rms_norm)
static int norm16(pgmi_model* m, const float* x, const float* w, const float* b, int rows, unsigned short* y16) {
    if (m->rms_norm) return launch_rmsnorm16(x, w, rows, m->cfg.embed_dim, m->ln_eps, y16, m->stream);
    launch_layernorm16(x, w, b, rows, m->cfg.embed_dim, m->ln_eps, y16, 1, m->stream);
    return PGMI_OK;
}

// x += W ctx + b: an attention's out-projection of the context rows in m->h16 into the residual stream
int out_proj(pgmi_model* m, const W16& wo16, const float* bo, int M) {
    const int D = m->cfg.embed_dim, Da = m->Da;
    ProfScope p(m, PGMI_K_GEMM_OUT, 2.0 * M * D * Da, 0);
    return linear(m, nullptr, m->h16, nullptr, wo16, bo, m->x, m->x, nullptr, M, D, Da, EPI_NONE);
}

static int mlp(pgmi_model* m, const Layer& L, int M) {                // x += fc_out(act(fc_in(h16)))
    const int D = m->cfg.embed_dim, F = m->cfg.ffn_dim;
    { ProfScope p(m, PGMI_K_GEMM_FC1, 2.0 * M * F * D, 0);
      int rc = linear(m, nullptr, m->h16, nullptr, L.w116, L.b1, nullptr, nullptr, m->g16, M, F, D, m->fc1_epi);
      if (rc) return rc; }
    ProfScope p(m, PGMI_K_GEMM_FC2, 2.0 * M * F * D, 0);
    return linear(m, nullptr, m->g16, nullptr, L.w216, L.b2, m->x, m->x, nullptr, M, D, F, EPI_NONE);
}

int ffn(pgmi_model* m, const Layer& L, int M) {
    { ProfScope p(m, PGMI_K_LAYERNORM, 0, 2.0 * M * m->cfg.embed_dim * 4);
      int rc = norm16(m, m->x, L.ln2_w, L.ln2_b, M, m->h16);
      if (rc) return rc; }
    return mlp(m, L, M);
}

// What differs per model is data: rotary tables (m->rot_cos) or none, a layer's depth-wise convolution (L.conv), the slopes.
int self_attention(pgmi_model* m, const Layer& L, int B, int T, const AttRagged* rg, int rows, double att_flops) {
    const int M = rg ? rows : B * T, D = m->cfg.embed_dim, Da = m->Da;
    int rc;
    { ProfScope p(m, PGMI_K_LAYERNORM, 0, 2.0 * M * D * 4);
      rc = norm16(m, m->x, L.ln1_w, L.ln1_b, M, m->h16);
      if (rc) return rc; }
    { ProfScope p(m, PGMI_K_GEMM_QKV, 2.0 * M * 3 * Da * D, 0);
      if (L.conv)                           // fp32 q | k | v rows: the attention's prep pass convolves and splits them
          rc = linear(m, nullptr, m->h16, nullptr, L.wqkv16, L.bqkv, nullptr, m->qkv, nullptr, M, 3 * Da, D, EPI_NONE);
      else {                                // fused QKV: the epilogue writes the attention's operand planes
          GemmLaunch g = qkv_launch(m, L.wqkv16, L.bqkv, M, Da, D, T, m->Hs);
          g.qkv.cos_t = m->rot_cos; g.qkv.sin_t = m->rot_sin; g.qkv.rotary = m->rot_cos != nullptr; g.qkv.rot_halves = m->rot_halves;
          rc = launch_gemm16(g);
      }
      if (rc) return rc; }
    if (m->parallel_residual) {             // the MLP branch first: it reads ln_1's output, which the context rows then overwrite
        rc = mlp(m, L, M);
        if (rc) return rc;
    }
    { ProfScope p(m, PGMI_K_ATTENTION, rg ? att_flops : 2.0 * M * T * Da, 0);     // causal: half of the 4 M T Da of a dense pass
      AttLaunch a;
      a.qk16 = m->qk16, a.qk_plane = m->qk16_plane, a.vt16 = m->vt16, a.vt_plane = m->vt16_plane;
      a.B = B, a.T = T, a.H = m->cfg.heads, a.head_dim = m->rot_halves * kHeadDim;
      a.slopes = m->slopes;
      a.out = ATT_OUT_SPLIT, a.ctx16 = m->h16;
      a.stream = m->stream;
      if (L.conv) a.qkv = m->qkv, a.conv = L.conv;
      rc = rg ? launch_attention_tr_ragged(a, *rg) : launch_attention_f16x3_v2(a);
      if (rc) return rc; }
    return out_proj(m, L.wo16, L.bo, M);
}

// The decoder body on tokens in m->tokens; leaves the residual stream after the last layer in m->x.  Dense: B sequences of T tokens,
// [B*T, D].  Ragged (rg != nullptr; Tranception's prefix-shared scoring, api_tranception.hip): `rows` packed suffix rows of sequences
// of T tokens, their attention over rg (att_flops for the profile).  What differs per model is data: the position kind (rotary tables
// rot_cos, a learned table embed_positions, or none), a layer's depth-wise convolution (L.conv), the slopes, FC1's epilogue and the
// residual order, the norm (LayerNorm, or ProGen3's RMSNorm) and the feed-forward block (dense, or ProGen3's routed experts: pg3_ffn,
// which runs the layer's second norm itself, fused with its router).
int run_decoder(pgmi_model* m, int B, int T, const AttRagged* rg, int rows, double att_flops) {
    const pgmi_config& c = m->cfg;
    const int M = rg ? rows : B * T, D = c.embed_dim;
    hipStream_t s = m->stream;
    int rc = rg ? PGMI_OK : reset_pad_keys(m, B, T);
    if (rc) return rc;
    { ProfScope p(m, PGMI_K_EMBED, 0, (double)M * D * (m->embed_positions ? 8 : 4));
      if (m->embed_positions) launch_embed_learned(m->tokens, m->embed_tokens, m->embed_positions, M, T, D, m->x, s);
      else launch_gather_rows(m->embed_tokens, m->tokens, M, D, m->x, s); }       // RITA, ProGen2, Tranception: no positional table
    for (int l = 0; l < c.layers; ++l) {
        const Layer& L = m->layers[l];
        rc = self_attention(m, L, B, T, rg, rows, att_flops);
        if (!rc && c.arch == PGMI_ARCH_PROGEN3) rc = pg3_ffn(m, L, l, M);
        else if (!rc && !m->parallel_residual) rc = ffn(m, L, M);
        if (rc) return rc;
    }
    return PGMI_OK;
}

// The model's last LayerNorm (m->final_norm) and the narrow head (V <= 64): the log-softmax over all V columns of n rows into m->lp.
int narrow_head(pgmi_model* m, const float* src, int n) {
    const int D = m->cfg.embed_dim, V = m->cfg.vocab;
    ProfScope p(m, PGMI_K_HEAD, 2.0 * n * D * V, 0);
    if (m->final_norm) {
        launch_layernorm(src, m->lna_w, m->lna_b, n, D, m->ln_eps, m->h, m->stream);
        src = m->h;
    }
    launch_vocab_logsoftmax(src, m->head_w, m->head_b, n, D, V, m->lp, m->nonfinite, m->stream);
    PGMI_HIP(hipGetLastError());
    return PGMI_OK;
}

// Wide head on R rows whose ln_f output is in m->h16: per chunk of gpt_head_rows, fp32 logits [rc][Vp] from the f16x3 GEMM against
// wte (profiled as PGMI_K_HEAD), then the log-softmax (PGMI_K_SCORE).  tgt != nullptr: out[r] = log p(tgt[r]) on the device; else
// each chunk's full rows go to host_out [R][V] (the stream is synchronized per chunk: m->lp holds one chunk).
static int wide_head_rows(pgmi_model* m, int R, const int32_t* tgt, float* out, float* host_out) {
    const int D = m->cfg.embed_dim, V = m->cfg.vocab, Vp = m->gpt_Vp;
    for (int r0 = 0; r0 < R; r0 += m->gpt_head_rows) {
        const int rc_rows = std::min(m->gpt_head_rows, R - r0);
        { ProfScope p(m, PGMI_K_HEAD, 2.0 * rc_rows * Vp * D, 0);
          int rc = linear(m, nullptr, m->h16 + (size_t)r0 * 2 * D, nullptr, m->gpt_head16, m->zeros, nullptr,
                          m->gpt_logits, nullptr, rc_rows, Vp, D, EPI_NONE);
          if (rc) return rc; }
        { ProfScope p(m, PGMI_K_SCORE, 0, (double)rc_rows * V * 4 * (tgt ? 1 : 3));
          launch_wide_logsoftmax(m->gpt_logits, Vp, rc_rows, V, tgt ? tgt + r0 : nullptr, tgt ? out + r0 : m->lp, m->nonfinite, m->stream); }
        if (!tgt) {
            PGMI_HIP(hipMemcpyAsync(host_out + (size_t)r0 * V, m->lp, (size_t)rc_rows * V * 4, hipMemcpyDeviceToHost, m->stream));
            PGMI_HIP(hipStreamSynchronize(m->stream));
        }
    }
    return PGMI_OK;
}

int loglik_tail(pgmi_model* m, const int32_t* row_idx, int R, const int32_t* d_off, int bc, double* sum) {
    const int D = m->cfg.embed_dim, V = m->cfg.vocab;
    const bool wide = wide_head(m->cfg);
    hipStream_t s = m->stream;
    if (R > 0) {
        if (row_idx) {
            ProfScope p(m, PGMI_K_EMBED, 0, 2.0 * R * D * 4);
            launch_gather_rows(m->x, row_idx, R, D, m->g, s);
        }
        const float* src = row_idx ? m->g : m->x;
        int rc;
        if (wide) {
            { ProfScope p(m, PGMI_K_LAYERNORM, 0, 2.0 * R * D * 4);
              rc = norm16(m, src, m->lna_w, m->lna_b, R, m->h16);
              if (rc) return rc; }
            rc = wide_head_rows(m, R, m->aux_i, m->denom, nullptr);        // its log-softmax picks the targets itself
        } else rc = narrow_head(m, src, R);
        if (rc) return rc;
    }
    { ProfScope p(m, PGMI_K_SCORE, 0, (double)R * 8);
      if (R > 0 && !wide) launch_pppl_pick(m->lp, m->aux_i, R, V, m->denom, s);
      launch_seq_sum(m->denom, d_off, bc, m->gpt_sum, s); }
    PGMI_HIP(hipGetLastError());
    PGMI_HIP(hipMemcpyAsync(sum, m->gpt_sum, (size_t)bc * sizeof(double), hipMemcpyDeviceToHost, s));
    return PGMI_OK;
}

// Arch, context and workspace checks of a causal-decoder entry for input length T; `arch` is the entry's, the messages its own.
int decoder_check(pgmi_model* m, int arch, int T) {
    const bool pg2 = arch == PGMI_ARCH_PROGEN2, pg3 = arch == PGMI_ARCH_PROGEN3;
    if (m->cfg.arch != arch) { set_error(pg2 ? "not a ProGen2 model" : pg3 ? "not a ProGen3 model" : "not a causal decoder (RITA / ProtGPT2) model"); return PGMI_EINVAL; }
    if (T > m->cfg.max_positions) {
        set_error(pg2 ? "sequence of %d tokens exceeds the model context n_positions=%d"
                  : pg3 ? "sequence of %d tokens exceeds the rotary table of max_positions=%d rows"
                      : "sequence of %d tokens exceeds the model context of %d positions", T, m->cfg.max_positions);
        return PGMI_EINVAL;
    }
    if (T + 31 > m->max_rows) { set_error("T=%d exceeds workspace rows %d", T, m->max_rows); return PGMI_EINVAL; }
    return PGMI_OK;
}

// pgmi_gpt_token_logprobs and pgmi_pg2_token_logprobs: log-probabilities over all V columns, [B,T,V] to out.
int decoder_token_logprobs(pgmi_model* m, int arch, const int32_t* tokens, int B, int T, float* out) {
    if (!m || !tokens || !out || B <= 0 || T <= 0) { set_error("bad argument"); return PGMI_EINVAL; }
    int rc = decoder_check(m, arch, T);
    if (rc) return rc;
    const pgmi_config& c = m->cfg;
    const int V = c.vocab, D = c.embed_dim;
    rc = check_vocab(tokens, B, T, V);
    if (rc) return rc;
    PGMI_HIP(hipSetDevice(m->device));
    hipStream_t s = m->stream;
    rc = for_each_chunk(m, B, T, [&](int b0, int bc) {
        const int M = bc * T;
        PGMI_HIP(hipMemcpyAsync(m->tokens, tokens + (size_t)b0 * T, (size_t)M * 4, hipMemcpyHostToDevice, s));
        int rc = run_decoder(m, bc, T);
        if (rc) return rc;
        float* dst = out + (size_t)b0 * T * V;
        if (wide_head(c)) {
            { ProfScope p(m, PGMI_K_LAYERNORM, 0, 2.0 * M * D * 4);
              rc = norm16(m, m->x, m->lna_w, m->lna_b, M, m->h16);
              if (rc) return rc; }
            return wide_head_rows(m, M, nullptr, nullptr, dst);
        }
        rc = narrow_head(m, m->x, M);
        if (rc) return rc;
        PGMI_HIP(hipMemcpyAsync(dst, m->lp, (size_t)M * V * 4, hipMemcpyDeviceToHost, s));
        return PGMI_OK;
    });
    return rc ? rc : check_nonfinite(m);
}

// pgmi_gpt_sequence_loglik and pgmi_pg3_sequence_loglik.  ProGen3: the positions beyond a row's length go in as <pad> (0), which its
// router leaves out; a <pad> among a row's real tokens is refused.
int decoder_sequence_loglik(pgmi_model* m, int arch, const int32_t* tokens, const int32_t* lens, int B, int T, double* sum, int32_t* n_targets) {
    if (!m || !tokens || !lens || !sum || B <= 0) { set_error("bad argument"); return PGMI_EINVAL; }
    if (T < 2) { set_error("rows of %d tokens: the model needs at least one input and one target token", T); return PGMI_EINVAL; }
    const int Ti = T - 1;                                           // the model reads tokens[:, :T-1]; targets are tokens[:, 1:]
    int rc = decoder_check(m, arch, Ti);
    if (!rc) rc = check_vocab(tokens, B, T, m->cfg.vocab);
    if (rc) return rc;
    for (int b = 0; b < B; ++b)
        if (lens[b] < 2 || lens[b] > T) { set_error("row %d of this call: length %d outside [2, T = %d]", b, lens[b], T); return PGMI_EINVAL; }
    std::vector<int32_t> in((size_t)B * Ti), idx, tgt, off;
    for (int b = 0; b < B; ++b) memcpy(&in[(size_t)b * Ti], tokens + (size_t)b * T, (size_t)Ti * 4);
    if (arch == PGMI_ARCH_PROGEN3)
        for (int b = 0; b < B; ++b) {
            for (int t = 0; t < lens[b]; ++t)
                if (tokens[(size_t)b * T + t] == 0) { set_error("row %d of this call: <pad> at position %d, inside its %d tokens", b, t, lens[b]); return PGMI_EINVAL; }
            for (int t = lens[b]; t < Ti; ++t) in[(size_t)b * Ti + t] = 0;
        }
    PGMI_HIP(hipSetDevice(m->device));
    hipStream_t s = m->stream;
    rc = for_each_chunk(m, B, Ti, [&](int b0, int bc) {
        // the rows that have a target, in (sequence, position) order; sequence b owns [off[b], off[b+1])
        idx.clear(); tgt.clear(); off.assign(1, 0);
        for (int b = 0; b < bc; ++b) {
            const int32_t* row = tokens + (size_t)(b0 + b) * T;
            for (int t = 0; t + 1 < lens[b0 + b]; ++t) {
                idx.push_back(b * Ti + t);
                tgt.push_back(row[t + 1]);
            }
            off.push_back((int32_t)idx.size());
        }
        const int R = (int)idx.size();
        PGMI_HIP(hipMemcpyAsync(m->tokens, in.data() + (size_t)b0 * Ti, (size_t)bc * Ti * 4, hipMemcpyHostToDevice, s));
        PGMI_HIP(hipMemcpyAsync(m->row_idx, idx.data(), (size_t)R * 4, hipMemcpyHostToDevice, s));
        PGMI_HIP(hipMemcpyAsync(m->aux_i, tgt.data(), (size_t)R * 4, hipMemcpyHostToDevice, s));
        PGMI_HIP(hipMemcpyAsync(m->kv_len, off.data(), (size_t)(bc + 1) * 4, hipMemcpyHostToDevice, s));
        int rc = run_decoder(m, bc, Ti);
        return rc ? rc : loglik_tail(m, m->row_idx, R, m->kv_len, bc, sum + b0);     // pad rows and last rows never reach the head
    });
    if (rc) return rc;
    if (n_targets)
        for (int b = 0; b < B; ++b) n_targets[b] = lens[b] - 1;
    return check_nonfinite(m);
}

}  // namespace pgmi

extern "C" {

int64_t pgmi_gpt_weight_count(const pgmi_config* cfg, int pos_kind) {
    if (!cfg || cfg->layers <= 0 || cfg->embed_dim <= 0 || cfg->ffn_dim <= 0 || cfg->vocab <= 0 || cfg->max_positions <= 0) return -1;
    return gpt_weight_count(cfg, pos_kind);
}

int pgmi_gpt_model_create(const pgmi_config* cfg, int pos_kind, const float* weights, int64_t n_weights, int device, pgmi_model** out) {
    if (out) *out = nullptr;
    if (!cfg || cfg->arch != PGMI_ARCH_GPT) { set_error("pgmi_gpt_model_create: arch must be PGMI_ARCH_GPT"); return PGMI_EINVAL; }
    return model_create(cfg, weights, n_weights, device, out, pos_kind);
}

int pgmi_gpt_token_logprobs(pgmi_model* m, const int32_t* tokens, int B, int T, float* out) {
    return decoder_token_logprobs(m, PGMI_ARCH_GPT, tokens, B, T, out);
}

int pgmi_gpt_sequence_loglik(pgmi_model* m, const int32_t* tokens, const int32_t* lens, int B, int T, double* sum, int32_t* n_targets) {
    return decoder_sequence_loglik(m, PGMI_ARCH_GPT, tokens, lens, B, T, sum, n_targets);
}

}  // extern "C"
