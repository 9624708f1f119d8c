// PoET (proteingym/baselines/PoET/poet/models/poet.py): model creation, the tiered forward over a prompt with its per-layer prefix
// cache, variant log-probabilities / log-likelihoods given that cache, and the C entries.
//
// Per layer (modules/transformer.py TieredTransformerEncoderLayer.forward_packed, causal, pre-LN, no dropout at inference):
//   x += out_proj(self_attn(norm1(x)))          attention WITHIN each sequence
//   x += out_proj(multihead_attn(norm2(x)))     causal attention over the sequence-of-sequences
//   x += linear2(gelu(linear1(norm3(x))))       erf GELU
// q / k / v_proj carry no bias, out_proj does.  Both attentions rotate q and k (modules/embedding.py RotaryEmbedding: interleaved pairs
// (2i, 2i + 1), inv_freq = 10000^(-2i / head_dim), fp32 angles) by the position INSIDE the sequence, and scale q by head_dim^-1/2.
// Scoring (poet.py logits / _apply_causal_prefix_attention): a variant's tier 1 sees the variant alone; its tier 2 sees the prompt's
// tier-2 keys and values of the same layer -- the "memory" embed() returns -- and then itself, causally.  Here that memory is the prefix
// cache: pgmi_poet_set_prompt runs the tiered forward over the prompt once, its tier-2 prep pass writes K (rotated) and V^T of every
// layer straight into the cache in the operand layout of attention_prefix.hip, and every variant launch reads it as the shared prefix.
// Rows are packed (no pad rows anywhere): a launch is a list of segments of arbitrary lengths.  Every stage is row-local or, in the
// attention, local to (row, its segment, the prefix): a variant's numbers do not depend on what shares its launch.
#include "model.h"

namespace pgmi {

int64_t poet_weight_count(const pgmi_config* c, int final_norm) {
    const int64_t D = c->embed_dim, F = c->ffn_dim, V = c->vocab;
    const int64_t att = 2 * D + 3 * D * D + D * D + D;
    return V * D + (int64_t)c->layers * (2 * att + 2 * D + (F * D + F) + (D * F + D)) + (final_norm ? 2 * D : 0) + V * D + V;
}

constexpr int kPoetRotLen = 32768;          // rotary table rows = the longest single sequence (prompt member or variant)

int create_poet(pgmi_model* m, const pgmi_config* cfg, const float* w, int64_t n_weights, int final_norm) {
    const size_t D = cfg->embed_dim, F = cfg->ffn_dim, V = cfg->vocab, dh = m->dh, Da = m->Da;
    m->poet_final_norm = final_norm != 0;
    m->fc1_epi = EPI_GELU;
    BlobCursor c(m, w, n_weights);
    c.upload(&m->embed_tokens, V * D);
    // the interleaved pair (2p, 2p + 1) of a head goes to the slots (p, p + 32) the prep pass rotates together (api_progen2.hip pg2_slot
    // with rotary_dim = head_dim <= 64); slots no dim takes stay zero
    auto slot = [&](size_t col) -> size_t { const size_t h = col / dh, j = col % dh; return h * 64 + j / 2 + 32 * (j & 1); };
    const float qscale = 1.0f / sqrtf((float)dh);              // attention.py: q *= head_dim^-0.5 before the rotation (linear: same map)
    m->layers.resize(cfg->layers);
    std::vector<float> wq(3 * Da * D, 0.0f), wo_r(D * Da, 0.0f);
    for (int l = 0; l < cfg->layers; ++l) {
        Layer& L = m->layers[l];
        c.upload(&L.ln1_w, D);
        c.upload(&L.ln1_b, D);
        pack_qkv_slots(c.take(3 * D * D), D, Da, slot, qscale, wq.data());
        c.w16(&L.wqkv16, wq.data(), wq.size(), D);
        pack_out_cols(c.take(D * D), D, Da, slot, wo_r.data());
        c.w16(&L.wo16, wo_r.data(), wo_r.size(), Da);
        c.upload(&L.bo, D);
        c.upload(&L.c_ln_w, D);                                 // c_*: the sequence-of-sequences tier (norm2, multihead_attn)
        c.upload(&L.c_ln_b, D);
        pack_qkv_slots(c.take(3 * D * D), D, Da, slot, qscale, wq.data());
        c.w16(&L.c_wqkv16, wq.data(), wq.size(), D);
        pack_out_cols(c.take(D * D), D, Da, slot, wo_r.data());
        c.w16(&L.c_wo16, wo_r.data(), wo_r.size(), Da);
        c.upload(&L.c_bo, D);
        L.bqkv = L.c_bqkv = m->zeros;
        c.upload(&L.ln2_w, D);                                  // norm3
        c.upload(&L.ln2_b, D);
        c.w16(&L.w116, F * D, D);
        c.upload(&L.b1, F);
        c.w16(&L.w216, D * F, F);
        c.upload(&L.b2, D);
    }
    if (final_norm) {
        c.upload(&m->lna_w, D);
        c.upload(&m->lna_b, D);
    }
    c.upload(&m->head_w, V * D);
    c.upload(&m->head_b, V);
    int rc = c.finish();
    if (rc) return rc;
    const int half = (int)dh / 2;
    std::vector<float> inv(half);
    for (int i = 0; i < half; ++i) inv[i] = 1.0f / powf(10000.0f, (float)(2 * i) / (float)dh);
    rc = upload_rotary(m, std::min(kPoetRotLen, m->max_rows), 1, [&](int t, int, int i) { return i < half ? (float)t * inv[i] : 0.0f; });
    m->poet_pitch = ((size_t)cfg->max_positions + 31) / 32 * 32;
    if (!rc && m->poet_pitch) {
        const size_t n = (size_t)cfg->layers * 2 * 2 * Da * m->poet_pitch;
        rc = dev_alloc(m->allocs, &m->poet_cache, n);
        if (!rc) PGMI_HIP(hipMemset(m->poet_cache, 0, n * sizeof(unsigned short)));
    }
    if (!rc) rc = dev_alloc(m->allocs, &m->poet_meta, (size_t)7 * m->max_rows + 8);
    if (!rc) rc = dev_alloc(m->allocs, &m->gpt_sum, (size_t)m->max_rows);
    return rc;
}

// The tiered forward over R packed rows (tokens in m->tokens, within-sequence positions in m->pos_idx); leaves the residual stream in
// m->x.  p1: the sequences.  Prompt (p2 != nullptr): tier 2 runs over p2 (one segment, the whole prompt) and its K / V^T planes are the
// cache of the layer.  Variants (p2 == nullptr): tier 2 runs over p1 with the first P cache rows as the shared prefix.
static int poet_forward(pgmi_model* m, int R, const PoetPlan& p1, const PoetPlan* p2, int P) {
    const pgmi_config& c = m->cfg;
    const int M = R, D = c.embed_dim, F = c.ffn_dim, H = c.heads, Da = m->Da;
    hipStream_t s = m->stream;
    { ProfScope p(m, PGMI_K_EMBED, 0, (double)M * D * 4);
      launch_gather_rows(m->embed_tokens, m->tokens, M, D, m->x, s); }
    const double ln_bytes = 2.0 * M * D * 4;
    const size_t cap = (size_t)m->max_rows, pitch = own_pitch(m), cache_plane = (size_t)Da * m->poet_pitch;
    double own1 = 0, own2 = 0;                                   // visible (query, key) pairs of the two tiers
    for (int b = 0; b < p1.n_seg(); ++b) { const double n = p1.seg_off[b + 1] - p1.seg_off[b]; own1 += n * (n + 1) / 2; }
    if (p2) own2 = (double)M * (M + 1) / 2; else own2 = own1 + (double)M * P;
    auto attention = [&](const PoetPlan& pl, const W16& wqkv16, unsigned short* k16, unsigned short* vt16, size_t kpitch,
                         const unsigned short* pk16, const unsigned short* pvt16, int Pn, double pairs) {
        { ProfScope p(m, PGMI_K_GEMM_QKV, 2.0 * M * 3 * Da * D, 0);
          int rc = linear(m, nullptr, m->h16, nullptr, wqkv16, m->zeros, nullptr, m->qkv, nullptr, M, 3 * Da, D, EPI_NONE);
          if (rc) return rc; }
        PrefixAttLaunch a;
        a.qkv = m->qkv; a.pos = m->pos_idx; a.cos_t = m->rot_cos; a.sin_t = m->rot_sin;
        a.seg_off = pl.d_seg_off; a.ent_seg = pl.d_ent_seg; a.ent_tile = pl.d_ent_tile;
        a.n_seg = pl.n_seg(); a.n_ent = pl.n_ent(); a.H = H;
        a.q16 = m->qk16; a.q_plane = cap * Da;
        a.k16 = k16; a.vt16 = vt16; a.pitch = kpitch;
        a.pk16 = pk16; a.pvt16 = pvt16; a.ppitch = m->poet_pitch; a.P = Pn;
        a.out = ATT_OUT_SPLIT; a.ctx16 = m->h16; a.stream = s;
        ProfScope p(m, PGMI_K_ATTENTION, 4.0 * pairs * Da, 0);
        int rc = launch_prefix_prep(a);
        return rc ? rc : launch_prefix_attention(a);
    };
    unsigned short* ownK = m->qk16 + 2 * cap * Da;               // behind the q planes; its own two planes are Da * pitch halfs apart
    for (int l = 0; l < c.layers; ++l) {
        const Layer& L = m->layers[l];
        { ProfScope p(m, PGMI_K_LAYERNORM, 0, ln_bytes);
          launch_layernorm16(m->x, L.ln1_w, L.ln1_b, M, D, m->ln_eps, m->h16, 1, s); }
        int rc = attention(p1, L.wqkv16, ownK, m->vt16, pitch, nullptr, nullptr, 0, own1);
        if (rc) return rc;
        { ProfScope p(m, PGMI_K_GEMM_OUT, 2.0 * M * D * Da, 0);
          rc = linear(m, nullptr, m->h16, nullptr, L.wo16, L.bo, m->x, m->x, nullptr, M, D, Da, EPI_NONE);
          if (rc) return rc; }
        { ProfScope p(m, PGMI_K_LAYERNORM, 0, ln_bytes);
          launch_layernorm16(m->x, L.c_ln_w, L.c_ln_b, M, D, m->ln_eps, m->h16, 1, s); }
        unsigned short* cK = m->poet_cache ? m->poet_cache + (size_t)l * 4 * cache_plane : nullptr;
        unsigned short* cV = cK ? cK + 2 * cache_plane : nullptr;
        if (p2) rc = attention(*p2, L.c_wqkv16, cK, cV, m->poet_pitch, nullptr, nullptr, 0, own2);
        else rc = attention(p1, L.c_wqkv16, ownK, m->vt16, pitch, cK, cV, P, own2);
        if (rc) return rc;
        { ProfScope p(m, PGMI_K_GEMM_OUT, 2.0 * M * D * Da, 0);
          rc = linear(m, nullptr, m->h16, nullptr, L.c_wo16, L.c_bo, m->x, m->x, nullptr, M, D, Da, EPI_NONE);
          if (rc) return rc; }
        { ProfScope p(m, PGMI_K_LAYERNORM, 0, ln_bytes);
          launch_layernorm16(m->x, L.ln2_w, L.ln2_b, M, D, m->ln_eps, m->h16, 1, s); }
        { ProfScope p(m, PGMI_K_GEMM_FC1, 2.0 * M * F * D, 0);
          rc = linear(m, nullptr, m->h16, nullptr, L.w116, L.b1, nullptr, nullptr, m->g16, M, F, D, EPI_GELU);
          if (rc) return rc; }
        { ProfScope p(m, PGMI_K_GEMM_FC2, 2.0 * M * F * D, 0);
          rc = linear(m, nullptr, m->g16, nullptr, L.w216, L.b2, m->x, m->x, nullptr, M, D, F, EPI_NONE);
          if (rc) return rc; }
    }
    PGMI_HIP(hipGetLastError());
    return PGMI_OK;
}

// norm (when the model has one) and the log-softmax head on n rows of src -> m->lp [n, V]
static int poet_head(pgmi_model* m, const float* src, int n) {
    const int D = m->cfg.embed_dim, V = m->cfg.vocab;
    ProfScope p(m, PGMI_K_HEAD, 2.0 * n * D * V, 0);
    if (m->poet_final_norm) {
        launch_layernorm(src, m->lna_w, m->lna_b, n, D, m->ln_eps, m->h, m->stream);
        src = m->h;
    }
    launch_vocab_logsoftmax(src, m->head_w, m->head_b, n, D, V, m->lp, m->nonfinite, m->stream);
    PGMI_HIP(hipGetLastError());
    return PGMI_OK;
}

static int poet_check(pgmi_model* m) {
    if (!m) { set_error("null model"); return PGMI_EINVAL; }
    if (m->cfg.arch != PGMI_ARCH_POET) { set_error("not a PoET model"); return PGMI_EINVAL; }
    return PGMI_OK;
}

// Variants [B][T] right-padded with the mask token, lens[b] real tokens.  loglik: the model reads tokens[b, :lens[b] - 1] and
// sum[b] = sum of log p(tokens[b, t + 1]) over the targets that are not the mask token; else the model reads all lens[b] tokens and
// every row's log-probabilities go to out [B][T][V] (rows beyond lens[b]: NaN).
static int poet_variants(pgmi_model* m, const int32_t* tokens, const int32_t* lens, int B, int T, bool loglik, float* out, double* sum) {
    int rc = poet_check(m);
    if (rc) return rc;
    if (!tokens || !lens || B <= 0 || T <= 0 || (loglik ? !sum : !out)) { set_error("bad argument"); return PGMI_EINVAL; }
    const int V = m->cfg.vocab, D = m->cfg.embed_dim, lo = loglik ? 2 : 1;
    for (int b = 0; b < B; ++b) {
        if (lens[b] < lo || lens[b] > T) { set_error("row %d of this call: length %d outside [%d, T = %d]", b, lens[b], lo, T); return PGMI_EINVAL; }
        if (lens[b] > m->rot_len) { set_error("row %d of this call: %d tokens exceed the %d rotary positions / workspace rows", b, lens[b], m->rot_len); return PGMI_EINVAL; }
    }
    rc = check_vocab(tokens, B, T, V);
    if (rc) return rc;
    PGMI_HIP(hipSetDevice(m->device));
    hipStream_t s = m->stream;
    const size_t pitch = own_pitch(m);
    if (!loglik) std::fill(out, out + (size_t)B * T * V, NAN);
    std::vector<int32_t> tok, pos, idx, tgt, off;
    for (int b0 = 0; b0 < B;) {
        // the chunk: as many variants as the packed rows and the padded key rows of the workspace take
        PoetPlan pl;
        tok.clear(); pos.clear(); idx.clear(); tgt.clear(); off.assign(1, 0);
        int b1 = b0;
        size_t rows = 0, padded = 0;
        for (; b1 < B; ++b1) {
            const int n = lens[b1] - (loglik ? 1 : 0);
            if (rows + n > (size_t)m->max_rows || padded + (size_t)(n + 31) / 32 * 32 > pitch) break;
            const int32_t* row = tokens + (size_t)b1 * T;
            for (int t = 0; t < n; ++t) {
                tok.push_back(row[t]);
                pos.push_back(t);
                if (loglik && row[t + 1] != PGMI_POET_TOK_MASK) { idx.push_back((int32_t)rows + t); tgt.push_back(row[t + 1]); }
            }
            off.push_back((int32_t)idx.size());
            pl.add(n);
            rows += n; padded += (size_t)(n + 31) / 32 * 32;
        }
        if (b1 == b0) { set_error("row %d of this call: %d tokens exceed the workspace of %d rows", b0, lens[b0], m->max_rows); return PGMI_EINVAL; }
        const int R = (int)rows, bc = b1 - b0;
        PGMI_HIP(hipMemcpyAsync(m->tokens, tok.data(), (size_t)R * 4, hipMemcpyHostToDevice, s));
        PGMI_HIP(hipMemcpyAsync(m->pos_idx, pos.data(), (size_t)R * 4, hipMemcpyHostToDevice, s));
        rc = upload_plan(m, pl, 0);
        if (!rc) rc = poet_forward(m, R, pl, nullptr, m->poet_P);
        if (rc) return rc;
        if (loglik) {
            const int Rt = (int)idx.size();
            int32_t* d_off = m->poet_meta + (size_t)2 * (3 * (size_t)m->max_rows + 2);
            PGMI_HIP(hipMemcpyAsync(d_off, off.data(), off.size() * 4, hipMemcpyHostToDevice, s));
            if (Rt > 0) {
                PGMI_HIP(hipMemcpyAsync(m->row_idx, idx.data(), (size_t)Rt * 4, hipMemcpyHostToDevice, s));
                PGMI_HIP(hipMemcpyAsync(m->aux_i, tgt.data(), (size_t)Rt * 4, hipMemcpyHostToDevice, s));
                { ProfScope p(m, PGMI_K_EMBED, 0, 2.0 * Rt * D * 4);
                  launch_gather_rows(m->x, m->row_idx, Rt, D, m->g, s); }             // only rows that have a target reach the head
                rc = poet_head(m, m->g, Rt);
                if (rc) return rc;
                ProfScope p(m, PGMI_K_SCORE, 0, (double)Rt * 8);
                launch_pppl_pick(m->lp, m->aux_i, Rt, V, m->denom, s);
            }
            launch_seq_sum(m->denom, d_off, bc, m->gpt_sum, s);
            PGMI_HIP(hipGetLastError());
            PGMI_HIP(hipMemcpyAsync(sum + b0, m->gpt_sum, (size_t)bc * sizeof(double), hipMemcpyDeviceToHost, s));
        } else {
            rc = poet_head(m, m->x, R);
            if (rc) return rc;
            for (int b = 0; b < bc; ++b)
                PGMI_HIP(hipMemcpyAsync(out + (size_t)(b0 + b) * T * V, m->lp + (size_t)pl.seg_off[b] * V,
                                        (size_t)lens[b0 + b] * V * 4, hipMemcpyDeviceToHost, s));
        }
        PGMI_HIP(hipStreamSynchronize(s));                      // the chunk's host buffers outlive their copies
        b0 = b1;
    }
    return check_nonfinite(m);
}

}  // namespace pgmi

extern "C" {

int64_t pgmi_poet_weight_count(const pgmi_config* cfg, int final_norm) {
    if (!cfg || cfg->layers <= 0 || cfg->embed_dim <= 0 || cfg->ffn_dim <= 0 || cfg->vocab <= 0) return -1;
    return poet_weight_count(cfg, final_norm);
}

int pgmi_poet_model_create(const pgmi_config* cfg, int final_norm, const float* weights, int64_t n_weights, int device, pgmi_model** out) {
    if (out) *out = nullptr;
    if (!cfg || cfg->arch != PGMI_ARCH_POET) { set_error("pgmi_poet_model_create: arch must be PGMI_ARCH_POET"); return PGMI_EINVAL; }
    return model_create(cfg, weights, n_weights, device, out, final_norm != 0);
}

int pgmi_poet_set_prompt(pgmi_model* m, const int32_t* tokens, const int32_t* seg_len, int n_seg) {
    int rc = poet_check(m);
    if (rc) return rc;
    m->poet_P = 0;                                              // whatever happens below, a stale cache is never read
    m->poet_prompt_lp.clear();
    if (n_seg == 0) return PGMI_OK;                             // memory = None: variants see themselves only
    if (!tokens || !seg_len || n_seg < 0) { set_error("bad argument"); return PGMI_EINVAL; }
    PoetPlan p1, p2;
    size_t total = 0, padded = 0;
    std::vector<int32_t> pos;
    for (int i = 0; i < n_seg; ++i) {
        if (seg_len[i] <= 0) { set_error("prompt sequence %d has length %d", i, seg_len[i]); return PGMI_EINVAL; }
        if (seg_len[i] > m->rot_len) { set_error("prompt sequence %d: %d tokens exceed the %d rotary positions", i, seg_len[i], m->rot_len); return PGMI_EINVAL; }
        p1.add(seg_len[i]);
        for (int t = 0; t < seg_len[i]; ++t) pos.push_back(t);
        total += seg_len[i];
        padded += ((size_t)seg_len[i] + 31) / 32 * 32;
        if (total > (size_t)m->cfg.max_positions) {
            set_error("prompt of more than %d tokens: the prefix cache was created for max_positions = %d", m->cfg.max_positions, m->cfg.max_positions);
            return PGMI_EINVAL;
        }
    }
    if (total > (size_t)m->max_rows || padded > own_pitch(m)) {
        set_error("prompt of %zu tokens (%zu with every sequence padded to 32) exceeds the workspace of %d rows", total, padded, m->max_rows);
        return PGMI_EINVAL;
    }
    const int R = (int)total, V = m->cfg.vocab;
    rc = check_vocab(tokens, 1, R, V);
    if (rc) return rc;
    p2.add(R);
    PGMI_HIP(hipSetDevice(m->device));
    hipStream_t s = m->stream;
    PGMI_HIP(hipMemcpyAsync(m->tokens, tokens, (size_t)R * 4, hipMemcpyHostToDevice, s));
    PGMI_HIP(hipMemcpyAsync(m->pos_idx, pos.data(), (size_t)R * 4, hipMemcpyHostToDevice, s));
    rc = upload_plan(m, p1, 0);
    if (!rc) rc = upload_plan(m, p2, 1);
    if (!rc) rc = poet_forward(m, R, p1, &p2, 0);
    if (!rc) rc = poet_head(m, m->x, R);
    if (rc) return rc;
    m->poet_prompt_lp.resize((size_t)R * V);
    PGMI_HIP(hipMemcpyAsync(m->poet_prompt_lp.data(), m->lp, (size_t)R * V * 4, hipMemcpyDeviceToHost, s));
    PGMI_HIP(hipStreamSynchronize(s));
    rc = check_nonfinite(m);
    if (rc) { m->poet_prompt_lp.clear(); return rc; }
    m->poet_P = R;
    return PGMI_OK;
}

int pgmi_poet_prompt_logprobs(pgmi_model* m, float* out) {
    int rc = poet_check(m);
    if (rc) return rc;
    if (!out) { set_error("bad argument"); return PGMI_EINVAL; }
    if (m->poet_P == 0) { set_error("no prompt is set"); return PGMI_EINVAL; }
    memcpy(out, m->poet_prompt_lp.data(), m->poet_prompt_lp.size() * sizeof(float));
    return PGMI_OK;
}

int pgmi_poet_token_logprobs(pgmi_model* m, const int32_t* tokens, const int32_t* lens, int B, int T, float* out) {
    return poet_variants(m, tokens, lens, B, T, false, out, nullptr);
}

int pgmi_poet_sequence_loglik(pgmi_model* m, const int32_t* tokens, const int32_t* lens, int B, int T, double* out) {
    return poet_variants(m, tokens, lens, B, T, true, nullptr, out);
}

}  // extern "C"
