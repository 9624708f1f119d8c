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
    m->final_norm = final_norm != 0;
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
    return rc ? rc : alloc_prefix_cache(m);                     // max_positions == 0: no planes, variants see themselves only
}

// The tiered forward over R packed rows (tokens in m->tokens, within-sequence positions in m->pos_idx); leaves the residual stream in
// m->x.  p1: the sequences.  Prompt (p2 != nullptr): tier 2 runs over p2 (one segment, the whole prompt) and its K / V^T planes are the
// cache of the layer.  Variants (p2 == nullptr): tier 2 runs over p1 with the first P cache rows as the shared prefix.
static int poet_forward(pgmi_model* m, int R, const SegPlan& p1, const SegPlan* p2, int P) {
    const pgmi_config& c = m->cfg;
    const int M = R, D = c.embed_dim, Da = m->Da;
    { ProfScope p(m, PGMI_K_EMBED, 0, (double)M * D * 4);
      launch_gather_rows(m->embed_tokens, m->tokens, M, D, m->x, m->stream); }
    const size_t pitch = own_pitch(m);
    double own1 = 0, own2 = 0;                                   // visible (query, key) pairs of the two tiers
    for (int b = 0; b < p1.n_seg(); ++b) { const double n = p1.seg_off[b + 1] - p1.seg_off[b]; own1 += n * (n + 1) / 2; }
    if (p2) own2 = (double)M * (M + 1) / 2; else own2 = own1 + (double)M * P;
    auto norm = [&](const float* w, const float* b) {
        ProfScope p(m, PGMI_K_LAYERNORM, 0, 2.0 * M * D * 4);
        launch_layernorm16(m->x, w, b, M, D, m->ln_eps, m->h16, 1, m->stream);
    };
    auto attention = [&](const SegPlan& pl, const W16& wqkv16, unsigned short* k16, unsigned short* vt16, size_t kpitch,
                         const unsigned short* pk16, const unsigned short* pvt16, int Pn, double pairs) {
        { ProfScope p(m, PGMI_K_GEMM_QKV, 2.0 * M * 3 * Da * D, 0);
          int rc = linear(m, nullptr, m->h16, nullptr, wqkv16, m->zeros, nullptr, m->qkv, nullptr, M, 3 * Da, D, EPI_NONE);
          if (rc) return rc; }
        PrefixAttLaunch a = prefix_launch(m, pl);
        a.qkv = m->qkv; a.pos = m->pos_idx; a.cos_t = m->rot_cos; a.sin_t = m->rot_sin;
        a.k16 = k16; a.vt16 = vt16; a.pitch = kpitch;
        a.pk16 = pk16; a.pvt16 = pvt16; a.ppitch = m->pfx.pitch; a.P = Pn;
        ProfScope p(m, PGMI_K_ATTENTION, 4.0 * pairs * Da, 0);
        int rc = launch_prefix_prep(a);
        return rc ? rc : launch_prefix_attention(a);
    };
    unsigned short* ownK = m->qk16 + 2 * (size_t)m->max_rows * Da;   // behind the q planes; its own two planes are Da * pitch halfs apart
    for (int l = 0; l < c.layers; ++l) {
        const Layer& L = m->layers[l];
        norm(L.ln1_w, L.ln1_b);
        int rc = attention(p1, L.wqkv16, ownK, m->vt16, pitch, nullptr, nullptr, 0, own1);
        if (!rc) rc = out_proj(m, L.wo16, L.bo, M);
        if (rc) return rc;
        norm(L.c_ln_w, L.c_ln_b);
        unsigned short *cK = m->pfx.k(l), *cV = m->pfx.vt(l);
        if (p2) rc = attention(*p2, L.c_wqkv16, cK, cV, m->pfx.pitch, nullptr, nullptr, 0, own2);
        else rc = attention(p1, L.c_wqkv16, ownK, m->vt16, pitch, cK, cV, P, own2);
        if (!rc) rc = out_proj(m, L.c_wo16, L.c_bo, M);
        if (!rc) rc = ffn(m, L, M);
        if (rc) return rc;
    }
    PGMI_HIP(hipGetLastError());
    return PGMI_OK;
}

static int poet_check(pgmi_model* m) {
    if (!m) { set_error("null model"); return PGMI_EINVAL; }
    if (m->cfg.arch != PGMI_ARCH_POET) { set_error("not a PoET model"); return PGMI_EINVAL; }
    return PGMI_OK;
}

int score_packed(pgmi_model* m, const PackedScorer& e, const int32_t* tokens, const int32_t* lens, int B, int T, bool loglik, float* out,
                 double* sum) {
    if (!tokens || !lens || B <= 0 || T <= 0 || (loglik ? !sum : !out)) { set_error("bad argument"); return PGMI_EINVAL; }
    if (e.not_ready) { set_error("%s", e.not_ready); return PGMI_EINVAL; }
    const int V = m->cfg.vocab, lo = loglik ? 2 : 1;
    int rc = PGMI_OK;
    for (int b = 0; b < B; ++b) {
        if (lens[b] < lo || lens[b] > T) { set_error("row %d of this call: length %d outside [%d, T = %d]", b, lens[b], lo, T); return PGMI_EINVAL; }
        if (lens[b] > e.pos_len) { set_error("row %d of this call: %d tokens exceed the %d %s / workspace rows", b, lens[b], e.pos_len, e.pos_what); return PGMI_EINVAL; }
        if (e.vocab_per_row && (rc = check_vocab(tokens + (size_t)b * T, 1, lens[b], V))) return rc;
    }
    if (!e.vocab_per_row && (rc = check_vocab(tokens, B, T, V))) return rc;
    PGMI_HIP(hipSetDevice(m->device));
    hipStream_t s = m->stream;
    if (!loglik) std::fill(out, out + (size_t)B * T * V, NAN);
    const bool gather = e.skip_target >= 0;                     // else every row has a target and the head reads m->x as it is
    std::vector<int32_t> tok, pos, idx, tgt, off;
    for (int b0 = 0; b0 < B;) {
        PackedChunk ch = pack_chunk(lens, b0, B, loglik, e.same_length, m->max_rows, own_pitch(m));
        if (ch.b1 == b0) { set_error("row %d of this call: %d tokens exceed the workspace of %d rows", b0, lens[b0], m->max_rows); return PGMI_EINVAL; }
        const int R = ch.rows, bc = ch.b1 - b0;
        tok.clear(); pos.clear(); idx.clear(); tgt.clear(); off.assign(1, 0);
        for (int b = b0; b < ch.b1; ++b) {
            const int32_t* row = tokens + (size_t)b * T;
            const int r0 = ch.plan.seg_off[b - b0], n = ch.plan.seg_off[b - b0 + 1] - r0;
            for (int t = 0; t < n; ++t) {
                tok.push_back(row[t]);
                pos.push_back(t);
                if (!loglik || row[t + 1] == e.skip_target) continue;
                if (gather) idx.push_back(r0 + t);              // only rows that have a target reach the head
                tgt.push_back(row[t + 1]);
            }
            off.push_back((int32_t)tgt.size());
        }
        PGMI_HIP(hipMemcpyAsync(m->tokens, tok.data(), (size_t)R * 4, hipMemcpyHostToDevice, s));
        PGMI_HIP(hipMemcpyAsync(m->pos_idx, pos.data(), (size_t)R * 4, hipMemcpyHostToDevice, s));
        const int Rt = (int)tgt.size();
        if (loglik) {                                           // every upload ahead of the first launch, as decoder_sequence_loglik has them
            PGMI_HIP(hipMemcpyAsync(m->pfx.seq_off(), off.data(), off.size() * 4, hipMemcpyHostToDevice, s));
            if (gather && Rt > 0) PGMI_HIP(hipMemcpyAsync(m->row_idx, idx.data(), (size_t)Rt * 4, hipMemcpyHostToDevice, s));
            if (Rt > 0) PGMI_HIP(hipMemcpyAsync(m->aux_i, tgt.data(), (size_t)Rt * 4, hipMemcpyHostToDevice, s));
        }
        rc = upload_plan(m, ch.plan, 0);
        if (!rc) rc = e.forward(m, bc, R, ch.plan);
        if (rc) return rc;
        if (loglik) {
            rc = loglik_tail(m, gather ? m->row_idx : nullptr, Rt, m->pfx.seq_off(), bc, sum + b0);
            if (rc) return rc;
        } else {
            rc = narrow_head(m, m->x, R);
            if (rc) return rc;
            for (int b = 0; b < bc; ++b)
                PGMI_HIP(hipMemcpyAsync(out + (size_t)(b0 + b) * T * V, m->lp + (size_t)ch.plan.seg_off[b] * V,
                                        (size_t)lens[b0 + b] * V * 4, hipMemcpyDeviceToHost, s));
        }
        PGMI_HIP(hipStreamSynchronize(s));                      // the chunk's host buffers outlive their copies
        if (loglik && e.mean)
            for (int b = b0; b < ch.b1; ++b) sum[b] /= (double)(lens[b] - 1);
        b0 = ch.b1;
    }
    return check_nonfinite(m);
}

// Variants right-padded with the mask token; a mask-token target does not count.
static int poet_variants(pgmi_model* m, const int32_t* tokens, const int32_t* lens, int B, int T, bool loglik, float* out, double* sum) {
    int rc = poet_check(m);
    if (rc) return rc;
    PackedScorer e = {};
    e.forward = [](pgmi_model* m, int, int R, const SegPlan& pl) { return poet_forward(m, R, pl, nullptr, m->pfx.rows); };
    e.pos_len = m->rot_len; e.pos_what = "rotary positions";
    e.skip_target = PGMI_POET_TOK_MASK;
    return score_packed(m, e, tokens, lens, B, T, loglik, out, sum);
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
    m->pfx.rows = 0;                                              // whatever happens below, a stale cache is never read
    m->poet_prompt_lp.clear();
    if (n_seg == 0) return PGMI_OK;                             // memory = None: variants see themselves only
    if (!tokens || !seg_len || n_seg < 0) { set_error("bad argument"); return PGMI_EINVAL; }
    SegPlan p1, p2;
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
    if (!rc) rc = narrow_head(m, m->x, R);
    if (rc) return rc;
    m->poet_prompt_lp.resize((size_t)R * V);
    PGMI_HIP(hipMemcpyAsync(m->poet_prompt_lp.data(), m->lp, (size_t)R * V * 4, hipMemcpyDeviceToHost, s));
    PGMI_HIP(hipStreamSynchronize(s));
    rc = check_nonfinite(m);
    if (rc) { m->poet_prompt_lp.clear(); return rc; }
    m->pfx.rows = R;
    return PGMI_OK;
}

int pgmi_poet_prompt_logprobs(pgmi_model* m, float* out) {
    int rc = poet_check(m);
    if (rc) return rc;
    if (!out) { set_error("bad argument"); return PGMI_EINVAL; }
    if (m->pfx.rows == 0) { set_error("no prompt is set"); return PGMI_EINVAL; }
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
