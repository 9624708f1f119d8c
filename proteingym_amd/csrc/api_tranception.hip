// Tranception (tranception/model_pytorch.py): model creation, prefix-shared scoring and the C entries.  The forward, dense and
// prefix-shared, is the causal decoder's (api_gpt.hip run_decoder) with the layers' depth-wise convolution (L.conv), the grouped ALiBi
// slopes and FC1's squared ReLU stored here; the head is its narrow one (narrow_head).
#include "model.h"

namespace pgmi {

// ALiBi slopes, grouped: tranception/model_pytorch.py:50-71 (get_slopes(n, "grouped_alibi"))
static void alibi_slopes_pow2(int n, std::vector<double>& out) {
    const double start = pow(2.0, -pow(2.0, -(log2((double)n) - 3.0)));
    double v = start;
    for (int i = 0; i < n; ++i) { out.push_back(v); v *= start; }
}
static std::vector<double> alibi_slopes(int n) {
    std::vector<double> r;
    const double l2 = log2((double)n);
    if (l2 == floor(l2)) { alibi_slopes_pow2(n, r); return r; }
    const int c = 1 << (int)floor(l2);
    alibi_slopes_pow2(c, r);
    std::vector<double> e = alibi_slopes(2 * c);
    for (int i = 0; i < (int)e.size() && (int)r.size() < n; i += 2) r.push_back(e[i]);
    return r;
}

// transpose an HF Conv1D weight [in,out] into nn.Linear layout [out,in], optionally scaling the
// first `scaled_cols` output columns (the q block) by `scale`
static void conv1d_to_linear(const float* w, size_t in, size_t out, size_t scaled_cols, float scale, std::vector<float>& dst) {
    dst.resize(in * out);
    for (size_t o = 0; o < out; ++o) {
        const float sc = o < scaled_cols ? scale : 1.0f;
        for (size_t i = 0; i < in; ++i) dst[o * in + i] = w[i * out + o] * sc;
    }
}

int create_tranception(pgmi_model* m, const pgmi_config* cfg, const float* w, int64_t n_weights) {
    const size_t D = cfg->embed_dim, F = cfg->ffn_dim, V = cfg->vocab, H = cfg->heads;
    BlobCursor c(m, w, n_weights);
    c.upload(&m->embed_tokens, V * D);
    const float qscale = 1.0f / sqrtf((float)kHeadDim);
    m->layers.resize(cfg->layers);
    std::vector<float> lin, bq(3 * D), conv(3 * 4 * 64 * 8);
    static const int ksz[3] = {3, 5, 7};
    for (int l = 0; l < cfg->layers; ++l) {
        Layer& L = m->layers[l];
        c.upload(&L.ln1_w, D);
        c.upload(&L.ln1_b, D);
        conv1d_to_linear(c.take(D * 3 * D), D, 3 * D, D, qscale, lin);
        c.w16(&L.wqkv16, lin.data(), lin.size(), D);
        const float* b = c.take(3 * D);
        for (size_t i = 0; i < 3 * D; ++i) bq[i] = b[i] * (i < D ? qscale : 1.0f);
        c.upload(&L.bqkv, bq.data(), bq.size());
        // conv table: group 0 = identity; groups 1..3 = kernels 3,5,7 right-aligned in 7 taps
        std::fill(conv.begin(), conv.end(), 0.0f);
        for (int which = 0; which < 3; ++which) {
            for (int d = 0; d < 64; ++d) conv[((which * 4 + 0) * 64 + d) * 8 + 6] = 1.0f;
            for (int ki = 0; ki < 3; ++ki) {
                const int k = ksz[ki];
                const float* taps = c.take(64 * k);
                for (int d = 0; d < 64; ++d)
                    for (int j = 0; j < k; ++j) conv[((which * 4 + ki + 1) * 64 + d) * 8 + (7 - k) + j] = taps[d * k + j];
                // the q projection is pre-scaled by 1/sqrt(dh): scale the q-conv bias the same way
                const float* bias = c.take(64);
                for (int d = 0; d < 64; ++d) conv[((which * 4 + ki + 1) * 64 + d) * 8 + 7] = bias[d] * (which == 0 ? qscale : 1.0f);
            }
        }
        c.upload(&L.conv, conv.data(), conv.size());
        conv1d_to_linear(c.take(D * D), D, D, 0, 1.0f, lin);
        c.w16(&L.wo16, lin.data(), lin.size(), D);
        c.upload(&L.bo, D);
        c.upload(&L.ln2_w, D);
        c.upload(&L.ln2_b, D);
        conv1d_to_linear(c.take(D * F), D, F, 0, 1.0f, lin);
        c.w16(&L.w116, lin.data(), lin.size(), D);
        c.upload(&L.b1, F);
        conv1d_to_linear(c.take(F * D), F, D, 0, 1.0f, lin);
        c.w16(&L.w216, lin.data(), lin.size(), F);
        c.upload(&L.b2, D);
    }
    c.upload(&m->lna_w, D);
    c.upload(&m->lna_b, D);
    c.upload(&m->head_w, V * D);
    m->head_b = m->zeros;
    std::vector<float> sl;
    std::vector<double> quarter = alibi_slopes((int)H / 4);          // grouped: slopes of n/4 heads, tiled 4x
    for (int rep = 0; rep < 4; ++rep)
        for (double v : quarter) sl.push_back((float)v);
    c.upload(&m->slopes, sl.data(), sl.size());
    m->fc1_epi = EPI_SQRELU;
    m->final_norm = true;
    return c.finish();
}

// TranceptEVE's second prior: host table [P, V] indexed like the retrieval prior, its weight and the fallback switch; dev is set by
// upload_prior
struct TrEve {
    const float* host = nullptr;
    float beta = 0.0f;
    int fallback = 0;
    const float* dev = nullptr;
};

// Device copy of the retrieval log-prior [P, V] (none: no retrieval), grown as needed; the EVE table, when given, sits behind it.
static int upload_prior(pgmi_model* m, const float* log_prior, int P, TrEve* eve = nullptr) {
    if (!log_prior) return PGMI_OK;
    const size_t n = (size_t)P * m->cfg.vocab;
    const bool two = eve && eve->host;
    int rc = ensure_cap(m, &m->tr_prior, &m->tr_prior_cap, two ? 2 * n : n);
    if (rc) return rc;
    PGMI_HIP(hipMemcpyAsync(m->tr_prior, log_prior, n * 4, hipMemcpyHostToDevice, m->stream));
    if (two) {
        PGMI_HIP(hipMemcpyAsync(m->tr_prior + n, eve->host, n * 4, hipMemcpyHostToDevice, m->stream));
        eve->dev = m->tr_prior + n;
    }
    return PGMI_OK;
}

// The dense entries' context check (the prefix-shared entry runs the same one before its workspace check).
static int check_ctx(const pgmi_model* m, int T) {
    if (T <= m->cfg.max_positions) return PGMI_OK;
    set_error("sequence of %d tokens exceeds the model context n_ctx=%d", T, m->cfg.max_positions);
    return PGMI_EINVAL;
}

// ---- Tranception: prefix-shared scoring ------------------------------------------------------------
// The reference forwards every mutated sequence in full, in both reading directions (scoring_utils.py:77-150, model_pytorch.py:878-928).
// The model is causal (attention model_pytorch.py:155-183; depth-wise convolution :73-88): every hidden state of a sequence before its
// first token that differs from the wild type IS the wild type's.  One chunk of work = ROOT sequences forwarded in full plus sequences
// that own only the rows from seq_p on (seq_p = the first token that differs from the root): LayerNorm, the four GEMMs of a layer and
// the head run on the packed suffix rows (row-local); the convolution takes its history -- and the head of seq_p's 32-token tile, which
// the attention wants whole -- from the root's input rows of the same launch, the attention its earlier key tiles from the root's
// operand planes, and the per-sequence reduction reads the root's log-probability rows before seq_p.
// Every row is computed by the same kernels from the same inputs in the same order as in a full forward: the same bits.
struct TrChunk {
    std::vector<int32_t> seq;                         // call-level index of every chunk-local sequence (a root may repeat over chunks)
    std::vector<int32_t> off, p, q, root;             // packed row of token p; first own token; operand row of its tile's first token; chunk-local root
    std::vector<uint32_t> vt;                         // V^T block offset (halfs per plane)
    std::vector<int32_t> tile_seq, tile_j, blk_seq, blk_j, tokens;
    int rows = 0, padded = 0;                         // packed rows; operand rows (every sequence from its tile on, rounded up to whole tiles)
    double att_flops = 0;
    int add(int call_index, const int32_t* tok, int T, int p0, int root_local, int D) {
        const int qrows = 32 * att16_waves_per_block(T);  // queries per attention block
        const int local = (int)seq.size(), a0 = p0 / 32 * 32, n = T - a0;
        seq.push_back(call_index);
        off.push_back(rows);
        p.push_back(p0);
        q.push_back(padded);
        root.push_back(root_local < 0 ? local : root_local);
        vt.push_back((uint32_t)((size_t)padded * (size_t)D));
        for (int j = 0; j < (n + 31) / 32; ++j) { tile_seq.push_back(local); tile_j.push_back(j); }
        for (int j = 0; j < (n + qrows - 1) / qrows; ++j) { blk_seq.push_back(local); blk_j.push_back(j); }
        tokens.insert(tokens.end(), tok + p0, tok + T);
        rows += T - p0;
        padded += (n + 31) / 32 * 32;
        att_flops += 2.0 * D * ((double)T * T - (double)p0 * p0);         // 4 D per (query, visible key) pair
        return local;
    }
};

// Runs one chunk: tokens (packed), index arrays and the retrieval arguments are uploaded, the forward leaves the suffix rows'
// log-probabilities in m->lp [rows, V] and the per-sequence reductions in m->denom [sequences].
int run_tranception_shared(pgmi_model* m, TrChunk& ck, int T, const float* prior_dev, const int32_t* a0, const int32_t* r0,
                           const int32_t* pn, const int32_t* fl, float alpha, const TrEve& eve) {
    const int M = ck.rows, V = m->cfg.vocab, S = (int)ck.seq.size();
    hipStream_t s = m->stream;
    // attention blocks with the most key tiles first: the launch's tail is made of the short ones
    {
        std::vector<int> order(ck.blk_seq.size());
        for (size_t i = 0; i < order.size(); ++i) order[i] = (int)i;
        const int qrows = 32 * att16_waves_per_block(T);
        auto keys = [&](int i) { return std::min(T, ck.p[ck.blk_seq[i]] / 32 * 32 + (ck.blk_j[i] + 1) * qrows); };
        std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return keys(x) > keys(y); });
        std::vector<int32_t> bs(order.size()), bj(order.size());
        for (size_t i = 0; i < order.size(); ++i) { bs[i] = ck.blk_seq[order[i]]; bj[i] = ck.blk_j[order[i]]; }
        ck.blk_seq.swap(bs);
        ck.blk_j.swap(bj);
    }
    const size_t nt = ck.tile_seq.size(), nb = ck.blk_seq.size();
    const size_t need = (size_t)9 * S + 2 * nt + 2 * nb;
    int rc = ensure_cap(m, &m->tr_meta, &m->tr_meta_cap, std::max(need, (size_t)1 << 16));
    if (rc) return rc;
    std::vector<int32_t> meta(need);
    int32_t* p = meta.data();
    auto put = [&](const void* src, size_t n) { memcpy(p, src, n * 4); p += n; return (int32_t*)(m->tr_meta + (p - n - meta.data())); };
    std::vector<int32_t> pa(S, 0), pr(S, 0), pc(S, 0), pf(S, 0);
    if (prior_dev)
        for (int i = 0; i < S; ++i) { pa[i] = a0[ck.seq[i]]; pr[i] = r0[ck.seq[i]]; pc[i] = pn[ck.seq[i]]; pf[i] = fl[ck.seq[i]]; }
    AttRagged rg{};
    rg.seq_off = put(ck.off.data(), S);
    rg.seq_p = put(ck.p.data(), S);
    rg.seq_q = put(ck.q.data(), S);
    rg.seq_root = put(ck.root.data(), S);
    rg.seq_vt = reinterpret_cast<const uint32_t*>(put(ck.vt.data(), S));
    const int32_t* d_pa = put(pa.data(), S);
    const int32_t* d_pr = put(pr.data(), S);
    const int32_t* d_pc = put(pc.data(), S);
    const int32_t* d_pf = put(pf.data(), S);
    rg.tile_seq = put(ck.tile_seq.data(), nt);
    rg.tile_j = put(ck.tile_j.data(), nt);
    rg.blk_seq = put(ck.blk_seq.data(), nb);
    rg.blk_j = put(ck.blk_j.data(), nb);
    rg.n_tiles = (int)nt;
    rg.n_blocks = (int)nb;
    PGMI_HIP(hipMemcpyAsync(m->tr_meta, meta.data(), need * 4, hipMemcpyHostToDevice, s));
    PGMI_HIP(hipMemcpyAsync(m->tokens, ck.tokens.data(), (size_t)M * 4, hipMemcpyHostToDevice, s));
    PGMI_HIP(hipStreamSynchronize(s));                 // the host vectors go out of scope with the caller's chunk
    m->last_B = m->last_T = 0;                          // the V^T planes now hold another layout: the dense path clears them again
    rc = run_decoder(m, 0, T, &rg, M, ck.att_flops);
    if (!rc) rc = narrow_head(m, m->x, M);
    if (rc) return rc;
    { ProfScope ps(m, PGMI_K_SCORE, 0, (double)S * T * 8);
      launch_seq_loglik_ragged(m->lp, m->tokens, rg.seq_off, rg.seq_p, rg.seq_root, S, T, V, prior_dev, d_pa, d_pr, d_pc, d_pf, alpha,
                               prior_dev ? eve.dev : nullptr, eve.beta, eve.fallback, m->denom, s); }
    PGMI_HIP(hipGetLastError());
    return PGMI_OK;
}

}  // namespace pgmi

extern "C" {

int pgmi_tr_token_logprobs(pgmi_model* m, const int32_t* tokens, int B, int T, float* out) {
    if (!m || !tokens || !out || B <= 0 || T <= 0) { set_error("bad argument"); return PGMI_EINVAL; }
    if (m->cfg.arch != PGMI_ARCH_TRANCEPTION) { set_error("not a Tranception model"); return PGMI_EINVAL; }
    const int V = m->cfg.vocab;
    int rc = check_vocab(tokens, B, T, V);
    if (rc) return rc;
    if (T + 31 > m->max_rows) { set_error("T=%d exceeds workspace rows %d", T, m->max_rows); return PGMI_EINVAL; }
    rc = check_ctx(m, T);
    if (rc) return rc;
    PGMI_HIP(hipSetDevice(m->device));
    rc = for_each_chunk(m, B, T, [&](int b0, int bc) {
        PGMI_HIP(hipMemcpyAsync(m->tokens, tokens + (size_t)b0 * T, (size_t)bc * T * 4, hipMemcpyHostToDevice, m->stream));
        int rc = run_decoder(m, bc, T);
        if (!rc) rc = narrow_head(m, m->x, bc * T);
        if (rc) return rc;
        PGMI_HIP(hipMemcpyAsync(out + (size_t)b0 * T * V, m->lp, (size_t)bc * T * V * 4, hipMemcpyDeviceToHost, m->stream));
        return PGMI_OK;
    });
    return rc ? rc : check_nonfinite(m);
}

int pgmi_tr_sequence_loglik(pgmi_model* m, const int32_t* tokens, const int32_t* lens, int B, int T,
                            const float* log_prior, int P, const int32_t* prior_a0, const int32_t* prior_row0,
                            const int32_t* prior_n, const int32_t* prior_flip, float alpha, float* out) {
    return pgmi_tr_sequence_loglik_eve(m, tokens, lens, B, T, log_prior, P, prior_a0, prior_row0, prior_n, prior_flip, alpha, nullptr, 0.0f,
                                       0, out);
}

int pgmi_tr_sequence_loglik_eve(pgmi_model* m, const int32_t* tokens, const int32_t* lens, int B, int T,
                                const float* log_prior, int P, const int32_t* prior_a0, const int32_t* prior_row0,
                                const int32_t* prior_n, const int32_t* prior_flip, float alpha, const float* eve_log_prior, float beta,
                                int eve_fallback, float* out) {
    if (!m || !tokens || !lens || !out || B <= 0 || T <= 0) { set_error("bad argument"); return PGMI_EINVAL; }
    if (eve_log_prior && !log_prior) { set_error("the EVE prior is fused on the retrieval prior's rows: log_prior is NULL"); return PGMI_EINVAL; }
    TrEve eve{eve_log_prior, beta, eve_fallback, nullptr};
    if (m->cfg.arch != PGMI_ARCH_TRANCEPTION) { set_error("not a Tranception model"); return PGMI_EINVAL; }
    if (log_prior && (!prior_a0 || !prior_row0 || !prior_n || !prior_flip || P <= 0)) { set_error("incomplete retrieval arguments"); return PGMI_EINVAL; }
    const int V = m->cfg.vocab;
    int rc = check_vocab(tokens, B, T, V);
    if (rc) return rc;
    for (int b = 0; b < B; ++b) {
        if (lens[b] < 1 || lens[b] > T) { set_error("lens[%d]=%d out of range", b, lens[b]); return PGMI_EINVAL; }
        if (log_prior && prior_n[b] > 0 &&
            (prior_a0[b] < 0 || prior_a0[b] + prior_n[b] > T - 1 || prior_row0[b] < 0 || prior_row0[b] + prior_n[b] > P)) {
            set_error("retrieval slice of sequence %d out of range", b);
            return PGMI_EINVAL;
        }
    }
    if (T + 31 > m->max_rows) { set_error("T=%d exceeds workspace rows %d", T, m->max_rows); return PGMI_EINVAL; }
    rc = check_ctx(m, T);
    if (rc) return rc;
    PGMI_HIP(hipSetDevice(m->device));
    hipStream_t s = m->stream;
    rc = upload_prior(m, log_prior, P, &eve);
    if (rc) return rc;
    rc = for_each_chunk(m, B, T, [&](int b0, int bc) {
        PGMI_HIP(hipMemcpyAsync(m->tokens, tokens + (size_t)b0 * T, (size_t)bc * T * 4, hipMemcpyHostToDevice, s));
        PGMI_HIP(hipMemcpyAsync(m->kv_len, lens + b0, (size_t)bc * 4, hipMemcpyHostToDevice, s));
        int32_t *da0 = nullptr, *dr0 = nullptr, *dn = nullptr, *dfl = nullptr;
        if (log_prior) {            // four small int arrays share aux_i / row_idx / pos_idx (pos_idx is unused by Tranception)
            da0 = m->aux_i; dr0 = m->row_idx; dn = m->pos_idx; dfl = m->pos_idx + bc;
            PGMI_HIP(hipMemcpyAsync(da0, prior_a0 + b0, (size_t)bc * 4, hipMemcpyHostToDevice, s));
            PGMI_HIP(hipMemcpyAsync(dr0, prior_row0 + b0, (size_t)bc * 4, hipMemcpyHostToDevice, s));
            PGMI_HIP(hipMemcpyAsync(dn, prior_n + b0, (size_t)bc * 4, hipMemcpyHostToDevice, s));
            PGMI_HIP(hipMemcpyAsync(dfl, prior_flip + b0, (size_t)bc * 4, hipMemcpyHostToDevice, s));
        }
        int rc = run_decoder(m, bc, T);
        if (!rc) rc = narrow_head(m, m->x, bc * T);
        if (rc) return rc;
        { ProfScope p(m, PGMI_K_SCORE, 0, (double)bc * T * 8);
          launch_seq_loglik(m->lp, m->tokens, m->kv_len, bc, T, V, log_prior ? m->tr_prior : nullptr, da0, dr0, dn, dfl, alpha,
                            eve.dev, eve.beta, eve.fallback, m->denom, s); }
        PGMI_HIP(hipMemcpyAsync(out + b0, m->denom, (size_t)bc * 4, hipMemcpyDeviceToHost, s));
        return PGMI_OK;
    });
    return rc ? rc : check_nonfinite(m);
}

int pgmi_tr_sequence_loglik_shared(pgmi_model* m, const int32_t* tokens, const int32_t* ref, int B, int T,
                                   const float* log_prior, int P, const int32_t* prior_a0, const int32_t* prior_row0,
                                   const int32_t* prior_n, const int32_t* prior_flip, float alpha, float* out, float* token_logprobs,
                                   int64_t* rows_forwarded) {
    return pgmi_tr_sequence_loglik_shared_eve(m, tokens, ref, B, T, log_prior, P, prior_a0, prior_row0, prior_n, prior_flip, alpha, nullptr,
                                              0.0f, 0, out, token_logprobs, rows_forwarded);
}

int pgmi_tr_sequence_loglik_shared_eve(pgmi_model* m, const int32_t* tokens, const int32_t* ref, int B, int T,
                                       const float* log_prior, int P, const int32_t* prior_a0, const int32_t* prior_row0,
                                       const int32_t* prior_n, const int32_t* prior_flip, float alpha, const float* eve_log_prior,
                                       float beta, int eve_fallback, float* out, float* token_logprobs, int64_t* rows_forwarded) {
    if (!m || !tokens || !ref || !out || B <= 0 || T <= 0) { set_error("bad argument"); return PGMI_EINVAL; }
    if (eve_log_prior && !log_prior) { set_error("the EVE prior is fused on the retrieval prior's rows: log_prior is NULL"); return PGMI_EINVAL; }
    TrEve eve{eve_log_prior, beta, eve_fallback, nullptr};
    if (m->cfg.arch != PGMI_ARCH_TRANCEPTION) { set_error("not a Tranception model"); return PGMI_EINVAL; }
    if (log_prior && (!prior_a0 || !prior_row0 || !prior_n || !prior_flip || P <= 0)) { set_error("incomplete retrieval arguments"); return PGMI_EINVAL; }
    if (check_ctx(m, T)) return PGMI_EINVAL;
    const int V = m->cfg.vocab, D = m->cfg.embed_dim;
    const int Tpad = (T + 31) / 32 * 32;
    if (2 * Tpad > m->max_rows) { set_error("T=%d exceeds workspace rows %d", T, m->max_rows); return PGMI_EINVAL; }
    int rc = check_vocab(tokens, B, T, V);
    if (rc) return rc;
    for (int b = 0; b < B; ++b) {
        if (ref[b] < 0 || ref[b] >= B || ref[ref[b]] != ref[b]) { set_error("ref[%d]=%d is not a root (a sequence that is its own reference)", b, ref[b]); return PGMI_EINVAL; }
        if (log_prior && prior_n[b] > 0 &&
            (prior_a0[b] < 0 || prior_a0[b] + prior_n[b] > T - 1 || prior_row0[b] < 0 || prior_row0[b] + prior_n[b] > P)) {
            set_error("retrieval slice of sequence %d out of range", b);
            return PGMI_EINVAL;
        }
    }
    PGMI_HIP(hipSetDevice(m->device));
    hipStream_t s = m->stream;
    rc = upload_prior(m, log_prior, P, &eve);
    if (rc) return rc;
    // first own token of every sequence: its first difference from its root (a copy of the root: the last token)
    std::vector<int> a0(B, 0);
    std::vector<std::vector<int>> members(B);
    std::vector<int> roots;
    for (int b = 0; b < B; ++b) {
        if (ref[b] == b) { roots.push_back(b); continue; }
        const int32_t *x = tokens + (size_t)b * T, *y = tokens + (size_t)ref[b] * T;
        int p = 0;
        while (p < T && x[p] == y[p]) ++p;
        a0[b] = std::min(p, T - 1);
        members[ref[b]].push_back(b);
    }
    const int cap = m->max_rows;
    int64_t forwarded = 0;
    std::vector<float> lp_host;
    TrChunk ck;
    auto flush = [&]() -> int {
        if (ck.seq.empty()) return PGMI_OK;
        int rc = run_tranception_shared(m, ck, T, log_prior ? m->tr_prior : nullptr, prior_a0, prior_row0, prior_n, prior_flip, alpha, eve);
        if (rc) return rc;
        const int S = (int)ck.seq.size();
        std::vector<float> res(S);
        PGMI_HIP(hipMemcpyAsync(res.data(), m->denom, (size_t)S * 4, hipMemcpyDeviceToHost, s));
        if (token_logprobs) {
            lp_host.resize((size_t)ck.rows * V);
            PGMI_HIP(hipMemcpyAsync(lp_host.data(), m->lp, lp_host.size() * 4, hipMemcpyDeviceToHost, s));
        }
        PGMI_HIP(hipStreamSynchronize(s));
        for (int i = 0; i < S; ++i) out[ck.seq[i]] = res[i];
        if (token_logprobs)
            for (int i = 0; i < S; ++i) {
                float* dst = token_logprobs + (size_t)ck.seq[i] * T * V;
                const int a = ck.p[i], r = ck.root[i];
                if (a > 0) memcpy(dst, lp_host.data() + (size_t)ck.off[r] * V, (size_t)a * V * 4);
                memcpy(dst + (size_t)a * V, lp_host.data() + (size_t)ck.off[i] * V, (size_t)(T - a) * V * 4);
            }
        forwarded += ck.rows;
        ck = TrChunk();
        return PGMI_OK;
    };
    for (int r : roots) {
        auto padded_rows = [&](int b) { return (T - a0[b] / 32 * 32 + 31) / 32 * 32; };
        const int first = members[r].empty() ? 0 : padded_rows(members[r][0]);
        if (!ck.seq.empty() && ck.padded + Tpad + first > cap) { int rc = flush(); if (rc) return rc; }
        int rl = ck.add(r, tokens + (size_t)r * T, T, 0, -1, D);
        for (int b : members[r]) {
            if (ck.padded + padded_rows(b) > cap) {
                int rc = flush();
                if (rc) return rc;
                rl = ck.add(r, tokens + (size_t)r * T, T, 0, -1, D);           // the root again: its rows serve the rest of the group
            }
            ck.add(b, tokens + (size_t)b * T, T, a0[b], rl, D);
        }
    }
    rc = flush();
    if (rc) return rc;
    if (rows_forwarded) *rows_forwarded = forwarded;
    return check_nonfinite(m);
}

}  // extern "C"
