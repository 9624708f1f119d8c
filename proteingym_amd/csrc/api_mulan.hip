// MULAN (proteingym/baselines/mulan/mulan/{model.py,model_utils.py}, compute_fitness.py): ESM2's encoder and LM head (api_esm.hip
// walk_esm, run_encoder, head_hidden) -- or SaProt's, over its 446-token vocabulary -- behind a structure adapter.  The adapter
// (model_utils.py:59-97) maps the seven backbone and side-chain angles of every token through Linear(7 -> D), one full ESM layer of
// width D and the EsmEncoder's closing LayerNorm; its EsmConfig names no position_embedding_type, so the layer's attention has neither
// rotary nor a position table.  The result is added to the word embeddings before token dropout (:156-176).  The scoring rule is
// SaProt's: one forward per distinct SET of mutated positions with the set's tokens replaced by <mask>; here the angle rows of the set
// are overwritten with -4 as well (compute_fitness.py:117-126), so the adapter runs per set too.  Its input rows are built on the
// device from the bound chunk (mulan_rows_kernel: no [n_sets][T][7] tensor exists anywhere), the layer is run_encoder's own body
// (encoder_layer) with rotary off, and mulan_embed_kernel forms the embedding with launch_embed's dropout factor and op order.
#include "model.h"

namespace pgmi {

constexpr int kMuAngles = 7;
constexpr int kSaFirst = 5, kSaGroups = PGMI_SAPROT_GROUPS, kSaWidth = 21;      // api_saprot.hip: the 446-token layout

static int64_t layer_count(int64_t D, int64_t F) { return 2 * D + 4 * (D * D + D) + 2 * D + (F * D + F) + (D * F + D); }

// ESM2's blob (pgmi_weight_count's last branch), then MLP.weight [D][7], MLP.bias, one layer (FC1 / FC2 of width 4 D), the adapter's
// final LayerNorm
int64_t mulan_weight_count(const pgmi_config* c) {
    const int64_t D = c->embed_dim, F = c->ffn_dim, V = c->vocab;
    int64_t n = V * D;
    if (c->emb_layer_norm_before) n += 2 * D;
    n += (int64_t)c->layers * layer_count(D, F) + 2 * D + (D * D + D) + 2 * D + V;
    return n + D * kMuAngles + D + layer_count(D, 4 * D) + 2 * D;      // the adapter's EsmConfig: intermediate_size = 4 hidden
}

int create_mulan(pgmi_model* m, const pgmi_config* cfg, const float* w, int64_t n_weights, int mask_id) {
    const bool fs = cfg->vocab == PGMI_SAPROT_VOCAB;
    const int n_special = fs ? kSaFirst : 4;                 // <cls> <pad> <eos> <unk> (and SaProt's <mask>); ESM2's <mask> is its last id
    if (mask_id < 0 || mask_id >= cfg->vocab || mask_id == PGMI_TOK_PAD || (fs && mask_id >= n_special) ||
        (!fs && mask_id >= n_special && mask_id != PGMI_TOK_MASK)) {
        set_error("MULAN <mask> id %d: must be a special token of the %d-token vocabulary and not <pad> (%d)", mask_id, cfg->vocab, PGMI_TOK_PAD);
        return PGMI_EINVAL;
    }
    if (cfg->embed_dim % 4) { set_error("MULAN: embed_dim %d must be a multiple of 4 (the embedding kernel's 16-byte rows)", cfg->embed_dim); return PGMI_EINVAL; }
    m->mask_id = mask_id;
    m->n_token_ids = cfg->vocab;
    m->mu_groups = fs ? kSaGroups : 0;
    const size_t D = cfg->embed_dim;
    BlobCursor c(m, w, n_weights);
    walk_esm(c);
    c.upload(&m->mu_w, D * kMuAngles);
    c.upload(&m->mu_b, D);
    m->mu_layer.ffn = 4 * (int)D;
    walk_esm_layer(c, &m->mu_layer, 4 * D);
    c.upload(&m->mu_lna_w, D);
    c.upload(&m->mu_lna_b, D);
    return c.finish();
}

// run_encoder's embed step.  m->x holds the adapter's input rows (launch_mulan_rows), m->denom / m->kv_len the statistics of m->tokens.
// The adapter layer and its LayerNorm leave the structure rows in m->h (fp32; free between layers), the embed kernel writes m->x.
int mulan_embed(pgmi_model* m, int B, int T) {
    const int M = B * T, D = m->cfg.embed_dim;
    int rc = encoder_layer(m, m->mu_layer, B, T, /*rotary=*/false);
    if (rc) return rc;
    launch_layernorm(m->x, m->mu_lna_w, m->mu_lna_b, M, D, 1e-5f, m->h, m->stream);
    launch_mulan_embed(m->tokens, m->denom, m->embed_tokens, m->h, m->cfg.token_dropout, M, T, D, m->x, m->stream, m->mask_id);
    return PGMI_OK;
}

static int mulan_check(pgmi_model* m, int T) {
    if (m->cfg.arch != PGMI_ARCH_MULAN) { set_error("not a MULAN model (arch %d)", m->cfg.arch); return PGMI_EINVAL; }
    // the reference forwards the whole chunk at once (no windows): what the workspace cannot hold in one sequence is refused
    if (T + 31 > m->max_rows) {
        set_error("T=%d exceeds workspace rows %d (max_rows; MULAN sequences are not windowed)", T, m->max_rows);
        return PGMI_EINVAL;
    }
    if (m->mu_T == 0) { set_error("MULAN: no structure bound (pgmi_mulan_set_structure)"); return PGMI_EINVAL; }
    if (T != m->mu_T) { set_error("MULAN: T=%d but the bound structure has %d tokens", T, m->mu_T); return PGMI_EINVAL; }
    return PGMI_OK;
}

// a position CSR over n rows: offsets from 0 and not descending; positions inside [0, T), ascending without repeats inside a row
static int check_csr(const int32_t* off, const int32_t* pos, int n, int T, bool allow_empty, const char* what) {
    if (off[0] != 0) { set_error("%s_off[0] must be 0", what); return PGMI_EINVAL; }
    for (int s = 0; s < n; ++s) {
        if (off[s + 1] < off[s] || (!allow_empty && off[s + 1] == off[s]) || off[s + 1] - off[s] > T) {
            set_error("position %s %d is empty or larger than T", what, s);
            return PGMI_EINVAL;
        }
        for (int e = off[s]; e < off[s + 1]; ++e)
            if (pos[e] < 0 || pos[e] >= T || (e > off[s] && pos[e] <= pos[e - 1])) {
                set_error("position %s %d: position %d out of range or not ascending", what, s, pos[e]);
                return PGMI_EINVAL;
            }
    }
    return PGMI_OK;
}

// the head on the R rows of m->x (row_idx: gathered first): the log-softmax rows [R][V] (full) or SaProt's group table [R][21]
static int mulan_head(pgmi_model* m, int R, const int32_t* row_idx, bool full) {
    const int D = m->cfg.embed_dim, V = m->cfg.vocab;
    ProfScope p(m, PGMI_K_HEAD, 2.0 * R * D * (D + V), 0);
    int rc = head_hidden(m, R, row_idx);
    if (rc) return rc;
    if (m->mu_groups)
        rc = launch_group_logsoftmax(m->g, m->head_w, m->head_b, R, D, V, kSaFirst, kSaGroups, kSaWidth, full ? m->lp : nullptr,
                                     full ? nullptr : m->lp, m->nonfinite, m->stream);
    else
        launch_vocab_logsoftmax(m->g, m->head_w, m->head_b, R, D, V, m->lp, m->nonfinite, m->stream);
    return rc;
}

}  // namespace pgmi

extern "C" {

int64_t pgmi_mulan_weight_count(const pgmi_config* cfg) {
    if (!cfg || cfg->layers <= 0 || cfg->embed_dim <= 0 || cfg->ffn_dim <= 0 || cfg->vocab <= 0) return -1;
    return mulan_weight_count(cfg);
}

int pgmi_mulan_model_create(const pgmi_config* cfg, int mask_id, int groups, const float* w, int64_t n_weights, int device,
                            pgmi_model** out) {
    if (cfg && cfg->arch != PGMI_ARCH_MULAN) {
        if (out) *out = nullptr;
        set_error("pgmi_mulan_model_create needs arch PGMI_ARCH_MULAN, got %d", cfg->arch);
        return PGMI_EINVAL;
    }
    if (cfg && !((groups == 0 && cfg->vocab == PGMI_VOCAB) || (groups == kSaGroups && cfg->vocab == PGMI_SAPROT_VOCAB))) {
        if (out) *out = nullptr;
        set_error("MULAN: groups %d with vocab %d (0 with the %d-token ESM alphabet, %d with SaProt's %d tokens)", groups, cfg->vocab,
                  PGMI_VOCAB, kSaGroups, PGMI_SAPROT_VOCAB);
        return PGMI_EINVAL;
    }
    return model_create(cfg, w, n_weights, device, out, mask_id);
}

int pgmi_mulan_set_structure(pgmi_model* m, const float* angles, const float* plddt, int T) {
    if (!m || m->cfg.arch != PGMI_ARCH_MULAN) { set_error("pgmi_mulan_set_structure: not a MULAN model"); return PGMI_EINVAL; }
    if (!angles || !plddt || T < 3) { set_error("bad argument (T counts <cls>, at least one residue and <eos>)"); return PGMI_EINVAL; }
    if (T + 31 > m->max_rows) { set_error("T=%d exceeds workspace rows %d (max_rows; MULAN sequences are not windowed)", T, m->max_rows); return PGMI_EINVAL; }
    for (int t = 1; t < T - 1; ++t) {
        bool ok = std::isfinite(plddt[t]);
        for (int k = 0; k < kMuAngles; ++k) ok = ok && std::isfinite(angles[(size_t)t * kMuAngles + k]);
        if (!ok) { set_error("non-finite angle or pLDDT at token %d", t); return PGMI_EINVAL; }
    }
    PGMI_HIP(hipSetDevice(m->device));
    PGMI_HIP(hipStreamSynchronize(m->stream));               // no forward is reading the previous chunk
    m->mu_T = 0;
    const size_t cap = std::max<size_t>(T, 1024);
    int rc = ensure_cap(m, &m->mu_angles, &m->mu_angles_cap, cap * kMuAngles);
    if (!rc) rc = ensure_cap(m, &m->mu_plddt, &m->mu_plddt_cap, cap);
    if (rc) return rc;
    PGMI_HIP(hipMemcpy(m->mu_angles, angles, (size_t)T * kMuAngles * 4, hipMemcpyHostToDevice));
    PGMI_HIP(hipMemcpy(m->mu_plddt, plddt, (size_t)T * 4, hipMemcpyHostToDevice));
    m->mu_T = T;
    return PGMI_OK;
}

int pgmi_mulan_token_logprobs(pgmi_model* m, const int32_t* tokens, int B, int T, const int32_t* row_off, const int32_t* row_pos, float* out) {
    if (!m || !tokens || !row_off || !row_pos || !out || B <= 0 || T <= 0) { set_error("bad argument"); return PGMI_EINVAL; }
    int rc = mulan_check(m, T);
    if (!rc) rc = check_vocab(tokens, B, T, m->n_token_ids);
    if (!rc) rc = check_csr(row_off, row_pos, B, T, true, "row");
    if (rc) return rc;
    for (size_t i = 0; i < (size_t)B * T; ++i)
        if (tokens[i] == PGMI_TOK_PAD) { set_error("<pad> at [%zu,%zu]: MULAN rows are whole chunks", i / T, i % T); return PGMI_EINVAL; }
    PGMI_HIP(hipSetDevice(m->device));
    hipStream_t st = m->stream;
    const int V = m->cfg.vocab, D = m->cfg.embed_dim;
    std::vector<void*> pool;
    auto cleanup = [&]() { for (void* p : pool) hipFree(p); };
    int32_t *d_off = nullptr, *d_pos = nullptr;
    rc = dev_upload(pool, &d_off, row_off, (size_t)B + 1);
    if (!rc) rc = dev_upload(pool, &d_pos, row_pos, (size_t)row_off[B]);
    if (rc) { cleanup(); return rc; }
    rc = for_each_chunk(m, B, T, [&](int b0, int bc) {
        const int M = bc * T;
        PGMI_HIP(hipMemcpyAsync(m->tokens, tokens + (size_t)b0 * T, (size_t)M * 4, hipMemcpyHostToDevice, st));
        { ProfScope p(m, PGMI_K_EMBED, 2.0 * M * D * kMuAngles, (double)M * D * 4);
          launch_mulan_rows(nullptr, d_off, d_pos, b0, bc, T, m->mask_id, m->mu_angles, m->mu_plddt, m->mu_w, m->mu_b, D, nullptr, nullptr,
                            m->x, st); }
        int rc = run_encoder(m, bc, T);
        if (!rc) rc = mulan_head(m, M, nullptr, true);
        if (rc) return rc;
        PGMI_HIP(hipGetLastError());
        PGMI_HIP(hipMemcpyAsync(out + (size_t)b0 * T * V, m->lp, (size_t)M * V * 4, hipMemcpyDeviceToHost, st));
        return PGMI_OK;
    });
    hipStreamSynchronize(st);
    cleanup();
    return rc ? rc : check_nonfinite(m);
}

int pgmi_mulan_set_logprobs(pgmi_model* m, const int32_t* wt_tokens, int T, const int32_t* set_off, const int32_t* set_pos, int n_sets,
                            float* out) {
    if (!m || !wt_tokens || !set_off || !set_pos || !out || T <= 0 || n_sets <= 0) { set_error("bad argument"); return PGMI_EINVAL; }
    int rc = mulan_check(m, T);
    if (rc) return rc;
    for (int t = 0; t < T; ++t)
        if (wt_tokens[t] < 0 || wt_tokens[t] >= m->n_token_ids || wt_tokens[t] == PGMI_TOK_PAD) {
            set_error("wt token %d invalid at %d", wt_tokens[t], t);
            return PGMI_EINVAL;
        }
    if ((rc = check_csr(set_off, set_pos, n_sets, T, false, "set"))) return rc;
    const int n_special = m->mu_groups ? kSaFirst : 4;
    for (int e = 0; e < set_off[n_sets]; ++e) {
        const int tk = wt_tokens[set_pos[e]];
        if (tk < n_special || tk == m->mask_id) { set_error("token %d at position %d of a position set is a special token", tk, set_pos[e]); return PGMI_EINVAL; }
    }
    PGMI_HIP(hipSetDevice(m->device));
    hipStream_t st = m->stream;
    const int D = m->cfg.embed_dim, W = m->mu_groups ? kSaGroups : m->cfg.vocab;
    std::vector<void*> pool;
    auto cleanup = [&]() { for (void* p : pool) hipFree(p); };
    int32_t *d_wt = nullptr, *d_off = nullptr, *d_pos = nullptr;
    rc = dev_upload(pool, &d_wt, wt_tokens, (size_t)T);
    if (!rc) rc = dev_upload(pool, &d_off, set_off, (size_t)n_sets + 1);
    if (!rc) rc = dev_upload(pool, &d_pos, set_pos, (size_t)set_off[n_sets]);
    if (rc) { cleanup(); return rc; }
    rc = for_each_chunk(m, n_sets, T, [&](int s0, int bc) {
        const int e0 = set_off[s0], R = set_off[s0 + bc] - e0;         // R <= bc * T <= max_rows kept rows
        { ProfScope p(m, PGMI_K_EMBED, 2.0 * bc * T * D * kMuAngles, (double)bc * T * (D * 4 + 8));
          launch_mulan_rows(d_wt, d_off, d_pos, s0, bc, T, m->mask_id, m->mu_angles, m->mu_plddt, m->mu_w, m->mu_b, D, m->tokens, m->row_idx,
                            m->x, st); }
        bool compacted = false;
        int rc = run_encoder(m, bc, T, m->row_idx, R, &compacted);
        if (!rc) rc = mulan_head(m, R, compacted ? nullptr : m->row_idx, false);
        if (rc) return rc;
        PGMI_HIP(hipGetLastError());
        PGMI_HIP(hipMemcpyAsync(out + (size_t)e0 * W, m->lp, (size_t)R * W * 4, hipMemcpyDeviceToHost, st));
        return PGMI_OK;
    });
    hipStreamSynchronize(st);
    cleanup();
    return rc ? rc : check_nonfinite(m);
}

}  // extern "C"
