// SaProt (proteingym/baselines/saprot/compute_fitness.py; HF EsmForMaskedLM): ESM2's encoder and LM head (api_esm.hip create_esm,
// run_encoder, head_hidden) over a 446-token vocabulary -- 5 specials, then 21 amino-acid letters x 21 Foldseek 3Di letters, the
// amino-acid letter major -- with <mask> at the id the caller names.  What this file adds is the scoring rule: the reference
// (compute_fitness.py:17-55) forwards every mutant once with the amino-acid half of its mutated tokens masked ('#' + structure letter)
// and adds, per sub-mutation, log(sum probs[mt group] / sum probs[wt group]) over the 21 tokens of an amino-acid letter.  The masked
// row depends on the SET of mutated positions only, so pgmi_saprot_group_logprobs forwards every distinct position set once: its rows
// are built on the device from the resident wild type (saprot_rows_kernel), the last layer and the head run on the rows of the
// masked positions only, and group_logsoftmax_kernel writes per (set, position) the 21 group log-probabilities the scores are
// differences of (pgmi_score_mutants with vocab = 21 over that table).  No windowing, like the reference.
#include "model.h"

namespace pgmi {

constexpr int kSaFirst = 5, kSaGroups = 21, kSaWidth = 21;      // include/pgmi.h: the vocabulary layout
static_assert(kSaFirst + kSaGroups * kSaWidth == PGMI_SAPROT_VOCAB, "SaProt vocabulary layout");

// Weight blob: ESM2's (include/pgmi.h pgmi_weight_count) with V = 446.
int create_saprot(pgmi_model* m, const pgmi_config* cfg, const float* w, int64_t n_weights, int mask_id) {
    if (mask_id < 0 || mask_id >= kSaFirst || mask_id == PGMI_TOK_PAD) {
        set_error("SaProt <mask> id %d: must be one of the %d special tokens and not <pad> (%d)", mask_id, kSaFirst, PGMI_TOK_PAD);
        return PGMI_EINVAL;
    }
    m->mask_id = mask_id;
    m->n_token_ids = cfg->vocab;
    return create_esm(m, cfg, w, n_weights);
}

static int saprot_check(pgmi_model* m, int T) {
    if (m->cfg.arch != PGMI_ARCH_SAPROT) { set_error("not a SaProt model (arch %d)", m->cfg.arch); return PGMI_EINVAL; }
    // the reference forwards the whole chunk at once (no windows): what the workspace cannot hold in one sequence is refused
    if (T + 31 > m->max_rows) {
        set_error("T=%d exceeds workspace rows %d (max_rows; SaProt sequences are not windowed)", T, m->max_rows);
        return PGMI_EINVAL;
    }
    return PGMI_OK;
}

}  // namespace pgmi

extern "C" {

int pgmi_saprot_model_create(const pgmi_config* cfg, int mask_id, const float* w, int64_t n_weights, int device, pgmi_model** out) {
    if (cfg && cfg->arch != PGMI_ARCH_SAPROT) {
        if (out) *out = nullptr;
        set_error("pgmi_saprot_model_create needs arch PGMI_ARCH_SAPROT, got %d", cfg->arch);
        return PGMI_EINVAL;
    }
    return model_create(cfg, w, n_weights, device, out, mask_id);
}

int pgmi_saprot_token_logprobs(pgmi_model* m, const int32_t* tokens, int B, int T, float* out) {
    if (!m || !tokens || !out || B <= 0 || T <= 0) { set_error("bad argument"); return PGMI_EINVAL; }
    int rc = saprot_check(m, T);
    if (!rc) rc = check_tokens(tokens, B, T, m->n_token_ids);
    if (rc) return rc;
    PGMI_HIP(hipSetDevice(m->device));
    const int V = m->cfg.vocab, D = m->cfg.embed_dim;
    rc = for_each_chunk(m, B, T, [&](int b0, int bc) {
        const int M = bc * T;
        PGMI_HIP(hipMemcpyAsync(m->tokens, tokens + (size_t)b0 * T, (size_t)M * 4, hipMemcpyHostToDevice, m->stream));
        int rc = run_encoder(m, bc, T);
        if (rc) return rc;
        { ProfScope p(m, PGMI_K_HEAD, 2.0 * M * D * (D + V), 0);
          rc = head_hidden(m, M, nullptr);
          if (!rc) rc = launch_group_logsoftmax(m->g, m->head_w, m->head_b, M, D, V, kSaFirst, kSaGroups, kSaWidth, m->lp, nullptr,
                                                m->nonfinite, m->stream);
          if (rc) return rc; }
        PGMI_HIP(hipGetLastError());
        PGMI_HIP(hipMemcpyAsync(out + (size_t)b0 * T * V, m->lp, (size_t)M * V * 4, hipMemcpyDeviceToHost, m->stream));
        return PGMI_OK;
    });
    return rc ? rc : check_nonfinite(m);
}

int pgmi_saprot_group_logprobs(pgmi_model* m, const int32_t* wt_tokens, int T, const int32_t* set_off, const int32_t* set_pos,
                               int n_sets, float* out) {
    if (!m || !wt_tokens || !set_off || !set_pos || !out || T <= 0 || n_sets <= 0) { set_error("bad argument"); return PGMI_EINVAL; }
    int rc = saprot_check(m, T);
    if (rc) return rc;
    for (int t = 0; t < T; ++t)
        if (wt_tokens[t] < 0 || wt_tokens[t] >= m->n_token_ids || wt_tokens[t] == PGMI_TOK_PAD) {
            set_error("wt token %d invalid at %d", wt_tokens[t], t);
            return PGMI_EINVAL;
        }
    if (set_off[0] != 0) { set_error("set_off[0] must be 0"); return PGMI_EINVAL; }
    for (int s = 0; s < n_sets; ++s) {
        // at least one position per set, ascending without repeats (a set), inside the sequence, on a residue token
        if (set_off[s + 1] <= set_off[s] || set_off[s + 1] - set_off[s] > T) { set_error("position set %d is empty or larger than T", s); return PGMI_EINVAL; }
        for (int e = set_off[s]; e < set_off[s + 1]; ++e) {
            const int p = set_pos[e];
            if (p < 0 || p >= T || (e > set_off[s] && p <= set_pos[e - 1])) { set_error("position set %d: position %d out of range or not ascending", s, p); return PGMI_EINVAL; }
            if (wt_tokens[p] < kSaFirst) { set_error("position set %d: token %d at position %d is a special token", s, wt_tokens[p], p); return PGMI_EINVAL; }
        }
    }
    PGMI_HIP(hipSetDevice(m->device));
    hipStream_t st = m->stream;
    const int n_entries = set_off[n_sets], D = m->cfg.embed_dim, V = m->cfg.vocab;
    std::vector<void*> pool;
    auto cleanup = [&]() { for (void* p : pool) hipFree(p); };
    int32_t *d_wt = nullptr, *d_off = nullptr, *d_pos = nullptr;
    rc = dev_upload(pool, &d_wt, wt_tokens, (size_t)T);
    if (!rc) rc = dev_upload(pool, &d_off, set_off, (size_t)n_sets + 1);
    if (!rc) rc = dev_upload(pool, &d_pos, set_pos, (size_t)n_entries);
    if (rc) { cleanup(); return rc; }
    rc = for_each_chunk(m, n_sets, T, [&](int s0, int bc) {
        const int e0 = set_off[s0], R = set_off[s0 + bc] - e0;         // R <= bc * T <= max_rows kept rows
        { ProfScope p(m, PGMI_K_EMBED, 0, (double)bc * T * 8);
          launch_saprot_rows(d_wt, d_off, d_pos, s0, bc, T, kSaFirst, kSaGroups, kSaWidth, m->tokens, m->row_idx, st); }
        bool compacted = false;
        int rc = run_encoder(m, bc, T, m->row_idx, R, &compacted);
        if (rc) return rc;
        { ProfScope p(m, PGMI_K_HEAD, 2.0 * R * D * (D + V), 0);
          rc = head_hidden(m, R, compacted ? nullptr : m->row_idx);
          if (!rc) rc = launch_group_logsoftmax(m->g, m->head_w, m->head_b, R, D, V, kSaFirst, kSaGroups, kSaWidth, nullptr, m->lp,
                                                m->nonfinite, st);
          if (rc) return rc; }
        PGMI_HIP(hipGetLastError());
        PGMI_HIP(hipMemcpyAsync(out + (size_t)e0 * kSaGroups, m->lp, (size_t)R * kSaGroups * 4, hipMemcpyDeviceToHost, st));
        return PGMI_OK;
    });
    hipStreamSynchronize(st);
    cleanup();
    return rc ? rc : check_nonfinite(m);
}

}  // extern "C"
