// ProtSSN entries of the C ABI (include/pgmi.h, ProtSSN section): the blob walk, the graph of one structure, the
// six-layer EGNN forward, the ESM2 residue rows that feed it and the op entry of one layer's message.  The kernels that are not GEMMs
// are in egnn.hip.
// Per layer: one GEMM on the L node rows gives the per-node tables of the first edge Linear; then, per chunk of edges, the edge share
// (an fp32 GEMM on the 94 structure columns, never kept beyond the chunk), the edge-row kernel and the W2 product; then the
// aggregation over a CSR by target, W3, SiLU, W4 with the residual.  Every per-edge stage is row-local and a GEMM output element's sum
// does not depend on the launch's row count, so a node's bits do not depend on the chunk size.
#include "model.h"

namespace pgmi {

constexpr int PROTSSN_CHUNK_DEFAULT = 8192, PROTSSN_MAX_L = 1 << 16, PROTSSN_MAX_E = 1 << 24;

struct EgnnLayer {
    float *we = nullptr, *b1 = nullptr, *b2 = nullptr, *b3 = nullptr, *b4 = nullptr;
    float *wij = nullptr, *w2 = nullptr, *w3 = nullptr, *w4 = nullptr;      // fp32 mode
    W16 wij16, w216, w316, w416;
};

}  // namespace pgmi

struct pgmi_protssn {
    pgmi_model pm;                       // device, stream, allocation pool and profiling state (pgmi_protssn_profile_model)
    pgmi_protssn_config cfg;
    int D = 0, h = 0, hp = 0, Hp = 0, A = 0, Ap = 0, chunk = 0;
    std::vector<EgnnLayer> layers;
    float *wlin = nullptr, *blin = nullptr;
    // the graph last set: edges in the caller's order, the CSR by neighbour (off [L + 1], eid [E]), ea [E][Ap] = attributes | d2 | 0
    int L = 0, E = 0;
    DevBuf<int32_t> centre, nb, off, eid;
    DevBuf<float> ea;
    // workspace: x [L][D]; P [L][2 Hp]; S [chunk][Hp]; msg [E][hp]; t [L][2 D]; lp [L][20]; the operands (split planes or fp32 rows, 4
    // bytes per element either way) x16 [L][D], a [chunk][Hp], nA [L][D + hp], g [L][2 D]
    DevBuf<float> x, P, S, msg, t, lp;
    DevBuf<uint32_t> x16, a, nA, g;
};

namespace pgmi {

static int protssn_check(const pgmi_protssn_config* c) {
    if (!c) { set_error("null config"); return PGMI_EINVAL; }
    if (c->abi_version != PGMI_ABI_VERSION) { set_error("ABI version mismatch: got %d, library is %d", c->abi_version, PGMI_ABI_VERSION); return PGMI_EINVAL; }
    if (c->node_in < 32 || c->node_in % 32 || c->node_in > 8192) { set_error("ProtSSN: node_in %d must be a multiple of 32 in 32 .. 8192", c->node_in); return PGMI_EINVAL; }
    if (c->hidden < 1 || c->hidden > 4096) { set_error("ProtSSN: hidden %d outside 1 .. 4096", c->hidden); return PGMI_EINVAL; }
    if (c->layers < 1 || c->layers > 64) { set_error("ProtSSN: %d layers (1 .. 64)", c->layers); return PGMI_EINVAL; }
    if (c->edge_attr_dim < 1 || c->edge_attr_dim > 1023) { set_error("ProtSSN: edge_attr_dim %d outside 1 .. 1023", c->edge_attr_dim); return PGMI_EINVAL; }
    if (c->precision != PGMI_PREC_FP32 && c->precision != PGMI_PREC_F16X3) { set_error("ProtSSN runs in precision f16x3 or fp32"); return PGMI_EINVAL; }
    if (c->edge_chunk < 0) { set_error("ProtSSN: negative edge_chunk"); return PGMI_EINVAL; }
    return PGMI_OK;
}

static int64_t protssn_count(const pgmi_protssn_config* c) {
    const int64_t D = c->node_in, hp = roundup32(c->hidden), Ap = roundup32(c->edge_attr_dim + 1),
                  Hp = roundup32(2 * (2 * c->node_in + c->edge_attr_dim + 1));
    const int64_t layer = 2 * Hp * D + Hp * Ap + Hp + hp * Hp + hp + 2 * D * (D + hp) + 2 * D + D * 2 * D + D;
    return c->layers * layer + 20 * D + 20;
}

static int protssn_build(pgmi_protssn* m, const float* w, int64_t n_weights) {
    const size_t D = m->D, hp = m->hp, Hp = m->Hp, Ap = m->Ap;
    BlobCursor c(&m->pm, w, n_weights);
    m->layers.resize(m->cfg.layers);
    for (EgnnLayer& l : m->layers) {
        c.linear(&l.wij, &l.wij16, 2 * Hp * D, D);
        c.upload(&l.we, Hp * Ap);
        c.upload(&l.b1, Hp);
        c.linear(&l.w2, &l.w216, hp * Hp, Hp); c.upload(&l.b2, hp);
        c.linear(&l.w3, &l.w316, 2 * D * (D + hp), D + hp); c.upload(&l.b3, 2 * D);
        c.linear(&l.w4, &l.w416, D * 2 * D, 2 * D); c.upload(&l.b4, D);
    }
    c.upload(&m->wlin, 20 * D);
    c.upload(&m->blin, 20);
    return c.finish();
}

static int protssn_workspace(pgmi_protssn* m) {
    const size_t L = m->L, E = m->E, D = m->D, hp = m->hp, Hp = m->Hp, C = std::min<size_t>(m->chunk, E);
    return reserve_all(&m->pm, m->x, L * D, m->x16, L * D, m->P, L * 2 * Hp, m->S, C * Hp, m->a, C * Hp, m->msg, E * hp, m->nA, L * (D + hp),
                       m->t, L * 2 * D, m->g, L * 2 * D, m->lp, L * 20);
}

// a Linear on `rows` operand rows (split planes in precision f16x3, fp32 rows otherwise)
static int protssn_gemm(pgmi_protssn* m, int cls, const void* in, const float* w32, const W16& w16, const float* bias, const float* residual,
                        float* out, int rows, int N, int K) {
    ProfScope p(&m->pm, cls, 2.0 * rows * (double)N * K, 0);
    return linear(&m->pm, static_cast<const float*>(in), static_cast<const unsigned short*>(in), w32, w16, bias, residual, out, nullptr, rows, N, K,
                  EPI_NONE);
}

// one layer's messages and their sums: m->x [L][D] -> m->nA [L][D + hp] = [x | m_i], the W3 product's operand
static int protssn_message(pgmi_protssn* m, const EgnnLayer& l) {
    pgmi_model* pm = &m->pm;
    hipStream_t st = pm->stream;
    const int L = m->L, E = m->E, D = m->D, hp = m->hp, Hp = m->Hp, Ap = m->Ap;
    const bool split = m->cfg.precision != PGMI_PREC_FP32;
    int rc;
    if (split) {
        ProfScope p(pm, PGMI_K_LAYERNORM, 0, (double)L * D * 8);
        launch_split16(m->x, (int64_t)L * D, 1.0f, 2, D, reinterpret_cast<unsigned short*>(m->x16.p), st);
    }
    if ((rc = protssn_gemm(m, PGMI_K_GEMM_QKV, split ? (const void*)m->x16 : (const void*)m->x, l.wij, l.wij16, nullptr, nullptr, m->P, L, 2 * Hp, D)))
        return rc;
    for (int e0 = 0; e0 < E; e0 += m->chunk) {
        const int ec = std::min(m->chunk, E - e0);
        {
            ProfScope p(pm, PGMI_K_EMBED, 2.0 * ec * (double)Hp * Ap, 0);
            if ((rc = launch_gemm_f32(m->ea + (size_t)e0 * Ap, l.we, l.b1, nullptr, m->S, ec, Hp, Ap, EPI_NONE, st))) return rc;
        }
        {
            ProfScope p(pm, PGMI_K_ATTENTION, 0, (double)ec * Hp * 16);
            launch_egnn_edge_rows(m->P, m->S, m->centre + e0, m->nb + e0, ec, Hp, split, m->a, st);
        }
        if ((rc = protssn_gemm(m, PGMI_K_GEMM_OUT, m->a, l.w2, l.w216, l.b2, nullptr, m->msg + (size_t)e0 * hp, ec, hp, Hp))) return rc;
    }
    ProfScope p(pm, PGMI_K_LAYERNORM, 0, ((double)E * hp + 2.0 * L * (D + hp)) * 4);
    launch_egnn_aggregate(m->x, m->msg, m->off, m->eid, L, D, hp, split, m->nA, st);
    return PGMI_OK;
}

static int protssn_layers(pgmi_protssn* m) {
    pgmi_model* pm = &m->pm;
    hipStream_t st = pm->stream;
    const int L = m->L, D = m->D, hp = m->hp;
    const bool split = m->cfg.precision != PGMI_PREC_FP32;
    int rc;
    for (const EgnnLayer& l : m->layers) {
        if ((rc = protssn_message(m, l))) return rc;
        if ((rc = protssn_gemm(m, PGMI_K_GEMM_FC1, m->nA, l.w3, l.w316, l.b3, nullptr, m->t, L, 2 * D, D + hp))) return rc;
        {
            ProfScope p(pm, PGMI_K_KEPT_ROWS, 0, (double)L * 2 * D * 8);
            if (split) launch_silu_split(m->t, L, 2 * D, reinterpret_cast<unsigned short*>(m->g.p), st);
            else launch_egnn_silu_rows(m->t, L, 2 * D, reinterpret_cast<float*>(m->g.p), st);
        }
        if ((rc = protssn_gemm(m, PGMI_K_GEMM_FC2, m->g, l.w4, l.w416, l.b4, m->x, m->x, L, D, 2 * D))) return rc;
        if (pm->prof && (rc = prof_drain(pm))) return rc;
    }
    ProfScope p(pm, PGMI_K_HEAD, 2.0 * L * D * 20, 0);
    launch_egnn_head(m->x, m->wlin, m->blin, L, D, m->lp, st);
    PGMI_HIP(hipGetLastError());
    return PGMI_OK;
}

static int protssn_new(const pgmi_protssn_config* cfg, const float* w, int64_t n_weights, int device, pgmi_protssn** out) {
    if (!out) { set_error("null out"); return PGMI_EINVAL; }
    *out = nullptr;
    int rc = protssn_check(cfg);
    if (rc) return rc;
    pgmi_protssn* m = new pgmi_protssn();
    rc = side_open(&m->pm, "ProtSSN", w, n_weights, protssn_count(cfg), true, device, cfg->precision, nullptr);
    if (rc) { delete m; return rc; }
    m->cfg = *cfg;
    m->D = cfg->node_in; m->h = cfg->hidden; m->hp = roundup32(cfg->hidden); m->A = cfg->edge_attr_dim; m->Ap = roundup32(cfg->edge_attr_dim + 1);
    m->Hp = roundup32(2 * (2 * cfg->node_in + cfg->edge_attr_dim + 1));
    m->chunk = cfg->edge_chunk > 0 ? cfg->edge_chunk : PROTSSN_CHUNK_DEFAULT;
    rc = protssn_build(m, w, n_weights);
    if (rc) { pgmi_protssn_destroy(m); return rc; }
    *out = m;
    return PGMI_OK;
}

static int protssn_check_graph(const pgmi_protssn* m, const float* pos, int L, int E, const int32_t* centre, const int32_t* nb, const float* ea) {
    if (!m || !pos || !centre || !nb || !ea) { set_error("bad argument"); return PGMI_EINVAL; }
    if (L < 2 || L > PROTSSN_MAX_L) { set_error("ProtSSN: L = %d outside 2 .. %d", L, PROTSSN_MAX_L); return PGMI_EINVAL; }
    if (E < 1 || E > PROTSSN_MAX_E) { set_error("ProtSSN: %d edges (1 .. %d)", E, PROTSSN_MAX_E); return PGMI_EINVAL; }
    for (int i = 0; i < 3 * L; ++i)
        if (!std::isfinite(pos[i])) { set_error("ProtSSN: coordinate of residue %d is not finite", i / 3); return PGMI_EINVAL; }
    for (int e = 0; e < E; ++e) {
        if (centre[e] < 0 || centre[e] >= L || nb[e] < 0 || nb[e] >= L) {
            set_error("ProtSSN: edge %d = (%d, %d) outside 0 .. %d", e, (int)centre[e], (int)nb[e], L - 1);
            return PGMI_EINVAL;
        }
        if (centre[e] == nb[e]) { set_error("ProtSSN: edge %d is a self edge of residue %d", e, (int)nb[e]); return PGMI_EINVAL; }
    }
    for (size_t i = 0; i < (size_t)E * m->A; ++i)
        if (!std::isfinite(ea[i])) { set_error("ProtSSN: edge attribute %d of edge %zu is not finite", (int)(i % m->A), i / m->A); return PGMI_EINVAL; }
    return PGMI_OK;
}

static int protssn_set_graph(pgmi_protssn* m, const float* pos, int L, int E, const int32_t* centre, const int32_t* nb, const float* ea) {
    pgmi_model* pm = &m->pm;
    hipStream_t st = pm->stream;
    const int A = m->A, Ap = m->Ap;
    m->L = 0;
    std::vector<float> h_ea((size_t)E * Ap, 0.0f);
    std::vector<int32_t> off((size_t)L + 1, 0), eid(E);
    for (int e = 0; e < E; ++e) {
        memcpy(&h_ea[(size_t)e * Ap], ea + (size_t)e * A, (size_t)A * sizeof(float));
        // rel_dist of EGNN_Sparse.forward: ((coors[edge_index[0]] - coors[edge_index[1]]) ** 2).sum(-1) in fp32, x then y then z
        float d2 = 0.0f;
        for (int k = 0; k < 3; ++k) {
            const float d = pos[3 * centre[e] + k] - pos[3 * nb[e] + k];
            d2 = k ? d2 + d * d : d * d;
        }
        h_ea[(size_t)e * Ap + A] = d2;
        off[nb[e] + 1] += 1;
    }
    for (int i = 0; i < L; ++i) off[i + 1] += off[i];
    {
        std::vector<int32_t> next(off.begin(), off.end() - 1);
        for (int e = 0; e < E; ++e) eid[next[nb[e]]++] = e;            // ascending e per node: a stable sort by target
    }
    const int rc = reserve_all(pm, m->centre, E, m->nb, E, m->eid, E, m->off, (size_t)L + 1, m->ea, (size_t)E * Ap);
    if (rc) return rc;
    {
        ProfScope p(pm, PGMI_K_EMBED, 0, (double)E * (Ap + 3) * 4);
        PGMI_HIP(hipMemcpyAsync(m->centre, centre, (size_t)E * 4, hipMemcpyHostToDevice, st));
        PGMI_HIP(hipMemcpyAsync(m->nb, nb, (size_t)E * 4, hipMemcpyHostToDevice, st));
        PGMI_HIP(hipMemcpyAsync(m->eid, eid.data(), (size_t)E * 4, hipMemcpyHostToDevice, st));
        PGMI_HIP(hipMemcpyAsync(m->off, off.data(), ((size_t)L + 1) * 4, hipMemcpyHostToDevice, st));
        PGMI_HIP(hipMemcpyAsync(m->ea, h_ea.data(), h_ea.size() * 4, hipMemcpyHostToDevice, st));
    }
    PGMI_HIP(hipStreamSynchronize(st));                   // the host arrays are free to go after this
    m->L = L;
    m->E = E;
    return protssn_workspace(m);
}

static int protssn_finish(pgmi_protssn* m, const char* what) {
    const int rc = side_sync(&m->pm, PGMI_OK, what);
    return rc || !m->pm.prof ? rc : prof_drain(&m->pm);
}

}  // namespace pgmi

extern "C" {

int64_t pgmi_protssn_weight_count(const pgmi_protssn_config* cfg) {
    if (protssn_check(cfg)) return -1;
    return protssn_count(cfg);
}

int pgmi_protssn_create(const pgmi_protssn_config* cfg, const float* w, int64_t n_weights, int device, pgmi_protssn** out) {
    return protssn_new(cfg, w, n_weights, device, out);
}

void pgmi_protssn_destroy(pgmi_protssn* m) {
    if (!m) return;
    side_release(&m->pm, true);
    delete m;
}

pgmi_model* pgmi_protssn_profile_model(pgmi_protssn* m) { return m ? &m->pm : nullptr; }

int pgmi_protssn_set_graph(pgmi_protssn* m, const float* pos, int L, int n_edges, const int32_t* centre, const int32_t* neighbour,
                           const float* edge_attr) {
    int rc = protssn_check_graph(m, pos, L, n_edges, centre, neighbour, edge_attr);
    if (rc) return rc;
    PGMI_HIP(hipSetDevice(m->pm.device));
    return protssn_set_graph(m, pos, L, n_edges, centre, neighbour, edge_attr);
}

int pgmi_protssn_forward(pgmi_protssn* m, const float* esm_rep, float* lp, float* hidden) {
    if (!m || !esm_rep || !lp) { set_error("bad argument"); return PGMI_EINVAL; }
    if (m->L <= 0) { set_error("ProtSSN: no graph set (pgmi_protssn_set_graph)"); return PGMI_EINVAL; }
    const size_t n = (size_t)m->L * m->D;
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(esm_rep[i])) { set_error("ProtSSN: esm_rep element %zu is not finite", i); return PGMI_EINVAL; }
    PGMI_HIP(hipSetDevice(m->pm.device));
    hipStream_t st = m->pm.stream;
    PGMI_HIP(hipMemcpyAsync(m->x, esm_rep, n * 4, hipMemcpyHostToDevice, st));
    int rc = protssn_layers(m);
    if (rc) { hipStreamSynchronize(st); return rc; }
    PGMI_HIP(hipMemcpyAsync(lp, m->lp, (size_t)m->L * 20 * 4, hipMemcpyDeviceToHost, st));
    if (hidden) PGMI_HIP(hipMemcpyAsync(hidden, m->x, n * 4, hipMemcpyDeviceToHost, st));
    if ((rc = protssn_finish(m, "ProtSSN forward"))) return rc;
    for (size_t i = 0; i < (size_t)m->L * 20; ++i)
        if (!std::isfinite(lp[i])) return overflow_error(m->cfg.precision);
    return PGMI_OK;
}

int pgmi_esm_residue_rows(pgmi_model* esm, const int32_t* tokens, int T, float* rows) {
    if (!esm || !tokens || !rows) { set_error("bad argument"); return PGMI_EINVAL; }
    if (esm->cfg.arch != PGMI_ARCH_ESM2) { set_error("residue rows: the model must be an ESM2 model (arch %d)", esm->cfg.arch); return PGMI_EINVAL; }
    if (T < 3) { set_error("residue rows: T = %d tokens (<cls> + at least one residue + <eos>)", T); return PGMI_EINVAL; }
    if (T + 31 > esm->max_rows) { set_error("T=%d exceeds the ESM2 model's workspace rows %d", T, esm->max_rows); return PGMI_EINVAL; }
    int rc = check_tokens(tokens, 1, T, esm->n_token_ids);
    if (rc) return rc;
    PGMI_HIP(hipSetDevice(esm->device));
    hipStream_t st = esm->stream;
    const int D = esm->cfg.embed_dim, R = T - 2;
    PGMI_HIP(hipMemcpyAsync(esm->tokens, tokens, (size_t)T * 4, hipMemcpyHostToDevice, st));
    if ((rc = run_encoder(esm, 1, T))) return rc;
    {   // emb_layer_norm_after on the residue rows, fp32, as pgmi_s2f_set_logprobs takes them
        ProfScope p(esm, PGMI_K_LAYERNORM, 0, (double)R * D * 8);
        launch_layernorm(esm->x + D, esm->lna_w, esm->lna_b, R, D, 1e-5f, esm->h, st);
    }
    PGMI_HIP(hipGetLastError());
    PGMI_HIP(hipMemcpyAsync(rows, esm->h, (size_t)R * D * 4, hipMemcpyDeviceToHost, st));
    PGMI_HIP(hipStreamSynchronize(st));
    if (esm->prof && (rc = prof_drain(esm))) return rc;
    for (size_t i = 0; i < (size_t)R * D; ++i)
        if (!std::isfinite(rows[i])) { set_error("non-finite residue rows: an activation left the fp16 range; re-run with precision fp32"); return PGMI_EOVERFLOW; }
    return PGMI_OK;
}

int pgmi_op_egnn_message(int device, const pgmi_protssn_config* cfg, const float* weights, int64_t n_weights, const float* pos, int L,
                         int n_edges, const int32_t* centre, const int32_t* neighbour, const float* edge_attr, const float* x, float* out) {
    if (!x || !out) { set_error("bad argument"); return PGMI_EINVAL; }
    if (cfg && cfg->layers != 1) { set_error("egnn message op: a one-layer config and blob"); return PGMI_EINVAL; }
    pgmi_protssn* m = nullptr;
    int rc = protssn_new(cfg, weights, n_weights, device, &m);
    if (rc) return rc;
    rc = protssn_check_graph(m, pos, L, n_edges, centre, neighbour, edge_attr);
    if (!rc) rc = protssn_set_graph(m, pos, L, n_edges, centre, neighbour, edge_attr);
    const size_t D = m->D, K = m->D + m->hp;
    std::vector<uint32_t> A(rc ? 0 : (size_t)L * K);
    if (!rc) {
        hipStream_t st = m->pm.stream;
        hipError_t e = hipMemcpyAsync(m->x, x, (size_t)L * D * 4, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) rc = protssn_message(m, m->layers[0]);
        if (!rc && e == hipSuccess) e = hipMemcpyAsync(A.data(), m->nA, A.size() * 4, hipMemcpyDeviceToHost, st);
        if (!rc && e != hipSuccess) { set_error("egnn message op failed: %s", hipGetErrorString(e)); rc = PGMI_EHIP; }
        if (!rc) rc = protssn_finish(m, "ProtSSN message op");
    }
    if (!rc) {
        const bool split = cfg->precision != PGMI_PREC_FP32;
        const unsigned short* a16 = reinterpret_cast<const unsigned short*>(A.data());
        const float* a32 = reinterpret_cast<const float*>(A.data());
        for (int r = 0; r < L; ++r)
            for (int k = 0; k < m->h; ++k) {
                float v;
                if (split) {
                    const size_t o = ki_off((size_t)r, (int)D + k, (int)K);
                    v = rebuild_split(a16[o], a16[o + 32]);
                } else {
                    v = a32[(size_t)r * K + D + k];
                }
                out[(size_t)r * m->h + k] = v;
            }
    }
    pgmi_protssn_destroy(m);
    return rc;
}

}  // extern "C"
