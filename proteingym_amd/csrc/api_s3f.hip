// S3F entries of the C ABI (include/pgmi.h, S3F section).  The handle owns two GVP-GNN handles of api_s2f.hip: the
// residue half, which is S2F's, and the surface half, a handle with fixed_degree = 16 whose graph this file builds on the device
// (s3f.hip's k-NN and edge kernels) and whose input rows come from the folded surface MLP.  Per masked copy the surface half ends in a
// fixed-order column sum of surf_W_out's rows; the copies of a pool group (the reference's loader batch) then share the mean of their
// sums, added to the residue half's W_out rows before the head.  Chunks never cut a group's head step: the W_out rows, the ESM logits
// and the sums of a run of whole groups are held until its last copy is through.  Every kernel before the group step works on one
// copy's rows alone, so a copy's sum has the same bits alone, in a batch and under any row cap.
#include <cmath>

#include "s2f_impl.h"

namespace pgmi {
constexpr int S3F_FEAT = 42, S3F_RES = 3;
constexpr int S3F_KF = 64;                            // the structure term's operand row: 42 features | mean distance | 0 pad
constexpr int S3F_MAX_NS = 1 << 20;
}  // namespace pgmi

struct pgmi_s3f {
    pgmi_s2f* res = nullptr;
    pgmi_s2f* surf = nullptr;
    pgmi_s3f_config cfg;
    int D = 0, H = 0;
    // folded surface MLP (device, owned by surf's pool) and surf_W_e's tensors
    float *Wz = nullptr, *Wsf = nullptr, *b1 = nullptr, *lnw = nullptr, *lnb = nullptr, *W2 = nullptr, *b2 = nullptr, *we = nullptr;
    // structure
    int Ns = 0;
    pgmi::DevBuf<float> spos, cpos, rdist;
    pgmi::DevBuf<int32_t> rnb;                         // [Ns][3] nearest C-alpha atoms
    std::vector<int32_t> h_src, h_rnb;
    std::vector<float> h_rdist;
    pgmi::DevBuf<float> T, Asf;                           // T [Ns][H]: the structure term of the MLP's first Linear
    // workspace
    pgmi::DevBuf<float> Z, Hd, part, hold_pre, hold_seq, hold_lp, hold_sum;
    pgmi::DevBuf<int32_t> grp;
};

namespace pgmi {

static int s3f_check(const pgmi_s3f_config* c) {
    if (!c) { set_error("null config"); return PGMI_EINVAL; }
    int rc = s2f_check(&c->s2f);
    if (rc) return rc;
    if (c->s2f.node_in > 4096) { set_error("S3F: node_in %d above 4096", c->s2f.node_in); return PGMI_EINVAL; }
    if (c->surf_feat != S3F_FEAT || c->surf_res_neighbors != S3F_RES || c->surf_neighbors != S3F_DEG) {
        set_error("S3F: surf_feat %d, surf_res_neighbors %d, surf_neighbors %d; this path runs 42, 3, 16", c->surf_feat, c->surf_res_neighbors,
                  c->surf_neighbors);
        return PGMI_EINVAL;
    }
    return PGMI_OK;
}

static int64_t s3f_mlp_count(const pgmi_s3f_config* c) {
    const int64_t D = c->s2f.node_in, H = 2 * D;
    return H * D + H * (S3F_FEAT + 1) + H + 2 * H + D * H + D;
}
static int64_t s3f_count(const pgmi_s3f_config* c) { return s2f_count(&c->s2f, false) + s3f_mlp_count(c) + s2f_count(&c->s2f, true); }

static int s3f_ready(pgmi_s3f* m) {
    if (!m) { set_error("bad argument"); return PGMI_EINVAL; }
    if (m->Ns <= 0 || m->res->L <= 0) { set_error("S3F: no structure set (pgmi_s3f_set_structure)"); return PGMI_EINVAL; }
    return PGMI_OK;
}

static int s3f_structure(pgmi_s3f* m, const float* pos, int L, const float* surf_pos, const float* surf_feat, int Ns) {
    pgmi_s2f* sf = m->surf;
    pgmi_model* pm = &sf->pm;
    hipStream_t st = pm->stream;
    const size_t E = (size_t)Ns * S3F_DEG;
    const int H = m->H;
    int rc = reserve_all(pm, m->spos, (size_t)Ns * 3, m->cpos, (size_t)L * 3, m->rnb, (size_t)Ns * S3F_RES, m->rdist, (size_t)Ns * S3F_RES,
                         sf->src, E, sf->es, E * S2F_ES, sf->ev, E * 3, m->T, (size_t)Ns * H, m->Asf, (size_t)Ns * S3F_KF);
    if (rc) return rc;
    ProfScope prof(pm, PGMI_K_EMBED, 2.0 * E * S2F_S * S2F_ES * sf->layers.size() + 2.0 * Ns * H * S3F_KF, 0);
    PGMI_HIP(hipMemcpyAsync(m->spos, surf_pos, (size_t)Ns * 3 * 4, hipMemcpyHostToDevice, st));
    PGMI_HIP(hipMemcpyAsync(m->cpos, pos, (size_t)L * 3 * 4, hipMemcpyHostToDevice, st));
    rc = launch_s3f_knn(m->spos, Ns, m->spos, Ns, S3F_DEG, sf->src, nullptr, st);
    if (!rc) rc = launch_s3f_knn(m->spos, Ns, m->cpos, L, S3F_RES, m->rnb, m->rdist, st);
    if (rc) return rc;
    m->h_src.resize(E);
    m->h_rnb.resize((size_t)Ns * S3F_RES);
    m->h_rdist.resize((size_t)Ns * S3F_RES);
    PGMI_HIP(hipMemcpyAsync(m->h_src.data(), sf->src, E * 4, hipMemcpyDeviceToHost, st));
    PGMI_HIP(hipMemcpyAsync(m->h_rnb.data(), m->rnb, (size_t)Ns * S3F_RES * 4, hipMemcpyDeviceToHost, st));
    PGMI_HIP(hipMemcpyAsync(m->h_rdist.data(), m->rdist, (size_t)Ns * S3F_RES * 4, hipMemcpyDeviceToHost, st));
    launch_s3f_edges(m->spos, sf->src, Ns, m->we, sf->es.p, sf->ev.p, st);
    rc = s2f_edge_tables(sf, E);
    if (rc) return rc;
    PGMI_HIP(hipStreamSynchronize(st));
    // the structure term's operand rows: [features | mean of the three distances | 0]
    std::vector<float> a((size_t)Ns * S3F_KF, 0.0f);
    for (int p = 0; p < Ns; ++p) {
        memcpy(&a[(size_t)p * S3F_KF], surf_feat + (size_t)p * S3F_FEAT, S3F_FEAT * sizeof(float));
        const float* d = &m->h_rdist[(size_t)p * S3F_RES];
        a[(size_t)p * S3F_KF + S3F_FEAT] = (float)(((double)d[0] + (double)d[1] + (double)d[2]) / 3.0);
    }
    PGMI_HIP(hipMemcpyAsync(m->Asf.p, a.data(), a.size() * 4, hipMemcpyHostToDevice, st));
    rc = launch_gemm_f32(m->Asf.p, m->Wsf, m->b1, nullptr, m->T.p, Ns, H, S3F_KF, EPI_NONE, st);
    return side_sync(pm, rc, "S3F structure pass");
}

// copies per chunk: a masked copy costs max(E, 16 Ns, L + 2) rows
static int s3f_per_chunk(const pgmi_s3f* m, int n) {
    const long long cost = std::max<long long>(std::max(m->res->E, m->res->L + 2), (long long)m->Ns * S3F_DEG);
    return (int)std::min<long long>(std::max<long long>(1, s2f_row_cap() / cost), n);
}

static int s3f_check_pools(const int32_t* pool_off, int n_pools, int n, int* max_pool) {
    if (!pool_off || n_pools <= 0 || pool_off[0] != 0 || pool_off[n_pools] != n) { set_error("S3F: the pool groups must cover the %d copies", n); return PGMI_EINVAL; }
    *max_pool = 0;
    for (int g = 0; g < n_pools; ++g) {
        if (pool_off[g + 1] <= pool_off[g]) { set_error("S3F: pool group %d is empty", g); return PGMI_EINVAL; }
        *max_pool = std::max(*max_pool, pool_off[g + 1] - pool_off[g]);
    }
    return PGMI_OK;
}

static int s3f_workspace(pgmi_s3f* m, int per, int hold) {
    pgmi_s2f* sf = m->surf;
    const size_t L = m->res->L, Ns = m->Ns, H = m->H;
    int rc = s2f_workspace(m->res, per);
    if (!rc) rc = s2f_workspace(sf, per);
    if (!rc) rc = reserve_all(&sf->pm, m->Z, per * L * H, m->Hd, per * Ns * H, m->part, (size_t)per * s3f_colsum_blocks(m->Ns) * S2F_S,
                              m->hold_pre, hold * L * S2F_S, m->hold_seq, hold * L * 20, m->hold_lp, hold * L * 20, m->hold_sum, (size_t)hold * S2F_S,
                              m->grp, (size_t)hold * 2);
    return rc;
}

// bc masked copies whose ESM2 rows are in res->feat and whose ESM logits are in res->seq: both halves up to W_out; the residue rows,
// the logits and the per-copy sums go to slots h0 .. h0 + bc of the hold buffers
static int s3f_copies(pgmi_s3f* m, int bc, int h0) {
    pgmi_s2f *rs = m->res, *sf = m->surf;
    hipStream_t st = sf->pm.stream;
    const int L = rs->L, Ns = m->Ns, D = m->D, H = m->H;
    const int64_t R = (int64_t)bc * L, RS = (int64_t)bc * Ns;
    int rc = s2f_embed(rs, bc);
    if (!rc) rc = s2f_layers(rs, bc);
    if (rc) return rc;
    PGMI_HIP(hipMemcpyAsync(m->hold_pre.p + (size_t)h0 * L * S2F_S, rs->pre.p, (size_t)R * S2F_S * 4, hipMemcpyDeviceToDevice, st));
    PGMI_HIP(hipMemcpyAsync(m->hold_seq.p + (size_t)h0 * L * 20, rs->seq.p, (size_t)R * 20 * 4, hipMemcpyDeviceToDevice, st));
    {
        ProfScope p(&sf->pm, PGMI_K_GEMM_OUT, 2.0 * R * H * D + 2.0 * RS * D * (H + S2F_S), (double)RS * H * 8);
        rc = launch_gemm_f32(rs->feat.p, m->Wz, nullptr, nullptr, m->Z.p, (int)R, H, D, EPI_NONE, st);
        if (!rc) rc = launch_s3f_rows(m->Z.p, m->T.p, m->rnb, m->lnw, m->lnb, L, Ns, H, RS, m->Hd.p, st);
        if (!rc) rc = launch_gemm_f32(m->Hd.p, m->W2, m->b2, nullptr, sf->h0.p, (int)RS, D, H, EPI_NONE, st);
        if (rc) return rc;
        launch_layernorm(sf->h0.p, sf->vnw, sf->vnb, (int)RS, D, 1e-5f, sf->h0.p, st);
        rc = launch_gemm_f32(sf->h0.p, sf->Wv, sf->bv, nullptr, sf->s.p, (int)RS, S2F_S, D, EPI_NONE, st);
        if (rc) return rc;
    }
    rc = s2f_layers(sf, bc);
    if (rc) return rc;
    {
        ProfScope p(&sf->pm, PGMI_K_HEAD, 0, (double)RS * S2F_S * 4);
        launch_s3f_colsum(sf->pre.p, Ns, bc, m->part.p, m->hold_sum.p + (size_t)h0 * S2F_S, st);
    }
    PGMI_HIP(hipGetLastError());
    return PGMI_OK;
}

// the group step on the n held copies [a, a + n) = pool groups [g0, g1): the head on relu(W_out) + the pooled row -> hold_lp
static int s3f_finish(pgmi_s3f* m, const int32_t* pool_off, int g0, int g1, std::vector<int32_t>& grp) {
    pgmi_s2f* rs = m->res;
    const int a = pool_off[g0], n = pool_off[g1] - a;
    grp.resize((size_t)n * 2);
    for (int g = g0; g < g1; ++g)
        for (int s = pool_off[g]; s < pool_off[g + 1]; ++s) { grp[(size_t)(s - a) * 2] = pool_off[g] - a; grp[(size_t)(s - a) * 2 + 1] = pool_off[g + 1] - a; }
    PGMI_HIP(hipMemcpyAsync(m->grp, grp.data(), grp.size() * 4, hipMemcpyHostToDevice, rs->pm.stream));
    return s2f_head(rs, m->hold_pre.p, m->hold_seq.p, m->hold_sum.p, m->grp, m->Ns, (int64_t)n * rs->L, m->hold_lp.p);
}

// runs of whole pool groups, each within `hold` copies; fill(s0, bc) puts copies [s0, s0 + bc) into res->feat / res->seq, chunk(s0, bc)
// runs after their GNNs, done(a, n) after the group step of copies [a, a + n)
template <typename Fill, typename Chunk, typename Done>
static int s3f_run(pgmi_s3f* m, const int32_t* pool_off, int n_pools, int per, int hold, Fill fill, Chunk chunk, Done done) {
    std::vector<int32_t> grp;
    int rc = PGMI_OK;
    for (int g0 = 0; g0 < n_pools && !rc;) {
        const int a = pool_off[g0];
        int g1 = g0 + 1;
        while (g1 < n_pools && pool_off[g1 + 1] - a <= hold) ++g1;
        const int b = pool_off[g1];
        for (int s0 = a; s0 < b && !rc; s0 += per) {
            const int bc = std::min(per, b - s0);
            rc = fill(s0, bc);
            if (!rc) rc = s3f_copies(m, bc, s0 - a);
            if (!rc) rc = chunk(s0, bc);
        }
        if (!rc) rc = s3f_finish(m, pool_off, g0, g1, grp);
        if (!rc) rc = done(a, b - a);                           // synchronises: grp is free after it
        g0 = g1;
    }
    return rc;
}

static int s3f_drain(pgmi_s3f* m) {
    int rc = m->res->pm.prof ? prof_drain(&m->res->pm) : PGMI_OK;
    if (!rc && m->surf->pm.prof) rc = prof_drain(&m->surf->pm);
    if (!rc && m->res->esm && m->res->esm->prof) rc = prof_drain(m->res->esm);
    return rc;
}

}  // namespace pgmi

using namespace pgmi;

extern "C" {

int64_t pgmi_s3f_weight_count(const pgmi_s3f_config* cfg) {
    if (s3f_check(cfg)) return -1;
    return s3f_count(cfg);
}

int pgmi_s3f_create(const pgmi_s3f_config* cfg, const float* w, int64_t n_weights, pgmi_model* esm, int device, pgmi_s3f** out) {
    if (!out) { set_error("null out"); return PGMI_EINVAL; }
    *out = nullptr;
    int rc = s3f_check(cfg);
    if (rc) return rc;
    if (!w || n_weights != s3f_count(cfg)) {
        set_error("S3F weight blob has %lld elements, config needs %lld", (long long)n_weights, (long long)s3f_count(cfg));
        return PGMI_EINVAL;
    }
    pgmi_s3f* m = new pgmi_s3f();
    m->cfg = *cfg;
    m->D = cfg->s2f.node_in;
    m->H = 2 * m->D;
    const int64_t n_res = s2f_count(&cfg->s2f, false), n_mlp = s3f_mlp_count(cfg);
    rc = s2f_new(&cfg->s2f, w, n_res, esm, nullptr, device, 0, &m->res);
    if (!rc) rc = s2f_new(&cfg->s2f, w + n_res + n_mlp, n_weights - n_res - n_mlp, nullptr, m->res, m->res->pm.device, S3F_DEG, &m->surf);
    if (!rc) {
        std::vector<void*>& pool = m->surf->pm.allocs;
        const size_t D = m->D, H = m->H;
        const float* p = w + n_res;
        auto up = [&](float** dst, size_t n) { if (!rc) rc = dev_upload(pool, dst, p, n); p += n; };
        up(&m->Wz, H * D);
        {   // [H][43] -> [H][64], zero padded along K
            std::vector<float> t(H * S3F_KF, 0.0f);
            for (size_t n = 0; n < H; ++n) memcpy(&t[n * S3F_KF], p + n * (S3F_FEAT + 1), (S3F_FEAT + 1) * sizeof(float));
            if (!rc) rc = dev_upload(pool, &m->Wsf, t.data(), t.size());
            p += H * (S3F_FEAT + 1);
        }
        up(&m->b1, H);
        up(&m->lnw, H);
        up(&m->lnb, H);
        up(&m->W2, D * H);
        up(&m->b2, D);
        if (!rc) rc = dev_upload(pool, &m->we, m->surf->we_host.data(), m->surf->we_host.size());
    }
    if (rc) { pgmi_s3f_destroy(m); return rc; }
    *out = m;
    return PGMI_OK;
}

void pgmi_s3f_destroy(pgmi_s3f* m) {
    if (!m) return;
    if (m->surf) pgmi_s2f_destroy(m->surf);              // borrows the residue half's stream: first
    if (m->res) pgmi_s2f_destroy(m->res);
    delete m;
}

pgmi_model* pgmi_s3f_profile_model(pgmi_s3f* m, int part) {
    if (!m) return nullptr;
    return part == 0 ? &m->res->pm : part == 1 ? &m->surf->pm : nullptr;
}

int pgmi_s3f_set_structure(pgmi_s3f* m, const float* pos, const float* plddt, int L, const float* surf_pos, const float* surf_feat, int Ns) {
    if (!m || !pos || !plddt || !surf_pos || !surf_feat) { set_error("bad argument"); return PGMI_EINVAL; }
    m->Ns = 0;
    m->surf->L = m->surf->E = 0;
    if (L < S3F_RES) { set_error("S3F: L = %d, a surface point needs %d C-alpha atoms", L, S3F_RES); return PGMI_EINVAL; }
    if (Ns < S3F_DEG + 1 || Ns > S3F_MAX_NS) {
        set_error("S3F: %d surface points outside %d .. %d (a point needs %d other points)", Ns, S3F_DEG + 1, S3F_MAX_NS, S3F_DEG);
        return PGMI_EINVAL;
    }
    for (size_t i = 0; i < (size_t)Ns * 3; ++i)
        if (!std::isfinite(surf_pos[i])) { set_error("S3F: coordinate of surface point %d is not finite", (int)(i / 3)); return PGMI_EINVAL; }
    for (size_t i = 0; i < (size_t)Ns * S3F_FEAT; ++i)
        if (!std::isfinite(surf_feat[i])) { set_error("S3F: feature of surface point %d is not finite", (int)(i / S3F_FEAT)); return PGMI_EINVAL; }
    int rc = pgmi_s2f_set_structure(m->res, pos, plddt, L);
    if (rc) return rc;
    rc = s3f_structure(m, pos, L, surf_pos, surf_feat, Ns);
    if (rc) return rc;
    if (m->surf->pm.prof) rc = prof_drain(&m->surf->pm);
    m->surf->L = Ns;
    m->surf->E = Ns * S3F_DEG;
    m->Ns = Ns;
    return rc;
}

int pgmi_s3f_graph(pgmi_s3f* m, int32_t* n_edges, int32_t* src, int32_t* dst, float* e_s, float* e_v, int32_t* surf_src, int32_t* surf_res,
                   float* surf_res_dist, float* surf_e_s, float* surf_e_v) {
    int rc = s3f_ready(m);
    if (rc) return rc;
    rc = pgmi_s2f_graph(m->res, n_edges, src, dst, e_s, e_v);
    if (rc) return rc;
    const size_t E = (size_t)m->Ns * S3F_DEG;
    if (surf_src) memcpy(surf_src, m->h_src.data(), E * 4);
    if (surf_res) memcpy(surf_res, m->h_rnb.data(), m->h_rnb.size() * 4);
    if (surf_res_dist) memcpy(surf_res_dist, m->h_rdist.data(), m->h_rdist.size() * 4);
    PGMI_HIP(hipSetDevice(m->surf->pm.device));
    if (surf_e_s) PGMI_HIP(hipMemcpy(surf_e_s, m->surf->es.p, E * S2F_ES * 4, hipMemcpyDeviceToHost));
    if (surf_e_v) PGMI_HIP(hipMemcpy(surf_e_v, m->surf->ev.p, E * 3 * 4, hipMemcpyDeviceToHost));
    return PGMI_OK;
}

int pgmi_s3f_gvp_forward(pgmi_s3f* m, const float* node_feat, const float* seq_logits, int B, const int32_t* pool_off, int n_pools, float* lp,
                         float* surf_s, float* surf_v, float* pool_sum) {
    int rc = s3f_ready(m);
    if (rc) return rc;
    if (!node_feat || !seq_logits || !lp || B <= 0) { set_error("bad argument"); return PGMI_EINVAL; }
    int max_pool = 0;
    rc = s3f_check_pools(pool_off, n_pools, B, &max_pool);
    if (rc) return rc;
    pgmi_s2f *rs = m->res, *sf = m->surf;
    PGMI_HIP(hipSetDevice(rs->pm.device));
    hipStream_t st = rs->pm.stream;
    const int L = rs->L, Ns = m->Ns, per = s3f_per_chunk(m, B), hold = std::max(per, max_pool);
    rc = s3f_workspace(m, per, hold);
    if (rc) return rc;
    auto fill = [&](int s0, int bc) { return s2f_fill_rows(rs, node_feat, seq_logits, s0, bc); };
    auto chunk = [&](int s0, int bc) {
        const size_t RS = (size_t)bc * Ns, r0 = (size_t)s0 * Ns;
        if (surf_s) PGMI_HIP(hipMemcpyAsync(surf_s + r0 * S2F_S, sf->s.p, RS * S2F_S * 4, hipMemcpyDeviceToHost, st));
        if (surf_v) PGMI_HIP(hipMemcpyAsync(surf_v + r0 * S2F_V * 3, sf->v.p, RS * S2F_V * 3 * 4, hipMemcpyDeviceToHost, st));
        PGMI_HIP(hipStreamSynchronize(st));
        return s3f_drain(m);
    };
    auto done = [&](int a, int n) {
        PGMI_HIP(hipMemcpyAsync(lp + (size_t)a * L * 20, m->hold_lp.p, (size_t)n * L * 20 * 4, hipMemcpyDeviceToHost, st));
        if (pool_sum) PGMI_HIP(hipMemcpyAsync(pool_sum + (size_t)a * S2F_S, m->hold_sum.p, (size_t)n * S2F_S * 4, hipMemcpyDeviceToHost, st));
        PGMI_HIP(hipStreamSynchronize(st));
        return s3f_drain(m);
    };
    rc = s3f_run(m, pool_off, n_pools, per, hold, fill, chunk, done);
    return side_sync(&rs->pm, rc, "S3F forward");
}

int pgmi_s3f_set_logprobs(pgmi_s3f* m, const int32_t* wt_tokens, int T, const int32_t* aa_cols, const int32_t* set_off,
                          const int32_t* set_pos, int n_sets, const int32_t* pool_off, int n_pools, float* out, float* full) {
    int rc = s3f_ready(m);
    if (rc) return rc;
    pgmi_s2f* rs = m->res;
    pgmi_model* esm = rs->esm;
    rc = s2f_check_sets(rs, "S3F", wt_tokens, T, aa_cols, set_off, set_pos, n_sets, out);
    if (rc) return rc;
    int max_pool = 0;
    rc = s3f_check_pools(pool_off, n_pools, n_sets, &max_pool);
    if (rc) return rc;
    PGMI_HIP(hipSetDevice(rs->pm.device));
    pgmi_model* pm = &rs->pm;
    hipStream_t st = pm->stream;
    const int L = rs->L, per = std::min(s3f_per_chunk(m, n_sets), rows_per_chunk(esm, T)), hold = std::max(per, max_pool);
    S2fSetHost host;
    rc = s3f_workspace(m, per, hold);
    if (!rc) rc = s2f_set_buffers(rs, per, T, aa_cols, &host);
    if (rc) return rc;
    std::vector<float> lp((size_t)hold * L * 20);
    auto fill = [&](int s0, int bc) { return s2f_fill_esm(rs, wt_tokens, T, set_off, set_pos, s0, bc, &host); };
    auto chunk = [&](int, int) {
        PGMI_HIP(hipStreamSynchronize(st));                    // the host scratch is free for the next chunk
        return s3f_drain(m);
    };
    auto done = [&](int a, int n) {
        PGMI_HIP(hipMemcpyAsync(lp.data(), m->hold_lp.p, (size_t)n * L * 20 * 4, hipMemcpyDeviceToHost, st));
        PGMI_HIP(hipStreamSynchronize(st));
        s2f_scatter(lp.data(), L, set_off, set_pos, a, n, out, full);
        return s3f_drain(m);
    };
    rc = s3f_run(m, pool_off, n_pools, per, hold, fill, chunk, done);
    rc = side_sync(pm, rc, "S3F scoring");
    return rc ? rc : check_nonfinite(esm);
}

}  // extern "C"
