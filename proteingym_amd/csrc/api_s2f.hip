// S2F entries of the C ABI (include/pgmi.h, S2F section): the blob walk, the per-structure pass (radius graph and W_e on
// the host in double, every layer's edge share of the first message GVP on the device) and the per-chunk GVP-GNN over the residue
// rows of the masked copies.  The kernels are in s2f.hip.  Dense Linears are launch_gemm_f32: a GEMM output element is a two-level sum
// whose order does not depend on the row count, the message kernel works on one node of one copy per block and sums its edges in
// ascending order, and every other kernel is one wave per row, so a masked copy's bits do not depend on the batch or the chunking.
#include <cctype>
#include <cmath>

#include "s2f_impl.h"

namespace pgmi {

static long long g_s2f_max_rows = 0;
long long s2f_row_cap() { return g_s2f_max_rows > 0 ? g_s2f_max_rows : 262144; }

int s2f_set_option(const char* name, long long value) {
    if (!strcmp(name, "s2f_max_rows")) { g_s2f_max_rows = std::min(std::max(value, 0LL), S2F_ROWS_LIMIT); return PGMI_OK; }
    return PGMI_EINVAL;
}

int s2f_check(const pgmi_s2f_config* c) {
    if (!c) { set_error("null config"); return PGMI_EINVAL; }
    if (c->abi_version != PGMI_ABI_VERSION) { set_error("ABI version mismatch: got %d, library is %d", c->abi_version, PGMI_ABI_VERSION); return PGMI_EINVAL; }
    if (c->node_in < 32 || c->node_in % 32 || c->node_in > 8192) { set_error("S2F: node_in %d must be a multiple of 32 in 32 .. 8192", c->node_in); return PGMI_EINVAL; }
    if (c->node_s != S2F_S || c->node_v != S2F_V || c->edge_s != S2F_ES || c->edge_v != 1 || c->rbf != S2F_RBF) {
        set_error("S2F: dimensions node (%d, %d) edge (%d, %d) rbf %d; this path runs node (256, 16), edge (64, 1), 16 RBFs", c->node_s,
                  c->node_v, c->edge_s, c->edge_v, c->rbf);
        return PGMI_EINVAL;
    }
    if (c->layers < 1 || c->layers > S2F_MAX_LAYERS) { set_error("S2F: 1 .. %d layers, got %d", S2F_MAX_LAYERS, c->layers); return PGMI_EINVAL; }
    if (c->max_neighbors < 1 || c->max_neighbors > 64) { set_error("S2F: max_neighbors %d outside 1 .. 64", c->max_neighbors); return PGMI_EINVAL; }
    if (!(c->radius > 0.0f) || !std::isfinite(c->radius)) { set_error("S2F: radius must be positive and finite"); return PGMI_EINVAL; }
    if (!std::isfinite(c->plddt_threshold)) { set_error("S2F: plddt_threshold is not finite"); return PGMI_EINVAL; }
    return PGMI_OK;
}

static int64_t gvp_count(int si, int vi, int so, int vo, int h) {   // wh, ws + b, wv, wsv + b
    return (int64_t)h * vi + (int64_t)so * (si + h) + so + (vo ? (int64_t)vo * h + (int64_t)vo * so + vo : 0);
}
static int64_t s2f_we_count() { return 2 * S2F_RBF + gvp_count(S2F_RBF, 1, S2F_ES, 1, 1); }
int64_t s2f_count(const pgmi_s2f_config* c, bool surface) {
    const int64_t D = c->node_in;
    int64_t n = (surface ? 0 : D * D) + 2 * D + (int64_t)S2F_S * D + S2F_S + s2f_we_count();
    const int64_t layer = gvp_count(2 * S2F_S + S2F_ES, S2F_H0, S2F_S, S2F_V, S2F_H0) + 2 * gvp_count(S2F_S, S2F_V, S2F_S, S2F_V, S2F_V) +
                          4 * S2F_S + gvp_count(S2F_S, S2F_V, S2F_FS, S2F_FV, S2F_FV) + gvp_count(S2F_FS, S2F_FV, S2F_S, S2F_V, S2F_FV);
    n += c->layers * layer;
    n += 2 * S2F_S + gvp_count(S2F_S, S2F_V, S2F_S, 0, S2F_V) + (surface ? 0 : 20 * S2F_S + 20);
    return n;
}

static int s2f_build(pgmi_s2f* m, const float* w, int64_t n_weights) {
    BlobCursor c(&m->pm, w, n_weights);
    auto gvp = [&](S2fGvp* g, int si, int vi, int so, int vo, int h, bool with_ws) {
        g->si = si, g->vi = vi, g->so = so, g->vo = vo, g->h = h, g->Kp = roundup32(si + h);
        c.upload(&g->wh, (size_t)h * vi);
        const float* ws = c.take((size_t)so * (si + h));
        if (with_ws) {
            std::vector<float> t((size_t)so * g->Kp, 0.0f);
            for (int n = 0; n < so; ++n) memcpy(&t[(size_t)n * g->Kp], ws + (size_t)n * (si + h), (size_t)(si + h) * sizeof(float));
            c.upload(&g->ws, t);
        }
        c.upload(&g->bs, so);
        if (vo) {
            c.upload(&g->wv, (size_t)vo * h);
            c.upload(&g->wsv, (size_t)vo * so);
            c.upload(&g->bsv, vo);
        }
        return ws;
    };
    const size_t D = m->D;
    if (!m->fixed_degree) c.upload(&m->Wre, D * D);
    c.upload(&m->vnw, D);
    c.upload(&m->vnb, D);
    c.upload(&m->Wv, S2F_S * D);
    c.upload(&m->bv, S2F_S);
    {
        const float* we = c.take((size_t)s2f_we_count());
        m->we_host.assign(we, we + s2f_we_count());
    }
    m->layers.resize(m->cfg.layers);
    for (S2fLayer& l : m->layers) {
        const int K0 = 2 * S2F_S + S2F_ES + S2F_H0;          // 609 columns: s_j | e_s | s_i | norms
        const float* wh = c.p;                                // [33][33]: v_j | e_v | v_i columns
        const float* ws = gvp(&l.m0, 2 * S2F_S + S2F_ES, S2F_H0, S2F_S, S2F_V, S2F_H0, false);
        l.b0 = l.m0.bs;
        std::vector<float> wji((size_t)2 * S2F_S * S2F_S), we((size_t)S2F_S * S2F_ES), wnt((size_t)S2F_H0 * S2F_S),
            whji((size_t)2 * S2F_H0 * S2F_V), whe(S2F_H0);
        for (int n = 0; n < S2F_S; ++n) {
            const float* row = ws + (size_t)n * K0;
            memcpy(&wji[(size_t)n * S2F_S], row, S2F_S * sizeof(float));
            memcpy(&we[(size_t)n * S2F_ES], row + S2F_S, S2F_ES * sizeof(float));
            memcpy(&wji[(size_t)(S2F_S + n) * S2F_S], row + S2F_S + S2F_ES, S2F_S * sizeof(float));
            for (int h = 0; h < S2F_H0; ++h) wnt[(size_t)h * S2F_S + n] = row[2 * S2F_S + S2F_ES + h];
        }
        for (int h = 0; h < S2F_H0; ++h) {
            memcpy(&whji[(size_t)h * S2F_V], wh + (size_t)h * S2F_H0, S2F_V * sizeof(float));
            whe[h] = wh[(size_t)h * S2F_H0 + S2F_V];
            memcpy(&whji[(size_t)(S2F_H0 + h) * S2F_V], wh + (size_t)h * S2F_H0 + S2F_V + 1, S2F_V * sizeof(float));
        }
        c.upload(&l.Wji, wji);
        c.upload(&l.We, we);
        c.upload(&l.Wnt, wnt);
        c.upload(&l.whji, whji);
        c.upload(&l.whe, whe);
        gvp(&l.m1, S2F_S, S2F_V, S2F_S, S2F_V, S2F_V, true);
        gvp(&l.m2, S2F_S, S2F_V, S2F_S, S2F_V, S2F_V, true);
        c.upload(&l.n0w, S2F_S); c.upload(&l.n0b, S2F_S);
        c.upload(&l.n1w, S2F_S); c.upload(&l.n1b, S2F_S);
        gvp(&l.f0, S2F_S, S2F_V, S2F_FS, S2F_FV, S2F_FV, true);
        gvp(&l.f1, S2F_FS, S2F_FV, S2F_S, S2F_V, S2F_FV, true);
    }
    c.upload(&m->onw, S2F_S);
    c.upload(&m->onb, S2F_S);
    gvp(&m->wout, S2F_S, S2F_V, S2F_S, 0, S2F_V, true);
    if (!m->fixed_degree) {
        c.upload(&m->Wlin, 20 * S2F_S);
        c.upload(&m->blin, 20);
    }
    return c.finish();
}

// radius_graph(pos, r, max_num_neighbors) without self loops, as torch_cluster's CUDA kernel keeps it: per centre i the candidates j in
// ascending index with squared distance < r^2, self included, the first max_neighbors + 1 kept, then the self edge dropped.  Edges
// (j -> i) sorted by (i, j); off [L + 1] is the CSR over centres.  Distances in double from the fp32 coordinates.
static void s2f_radius_graph(const float* pos, int L, double radius, int max_nb, std::vector<int32_t>& src, std::vector<int32_t>& dst,
                             std::vector<int32_t>& off) {
    src.clear(); dst.clear(); off.assign(1, 0);
    const double r2 = radius * radius;
    for (int i = 0; i < L; ++i) {
        int kept = 0;
        for (int j = 0; j < L && kept < max_nb + 1; ++j) {
            const double dx = (double)pos[3 * i] - pos[3 * j], dy = (double)pos[3 * i + 1] - pos[3 * j + 1], dz = (double)pos[3 * i + 2] - pos[3 * j + 2];
            if (dx * dx + dy * dy + dz * dz < r2) {
                ++kept;
                if (j != i) { src.push_back(j); dst.push_back(i); }
            }
        }
        off.push_back((int32_t)src.size());
    }
}

// W_e on the host in double: rbf -> tuple LayerNorm (16, 1) -> GVP (16, 1) -> (64, 1), vector gate, no activation.  vec = pos_i - pos_j.
static void s2f_edge_embed(const pgmi_s2f* m, const float* pos, std::vector<float>& es, std::vector<float>& ev) {
    const float* w = m->we_host.data();
    const float *lnw = w, *lnb = w + 16, *wh = w + 32, *ws = w + 33, *bs = ws + 64 * 17, *wv = bs + 64, *wsv = wv + 1, *bsv = wsv + 64;
    const int E = m->E;
    es.assign((size_t)E * S2F_ES, 0.0f);
    ev.assign((size_t)E * 3, 0.0f);
    for (int e = 0; e < E; ++e) {
        const int i = m->h_dst[e], j = m->h_src[e];
        double vec[3], d2 = 0.0;
        for (int c = 0; c < 3; ++c) { vec[c] = (double)pos[3 * i + c] - (double)pos[3 * j + c]; d2 += vec[c] * vec[c]; }
        const double d = std::sqrt(d2);
        double f[17], mean = 0.0, var = 0.0;
        // the centres are torch.linspace(0, 20, 16) in float32, as the reference builds them: start + step k below the middle,
        // end - step (15 - k) above it
        const float step = 20.0f / 15.0f;
        for (int k = 0; k < 16; ++k) {
            const float mu = k < 8 ? step * (float)k : 20.0f - step * (float)(15 - k);
            const double z = (d - (double)mu) / 1.25;
            f[k] = std::exp(-z * z);
            mean += f[k];
        }
        mean /= 16.0;
        for (int k = 0; k < 16; ++k) var += (f[k] - mean) * (f[k] - mean);
        const double rstd = 1.0 / std::sqrt(var / 16.0 + 1e-5);
        for (int k = 0; k < 16; ++k) f[k] = (f[k] - mean) * rstd * lnw[k] + lnb[k];
        const double vden = std::sqrt(std::max(d2, 1e-8));            // one channel: the mean over channels is the channel
        double vh[3], n2 = 0.0;
        for (int c = 0; c < 3; ++c) { vh[c] = (double)wh[0] * (vec[c] / vden); n2 += vh[c] * vh[c]; }
        f[16] = std::sqrt(std::max(n2, 1e-8));
        double gate = bsv[0];
        for (int n = 0; n < S2F_ES; ++n) {
            double a = bs[n];
            for (int k = 0; k < 17; ++k) a += (double)ws[n * 17 + k] * f[k];
            es[(size_t)e * S2F_ES + n] = (float)a;
            gate += (double)wsv[n] * a;
        }
        const double sg = 1.0 / (1.0 + std::exp(-gate));
        for (int c = 0; c < 3; ++c) ev[(size_t)e * 3 + c] = (float)((double)wv[0] * vh[c] * sg);
    }
}

// every layer's edge share of the first message GVP from the E > 0 rows of m->es: Es = We e_s + b [E][256]
int s2f_edge_tables(pgmi_s2f* m, size_t E) {
    int rc = PGMI_OK;
    for (S2fLayer& l : m->layers) {
        if (!rc) rc = l.Es.reserve(&m->pm, E * S2F_S);
        if (!rc) rc = launch_gemm_f32(m->es.p, l.We, l.b0, nullptr, l.Es, (int)E, S2F_S, S2F_ES, EPI_NONE, m->pm.stream);
    }
    return rc;
}

int s2f_structure(pgmi_s2f* m, const float* pos, const float* plddt, int L) {
    pgmi_model* pm = &m->pm;
    hipStream_t st = pm->stream;
    m->L = 0;
    s2f_radius_graph(pos, L, (double)m->cfg.radius, m->cfg.max_neighbors, m->h_src, m->h_dst, m->h_off);
    const int E = m->E = (int)m->h_src.size();
    s2f_edge_embed(m, pos, m->h_es, m->h_ev);
    const size_t En = std::max(E, 1);
    int rc = reserve_all(pm, m->src, En, m->off, (size_t)L + 1, m->es, En * S2F_ES, m->ev, En * 3, m->plddt, (size_t)L);
    if (rc) return rc;
    auto upload = [&](void* dst, const void* src, size_t bytes) {
        if (rc || !bytes || hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st) == hipSuccess) return;
        set_error("S2F: structure upload failed");
        rc = PGMI_EHIP;
    };
    upload(m->src, m->h_src.data(), (size_t)E * 4);
    upload(m->off, m->h_off.data(), ((size_t)L + 1) * 4);
    upload(m->es.p, m->h_es.data(), (size_t)E * S2F_ES * 4);
    upload(m->ev.p, m->h_ev.data(), (size_t)E * 3 * 4);
    upload(m->plddt.p, plddt, (size_t)L * 4);
    if (!rc && E > 0) {
        ProfScope prof(pm, PGMI_K_EMBED, 2.0 * E * S2F_S * S2F_ES * m->layers.size(), 0);
        rc = s2f_edge_tables(m, (size_t)E);
    }
    rc = side_sync(pm, rc, "S2F structure pass");         // the caller's arrays are free to go after this
    if (!rc) m->L = L;
    return rc;
}

// rows a masked copy costs in the widest stage, and copies per chunk
static int s2f_per_chunk(const pgmi_s2f* m, int B) {
    const long long cap = s2f_row_cap();
    const long long cost = std::max(m->E, m->L + 2);
    return (int)std::min<long long>(std::max<long long>(1, cap / cost), B);
}

int s2f_workspace(pgmi_s2f* m, int per) {
    const size_t R = (size_t)per * m->L, D = m->D;
    const bool surface = m->fixed_degree != 0;           // a surface half takes its rows from the surface MLP and has no head
    pgmi_model* pm = &m->pm;
    int rc = reserve_all(pm, m->h0, R * D, m->s, R * S2F_S, m->v, R * S2F_V * 3, m->s1, R * S2F_S, m->v1, R * S2F_V * 3, m->P, R * 2 * S2F_S,
                         m->VT, R * 2 * S2F_H0 * 3, m->pre, R * S2F_FS, m->gate, R * S2F_FV, m->A, R * S2F_FK, m->vhA, R * S2F_FV * 3,
                         m->vhB, R * S2F_FV * 3, m->mV, R * S2F_V * 3);
    if (!rc && !surface) rc = reserve_all(pm, m->feat, R * D, m->seq, R * 20, m->lp, R * 20);
    return rc;
}

// one GVP after the first of a chain: ws GEMM on its operand rows in m->A (timed as cls_gemm), then its gate GEMM (wsv on the ws output,
// vo columns: one column tile) and its vector half (cls_mid); `next` (nullable) is the GVP that follows
static int s2f_gvp(pgmi_s2f* m, const S2fGvp& g, const float* vh_in, int relu, const S2fGvp* next, int64_t rows, float* outV, int cls_gemm,
                   int cls_mid) {
    hipStream_t st = m->pm.stream;
    int rc;
    {
        ProfScope p(&m->pm, cls_gemm, 2.0 * rows * g.so * g.Kp, 0);
        rc = launch_gemm_f32(m->A.p, g.ws, g.bs, nullptr, m->pre.p, (int)rows, g.so, g.Kp, EPI_NONE, st);
    }
    if (rc) return rc;
    ProfScope p(&m->pm, cls_mid, 2.0 * rows * g.vo * (g.so + 3.0 * g.h), (double)rows * (g.so + (next ? next->Kp : 0)) * 4);
    rc = launch_gemm_f32(m->pre.p, g.wsv, g.bsv, nullptr, m->gate.p, (int)rows, g.vo, g.so, EPI_NONE, st);      // the gate, before the activation
    if (rc) return rc;
    return launch_s2f_gvp_mid(m->pre.p, vh_in, g.wv, m->gate.p, next ? next->wh : nullptr, g.so, g.vo, g.h, next ? next->h : 0, relu,
                              next ? next->Kp : 0, rows, next ? m->A.p : nullptr, outV, st);
}

// bc masked copies: m->feat [bc L][D] (device) -> m->s [bc L][256] = W_v (LayerNorm (residue_embdding feat))
int s2f_embed(pgmi_s2f* m, int bc) {
    pgmi_model* pm = &m->pm;
    hipStream_t st = pm->stream;
    const int D = m->D;
    const int64_t R = (int64_t)bc * m->L;
    ProfScope p(pm, PGMI_K_GEMM_QKV, 2.0 * R * D * (D + S2F_S), 0);
    int rc = launch_gemm_f32(m->feat.p, m->Wre, nullptr, nullptr, m->h0.p, (int)R, D, D, EPI_NONE, st);
    if (rc) return rc;
    launch_layernorm(m->h0.p, m->vnw, m->vnb, (int)R, D, 1e-5f, m->h0.p, st);
    return launch_gemm_f32(m->h0.p, m->Wv, m->bv, nullptr, m->s.p, (int)R, S2F_S, D, EPI_NONE, st);
}

// the layers on m->s (v = 0 before the first), then W_out -> m->pre [bc L][256]; the node state after the last layer stays in m->s / m->v
int s2f_layers(pgmi_s2f* m, int bc) {
    pgmi_model* pm = &m->pm;
    hipStream_t st = pm->stream;
    const int L = m->L, E = m->E;
    const int64_t R = (int64_t)bc * L, RE = (int64_t)bc * E;
    int rc;
    const size_t nl = m->layers.size();
    for (size_t li = 0; li < nl; ++li) {
        const S2fLayer& l = m->layers[li];
        const bool first = li == 0, last = li + 1 == nl;       // layer 0: v = 0, so no VT table and no vector residual
        if (E > 0) {
            {
                ProfScope p(pm, PGMI_K_GEMM_QKV, 2.0 * R * S2F_S * 2 * S2F_S, 0);
                rc = launch_gemm_f32(m->s.p, l.Wji, nullptr, nullptr, m->P.p, (int)R, 2 * S2F_S, S2F_S, EPI_NONE, st);
                if (rc) return rc;
            }
            {   // the message GVPs and the mean, the node's edge rows on chip: ds in m->pre, dv in m->mV
                ProfScope p(pm, PGMI_K_ATTENTION, 2.0 * RE * S2F_S * (S2F_H0 + 2.0 * S2F_KP + 3.0 * S2F_V), (double)R * (3 * S2F_S + 2 * S2F_H0 * 3) * 4);
                const S2fMsgWeights w = {l.m0.wv, l.m0.wsv, l.m0.bsv, l.m1.wh, l.m1.ws, l.m1.bs, l.m1.wv, l.m1.wsv, l.m1.bsv,
                                         l.m2.wh, l.m2.ws, l.m2.bs, l.m2.wv, l.m2.wsv, l.m2.bsv, l.m1.Kp};
                rc = m->fixed_degree ? launch_s3f_message(m->P.p, first ? nullptr : m->VT.p, l.Es, m->ev.p, l.whe, l.Wnt, w, m->src, L, R, m->pre.p, m->mV.p, st)
                                     : launch_s2f_message(m->P.p, first ? nullptr : m->VT.p, l.Es, m->ev.p, l.whe, l.Wnt, w, m->src, m->off, L, R, m->pre.p, m->mV.p, st);
                if (rc) return rc;
            }
        }
        {
            ProfScope p(pm, PGMI_K_LAYERNORM, 0, (double)R * S2F_S * 12);
            rc = launch_s2f_node_ln(m->s.p, first ? nullptr : m->v.p, E > 0 ? m->pre.p : nullptr, m->mV.p, l.n0w, l.n0b, l.f0.wh, l.f0.h,
                                    1, l.f0.Kp, R, m->s1.p, m->v1.p, m->A.p, m->vhA.p, st);
            if (rc) return rc;
        }
        rc = s2f_gvp(m, l.f0, m->vhA.p, 1, &l.f1, R, m->vhB.p, PGMI_K_GEMM_FC1, PGMI_K_KEPT_ROWS);
        if (!rc) rc = s2f_gvp(m, l.f1, m->vhB.p, 0, nullptr, R, m->mV.p, PGMI_K_GEMM_FC2, PGMI_K_KEPT_ROWS);
        if (rc) return rc;
        {
            ProfScope p(pm, PGMI_K_LAYERNORM, 0, (double)R * S2F_S * 12);
            rc = launch_s2f_node_ln(m->s1.p, m->v1.p, m->pre.p, m->mV.p, l.n1w, l.n1b, last ? nullptr : m->layers[li + 1].whji,
                                    last ? 0 : 2 * S2F_H0, 0, 0, R, m->s.p, m->v.p, nullptr, m->VT.p, st);
            if (rc) return rc;
        }
    }
    {
        ProfScope p(pm, PGMI_K_HEAD, 2.0 * R * S2F_S * S2F_KP, 0);
        rc = launch_s2f_node_ln(m->s.p, m->v.p, nullptr, nullptr, m->onw, m->onb, m->wout.wh, m->wout.h, 1, m->wout.Kp, R,
                                m->s1.p, m->v1.p, m->A.p, m->vhA.p, st);
        if (!rc) rc = launch_gemm_f32(m->A.p, m->wout.ws, m->wout.bs, nullptr, m->pre.p, (int)R, S2F_S, m->wout.Kp, EPI_NONE, st);
        if (rc) return rc;
    }
    PGMI_HIP(hipGetLastError());
    return PGMI_OK;
}

// relu, the 20-way Linear, the ESM logits on low-pLDDT rows and the log-softmax on `rows` rows of W_out's output; S3F adds the pooled
// row of a row's pool group (sums, grp, Ns: s2f_head_kernel; null, null, 0 without)
int s2f_head(pgmi_s2f* m, const float* pre, const float* seq, const float* sums, const int32_t* grp, int Ns, int64_t rows, float* lp) {
    ProfScope p(&m->pm, PGMI_K_HEAD, 2.0 * rows * S2F_S * 20, 0);
    launch_s2f_head(pre, sums, grp, Ns, m->Wlin, m->blin, seq, m->plddt.p, m->cfg.plddt_threshold, m->L, rows, lp, m->pm.stream);
    PGMI_HIP(hipGetLastError());
    return PGMI_OK;
}

// bc masked copies: m->feat [bc L][D] (device) and m->seq [bc L][20] -> m->lp [bc L][20]
static int s2f_gnn(pgmi_s2f* m, int bc) {
    int rc = s2f_embed(m, bc);
    if (!rc) rc = s2f_layers(m, bc);
    if (!rc) rc = s2f_head(m, m->pre.p, m->seq.p, nullptr, nullptr, 0, (int64_t)bc * m->L, m->lp.p);
    return rc;
}

// copies [s0, s0 + bc) of a gvp_forward call: their rows of node_feat [.][L][D] and seq_logits [.][L][20] -> m->feat, m->seq
int s2f_fill_rows(pgmi_s2f* m, const float* node_feat, const float* seq_logits, int s0, int bc) {
    const size_t R = (size_t)bc * m->L, r0 = (size_t)s0 * m->L, D = m->D;
    PGMI_HIP(hipMemcpyAsync(m->feat.p, node_feat + r0 * D, R * D * 4, hipMemcpyHostToDevice, m->pm.stream));
    PGMI_HIP(hipMemcpyAsync(m->seq.p, seq_logits + r0 * 20, R * 20 * 4, hipMemcpyHostToDevice, m->pm.stream));
    return PGMI_OK;
}

// the arguments of a set_logprobs entry of model `name` ("S2F", "S3F") on a handle with a structure
int s2f_check_sets(const pgmi_s2f* m, const char* name, const int32_t* wt_tokens, int T, const int32_t* aa_cols, const int32_t* set_off,
                   const int32_t* set_pos, int n_sets, const float* out) {
    const pgmi_model* esm = m->esm;
    if (!esm) {
        char fn[8] = {0};                                      // the entry's prefix: the name in lower case
        for (int i = 0; i < 7 && name[i]; ++i) fn[i] = (char)tolower(name[i]);
        set_error("%s: this handle was created without an ESM2 model (pgmi_%s_gvp_forward only)", name, fn);
        return PGMI_EINVAL;
    }
    if (!wt_tokens || !aa_cols || !set_off || !set_pos || !out || n_sets <= 0) { set_error("bad argument"); return PGMI_EINVAL; }
    const int L = m->L, V = esm->cfg.vocab;
    if (T != L + 2) { set_error("%s: T = %d tokens, the structure has %d residues (<cls> + residues + <eos>)", name, T, L); return PGMI_EINVAL; }
    if (T + 31 > esm->max_rows) { set_error("T=%d exceeds the ESM2 model's workspace rows %d", T, esm->max_rows); return PGMI_EINVAL; }
    const int rc = check_tokens(wt_tokens, 1, T, esm->n_token_ids);
    if (rc) return rc;
    for (int c = 0; c < 20; ++c)
        if (aa_cols[c] < 0 || aa_cols[c] >= V) { set_error("%s: amino-acid column %d = %d outside the vocabulary (%d)", name, c, aa_cols[c], V); return PGMI_EINVAL; }
    if (set_off[0] != 0) { set_error("set_off[0] must be 0"); return PGMI_EINVAL; }
    for (int s = 0; s < n_sets; ++s) {
        if (set_off[s + 1] <= set_off[s] || set_off[s + 1] - set_off[s] > L) { set_error("position set %d is empty or larger than L", s); return PGMI_EINVAL; }
        for (int e = set_off[s]; e < set_off[s + 1]; ++e) {
            const int p = set_pos[e];
            if (p < 0 || p >= L || (e > set_off[s] && p <= set_pos[e - 1])) { set_error("position set %d: residue %d out of range or not ascending", s, p); return PGMI_EINVAL; }
        }
    }
    return PGMI_OK;
}

// what the ESM2 fill of chunks of `per` copies needs: the device index arrays, aa_cols on the device, the host scratch
int s2f_set_buffers(pgmi_s2f* m, int per, int T, const int32_t* aa_cols, S2fSetHost* h) {
    pgmi_model* pm = &m->pm;
    const int rc = reserve_all(pm, m->ridx, (size_t)per * m->L, m->toks, (size_t)per * T, m->cols, 20);
    if (rc) return rc;
    PGMI_HIP(hipMemcpyAsync(m->cols, aa_cols, 20 * 4, hipMemcpyHostToDevice, pm->stream));
    h->toks.resize((size_t)per * T);
    h->ridx.resize((size_t)per * m->L);
    return PGMI_OK;
}

// masked copies [s0, s0 + bc) of the wild type, one per position set: ESM2 on them, then m->feat [bc L][D] = emb_layer_norm_after of
// the residue rows and m->seq [bc L][20] = the amino-acid columns of ESM2's log-probability rows, both left on the stream
int s2f_fill_esm(pgmi_s2f* m, const int32_t* wt_tokens, int T, const int32_t* set_off, const int32_t* set_pos, int s0, int bc, S2fSetHost* h) {
    pgmi_model* esm = m->esm;
    hipStream_t st = m->pm.stream;
    const int L = m->L, D = m->D, M = bc * T;
    const int64_t R = (int64_t)bc * L;
    for (int b = 0; b < bc; ++b) {
        memcpy(&h->toks[(size_t)b * T], wt_tokens, (size_t)T * 4);
        for (int e = set_off[s0 + b]; e < set_off[s0 + b + 1]; ++e) h->toks[(size_t)b * T + 1 + set_pos[e]] = esm->mask_id;
        for (int i = 0; i < L; ++i) h->ridx[(size_t)b * L + i] = b * T + 1 + i;
    }
    PGMI_HIP(hipMemcpyAsync(esm->tokens, h->toks.data(), (size_t)M * 4, hipMemcpyHostToDevice, st));
    PGMI_HIP(hipMemcpyAsync(m->ridx, h->ridx.data(), (size_t)R * 4, hipMemcpyHostToDevice, st));
    int rc = run_encoder(esm, bc, T);
    if (rc) return rc;
    {   // residue_feature: emb_layer_norm_after on the L residue rows, fp32
        ProfScope p(esm, PGMI_K_LAYERNORM, 0, (double)R * D * 8);
        launch_gather_rows(esm->x, m->ridx, (int)R, D, m->feat.p, st);
        launch_layernorm(m->feat.p, esm->lna_w, esm->lna_b, (int)R, D, 1e-5f, m->feat.p, st);
    }
    rc = run_head(esm, M, nullptr);                        // esm->lp [M][V]: the log-softmax rows; the 20-way log-softmax drops the shift
    if (rc) return rc;
    launch_s2f_pick_logits(esm->lp, m->cols, L, T, esm->cfg.vocab, R, m->seq.p, st);
    return PGMI_OK;
}

// lp [bc][L][20] (host) = the tables of sets [s0, s0 + bc): each whole into `full` (nullable), its set's rows into `out`
void s2f_scatter(const float* lp, int L, const int32_t* set_off, const int32_t* set_pos, int s0, int bc, float* out, float* full) {
    for (int b = 0; b < bc; ++b) {
        if (full) memcpy(full + (size_t)(s0 + b) * L * 20, lp + (size_t)b * L * 20, (size_t)L * 20 * 4);
        for (int e = set_off[s0 + b]; e < set_off[s0 + b + 1]; ++e)
            memcpy(out + (size_t)e * 20, lp + ((size_t)b * L + set_pos[e]) * 20, 20 * 4);
    }
}

static int s2f_ready(pgmi_s2f* m) {
    if (!m) { set_error("bad argument"); return PGMI_EINVAL; }
    if (m->L <= 0) { set_error("S2F: no structure set (pgmi_s2f_set_structure)"); return PGMI_EINVAL; }
    return PGMI_OK;
}

}  // namespace pgmi

extern "C" {

int64_t pgmi_s2f_weight_count(const pgmi_s2f_config* cfg) {
    if (pgmi::s2f_check(cfg)) return -1;
    return pgmi::s2f_count(cfg, false);
}

int pgmi_s2f_create(const pgmi_s2f_config* cfg, const float* w, int64_t n_weights, pgmi_model* esm, int device, pgmi_s2f** out) {
    return pgmi::s2f_new(cfg, w, n_weights, esm, nullptr, device, 0, out);
}

}  // extern "C"

namespace pgmi {

int s2f_new(const pgmi_s2f_config* cfg, const float* w, int64_t n_weights, pgmi_model* esm, pgmi_s2f* stream_of, int device, int fixed_degree,
            pgmi_s2f** out) {
    if (!out) { set_error("null out"); return PGMI_EINVAL; }
    *out = nullptr;
    int rc = s2f_check(cfg);
    if (rc) return rc;
    if (esm) {
        if (esm->cfg.arch != PGMI_ARCH_ESM2) { set_error("S2F: the sequence model must be an ESM2 model (arch %d)", esm->cfg.arch); return PGMI_EINVAL; }
        if (esm->cfg.embed_dim != cfg->node_in) { set_error("S2F: node_in %d differs from the ESM2 model's width %d", cfg->node_in, esm->cfg.embed_dim); return PGMI_EINVAL; }
        device = esm->device;
    }
    // one stream with the ESM2 model: the GNN reads what the encoder just wrote
    hipStream_t lend = esm ? esm->stream : stream_of ? stream_of->pm.stream : nullptr;
    pgmi_s2f* m = new pgmi_s2f();
    rc = side_open(&m->pm, "S2F", w, n_weights, s2f_count(cfg, fixed_degree != 0), false, device, PGMI_PREC_FP32, lend);
    if (rc) { delete m; return rc; }
    m->cfg = *cfg;
    m->D = cfg->node_in;
    m->esm = esm;
    m->fixed_degree = fixed_degree;
    m->own_stream = !lend;
    rc = s2f_build(m, w, n_weights);
    if (rc) { pgmi_s2f_destroy(m); return rc; }
    *out = m;
    return PGMI_OK;
}

}  // namespace pgmi

extern "C" {

void pgmi_s2f_destroy(pgmi_s2f* m) {
    if (!m) return;
    side_release(&m->pm, m->own_stream);
    delete m;
}

pgmi_model* pgmi_s2f_profile_model(pgmi_s2f* m) { return m ? &m->pm : nullptr; }

int pgmi_s2f_set_structure(pgmi_s2f* m, const float* pos, const float* plddt, int L) {
    if (!m || !pos || !plddt) { set_error("bad argument"); return PGMI_EINVAL; }
    if (L < 1 || L > S2F_MAX_L) { set_error("S2F: L = %d outside 1 .. %d", L, S2F_MAX_L); return PGMI_EINVAL; }
    for (int i = 0; i < L; ++i) {
        if (!std::isfinite(plddt[i])) { set_error("S2F: pLDDT of residue %d is not finite", i); return PGMI_EINVAL; }
        for (int c = 0; c < 3; ++c)
            if (!std::isfinite(pos[(size_t)i * 3 + c])) { set_error("S2F: coordinate of residue %d is not finite", i); return PGMI_EINVAL; }
    }
    PGMI_HIP(hipSetDevice(m->pm.device));
    return s2f_structure(m, pos, plddt, L);
}

int pgmi_s2f_graph(pgmi_s2f* m, int32_t* n_edges, int32_t* src, int32_t* dst, float* e_s, float* e_v) {
    int rc = s2f_ready(m);
    if (rc) return rc;
    if (n_edges) *n_edges = m->E;
    if (src) memcpy(src, m->h_src.data(), (size_t)m->E * 4);
    if (dst) memcpy(dst, m->h_dst.data(), (size_t)m->E * 4);
    if (e_s) memcpy(e_s, m->h_es.data(), m->h_es.size() * 4);
    if (e_v) memcpy(e_v, m->h_ev.data(), m->h_ev.size() * 4);
    return PGMI_OK;
}

int pgmi_s2f_gvp_forward(pgmi_s2f* m, const float* node_feat, const float* seq_logits, int B, float* lp, float* node_s, float* node_v) {
    int rc = s2f_ready(m);
    if (rc) return rc;
    if (!node_feat || !seq_logits || !lp || B <= 0) { set_error("bad argument"); return PGMI_EINVAL; }
    PGMI_HIP(hipSetDevice(m->pm.device));
    pgmi_model* pm = &m->pm;
    hipStream_t st = pm->stream;
    const int L = m->L, per = s2f_per_chunk(m, B);
    rc = s2f_workspace(m, per);
    for (int b0 = 0; b0 < B && !rc; b0 += per) {
        const int bc = std::min(per, B - b0);
        const size_t R = (size_t)bc * L, r0 = (size_t)b0 * L;
        rc = s2f_fill_rows(m, node_feat, seq_logits, b0, bc);
        if (!rc) rc = s2f_gnn(m, bc);
        if (rc) break;
        PGMI_HIP(hipMemcpyAsync(lp + r0 * 20, m->lp.p, R * 20 * 4, hipMemcpyDeviceToHost, st));
        if (node_s) PGMI_HIP(hipMemcpyAsync(node_s + r0 * S2F_S, m->s.p, R * S2F_S * 4, hipMemcpyDeviceToHost, st));
        if (node_v) PGMI_HIP(hipMemcpyAsync(node_v + r0 * S2F_V * 3, m->v.p, R * S2F_V * 3 * 4, hipMemcpyDeviceToHost, st));
        PGMI_HIP(hipStreamSynchronize(st));
        if (pm->prof) rc = prof_drain(pm);
    }
    return side_sync(pm, rc, "S2F forward");
}

int pgmi_s2f_set_logprobs(pgmi_s2f* m, const int32_t* wt_tokens, int T, const int32_t* aa_cols, const int32_t* set_off,
                          const int32_t* set_pos, int n_sets, float* out, float* full) {
    int rc = s2f_ready(m);
    if (rc) return rc;
    rc = s2f_check_sets(m, "S2F", wt_tokens, T, aa_cols, set_off, set_pos, n_sets, out);
    if (rc) return rc;
    PGMI_HIP(hipSetDevice(m->pm.device));
    pgmi_model *pm = &m->pm, *esm = m->esm;
    hipStream_t st = pm->stream;
    const int L = m->L, per = std::min(s2f_per_chunk(m, n_sets), rows_per_chunk(esm, T));
    S2fSetHost host;
    rc = s2f_workspace(m, per);
    if (!rc) rc = s2f_set_buffers(m, per, T, aa_cols, &host);
    if (rc) return rc;
    std::vector<float> lp((size_t)per * L * 20);
    for (int s0 = 0; s0 < n_sets && !rc; s0 += per) {
        const int bc = std::min(per, n_sets - s0);
        rc = s2f_fill_esm(m, wt_tokens, T, set_off, set_pos, s0, bc, &host);
        if (!rc) rc = s2f_gnn(m, bc);
        if (rc) break;
        PGMI_HIP(hipMemcpyAsync(lp.data(), m->lp.p, (size_t)bc * L * 20 * 4, hipMemcpyDeviceToHost, st));
        PGMI_HIP(hipStreamSynchronize(st));
        s2f_scatter(lp.data(), L, set_off, set_pos, s0, bc, out, full);
        if (pm->prof) rc = prof_drain(pm);
        if (!rc && esm->prof) rc = prof_drain(esm);
    }
    rc = side_sync(pm, rc, "S2F scoring");
    return rc ? rc : check_nonfinite(esm);
}

}  // extern "C"
