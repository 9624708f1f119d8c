// ProSST entries of the C ABI (include/pgmi.h, ProSST section): the blob walk, the per-structure pass (distances, the
// global edges, the subgraphs, the input features, W_v and W_e on the host in double; every layer's edge share of the first message GVP
// and layer 0's messages over the global edges on the device), the per-chunk GVP-GNN over the node copies of a run of subgraphs, the
// readout and the codebook assignment.  The kernels are in prosst_gvp.hip.  Dense Linears are launch_gemm_f32: a GEMM output element
// is a two-level sum whose order does not depend on the row count, and every other kernel works on one row, so a subgraph's bits do
// not depend on the chunking or on what else is in the call.
#include <cmath>
#include <numeric>

#include "prosst_impl.h"

namespace pgmi {

static long long g_prosst_max_rows = 0;
static int g_prosst_share0 = 1;
static long long prosst_row_cap() { return g_prosst_max_rows > 0 ? g_prosst_max_rows : 32768; }

int prosst_set_option(const char* name, long long value) {
    if (!strcmp(name, "prosst_max_rows")) { g_prosst_max_rows = std::min(std::max(value, 0LL), PQ_ROWS_LIMIT); return PGMI_OK; }
    if (!strcmp(name, "prosst_share_layer0")) { g_prosst_share0 = value != 0; return PGMI_OK; }
    return PGMI_EINVAL;
}

static int prosst_check(const pgmi_prosst_config* c) {
    if (!c) { set_error("null config"); return PGMI_EINVAL; }
    if (c->abi_version != PGMI_ABI_VERSION) { set_error("ABI version mismatch: got %d, library is %d", c->abi_version, PGMI_ABI_VERSION); return PGMI_EINVAL; }
    if (c->node_s != PQ_S || c->node_v != PQ_V || c->edge_s != PQ_ES || c->edge_v != PQ_EV) {
        set_error("ProSST: dimensions node (%d, %d) edge (%d, %d); this path runs node (256, 32), edge (64, 2)", c->node_s, c->node_v, c->edge_s,
                  c->edge_v);
        return PGMI_EINVAL;
    }
    if (c->layers < 1 || c->layers > PQ_MAX_LAYERS) { set_error("ProSST: 1 .. %d layers, got %d", PQ_MAX_LAYERS, c->layers); return PGMI_EINVAL; }
    if (c->max_nodes < 1 || c->max_nodes > 40 || c->threshold < 0 || c->threshold > c->max_nodes) {
        set_error("ProSST: max_nodes %d / threshold %d: 1 <= max_nodes <= 40 and 0 <= threshold <= max_nodes", c->max_nodes, c->threshold);
        return PGMI_EINVAL;
    }
    if (!(c->radius > 0.0f) || !std::isfinite(c->radius)) { set_error("ProSST: radius must be positive and finite"); return PGMI_EINVAL; }
    return PGMI_OK;
}

static int64_t gvp_count(int si, int vi, int so, int vo, int h) {   // wh, ws + b, wv
    return (int64_t)h * vi + (int64_t)so * (si + h) + so + (int64_t)vo * h;
}
static int64_t wv_count() { return 2 * PQ_NS_IN + gvp_count(PQ_NS_IN, PQ_NV_IN, PQ_S, PQ_V, PQ_V); }
static int64_t we_count() { return 2 * PQ_ES_IN + gvp_count(PQ_ES_IN, 1, PQ_ES, PQ_EV, PQ_EV); }
static int64_t prosst_count(const pgmi_prosst_config* c) {
    const int64_t layer = gvp_count(2 * PQ_S + PQ_ES, PQ_H0, PQ_S, PQ_V, PQ_H0) + 2 * gvp_count(PQ_S, PQ_V, PQ_S, PQ_V, PQ_V) + 4 * PQ_S +
                          gvp_count(PQ_S, PQ_V, PQ_FS, PQ_FV, PQ_FV) + gvp_count(PQ_FS, PQ_FV, PQ_S, PQ_V, PQ_FV);
    return wv_count() + we_count() + c->layers * layer + 2 * PQ_S + gvp_count(PQ_S, PQ_V, PQ_S, 0, PQ_V);
}

static int prosst_build(pgmi_prosst* m, const float* w, int64_t n_weights) {
    BlobCursor c(&m->pm, w, n_weights);
    auto gvp = [&](ProsstGvp* g, int si, int vi, int so, int vo, int h, bool with_ws) {
        c.upload(&g->wh, (size_t)h * vi);
        const float* ws = c.take((size_t)so * (si + h));
        if (with_ws) c.upload(&g->ws, ws, (size_t)so * (si + h));
        c.upload(&g->bs, so);
        if (vo) c.upload(&g->wv, (size_t)vo * h);
        return ws;
    };
    { const float* p = c.take((size_t)wv_count()); m->wv_host.assign(p, p + wv_count()); }
    { const float* p = c.take((size_t)we_count()); m->we_host.assign(p, p + we_count()); }
    m->layers.resize(m->cfg.layers);
    for (ProsstLayer& l : m->layers) {
        const int K0 = 2 * PQ_S + PQ_ES + PQ_H0;                 // 642 columns: s_j | e_s | s_i | norms
        const float* wh = c.p;                                  // [66][66]: v_j | e_v | v_i columns
        const float* ws = gvp(&l.m0, 2 * PQ_S + PQ_ES, PQ_H0, PQ_S, PQ_V, PQ_H0, false);
        l.b0 = l.m0.bs;
        std::vector<float> wji((size_t)2 * PQ_S * PQ_S), we((size_t)PQ_S * PQ_ES), wnt((size_t)PQ_H0 * PQ_S), whji((size_t)2 * PQ_H0 * PQ_V),
            whe((size_t)PQ_H0 * PQ_EV);
        for (int n = 0; n < PQ_S; ++n) {
            const float* row = ws + (size_t)n * K0;
            memcpy(&wji[(size_t)n * PQ_S], row, PQ_S * sizeof(float));
            memcpy(&we[(size_t)n * PQ_ES], row + PQ_S, PQ_ES * sizeof(float));
            memcpy(&wji[(size_t)(PQ_S + n) * PQ_S], row + PQ_S + PQ_ES, PQ_S * sizeof(float));
            for (int h = 0; h < PQ_H0; ++h) wnt[(size_t)h * PQ_S + n] = row[2 * PQ_S + PQ_ES + h];
        }
        for (int h = 0; h < PQ_H0; ++h) {
            memcpy(&whji[(size_t)h * PQ_V], wh + (size_t)h * PQ_H0, PQ_V * sizeof(float));
            memcpy(&whe[(size_t)h * PQ_EV], wh + (size_t)h * PQ_H0 + PQ_V, PQ_EV * sizeof(float));
            memcpy(&whji[(size_t)(PQ_H0 + h) * PQ_V], wh + (size_t)h * PQ_H0 + PQ_V + PQ_EV, PQ_V * sizeof(float));
        }
        c.upload(&l.Wji, wji);
        c.upload(&l.We, we);
        c.upload(&l.Wnt, wnt);
        c.upload(&l.whji, whji);
        c.upload(&l.whe, whe);
        gvp(&l.m1, PQ_S, PQ_V, PQ_S, PQ_V, PQ_V, true);
        gvp(&l.m2, PQ_S, PQ_V, PQ_S, PQ_V, PQ_V, true);
        c.upload(&l.n0w, PQ_S); c.upload(&l.n0b, PQ_S);
        c.upload(&l.n1w, PQ_S); c.upload(&l.n1b, PQ_S);
        gvp(&l.f0, PQ_S, PQ_V, PQ_FS, PQ_FV, PQ_FV, true);
        gvp(&l.f1, PQ_FS, PQ_FV, PQ_S, PQ_V, PQ_FV, true);
    }
    c.upload(&m->onw, PQ_S);
    c.upload(&m->onb, PQ_S);
    gvp(&m->wout, PQ_S, PQ_V, PQ_S, 0, PQ_V, true);
    return c.finish();
}

// ---- the structure pass on the host, in double on the float32 coordinates ---------------------------------------------------------
static inline double ca_dist(const float* X, int a, int b) {
    const float *p = X + (size_t)a * 12 + 3, *q = X + (size_t)b * 12 + 3;
    const double dx = (double)p[0] - q[0], dy = (double)p[1] - q[1], dz = (double)p[2] - q[2];
    return std::sqrt(dx * dx + dy * dy + dz * dz);
}
static inline void unit3(const double* x, double* o) {          // _normalize: x / |x| with nan_to_num (a zero vector stays zero)
    const double n = std::sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
    for (int c = 0; c < 3; ++c) { const double y = x[c] / n; o[c] = std::isfinite(y) ? y : 0.0; }
}

// The global edges (a -> b), a != b, d < radius, in row-major order of (a, b) with the CSR goff over a; and per anchor the subgraph's
// nodes: the anchor's row of distances sorted ascending (ties: lower index first), the first 50, those with d < radius, the first
// max_nodes of them when more than `threshold` remain, sorted by index.
static void prosst_graph(pgmi_prosst* m, const float* X, int L) {
    const double radius = (double)m->cfg.radius;
    m->h_a.clear(); m->h_b.clear(); m->h_nodes.clear();
    m->h_goff.assign(1, 0); m->h_node_off.assign(1, 0);
    std::vector<double> d(L);
    std::vector<int32_t> order(L);
    for (int i = 0; i < L; ++i) {
        for (int j = 0; j < L; ++j) {
            d[j] = ca_dist(X, i, j);
            if (j != i && d[j] < radius) { m->h_a.push_back(i); m->h_b.push_back(j); }
        }
        m->h_goff.push_back((int32_t)m->h_a.size());
        std::iota(order.begin(), order.end(), 0);
        const int depth = std::min(L, PQ_DEPTH);
        std::partial_sort(order.begin(), order.begin() + depth, order.end(),
                          [&](int32_t x, int32_t y) { return d[x] < d[y] || (d[x] == d[y] && x < y); });
        int n = 0;
        while (n < depth && d[order[n]] < radius) ++n;          // ascending distances: the kept ones are a prefix
        if (n > m->cfg.threshold) n = std::min(n, m->cfg.max_nodes);
        std::sort(order.begin(), order.begin() + n);
        m->h_nodes.insert(m->h_nodes.end(), order.begin(), order.begin() + n);
        m->h_node_off.push_back((int32_t)m->h_nodes.size());
    }
    m->E = (int)m->h_a.size();
    m->N = (int64_t)m->h_nodes.size();
    // per node copy (anchor i, node q): its incoming subgraph edges p -> q, p in the subgraph, ascending p: the global edge and the copy of p
    m->h_in_off.assign(1, 0); m->h_in_gid.clear(); m->h_in_src.clear();
    for (int i = 0; i < L; ++i) {
        const int32_t n0 = m->h_node_off[i], n1 = m->h_node_off[i + 1];
        for (int32_t r = n0; r < n1; ++r) {
            const int q = m->h_nodes[r];
            // the neighbours of q are the b of q's row (the graph is symmetric); the edge p -> q is in p's row
            int32_t g = m->h_goff[q];
            const int32_t g1 = m->h_goff[q + 1];
            for (int32_t t = n0; t < n1 && g < g1; ++t) {
                const int p = m->h_nodes[t];
                while (g < g1 && m->h_b[g] < p) ++g;
                if (g < g1 && m->h_b[g] == p) {
                    const int32_t* lo = m->h_b.data() + m->h_goff[p];
                    const int32_t* hi = m->h_b.data() + m->h_goff[p + 1];
                    m->h_in_gid.push_back((int32_t)(std::lower_bound(lo, hi, q) - m->h_b.data()));
                    m->h_in_src.push_back(t);
                }
            }
            m->h_in_off.push_back((int32_t)m->h_in_gid.size());
        }
    }
    m->ES = (int64_t)m->h_in_gid.size();
}

// tuple LayerNorm + GVP without activations on one row, in double: s_in [si] (LayerNorm lnw, lnb, eps 1e-5), v_in [vi][3] -> s_out [so],
// v_out [vo][3]; w = wh [h][vi], ws [so][si + h], bs [so], wv [vo][h]
static void host_ln_gvp(const float* lnw, const float* lnb, const float* w, int si, int vi, int so, int vo, int h, const double* s_in,
                        const double* v_in, double* s_out, double* v_out) {
    const float *wh = w, *ws = wh + (size_t)h * vi, *bs = ws + (size_t)so * (si + h), *wv = bs + so;
    double f[PQ_ES_IN + PQ_V], vn[PQ_NV_IN * 3], vh[PQ_V * 3];     // si + h <= 52, vi <= 3, h <= 32: W_v and W_e only
    double mean = 0.0, var = 0.0;
    for (int k = 0; k < si; ++k) mean += s_in[k];
    mean /= si;
    for (int k = 0; k < si; ++k) var += (s_in[k] - mean) * (s_in[k] - mean);
    const double rstd = 1.0 / std::sqrt(var / si + 1e-5);
    for (int k = 0; k < si; ++k) f[k] = (s_in[k] - mean) * rstd * lnw[k] + lnb[k];
    double n2 = 0.0;
    for (int c = 0; c < vi; ++c) n2 += std::max(v_in[c * 3] * v_in[c * 3] + v_in[c * 3 + 1] * v_in[c * 3 + 1] + v_in[c * 3 + 2] * v_in[c * 3 + 2], 1e-8);
    const double vden = std::sqrt(n2 / vi);
    for (int t = 0; t < vi * 3; ++t) vn[t] = v_in[t] / vden;
    for (int q = 0; q < h; ++q) {
        for (int dd = 0; dd < 3; ++dd) {
            double a = 0.0;
            for (int c = 0; c < vi; ++c) a += (double)wh[q * vi + c] * vn[c * 3 + dd];
            vh[q * 3 + dd] = a;
        }
        f[si + q] = std::sqrt(std::max(vh[q * 3] * vh[q * 3] + vh[q * 3 + 1] * vh[q * 3 + 1] + vh[q * 3 + 2] * vh[q * 3 + 2], 1e-8));
    }
    for (int n = 0; n < so; ++n) {
        double a = bs[n];
        for (int k = 0; k < si + h; ++k) a += (double)ws[(size_t)n * (si + h) + k] * f[k];
        s_out[n] = a;
    }
    for (int o = 0; o < vo; ++o)
        for (int dd = 0; dd < 3; ++dd) {
            double a = 0.0;
            for (int q = 0; q < h; ++q) a += (double)wv[o * h + q] * vh[q * 3 + dd];
            v_out[o * 3 + dd] = a;
        }
}

// node features -> W_v -> gs [L][256], gv [L][32][3]; edge features -> W_e -> es [E][64], ev [E][2][3]
static void prosst_features(const pgmi_prosst* m, const float* X, int L, std::vector<float>& gs, std::vector<float>& gv, std::vector<float>& es,
                            std::vector<float>& ev) {
    gs.assign((size_t)L * PQ_S, 0.0f); gv.assign((size_t)L * PQ_V * 3, 0.0f);
    const int E = m->E;
    es.assign((size_t)E * PQ_ES, 0.0f); ev.assign((size_t)E * PQ_EV * 3, 0.0f);
    auto at = [&](int i, int atom, int c) { return (double)X[(size_t)i * 12 + atom * 3 + c]; };
    const double s13 = std::sqrt(1.0 / 3.0), s23 = std::sqrt(2.0 / 3.0);
    std::vector<double> so(PQ_S), vo(PQ_V * 3);
    {
        const float* w = m->wv_host.data();
        const double zeros[PQ_NS_IN] = {0.0};
        for (int i = 0; i < L; ++i) {
            double v[9] = {0.0}, t[3], cc[3], nn[3], bis[3], perp[3], cr[3];
            if (i + 1 < L) { for (int c = 0; c < 3; ++c) t[c] = at(i + 1, 1, c) - at(i, 1, c); unit3(t, v); }
            if (i > 0) { for (int c = 0; c < 3; ++c) t[c] = at(i - 1, 1, c) - at(i, 1, c); unit3(t, v + 3); }
            for (int c = 0; c < 3; ++c) t[c] = at(i, 2, c) - at(i, 1, c);
            unit3(t, cc);
            for (int c = 0; c < 3; ++c) t[c] = at(i, 0, c) - at(i, 1, c);
            unit3(t, nn);
            for (int c = 0; c < 3; ++c) t[c] = cc[c] + nn[c];
            unit3(t, bis);
            cr[0] = cc[1] * nn[2] - cc[2] * nn[1]; cr[1] = cc[2] * nn[0] - cc[0] * nn[2]; cr[2] = cc[0] * nn[1] - cc[1] * nn[0];
            unit3(cr, perp);
            for (int c = 0; c < 3; ++c) v[6 + c] = -bis[c] * s13 - perp[c] * s23;
            host_ln_gvp(w, w + PQ_NS_IN, w + 2 * PQ_NS_IN, PQ_NS_IN, PQ_NV_IN, PQ_S, PQ_V, PQ_V, zeros, v, so.data(), vo.data());
            for (int n = 0; n < PQ_S; ++n) gs[(size_t)i * PQ_S + n] = (float)so[n];
            for (int n = 0; n < PQ_V * 3; ++n) gv[(size_t)i * PQ_V * 3 + n] = (float)vo[n];
        }
    }
    const float* w = m->we_host.data();
    const float step = 20.0f / 15.0f;                           // torch.linspace(0, 20, 16) in float32: start + step k below the middle, end - step (15 - k) above
    double freq[8];
    for (int k = 0; k < 8; ++k) freq[k] = (double)std::exp((float)(2 * k) * -(float)(std::log(10000.0) / 16.0));   // the reference's float32 frequencies
    for (int e = 0; e < E; ++e) {
        const int a = m->h_a[e], b = m->h_b[e];
        double vec[3], f[PQ_ES_IN], u[3];
        for (int c = 0; c < 3; ++c) vec[c] = at(a, 1, c) - at(b, 1, c);
        const double dist = std::sqrt(vec[0] * vec[0] + vec[1] * vec[1] + vec[2] * vec[2]);
        for (int k = 0; k < 16; ++k) {
            const float mu = k < 8 ? step * (float)k : 20.0f - step * (float)(15 - k);
            const double z = (dist - (double)mu) / 1.25;
            f[k] = std::exp(-z * z);
        }
        for (int k = 0; k < 8; ++k) { const double ang = (double)(a - b) * freq[k]; f[16 + k] = std::cos(ang); f[24 + k] = std::sin(ang); }
        unit3(vec, u);
        host_ln_gvp(w, w + PQ_ES_IN, w + 2 * PQ_ES_IN, PQ_ES_IN, 1, PQ_ES, PQ_EV, PQ_EV, f, u, so.data(), vo.data());
        for (int n = 0; n < PQ_ES; ++n) es[(size_t)e * PQ_ES + n] = (float)so[n];
        for (int n = 0; n < PQ_EV * 3; ++n) ev[(size_t)e * PQ_EV * 3 + n] = (float)vo[n];
    }
}

static ProsstMsgWeights msg_weights(const ProsstLayer& l) {
    return {l.m0.wv, l.m1.wh, l.m1.ws, l.m1.bs, l.m1.wv, l.m2.wh, l.m2.ws, l.m2.bs, l.m2.wv};
}

// the per-node tables of a layer's first message GVP on `rows` rows of (s, v): P [rows][512] and VT [rows][132][3]
static int prosst_tables(pgmi_prosst* m, const ProsstLayer& l, const float* s, const float* v, int64_t rows, float* P, float* VT) {
    int rc = launch_gemm_f32(s, l.Wji, nullptr, nullptr, P, (int)rows, 2 * PQ_S, PQ_S, EPI_NONE, m->pm.stream);
    if (!rc) rc = launch_prosst_vtab(v, l.whji, 2 * PQ_H0, 0, rows, VT, nullptr, m->pm.stream);
    return rc;
}

static int prosst_structure(pgmi_prosst* m, const float* X, int L) {
    pgmi_model* pm = &m->pm;
    hipStream_t st = pm->stream;
    m->L = 0;
    m->have_emb = m->have_msg0 = false;
    prosst_graph(m, X, L);
    if (m->ES > 0x7fffffffLL / 2) { set_error("ProSST: %lld subgraph edges", (long long)m->ES); return PGMI_EINVAL; }
    std::vector<float> gs, gv;
    prosst_features(m, X, L, gs, gv, m->h_es, m->h_ev);
    const size_t E = (size_t)m->E, En = std::max<size_t>(E, 1), N = (size_t)m->N, ESn = std::max<size_t>((size_t)m->ES, 1);
    std::vector<int32_t> in_dst((size_t)m->ES);
    for (size_t r = 0; r < N; ++r)
        for (int32_t k = m->h_in_off[r]; k < m->h_in_off[r + 1]; ++k) in_dst[k] = (int32_t)r;
    int rc = reserve_all(pm, m->ea, En, m->eb, En, m->nodes, N, m->node_off, (size_t)L + 1, m->in_off, N + 1, m->in_gid, ESn, m->in_src, ESn,
                         m->in_dst, ESn, m->gs, (size_t)L * PQ_S, m->gv, (size_t)L * PQ_V * 3, m->es, En * PQ_ES, m->ev, En * PQ_EV * 3,
                         m->P0, (size_t)L * 2 * PQ_S, m->VT0, (size_t)L * 2 * PQ_H0 * 3, m->msg0, En * PQ_MSG);
    if (rc) return rc;
    auto upload = [&](void* dst, const void* src, size_t bytes) {
        if (rc || !bytes || hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st) == hipSuccess) return;
        set_error("ProSST: structure upload failed");
        rc = PGMI_EHIP;
    };
    upload(m->ea, m->h_a.data(), E * 4);
    upload(m->eb, m->h_b.data(), E * 4);
    upload(m->nodes, m->h_nodes.data(), N * 4);
    upload(m->node_off, m->h_node_off.data(), ((size_t)L + 1) * 4);
    upload(m->in_off, m->h_in_off.data(), (N + 1) * 4);
    upload(m->in_gid, m->h_in_gid.data(), (size_t)m->ES * 4);
    upload(m->in_src, m->h_in_src.data(), (size_t)m->ES * 4);
    upload(m->in_dst, in_dst.data(), (size_t)m->ES * 4);
    upload(m->gs.p, gs.data(), gs.size() * 4);
    upload(m->gv.p, gv.data(), gv.size() * 4);
    upload(m->es.p, m->h_es.data(), m->h_es.size() * 4);
    upload(m->ev.p, m->h_ev.data(), m->h_ev.size() * 4);
    if (!rc && E > 0) {
        ProfScope prof(pm, PGMI_K_EMBED, 2.0 * E * PQ_S * PQ_ES * m->layers.size() + 2.0 * E * PQ_S * (PQ_H0 + 2.0 * PQ_KM), 0);
        for (ProsstLayer& l : m->layers) {
            if (!rc) rc = l.Es.reserve(pm, E * PQ_S);
            if (!rc) rc = launch_gemm_f32(m->es.p, l.We, l.b0, nullptr, l.Es, (int)E, PQ_S, PQ_ES, EPI_NONE, st);
        }
        // layer 0 over the global edges: every copy of a residue enters it with the same state, so its messages are the global edges'
        const ProsstLayer& l0 = m->layers[0];
        if (!rc) rc = prosst_tables(m, l0, m->gs.p, m->gv.p, L, m->P0.p, m->VT0.p);
        if (!rc) rc = launch_prosst_message(m->P0.p, m->VT0.p, l0.Es, m->ev.p, l0.whe, l0.Wnt, msg_weights(l0), nullptr, m->ea, m->eb, 0, (int64_t)E,
                                            m->msg0.p, st);
        m->have_msg0 = !rc;
    }
    rc = side_sync(pm, rc, "ProSST structure pass");       // the host arrays of this call are free to go after this
    if (!rc) m->L = L;
    return rc;
}

// one feed-forward or output GVP's ws GEMM on its operand rows
static int prosst_ws(pgmi_prosst* m, int cls, const float* A, const ProsstGvp& g, int so, int K, int64_t rows, float* out) {
    ProfScope p(&m->pm, cls, 2.0 * rows * so * K, 0);
    return launch_gemm_f32(A, g.ws, g.bs, nullptr, out, (int)rows, so, K, EPI_NONE, m->pm.stream);
}

// subgraphs [a0, a1): their node copies through the layers, W_out and the readout -> m->pooled / m->emb rows [a0, a1); the node state
// after the last layer stays in m->s / m->v (chunk-relative rows)
static int prosst_chunk(pgmi_prosst* m, int a0, int a1) {
    pgmi_model* pm = &m->pm;
    hipStream_t st = pm->stream;
    const int32_t r0 = m->h_node_off[a0];
    const int64_t R = m->h_node_off[a1] - r0;
    const int32_t k0 = m->h_in_off[r0];
    const int64_t EC = m->h_in_off[r0 + R] - k0;
    const int32_t* off = m->in_off + r0;
    int rc = PGMI_OK;
    launch_prosst_gather(m->gs.p, m->gv.p, m->nodes + r0, R, m->s.p, m->v.p, st);
    const size_t nl = m->layers.size();
    for (size_t li = 0; li < nl && !rc; ++li) {
        const ProsstLayer& l = m->layers[li];
        const bool shared = li == 0 && g_prosst_share0 && m->have_msg0;
        if (EC > 0 && !shared) {
            {
                ProfScope p(pm, PGMI_K_GEMM_QKV, 2.0 * R * PQ_S * 2 * PQ_S, 0);
                rc = prosst_tables(m, l, m->s.p, m->v.p, R, m->P.p, m->VT.p);
                if (rc) return rc;
            }
            ProfScope p(pm, PGMI_K_ATTENTION, 2.0 * EC * PQ_S * (PQ_H0 + 2.0 * PQ_KM), (double)EC * PQ_MSG * 4);
            rc = launch_prosst_message(m->P.p, m->VT.p, l.Es, m->ev.p, l.whe, l.Wnt, msg_weights(l), m->in_gid + k0, m->in_src + k0, m->in_dst + k0, r0,
                                       EC, m->msg.p, st);
            if (rc) return rc;
        }
        {
            ProfScope p(pm, PGMI_K_LAYERNORM, 0, (double)(EC + 3 * R) * PQ_MSG * 4);
            launch_prosst_aggregate(shared ? m->msg0.p : m->msg.p, off, shared ? (const int32_t*)m->in_gid : nullptr, R, m->ds.p, m->dv.p, st);
            launch_prosst_node_ln(m->s.p, m->v.p, m->ds.p, m->dv.p, l.n0w, l.n0b, PQ_K0, R, m->s1.p, m->v1.p, m->A.p, st);
            rc = launch_prosst_vtab(m->v1.p, l.f0.wh, PQ_FV, PQ_K0, R, m->vhA.p, m->A.p, st);
            if (rc) return rc;
        }
        rc = prosst_ws(m, PGMI_K_GEMM_FC1, m->A.p, l.f0, PQ_FS, PQ_K0, R, m->pre.p);
        if (rc) return rc;
        {
            ProfScope p(pm, PGMI_K_KEPT_ROWS, 2.0 * R * 3 * PQ_FV * 2 * PQ_FV, (double)R * (PQ_FS + PQ_K1) * 4);
            rc = launch_prosst_gvp_mid(m->pre.p, m->vhA.p, l.f0.wv, l.f1.wh, PQ_FS, PQ_FV, PQ_FV, PQ_FV, 1, PQ_K1, R, m->A2.p, m->vhB.p, st);
            if (rc) return rc;
        }
        rc = prosst_ws(m, PGMI_K_GEMM_FC2, m->A2.p, l.f1, PQ_S, PQ_K1, R, m->ds.p);
        if (rc) return rc;
        {
            ProfScope p(pm, PGMI_K_KEPT_ROWS, 2.0 * R * 3 * PQ_V * PQ_FV, 0);
            rc = launch_prosst_gvp_mid(m->ds.p, m->vhB.p, l.f1.wv, nullptr, PQ_S, PQ_V, PQ_FV, 0, 0, 0, R, nullptr, m->dv.p, st);
            if (rc) return rc;
        }
        ProfScope p(pm, PGMI_K_LAYERNORM, 0, (double)R * PQ_MSG * 12);
        launch_prosst_node_ln(m->s1.p, m->v1.p, m->ds.p, m->dv.p, l.n1w, l.n1b, 0, R, m->s.p, m->v.p, nullptr, st);
    }
    if (rc) return rc;
    {
        ProfScope p(pm, PGMI_K_HEAD, 2.0 * R * PQ_S * PQ_KM, 0);
        launch_prosst_node_ln(m->s.p, m->v.p, nullptr, nullptr, m->onw, m->onb, PQ_KM, R, m->s1.p, m->v1.p, m->A.p, st);
        rc = launch_prosst_vtab(m->v1.p, m->wout.wh, PQ_V, PQ_KM, R, m->vhA.p, m->A.p, st);
        if (!rc) rc = launch_gemm_f32(m->A.p, m->wout.ws, m->wout.bs, nullptr, m->pre.p, (int)R, PQ_S, PQ_KM, EPI_NONE, st);
        if (rc) return rc;
        launch_prosst_pool(m->pre.p, m->node_off + a0, a1 - a0, m->pooled.p + (size_t)a0 * PQ_S, m->emb.p + (size_t)a0 * PQ_S, st);
    }
    PGMI_HIP(hipGetLastError());
    return PGMI_OK;
}

// emb [n][256] on the device against centres [K][256] (host) -> tokens [n] (host): |c|^2 - 2 x.c, lowest index on a tie
static int prosst_assign(pgmi_model* pm, DevBuf<float>& cent, DevBuf<float>& cn, DevBuf<float>& G, DevBuf<int32_t>& tok, const float* emb,
                         int64_t n, const float* centres, int K, int32_t* tokens) {
    hipStream_t st = pm->stream;
    int rc = reserve_all(pm, cent, (size_t)K * PQ_S, cn, (size_t)K, G, (size_t)n * K, tok, (size_t)n);
    if (rc) return rc;
    PGMI_HIP(hipMemcpyAsync(cent.p, centres, (size_t)K * PQ_S * 4, hipMemcpyHostToDevice, st));
    {
        ProfScope p(pm, PGMI_K_SCORE, 2.0 * n * K * PQ_S, 0);
        launch_prosst_centre_norms(cent.p, K, cn.p, st);
        rc = launch_gemm_f32(emb, cent.p, nullptr, nullptr, G.p, (int)n, K, PQ_S, EPI_NONE, st);
        if (rc) return rc;
        launch_prosst_argmin(G.p, cn.p, n, K, tok, st);
    }
    PGMI_HIP(hipMemcpyAsync(tokens, tok, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    return PGMI_OK;
}

static int check_centres(const float* centres, int K) {
    if (!centres || K < 1 || K > PQ_MAX_K) { set_error("ProSST: K = %d centres outside 1 .. %d", K, PQ_MAX_K); return PGMI_EINVAL; }
    for (size_t t = 0; t < (size_t)K * PQ_S; ++t)
        if (!std::isfinite(centres[t])) { set_error("ProSST: centre %d is not finite", (int)(t / PQ_S)); return PGMI_EINVAL; }
    return PGMI_OK;
}

// the structure arguments of pgmi_prosst_set_structure and pgmi_op_prosst_subgraphs
static int check_structure(const float* X, int L) {
    if (!X) { set_error("bad argument"); return PGMI_EINVAL; }
    if (L < 1 || L > PQ_MAX_L) { set_error("ProSST: L = %d outside 1 .. %d", L, PQ_MAX_L); return PGMI_EINVAL; }
    if (L == 3) { set_error("ProSST: L = 3: the reference's torch.cross without dim runs over the residue axis there, not over x, y, z"); return PGMI_EINVAL; }
    for (size_t t = 0; t < (size_t)L * 12; ++t)
        if (!std::isfinite(X[t])) { set_error("ProSST: coordinate of residue %d is not finite", (int)(t / 12)); return PGMI_EINVAL; }
    return PGMI_OK;
}

// what prosst_graph left in m, for L anchors, into the caller's arrays (each nullable)
static void prosst_view(const pgmi_prosst* m, int L, int64_t* counts, int32_t* edges, int32_t* node_off, int32_t* nodes, int32_t* edge_off,
                        int32_t* edge_gid) {
    if (counts) { counts[0] = m->E; counts[1] = m->N; counts[2] = m->ES; }
    if (edges) {
        memcpy(edges, m->h_a.data(), (size_t)m->E * 4);
        memcpy(edges + m->E, m->h_b.data(), (size_t)m->E * 4);
    }
    if (node_off) memcpy(node_off, m->h_node_off.data(), ((size_t)L + 1) * 4);
    if (nodes) memcpy(nodes, m->h_nodes.data(), (size_t)m->N * 4);
    if (edge_off || edge_gid) {          // the reference's order: row-major (p, q) over the sorted node set = ascending global edge
        std::vector<int32_t> g;
        for (int i = 0; i < L; ++i) {
            const int32_t r0 = m->h_node_off[i], r1 = m->h_node_off[i + 1];
            const int32_t k0 = m->h_in_off[r0], k1 = m->h_in_off[r1];
            if (edge_off) { edge_off[i] = k0; edge_off[i + 1] = k1; }
            if (edge_gid) {
                g.assign(m->h_in_gid.begin() + k0, m->h_in_gid.begin() + k1);
                std::sort(g.begin(), g.end());
                if (!g.empty()) memcpy(edge_gid + k0, g.data(), g.size() * 4);
            }
        }
    }
}

static int prosst_ready(pgmi_prosst* m) {
    if (!m) { set_error("bad argument"); return PGMI_EINVAL; }
    if (m->L <= 0) { set_error("ProSST: no structure set (pgmi_prosst_set_structure)"); return PGMI_EINVAL; }
    return PGMI_OK;
}

}  // namespace pgmi

using namespace pgmi;

extern "C" {

int64_t pgmi_prosst_weight_count(const pgmi_prosst_config* cfg) {
    if (prosst_check(cfg)) return -1;
    return prosst_count(cfg);
}

int pgmi_prosst_create(const pgmi_prosst_config* cfg, const float* w, int64_t n_weights, int device, pgmi_prosst** out) {
    if (!out) { set_error("null out"); return PGMI_EINVAL; }
    *out = nullptr;
    int rc = prosst_check(cfg);
    if (rc) return rc;
    pgmi_prosst* m = new pgmi_prosst();
    rc = side_open(&m->pm, "ProSST", w, n_weights, prosst_count(cfg), true, device, PGMI_PREC_FP32, nullptr);
    if (rc) { delete m; return rc; }
    m->cfg = *cfg;
    rc = prosst_build(m, w, n_weights);
    if (rc) { pgmi_prosst_destroy(m); return rc; }
    *out = m;
    return PGMI_OK;
}

void pgmi_prosst_destroy(pgmi_prosst* m) {
    if (!m) return;
    side_release(&m->pm, true);
    delete m;
}

pgmi_model* pgmi_prosst_profile_model(pgmi_prosst* m) { return m ? &m->pm : nullptr; }

int pgmi_prosst_set_structure(pgmi_prosst* m, const float* X, int L) {
    if (!m) { set_error("bad argument"); return PGMI_EINVAL; }
    m->L = 0;                                              // a refused structure leaves none behind
    m->have_emb = false;
    const int rc = check_structure(X, L);
    if (rc) return rc;
    PGMI_HIP(hipSetDevice(m->pm.device));
    return prosst_structure(m, X, L);
}

int pgmi_prosst_subgraphs(pgmi_prosst* m, int64_t* counts, int32_t* edges, float* e_s, float* e_v, int32_t* node_off, int32_t* nodes,
                          int32_t* edge_off, int32_t* edge_gid) {
    int rc = prosst_ready(m);
    if (rc) return rc;
    prosst_view(m, m->L, counts, edges, node_off, nodes, edge_off, edge_gid);
    if (e_s) memcpy(e_s, m->h_es.data(), m->h_es.size() * 4);
    if (e_v) memcpy(e_v, m->h_ev.data(), m->h_ev.size() * 4);
    return PGMI_OK;
}

int pgmi_op_prosst_subgraphs(const pgmi_prosst_config* cfg, const float* X, int L, int64_t* counts, int32_t* edges, int32_t* node_off,
                             int32_t* nodes, int32_t* edge_off, int32_t* edge_gid, int32_t* in_off, int32_t* in_gid, int32_t* in_src) {
    int rc = prosst_check(cfg);
    if (!rc) rc = check_structure(X, L);
    if (rc) return rc;
    pgmi_prosst m;                                         // host arrays only: no device, no stream
    m.cfg = *cfg;
    prosst_graph(&m, X, L);
    prosst_view(&m, L, counts, edges, node_off, nodes, edge_off, edge_gid);
    if (in_off) memcpy(in_off, m.h_in_off.data(), ((size_t)m.N + 1) * 4);
    if (in_gid) memcpy(in_gid, m.h_in_gid.data(), (size_t)m.ES * 4);
    if (in_src) memcpy(in_src, m.h_in_src.data(), (size_t)m.ES * 4);
    return PGMI_OK;
}

int pgmi_prosst_embed(pgmi_prosst* m, float* out, float* pooled, int sub, float* node_s, float* node_v) {
    int rc = prosst_ready(m);
    if (rc) return rc;
    const int L = m->L;
    if (!out || ((node_s || node_v) && (sub < 0 || sub >= L))) { set_error("bad argument"); return PGMI_EINVAL; }
    PGMI_HIP(hipSetDevice(m->pm.device));
    pgmi_model* pm = &m->pm;
    hipStream_t st = pm->stream;
    m->have_emb = false;
    // chunks: runs of subgraphs whose node copies fit the row cap (a subgraph is never cut)
    const long long cap = prosst_row_cap();
    std::vector<int> cuts(1, 0);
    size_t Rmax = 0, Emax = 0;
    for (int a = 0; a < L;) {
        int b = a + 1;
        while (b < L && m->h_node_off[b + 1] - m->h_node_off[a] <= cap) ++b;
        Rmax = std::max<size_t>(Rmax, m->h_node_off[b] - m->h_node_off[a]);
        Emax = std::max<size_t>(Emax, m->h_in_off[m->h_node_off[b]] - m->h_in_off[m->h_node_off[a]]);
        cuts.push_back(b);
        a = b;
    }
    Emax = std::max<size_t>(Emax, 1);
    rc = reserve_all(pm, m->s, Rmax * PQ_S, m->v, Rmax * PQ_V * 3, m->s1, Rmax * PQ_S, m->v1, Rmax * PQ_V * 3, m->P, Rmax * 2 * PQ_S, m->VT,
                     Rmax * 2 * PQ_H0 * 3, m->msg, Emax * PQ_MSG, m->ds, Rmax * PQ_S, m->dv, Rmax * PQ_V * 3, m->A, Rmax * PQ_K0, m->A2,
                     Rmax * PQ_K1, m->pre, Rmax * PQ_FS, m->vhA, Rmax * PQ_FV * 3, m->vhB, Rmax * PQ_FV * 3, m->pooled, (size_t)L * PQ_S, m->emb,
                     (size_t)L * PQ_S);
    for (size_t c = 0; c + 1 < cuts.size() && !rc; ++c) {
        const int a0 = cuts[c], a1 = cuts[c + 1];
        rc = prosst_chunk(m, a0, a1);
        if (rc) break;
        if ((node_s || node_v) && sub >= a0 && sub < a1) {
            const size_t r = m->h_node_off[sub] - m->h_node_off[a0], n = m->h_node_off[sub + 1] - m->h_node_off[sub];
            if (node_s) PGMI_HIP(hipMemcpyAsync(node_s, m->s.p + r * PQ_S, n * PQ_S * 4, hipMemcpyDeviceToHost, st));
            if (node_v) PGMI_HIP(hipMemcpyAsync(node_v, m->v.p + r * PQ_V * 3, n * PQ_V * 3 * 4, hipMemcpyDeviceToHost, st));
        }
        if (pm->prof) {                                     // the chunks share one stream and one workspace in order: no wait between them
            PGMI_HIP(hipStreamSynchronize(st));
            rc = prof_drain(pm);
        }
    }
    if (!rc) {
        PGMI_HIP(hipMemcpyAsync(out, m->emb.p, (size_t)L * PQ_S * 4, hipMemcpyDeviceToHost, st));
        if (pooled) PGMI_HIP(hipMemcpyAsync(pooled, m->pooled.p, (size_t)L * PQ_S * 4, hipMemcpyDeviceToHost, st));
    }
    rc = side_sync(pm, rc, "ProSST embedding");
    m->have_emb = !rc;
    return rc;
}

int pgmi_prosst_assign(pgmi_prosst* m, const float* centres, int K, int32_t* tokens) {
    int rc = prosst_ready(m);
    if (rc) return rc;
    if (!m->have_emb) { set_error("ProSST: no embedding of this structure yet (pgmi_prosst_embed)"); return PGMI_EINVAL; }
    if (!tokens) { set_error("bad argument"); return PGMI_EINVAL; }
    rc = check_centres(centres, K);
    if (rc) return rc;
    PGMI_HIP(hipSetDevice(m->pm.device));
    rc = prosst_assign(&m->pm, m->cent, m->cn, m->G, m->tok, m->emb.p, m->L, centres, K, tokens);
    rc = side_sync(&m->pm, rc, "ProSST assignment");
    if (!rc && m->pm.prof) rc = prof_drain(&m->pm);
    return rc;
}

int pgmi_op_prosst_assign(int device, const float* emb, int64_t n, const float* centres, int K, int32_t* tokens) {
    if (!emb || !tokens || n < 1) { set_error("bad argument"); return PGMI_EINVAL; }
    int rc = check_centres(centres, K);
    if (rc) return rc;
    if (n > PQ_OP_ROWS || n * K > PQ_OP_PRODUCTS) {             // the [n][K] product table is one allocation: refused here, not in the allocator
        set_error("ProSST assign op: n = %lld rows with K = %d; at most %d rows and %lld products (n K) per call", (long long)n, K, PQ_OP_ROWS,
                  (long long)PQ_OP_PRODUCTS);
        return PGMI_EINVAL;
    }
    OpScope s("ProSST assign op", device);
    if (s.rc) return s.rc;
    float* dx = s.up(emb, (size_t)n * PQ_S);
    float* dc = s.up(centres, (size_t)K * PQ_S);
    float* cn = s.alloc<float>((size_t)K);
    float* G = s.alloc<float>((size_t)n * K);
    int32_t* tok = s.alloc<int32_t>((size_t)n);
    if (s.rc) return s.rc;
    launch_prosst_centre_norms(dc, K, cn, nullptr);
    s.rc = launch_gemm_f32(dx, dc, nullptr, nullptr, G, (int)n, K, PQ_S, EPI_NONE, nullptr);
    if (!s.rc) launch_prosst_argmin(G, cn, n, K, tok, nullptr);
    s.sync();
    s.down(tokens, tok, (size_t)n);
    return s.rc;
}

}  // extern "C"
