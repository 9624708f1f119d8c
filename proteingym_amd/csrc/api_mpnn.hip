// ProteinMPNN entries of the C ABI (include/pgmi.h, ProteinMPNN section): the blob walk in state_dict() order, the per-structure pass
// (graph, edge features, the three encoder layers, the hoisted decoder tables) and the per-batch decoder (edge kernel, node side, head).
// The kernels are in mpnn.hip.  Node side: launch_gemm_f32 (W3, the FFN, the next layer's [A | P] projection) plus the row-local
// mpnn_add_ln kernel.  A GEMM output element is a two-level sum (one MFMA chain per 32-wide K tile, the tiles' partial sums added in
// fp32, tile by tile) whose order does not depend on the row count, and every other kernel is row-local or per (mutant, node), so a
// mutant's bits do not depend on the batch or the chunking.
#include <optional>

#include "model.h"

namespace pgmi {

constexpr long long MPNN_ROWS_LIMIT = 1 << 20;   // rows of a chunk are `int` in the GEMM launcher and the grids: L <= 8192 keeps one mutant below it
static long long g_mpnn_max_rows = 0;

int mpnn_set_option(const char* name, long long value) {
    if (!strcmp(name, "mpnn_max_rows")) { g_mpnn_max_rows = std::min(std::max(value, 0LL), MPNN_ROWS_LIMIT); return PGMI_OK; }
    return PGMI_EINVAL;
}

constexpr int H = 128, FF = 512, V = 21, MPNN_MAX_L = 8192, MPNN_MAX_EDGES = 48;

struct MpnnLin { float *w = nullptr, *b = nullptr; };
struct MpnnEnc {
    float *n1w, *n1b, *n2w, *n2b, *n3w, *n3b;
    MpnnLin W1, W2, W3, W11, W12, W13, Win, Wout;
};
struct MpnnDec {
    float *n1w, *n1b, *n2w, *n2b;
    float *Wap = nullptr, *bap = nullptr;     // [256][128]: W1a rows then W1d rows; bias b1 | 0
    float *W1b = nullptr;                     // [128][128]
    float *T = nullptr;                       // [22][128]: W1c W_s[s], row 21 zeros
    MpnnLin W2, W3, Win, Wout;
    DevBuf<float> Ep, Penc;                   // per structure: W1b h_E [L K][128], W1d h_V^enc [L][128]
};

}  // namespace pgmi

struct pgmi_mpnn {
    pgmi_model pm;                       // device, stream, allocation pool and profiling state (pgmi_mpnn_profile_model)
    pgmi_mpnn_config cfg;
    float *Wpos = nullptr, *bpos = nullptr, *Wt = nullptr, *nEw = nullptr, *nEb = nullptr;
    MpnnLin We, Whead;
    std::vector<MpnnEnc> enc;
    std::vector<MpnnDec> dec;
    // structure
    int L = 0, K = 0;
    DevBuf<float> X, mask, Dnb, E, hE, hV, AP0;
    DevBuf<int32_t> ridx, chain, E_idx;
    // workspace of the structure pass
    DevBuf<float> cat, t1, t2, n1, n2, nf;
    // workspace of a chunk of mutants
    DevBuf<uint8_t> S;
    DevBuf<int32_t> rank;
    DevBuf<float> sum, tmp, h1, h, ffn, AP, nll, lp;
    DevBuf<double> score;
};

namespace pgmi {

static int mpnn_check(const pgmi_mpnn_config* c) {
    if (!c) { set_error("null config"); return PGMI_EINVAL; }
    if (c->abi_version != PGMI_ABI_VERSION) { set_error("ABI version mismatch: got %d, library is %d", c->abi_version, PGMI_ABI_VERSION); return PGMI_EINVAL; }
    if (c->hidden != H) { set_error("ProteinMPNN: hidden width must be 128, got %d", c->hidden); return PGMI_EINVAL; }
    if (c->num_edges < 1 || c->num_edges > MPNN_MAX_EDGES) {
        set_error("ProteinMPNN: num_edges %d outside 1 .. %d", c->num_edges, MPNN_MAX_EDGES);
        return PGMI_EINVAL;
    }
    if (c->enc_layers < 1 || c->enc_layers > PGMI_MPNN_MAX_LAYERS || c->dec_layers < 1 || c->dec_layers > PGMI_MPNN_MAX_LAYERS) {
        set_error("ProteinMPNN: 1 .. %d layers per stack, got %d / %d", PGMI_MPNN_MAX_LAYERS, c->enc_layers, c->dec_layers);
        return PGMI_EINVAL;
    }
    if (c->precision != PGMI_PREC_FP32) { set_error("ProteinMPNN runs in precision fp32 only"); return PGMI_EINVAL; }
    return PGMI_OK;
}

static int64_t mpnn_count(const pgmi_mpnn_config* c) {
    const int64_t lin = H * H + H, ffn = (int64_t)FF * H + FF + (int64_t)H * FF + H;
    int64_t n = 16 * 66 + 16 + (int64_t)H * 416 + 2 * H + lin + (int64_t)V * H;
    n += c->enc_layers * (6 * H + 2 * ((int64_t)H * 3 * H + H) + 4 * lin + ffn);
    n += c->dec_layers * (4 * H + ((int64_t)H * 4 * H + H) + 2 * lin + ffn);
    n += (int64_t)V * H + V;
    return n;
}

static int mpnn_build(pgmi_mpnn* m, const float* w, int64_t n_weights) {
    BlobCursor blob(&m->pm, w, n_weights);
    auto lin = [&](MpnnLin* l, size_t N, size_t K) { blob.upload(&l->w, N * K); blob.upload(&l->b, N); };
    blob.upload(&m->Wpos, 16 * 66);
    blob.upload(&m->bpos, 16);
    {   // edge_embedding [128][416] -> transposed [416][128]: the feature kernel reads a feature's 128 columns as one line
        const float* we = blob.take((size_t)H * 416);
        std::vector<float> t((size_t)416 * H);
        for (int n = 0; n < H; ++n)
            for (int f = 0; f < 416; ++f) t[(size_t)f * H + n] = we[(size_t)n * 416 + f];
        blob.upload(&m->Wt, t);
    }
    blob.upload(&m->nEw, H);
    blob.upload(&m->nEb, H);
    lin(&m->We, H, H);
    const float* Ws = blob.take((size_t)V * H);
    m->enc.resize(m->cfg.enc_layers);
    for (MpnnEnc& e : m->enc) {
        blob.upload(&e.n1w, H); blob.upload(&e.n1b, H);
        blob.upload(&e.n2w, H); blob.upload(&e.n2b, H);
        blob.upload(&e.n3w, H); blob.upload(&e.n3b, H);
        lin(&e.W1, H, 3 * H); lin(&e.W2, H, H); lin(&e.W3, H, H);
        lin(&e.W11, H, 3 * H); lin(&e.W12, H, H); lin(&e.W13, H, H);
        lin(&e.Win, FF, H); lin(&e.Wout, H, FF);
    }
    m->dec.resize(m->cfg.dec_layers);
    for (MpnnDec& d : m->dec) {
        blob.upload(&d.n1w, H); blob.upload(&d.n1b, H);
        blob.upload(&d.n2w, H); blob.upload(&d.n2b, H);
        const float* W1 = blob.take((size_t)H * 4 * H);          // [128][512] = [W1a | W1b | W1c | W1d] by input block
        const float* b1 = blob.take(H);
        std::vector<float> wap((size_t)2 * H * H), bap((size_t)2 * H, 0.0f), w1b((size_t)H * H), T((size_t)(V + 1) * H, 0.0f);
        for (int n = 0; n < H; ++n) {
            memcpy(&wap[(size_t)n * H], W1 + (size_t)n * 4 * H, H * sizeof(float));
            memcpy(&wap[(size_t)(H + n) * H], W1 + (size_t)n * 4 * H + 3 * H, H * sizeof(float));
            memcpy(&w1b[(size_t)n * H], W1 + (size_t)n * 4 * H + H, H * sizeof(float));
            bap[n] = b1[n];
            for (int s = 0; s < V; ++s) {
                double a = 0.0;
                for (int c = 0; c < H; ++c) a += (double)W1[(size_t)n * 4 * H + 2 * H + c] * (double)Ws[(size_t)s * H + c];
                T[(size_t)s * H + n] = (float)a;
            }
        }
        blob.upload(&d.Wap, wap);
        blob.upload(&d.bap, bap);
        blob.upload(&d.W1b, w1b);
        blob.upload(&d.T, T);
        lin(&d.W2, H, H); lin(&d.W3, H, H);
        lin(&d.Win, FF, H); lin(&d.Wout, H, FF);
    }
    lin(&m->Whead, V, H);
    return blob.finish();
}

// one edge MLP of an encoder layer on the concatenated rows: out = W_c GELU(W_b GELU(W_a cat)) (+ residual)
static int mpnn_edge_mlp(pgmi_mpnn* m, const MpnnLin& a, const MpnnLin& b, const MpnnLin& c, const float* residual, float* out) {
    hipStream_t st = m->pm.stream;
    const int M = m->L * m->K;
    launch_mpnn_concat(m->hV, m->hE, m->E_idx, m->L, m->K, m->cat, st);
    int rc = launch_gemm_f32(m->cat, a.w, a.b, nullptr, m->t1, M, H, 3 * H, EPI_GELU, st);
    if (!rc) rc = launch_gemm_f32(m->t1, b.w, b.b, nullptr, m->t2, M, H, H, EPI_GELU, st);
    if (!rc) rc = launch_gemm_f32(m->t2, c.w, c.b, residual, out, M, H, H, EPI_NONE, st);
    return rc;
}

// FFN block of both stacks: h_out = LayerNorm2(h1 + W_out GELU(W_in h1)) * mask.  `timed`: the decoder's call, which times its three
// launches under the FFN and LayerNorm classes.  The structure pass is one PGMI_K_EMBED scope and passes false: scopes never nest (a
// ProfScope points into pm->events, which an inner scope may grow, and the time would be counted under two classes).
static int mpnn_ffn(pgmi_mpnn* m, const MpnnLin& Win, const MpnnLin& Wout, const float* n2w, const float* n2b, const float* h1, float* ffn,
                    float* tmp, float* out, int64_t rows, bool timed) {
    hipStream_t st = m->pm.stream;
    std::optional<ProfScope> p;
    if (timed) p.emplace(&m->pm, PGMI_K_GEMM_FC1, 2.0 * rows * H * FF, 0);
    int rc = launch_gemm_f32(h1, Win.w, Win.b, nullptr, ffn, (int)rows, FF, H, EPI_GELU, st);
    p.reset();
    if (rc) return rc;
    if (timed) p.emplace(&m->pm, PGMI_K_GEMM_FC2, 2.0 * rows * H * FF, 0);
    rc = launch_gemm_f32(ffn, Wout.w, Wout.b, h1, tmp, (int)rows, H, FF, EPI_NONE, st);
    p.reset();
    if (rc) return rc;
    if (timed) p.emplace(&m->pm, PGMI_K_LAYERNORM, 0, (double)rows * H * 8);
    launch_mpnn_add_ln(tmp, rows, nullptr, nullptr, 0.0f, 1.0f, n2w, n2b, m->mask, m->L, rows, out, st);
    return PGMI_OK;
}

static int mpnn_structure(pgmi_mpnn* m, const float* X, const float* mask, const int32_t* ridx, const int32_t* chain, int L) {
    pgmi_model* pm = &m->pm;
    hipStream_t st = pm->stream;
    const int K = std::min(m->cfg.num_edges, L);
    const size_t LK = (size_t)L * K;
    m->L = 0;                                    // no structure while this pass has not succeeded
    const size_t Ln = L;
    int rc = reserve_all(pm, m->X, Ln * 12, m->mask, Ln, m->ridx, Ln, m->chain, Ln, m->E_idx, LK, m->Dnb, LK, m->E, LK * H, m->hE, LK * H,
                         m->hV, Ln * H, m->AP0, Ln * 2 * H, m->cat, LK * 3 * H, m->t1, LK * H, m->t2, LK * H, m->n1, Ln * H, m->n2, Ln * H,
                         m->nf, Ln * FF);
    for (MpnnDec& d : m->dec)
        if (!rc) rc = reserve_all(pm, d.Ep, LK * H, d.Penc, Ln * H);
    if (rc) return rc;
    m->K = K;
    m->L = L;                                    // the helpers below read m->L / m->K; back to 0 at the end if anything failed
    auto upload = [&](void* dst, const void* src, size_t bytes) {
        if (rc || hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st) == hipSuccess) return;
        set_error("ProteinMPNN: structure upload failed");
        rc = PGMI_EHIP;
    };
    upload(m->X, X, (size_t)L * 12 * 4);
    upload(m->mask, mask, (size_t)L * 4);
    upload(m->ridx, ridx, (size_t)L * 4);
    upload(m->chain, chain, (size_t)L * 4);
    if (!rc) {   // one scope over the whole pass; nothing inside opens another (mpnn_ffn: timed = false)
        ProfScope prof(pm, PGMI_K_EMBED, 0, 0);
        launch_mpnn_graph(m->X, m->mask, L, K, m->E_idx, m->Dnb, st);
        launch_mpnn_edge_feat(m->X, m->ridx, m->chain, m->E_idx, m->Dnb, m->Wpos, m->bpos, m->Wt, m->nEw, m->nEb, L, K, m->E, st);
        rc = launch_gemm_f32(m->E, m->We.w, m->We.b, nullptr, m->hE, (int)LK, H, H, EPI_NONE, st);
        if (!rc && hipMemsetAsync(m->hV, 0, (size_t)L * H * 4, st) != hipSuccess) { set_error("hipMemsetAsync failed"); rc = PGMI_EHIP; }
        for (size_t l = 0; l < m->enc.size() && !rc; ++l) {
            const MpnnEnc& e = m->enc[l];
            rc = mpnn_edge_mlp(m, e.W1, e.W2, e.W3, nullptr, m->t1);
            if (rc) break;
            launch_mpnn_edge_sum(m->t1, m->mask, m->E_idx, L, K, m->n1, st);
            launch_mpnn_add_ln(m->hV, L, m->n1, nullptr, 0.0f, 1.0f, e.n1w, e.n1b, nullptr, L, L, m->n2, st);
            rc = mpnn_ffn(m, e.Win, e.Wout, e.n2w, e.n2b, m->n2, m->nf, m->n1, m->hV, L, false);
            if (rc) break;
            rc = mpnn_edge_mlp(m, e.W11, e.W12, e.W13, m->hE, m->t1);
            if (rc) break;
            launch_mpnn_add_ln(m->t1, (int64_t)LK, nullptr, nullptr, 0.0f, 1.0f, e.n3w, e.n3b, nullptr, L, (int64_t)LK, m->hE, st);
        }
        // the mutant-independent pieces of every decoder layer
        for (size_t l = 0; l < m->dec.size() && !rc; ++l) {
            MpnnDec& d = m->dec[l];
            rc = launch_gemm_f32(m->hE, d.W1b, nullptr, nullptr, d.Ep, (int)LK, H, H, EPI_NONE, st);
            if (!rc) rc = launch_gemm_f32(m->hV, d.Wap + (size_t)H * H, nullptr, nullptr, d.Penc, L, H, H, EPI_NONE, st);
        }
        if (!rc) rc = launch_gemm_f32(m->hV, m->dec[0].Wap, m->dec[0].bap, nullptr, m->AP0, L, 2 * H, H, EPI_NONE, st);
    }
    // always reached once a copy may be in flight: the caller's arrays are free to go when this returns
    rc = side_sync(pm, rc, "ProteinMPNN structure pass");
    if (rc) m->L = 0;
    return rc;
}

static int mpnn_per_chunk(const pgmi_mpnn* m, int B) {
    long long rows = 32768;
    if (g_mpnn_max_rows > 0) rows = g_mpnn_max_rows;
    return (int)std::min<long long>(std::max<long long>(1, rows / m->L), B);
}

// mutants [b0, b0 + bc): the decoder; lp_host (nullable) receives [bc][L][21], the scores land in m->score[b0 ..]
static int mpnn_chunk(pgmi_mpnn* m, const uint8_t* S, const int32_t* rank, int b0, int bc, float* lp_host) {
    pgmi_model* pm = &m->pm;
    hipStream_t st = pm->stream;
    const int L = m->L, K = m->K;
    const int64_t R = (int64_t)bc * L;
    PGMI_HIP(hipMemcpyAsync(m->S, S + (size_t)b0 * L, (size_t)R, hipMemcpyHostToDevice, st));
    PGMI_HIP(hipMemcpyAsync(m->rank, rank + (size_t)b0 * L, (size_t)R * 4, hipMemcpyHostToDevice, st));
    int rc = PGMI_OK;
    for (size_t l = 0; l < m->dec.size() && !rc; ++l) {
        const MpnnDec& d = m->dec[l];
        const bool first = l == 0;
        {
            const int rows16 = (K + 15) / 16 * 16;
            ProfScope p(pm, PGMI_K_ATTENTION, 2.0 * R * rows16 * H * H, 0);
            rc = launch_mpnn_dec_edge(d.Ep, d.T, d.Penc, first ? m->AP0 : m->AP, first ? 0 : (int64_t)L * 2 * H, d.W2.w, d.W2.b, m->E_idx,
                                      m->mask, m->S, m->rank, bc, L, K, m->sum, st);
        }
        if (rc) break;
        {
            ProfScope p(pm, PGMI_K_GEMM_OUT, 2.0 * R * H * H, 0);
            rc = launch_gemm_f32(m->sum, d.W3.w, nullptr, nullptr, m->tmp, (int)R, H, H, EPI_NONE, st);
        }
        if (rc) break;
        {   // h1 = LayerNorm1(h_V + (W3 sum + K b3) / 30); layer 0 reads the encoder's h_V for every mutant
            ProfScope p(pm, PGMI_K_LAYERNORM, 0, (double)R * H * 12);
            launch_mpnn_add_ln(first ? m->hV : m->h, first ? (int64_t)L : R, m->tmp, d.W3.b, (float)K, 30.0f, d.n1w, d.n1b, nullptr, L, R, m->h1, st);
        }
        rc = mpnn_ffn(m, d.Win, d.Wout, d.n2w, d.n2b, m->h1, m->ffn, m->tmp, m->h, R, true);
        if (!rc && l + 1 < m->dec.size()) {
            const MpnnDec& nx = m->dec[l + 1];
            ProfScope p(pm, PGMI_K_GEMM_QKV, 2.0 * R * H * 2 * H, 0);
            rc = launch_gemm_f32(m->h, nx.Wap, nx.bap, nullptr, m->AP, (int)R, 2 * H, H, EPI_NONE, st);
        }
    }
    if (rc) return rc;
    {
        ProfScope p(pm, PGMI_K_HEAD, 2.0 * R * H * V, 0);
        launch_mpnn_head(m->h, m->Whead.w, m->Whead.b, m->S, R, lp_host ? m->lp : nullptr, m->nll, st);
    }
    {
        ProfScope p(pm, PGMI_K_SCORE, 0, 0);
        launch_mpnn_score(m->nll, m->mask, bc, L, m->score + b0, st);
    }
    PGMI_HIP(hipGetLastError());
    if (lp_host) {   // the next chunk overwrites m->lp
        PGMI_HIP(hipMemcpyAsync(lp_host, m->lp, (size_t)R * V * 4, hipMemcpyDeviceToHost, st));
        PGMI_HIP(hipStreamSynchronize(st));
    }
    // the chunk's S / rank buffers are reused by the next chunk's copies: they are stream-ordered behind these kernels
    return PGMI_OK;
}

static int mpnn_run(pgmi_mpnn* m, const uint8_t* S, const int32_t* rank, int B, float* lp, double* scores) {
    if (!m || !S || !rank || B <= 0) { set_error("bad argument"); return PGMI_EINVAL; }
    if (m->L <= 0) { set_error("ProteinMPNN: no structure set (pgmi_mpnn_set_structure)"); return PGMI_EINVAL; }
    const int L = m->L;
    for (size_t t = 0; t < (size_t)B * L; ++t)
        if (S[t] >= V) { set_error("ProteinMPNN: residue code %d at element %zu (0 .. 20 are valid)", (int)S[t], t); return PGMI_EINVAL; }
    PGMI_HIP(hipSetDevice(m->pm.device));
    pgmi_model* pm = &m->pm;
    const int per = mpnn_per_chunk(m, B);
    const size_t R = (size_t)per * L;
    int rc = reserve_all(pm, m->S, R, m->rank, R, m->sum, R * H, m->tmp, R * H, m->h1, R * H, m->h, R * H, m->ffn, R * FF, m->AP, R * 2 * H,
                         m->nll, R, m->score, (size_t)B);
    if (!rc && lp) rc = m->lp.reserve(pm, R * V);
    if (rc) return rc;
    int chunks = 0;
    for (int b0 = 0; b0 < B && !rc; b0 += per) {
        const int bc = std::min(per, B - b0);
        rc = mpnn_chunk(m, S, rank, b0, bc, lp ? lp + (size_t)b0 * L * V : nullptr);
        if (!rc && pm->prof && (++chunks & 15) == 15) rc = prof_drain(pm);
    }
    if (!rc && scores && hipMemcpyAsync(scores, m->score, (size_t)B * 8, hipMemcpyDeviceToHost, pm->stream) != hipSuccess) rc = PGMI_EHIP;
    return side_sync(pm, rc, "ProteinMPNN decoder");
}

}  // namespace pgmi

extern "C" {

int64_t pgmi_mpnn_weight_count(const pgmi_mpnn_config* cfg) {
    if (mpnn_check(cfg)) return -1;
    return mpnn_count(cfg);
}

int pgmi_mpnn_create(const pgmi_mpnn_config* cfg, const float* w, int64_t n_weights, int device, pgmi_mpnn** out) {
    if (!out) { set_error("null out"); return PGMI_EINVAL; }
    *out = nullptr;
    int rc = mpnn_check(cfg);
    if (rc) return rc;
    pgmi_mpnn* m = new pgmi_mpnn();
    rc = side_open(&m->pm, "ProteinMPNN", w, n_weights, mpnn_count(cfg), false, device, cfg->precision, nullptr);
    if (rc) { delete m; return rc; }
    m->cfg = *cfg;
    rc = mpnn_build(m, w, n_weights);
    if (rc) { pgmi_mpnn_destroy(m); return rc; }
    *out = m;
    return PGMI_OK;
}

void pgmi_mpnn_destroy(pgmi_mpnn* m) {
    if (!m) return;
    side_release(&m->pm, true);
    delete m;
}

pgmi_model* pgmi_mpnn_profile_model(pgmi_mpnn* m) { return m ? &m->pm : nullptr; }

int pgmi_mpnn_set_structure(pgmi_mpnn* m, const float* X, const float* mask, const int32_t* residue_idx, const int32_t* chain_label, int L) {
    if (!m || !X || !mask || !residue_idx || !chain_label) { set_error("bad argument"); return PGMI_EINVAL; }
    if (L < 1 || L > MPNN_MAX_L) { set_error("ProteinMPNN: L = %d outside 1 .. %d", L, MPNN_MAX_L); return PGMI_EINVAL; }
    for (int i = 0; i < L; ++i) {
        if (mask[i] != 0.0f && mask[i] != 1.0f) { set_error("ProteinMPNN: mask[%d] is neither 0 nor 1", i); return PGMI_EINVAL; }
        for (int c = 0; c < 12; ++c)
            if (!std::isfinite(X[(size_t)i * 12 + c])) { set_error("ProteinMPNN: coordinate of residue %d is not finite (missing atoms are 0 with mask 0)", i); return PGMI_EINVAL; }
    }
    PGMI_HIP(hipSetDevice(m->pm.device));
    return mpnn_structure(m, X, mask, residue_idx, chain_label, L);
}

int pgmi_mpnn_graph(pgmi_mpnn* m, int32_t* E_idx, float* E) {
    if (!m || m->L <= 0) { set_error("ProteinMPNN: no structure set"); return PGMI_EINVAL; }
    PGMI_HIP(hipSetDevice(m->pm.device));
    const size_t LK = (size_t)m->L * m->K;
    if (E_idx) PGMI_HIP(hipMemcpy(E_idx, m->E_idx, LK * 4, hipMemcpyDeviceToHost));
    if (E) PGMI_HIP(hipMemcpy(E, m->E, LK * H * 4, hipMemcpyDeviceToHost));
    return PGMI_OK;
}

int pgmi_mpnn_encoder(pgmi_mpnn* m, float* h_V, float* h_E) {
    if (!m || m->L <= 0) { set_error("ProteinMPNN: no structure set"); return PGMI_EINVAL; }
    PGMI_HIP(hipSetDevice(m->pm.device));
    if (h_V) PGMI_HIP(hipMemcpy(h_V, m->hV, (size_t)m->L * H * 4, hipMemcpyDeviceToHost));
    if (h_E) PGMI_HIP(hipMemcpy(h_E, m->hE, (size_t)m->L * m->K * H * 4, hipMemcpyDeviceToHost));
    return PGMI_OK;
}

int pgmi_mpnn_log_probs(pgmi_mpnn* m, const uint8_t* S, const int32_t* rank, int B, float* out) {
    if (!out) { set_error("bad argument"); return PGMI_EINVAL; }
    return mpnn_run(m, S, rank, B, out, nullptr);
}

int pgmi_mpnn_scores(pgmi_mpnn* m, const uint8_t* S, const int32_t* rank, int B, double* out) {
    if (!out) { set_error("bad argument"); return PGMI_EINVAL; }
    return mpnn_run(m, S, rank, B, nullptr, out);
}

}  // extern "C"
