// CARP entries of the C ABI (include/pgmi.h, CARP section): the blob walk, the ByteNet forward over packed sequences and the three
// scoring entries.  The kernels of a block that are not GEMMs are in conv_f16.hip.
// Every kernel of the forward is row-local, or (the convolution) local to a row's own segment, and a GEMM output element's sum does not
// depend on the launch's row count: a sequence computes the same bits alone, inside a batch and under any row cap.  Chunks are cut
// between sequences only, so no chunk ever needs a halo.
#include "model.h"

namespace pgmi {

constexpr long long CARP_ROWS_DEFAULT = 16384, CARP_ROWS_LIMIT = 1 << 20;
constexpr int CARP_MAX_LEN = 1 << 20;

struct CarpBlock {
    float *ln1_w, *ln1_b, *b1, *ln2_w, *ln2_b, *bc, *ln3_w, *ln3_b, *b2;
    float *w1 = nullptr, *wc = nullptr, *w2 = nullptr;      // fp32 mode: [dh][D], [dh][taps dh], [D][dh]
    W16 w116, wc16, w216;
    int dilation = 1;
};

}  // namespace pgmi

struct pgmi_carp {
    pgmi_model pm;                       // device, stream, allocation pool and profiling state (pgmi_carp_profile_model)
    pgmi_carp_config cfg;
    int D = 0, dh = 0, V = 0, taps = 0;
    float *table = nullptr, *lnf_w = nullptr, *lnf_b = nullptr, *dec_w = nullptr, *dec_b = nullptr;
    std::vector<CarpBlock> blocks;
    // workspace of a chunk of R rows: residual stream x [R][D]; t [R][dh] (PFF1's and the convolution's output); the operand of the
    // next product hs (split rows, or fp32 rows: 4 bytes per element either way) [R][max(D, dh)]; col: the fp32 convolution's im2col
    int32_t* nonfinite = nullptr;
    DevBuf<int32_t> tokens, seg_off, row_idx;
    DevBuf<float> x, t, g, col, lp, terms;
    DevBuf<uint32_t> hs;
    DevBuf<double> sums;
};

namespace pgmi {

static int carp_check(const pgmi_carp_config* c) {
    if (!c) { set_error("null config"); return PGMI_EINVAL; }
    if (c->abi_version != PGMI_ABI_VERSION) { set_error("ABI version mismatch: got %d, library is %d", c->abi_version, PGMI_ABI_VERSION); return PGMI_EINVAL; }
    if (c->d_model < 32 || c->d_model % 32 || c->d_model > 5120) { set_error("CARP: d_model %d must be a multiple of 32 in 32 .. 5120", c->d_model); return PGMI_EINVAL; }
    if (c->d_hidden < 32 || c->d_hidden % 32 || c->d_hidden > 5120) { set_error("CARP: d_hidden %d must be a multiple of 32 in 32 .. 5120", c->d_hidden); return PGMI_EINVAL; }
    if (c->n_layers < 1 || c->n_layers > 1024) { set_error("CARP: %d layers", c->n_layers); return PGMI_EINVAL; }
    if (c->kernel_size < 1 || c->kernel_size > 15 || !(c->kernel_size & 1)) { set_error("CARP: kernel size %d (odd, 1 .. 15)", c->kernel_size); return PGMI_EINVAL; }
    if (c->r < 1 || c->r > (1 << 16) || (c->r & (c->r - 1))) { set_error("CARP: r = %d must be a power of two up to 65536", c->r); return PGMI_EINVAL; }
    if (c->vocab < 2 || c->vocab > 64) { set_error("CARP: vocabulary %d outside 2 .. 64", c->vocab); return PGMI_EINVAL; }
    if (c->mask_id < 0 || c->mask_id >= c->vocab) { set_error("CARP: mask id %d outside the vocabulary of %d", c->mask_id, c->vocab); return PGMI_EINVAL; }
    if (c->precision != PGMI_PREC_FP32 && c->precision != PGMI_PREC_F16X3) { set_error("CARP runs in precision f16x3 or fp32"); return PGMI_EINVAL; }
    if (c->max_rows < 0) { set_error("CARP: negative max_rows"); return PGMI_EINVAL; }
    if (!(c->ln_eps > 0.0f) || !std::isfinite(c->ln_eps)) { set_error("CARP: ln_eps must be positive"); return PGMI_EINVAL; }
    return PGMI_OK;
}

static int64_t carp_count(const pgmi_carp_config* c) {
    const int64_t D = c->d_model, H = c->d_hidden, V = c->vocab, k = c->kernel_size;
    const int64_t block = 2 * D + (H * D + H) + 2 * H + (H * k * H + H) + 2 * H + (D * H + D);
    return V * D + c->n_layers * block + 2 * D + V * D + V;
}

static int carp_build(pgmi_carp* m, const float* w, int64_t n_weights) {
    const size_t D = m->D, H = m->dh, V = m->V, k = m->taps;
    int n_dil = 1;
    while ((1 << (n_dil - 1)) < m->cfg.r) ++n_dil;           // log2(r) + 1 dilations per cycle
    BlobCursor c(&m->pm, w, n_weights);
    c.upload(&m->table, V * D);
    m->blocks.resize(m->cfg.n_layers);
    for (int l = 0; l < m->cfg.n_layers; ++l) {
        CarpBlock& b = m->blocks[l];
        b.dilation = 1 << (l % n_dil);
        c.upload(&b.ln1_w, D); c.upload(&b.ln1_b, D);
        c.linear(&b.w1, &b.w116, H * D, D); c.upload(&b.b1, H);
        c.upload(&b.ln2_w, H); c.upload(&b.ln2_b, H);
        c.linear(&b.wc, &b.wc16, H * k * H, k * H); c.upload(&b.bc, H);
        c.upload(&b.ln3_w, H); c.upload(&b.ln3_b, H);
        c.linear(&b.w2, &b.w216, D * H, H); c.upload(&b.b2, D);
    }
    c.upload(&m->lnf_w, D); c.upload(&m->lnf_b, D);
    c.upload(&m->dec_w, V * D); c.upload(&m->dec_b, V);
    int rc = c.finish();
    if (!rc) rc = dev_alloc(m->pm.allocs, &m->nonfinite, 1);
    if (!rc) PGMI_HIP(hipMemset(m->nonfinite, 0, 4));
    return rc;
}

static int carp_rows_cap(const pgmi_carp* m) {
    const long long r = m->cfg.max_rows > 0 ? m->cfg.max_rows : CARP_ROWS_DEFAULT;
    return (int)std::min(std::max(r, 1LL), CARP_ROWS_LIMIT);
}

static int carp_workspace(pgmi_carp* m, size_t R, size_t n_seq) {
    pgmi_model* pm = &m->pm;
    const size_t D = m->D, H = m->dh, W = std::max(D, H);
    int rc = reserve_all(pm, m->tokens, R, m->seg_off, n_seq + 1, m->row_idx, n_seq, m->x, R * D, m->t, R * H, m->g, R * D, m->hs, R * W,
                         m->lp, R * (size_t)m->V, m->terms, R, m->sums, n_seq);
    if (!rc && m->cfg.precision == PGMI_PREC_FP32) rc = m->col.reserve(pm, R * H * (size_t)m->taps);
    return rc;
}

// The blocks on the R packed rows of m->tokens (n_seq sequences, m->seg_off): m->x = the rows in front of last_norm.
static int carp_forward(pgmi_carp* m, int R, int n_seq) {
    pgmi_model* pm = &m->pm;
    hipStream_t st = pm->stream;
    const int D = m->D, H = m->dh, k = m->taps;
    const float eps = m->cfg.ln_eps;
    const bool f32 = m->cfg.precision == PGMI_PREC_FP32;
    unsigned short* h16 = reinterpret_cast<unsigned short*>(m->hs.p);
    float* h32 = reinterpret_cast<float*>(m->hs.p);
    auto ln_gelu = [&](const float* src, const float* w, const float* b, int width) {
        ProfScope p(pm, PGMI_K_LAYERNORM, 0, (double)R * width * 8);
        return f32 ? launch_ln_gelu32(src, w, b, R, width, eps, h32, st) : launch_ln_gelu16(src, w, b, R, width, eps, h16, st);
    };
    auto gemm = [&](int cls, const float* w32, const W16& w16, const float* bias, const float* residual, float* out, int N, int K) {
        ProfScope p(pm, cls, 2.0 * R * (double)N * K, 0);
        return linear(pm, h32, h16, w32, w16, bias, residual, out, nullptr, R, N, K, EPI_NONE);
    };
    {
        ProfScope p(pm, PGMI_K_EMBED, 0, (double)R * D * 8);
        launch_gather_rows(m->table, m->tokens, R, D, m->x, st);
    }
    int rc;
    for (size_t l = 0; l < m->blocks.size(); ++l) {
        const CarpBlock& b = m->blocks[l];
        if ((rc = ln_gelu(m->x, b.ln1_w, b.ln1_b, D))) return rc;
        if ((rc = gemm(PGMI_K_GEMM_FC1, b.w1, b.w116, b.b1, nullptr, m->t, H, D))) return rc;
        if ((rc = ln_gelu(m->t, b.ln2_w, b.ln2_b, H))) return rc;
        {
            ProfScope p(pm, PGMI_K_ATTENTION, 2.0 * R * (double)H * k * H, 0);
            rc = f32 ? launch_dilated_conv32(h32, b.wc, b.bc, m->seg_off, n_seq, R, H, k, b.dilation, m->col, m->t, st)
                     : launch_dilated_conv16(h16, b.wc16.p, b.wc16.out_scale, b.bc, m->seg_off, n_seq, R, H, k, b.dilation, m->t, st);
        }
        if (rc) return rc;
        if ((rc = ln_gelu(m->t, b.ln3_w, b.ln3_b, H))) return rc;
        if ((rc = gemm(PGMI_K_GEMM_FC2, b.w2, b.w216, b.b2, m->x, m->x, D, H))) return rc;
        if (pm->prof && (l & 7) == 7 && (rc = prof_drain(pm))) return rc;
    }
    return PGMI_OK;
}

// last_norm, decoder and log-softmax on n rows: rows row_idx[i] of m->x (on the device; nullptr: the first n rows) -> m->lp [n][V]
static int carp_head(pgmi_carp* m, const int32_t* row_idx, int n) {
    pgmi_model* pm = &m->pm;
    ProfScope p(pm, PGMI_K_HEAD, 2.0 * n * (double)m->D * m->V, 0);
    const float* src = m->x;
    if (row_idx) {
        launch_gather_rows(m->x, row_idx, n, m->D, m->g, pm->stream);
        src = m->g;
    }
    launch_layernorm(src, m->lnf_w, m->lnf_b, n, m->D, m->cfg.ln_eps, m->g, pm->stream);
    launch_vocab_logsoftmax(m->g, m->dec_w, m->dec_b, n, m->D, m->V, m->lp, m->nonfinite, pm->stream);
    return PGMI_OK;
}

// after the chunk's copies are queued: waits for the stream; PGMI_EOVERFLOW when the head saw a non-finite value
static int carp_finish(pgmi_carp* m) {
    int32_t flag = 0;
    PGMI_HIP(hipMemcpyAsync(&flag, m->nonfinite, 4, hipMemcpyDeviceToHost, m->pm.stream));
    const int rc = side_sync(&m->pm, PGMI_OK, "CARP forward");
    if (rc || !flag) return rc;
    PGMI_HIP(hipMemsetAsync(m->nonfinite, 0, 4, m->pm.stream));
    return overflow_error(m->cfg.precision);
}

static int carp_check_batch(const pgmi_carp* m, const int32_t* tokens, const int32_t* lens, int B, int64_t* total) {
    if (!m || !tokens || !lens || B < 1) { set_error("bad argument"); return PGMI_EINVAL; }
    int64_t n = 0;
    for (int b = 0; b < B; ++b) {
        if (lens[b] < 1 || lens[b] > CARP_MAX_LEN) { set_error("CARP: sequence %d has %d tokens (1 .. %d)", b, (int)lens[b], CARP_MAX_LEN); return PGMI_EINVAL; }
        n += lens[b];
    }
    if (n > (1LL << 31) - 1) { set_error("CARP: %lld tokens in one call", (long long)n); return PGMI_EINVAL; }
    for (int64_t i = 0; i < n; ++i)
        if (tokens[i] < 0 || tokens[i] >= m->V) { set_error("CARP: token %d at element %lld (0 .. %d are valid)", (int)tokens[i], (long long)i, m->V - 1); return PGMI_EINVAL; }
    *total = n;
    return PGMI_OK;
}

// Packed sequences through the forward in chunks cut between sequences: out (nullable) [sum lens][V] log-probabilities; sum
// (nullable) [B] = per sequence, the sum of log p(its own token).
static int carp_score_packed(pgmi_carp* m, const int32_t* tokens, const int32_t* lens, int B, float* out, double* sum) {
    PGMI_HIP(hipSetDevice(m->pm.device));
    hipStream_t st = m->pm.stream;
    const int cap = carp_rows_cap(m);
    std::vector<int32_t> off;
    int64_t row0 = 0;
    for (int b0 = 0; b0 < B;) {
        int b1 = b0;
        int64_t R = 0;
        off.assign(1, 0);
        while (b1 < B && (b1 == b0 || R + lens[b1] <= cap)) { R += lens[b1]; off.push_back((int32_t)R); ++b1; }
        const int bc = b1 - b0;
        int rc = carp_workspace(m, (size_t)R, (size_t)bc);
        if (rc) return rc;
        PGMI_HIP(hipMemcpyAsync(m->tokens, tokens + row0, (size_t)R * 4, hipMemcpyHostToDevice, st));
        PGMI_HIP(hipMemcpyAsync(m->seg_off, off.data(), off.size() * 4, hipMemcpyHostToDevice, st));
        if ((rc = carp_forward(m, (int)R, bc))) return rc;
        if ((rc = carp_head(m, nullptr, (int)R))) return rc;
        if (out) PGMI_HIP(hipMemcpyAsync(out + (size_t)row0 * m->V, m->lp, (size_t)R * m->V * 4, hipMemcpyDeviceToHost, st));
        if (sum) {
            ProfScope p(&m->pm, PGMI_K_SCORE, 0, 0);
            launch_pppl_pick(m->lp, m->tokens, (int)R, m->V, m->terms, st);
            launch_seq_sum(m->terms, m->seg_off, bc, m->sums, st);
        }
        if (sum) PGMI_HIP(hipMemcpyAsync(sum + b0, m->sums, (size_t)bc * 8, hipMemcpyDeviceToHost, st));
        if ((rc = carp_finish(m))) return rc;             // the chunk's host arrays and the workspace are reused by the next chunk
        row0 += R;
        b0 = b1;
    }
    return PGMI_OK;
}

}  // namespace pgmi

extern "C" {

int64_t pgmi_carp_weight_count(const pgmi_carp_config* cfg) {
    if (carp_check(cfg)) return -1;
    return carp_count(cfg);
}

int pgmi_carp_create(const pgmi_carp_config* cfg, const float* w, int64_t n_weights, int device, pgmi_carp** out) {
    if (!out) { set_error("null out"); return PGMI_EINVAL; }
    *out = nullptr;
    int rc = carp_check(cfg);
    if (rc) return rc;
    pgmi_carp* m = new pgmi_carp();
    rc = side_open(&m->pm, "CARP", w, n_weights, carp_count(cfg), true, device, cfg->precision, nullptr);
    if (rc) { delete m; return rc; }
    m->cfg = *cfg;
    m->D = cfg->d_model; m->dh = cfg->d_hidden; m->V = cfg->vocab; m->taps = cfg->kernel_size;
    rc = carp_build(m, w, n_weights);
    if (rc) { pgmi_carp_destroy(m); return rc; }
    *out = m;
    return PGMI_OK;
}

void pgmi_carp_destroy(pgmi_carp* m) {
    if (!m) return;
    side_release(&m->pm, true);
    delete m;
}

pgmi_model* pgmi_carp_profile_model(pgmi_carp* m) { return m ? &m->pm : nullptr; }

int pgmi_carp_token_logprobs(pgmi_carp* m, const int32_t* tokens, const int32_t* lens, int B, float* out) {
    int64_t n = 0;
    int rc = carp_check_batch(m, tokens, lens, B, &n);
    if (rc) return rc;
    if (!out) { set_error("null out"); return PGMI_EINVAL; }
    return carp_score_packed(m, tokens, lens, B, out, nullptr);
}

int pgmi_carp_sequence_loglik(pgmi_carp* m, const int32_t* tokens, const int32_t* lens, int B, double* out) {
    int64_t n = 0;
    int rc = carp_check_batch(m, tokens, lens, B, &n);
    if (rc) return rc;
    if (!out) { set_error("null out"); return PGMI_EINVAL; }
    return carp_score_packed(m, tokens, lens, B, nullptr, out);
}

int pgmi_carp_masked_logprobs(pgmi_carp* m, const int32_t* wt, int L, const int32_t* positions, int n_pos, float* out) {
    if (!m || !wt || !positions || !out) { set_error("bad argument"); return PGMI_EINVAL; }
    if (L < 1 || L > CARP_MAX_LEN) { set_error("CARP: sequence of %d tokens (1 .. %d)", L, CARP_MAX_LEN); return PGMI_EINVAL; }
    if (n_pos < 1) { set_error("CARP: empty position list"); return PGMI_EINVAL; }
    for (int i = 0; i < L; ++i)
        if (wt[i] < 0 || wt[i] >= m->V) { set_error("CARP: token %d at element %d (0 .. %d are valid)", (int)wt[i], i, m->V - 1); return PGMI_EINVAL; }
    for (int i = 0; i < n_pos; ++i)
        if (positions[i] < 0 || positions[i] >= L) { set_error("CARP: position %d (entry %d) outside the sequence of %d tokens", (int)positions[i], i, L); return PGMI_EINVAL; }
    PGMI_HIP(hipSetDevice(m->pm.device));
    hipStream_t st = m->pm.stream;
    const int per = std::max(1, carp_rows_cap(m) / L);     // masked copies per chunk
    std::vector<int32_t> tok, off, idx;
    for (int p0 = 0; p0 < n_pos; p0 += per) {
        const int bc = std::min(per, n_pos - p0);
        const size_t R = (size_t)bc * L;
        tok.resize(R); off.resize(bc + 1); idx.resize(bc);
        for (int i = 0; i < bc; ++i) {
            memcpy(&tok[(size_t)i * L], wt, (size_t)L * 4);
            tok[(size_t)i * L + positions[p0 + i]] = m->cfg.mask_id;
            off[i] = i * L;
            idx[i] = i * L + positions[p0 + i];
        }
        off[bc] = bc * L;
        int rc = carp_workspace(m, R, (size_t)bc);
        if (rc) return rc;
        PGMI_HIP(hipMemcpyAsync(m->tokens, tok.data(), R * 4, hipMemcpyHostToDevice, st));
        PGMI_HIP(hipMemcpyAsync(m->seg_off, off.data(), off.size() * 4, hipMemcpyHostToDevice, st));
        PGMI_HIP(hipMemcpyAsync(m->row_idx, idx.data(), idx.size() * 4, hipMemcpyHostToDevice, st));
        if ((rc = carp_forward(m, (int)R, bc))) return rc;
        if ((rc = carp_head(m, m->row_idx, bc))) return rc;
        PGMI_HIP(hipMemcpyAsync(out + (size_t)p0 * m->V, m->lp, (size_t)bc * m->V * 4, hipMemcpyDeviceToHost, st));
        if ((rc = carp_finish(m))) return rc;
    }
    return PGMI_OK;
}

int pgmi_op_dilated_conv(int device, int precision, const float* x, const float* W, const float* bias, const int32_t* seg_off, int n_seg,
                         int C, int taps, int dilation, float* out) {
    if (!x || !W || !bias || !seg_off || !out || n_seg < 1) { set_error("bad argument"); return PGMI_EINVAL; }
    if (precision != PGMI_PREC_FP32 && precision != PGMI_PREC_F16X3) { set_error("dilated conv op: precision f16x3 or fp32"); return PGMI_EINVAL; }
    if (C < 32 || C % 32 || C > 8192 || taps < 1 || taps > 15 || !(taps & 1) || dilation < 1) { set_error("dilated conv op: C = %d, %d taps, dilation %d", C, taps, dilation); return PGMI_EINVAL; }
    if (seg_off[0] != 0) { set_error("dilated conv op: seg_off[0] must be 0"); return PGMI_EINVAL; }
    for (int s = 0; s < n_seg; ++s)
        if (seg_off[s + 1] <= seg_off[s]) { set_error("dilated conv op: segment %d is empty or out of order", s); return PGMI_EINVAL; }
    const size_t M = (size_t)seg_off[n_seg], K = (size_t)taps * C;
    if (M > (1u << 20)) { set_error("dilated conv op: %zu rows", M); return PGMI_EINVAL; }
    OpScope s("dilated conv op", device);
    const bool f32 = precision == PGMI_PREC_FP32;
    float* dx = s.up(x, M * C);
    float* db = s.up(bias, (size_t)C);
    int32_t* dseg = s.up(seg_off, (size_t)n_seg + 1);
    float* dy = s.alloc<float>(M * C);
    float* dw = f32 ? s.up(W, (size_t)C * K) : nullptr;
    float* col = f32 ? s.alloc<float>(M * K) : nullptr;
    const W16 w16 = f32 ? W16() : s.w16(W, (size_t)C * K, K, precision);
    unsigned short* x16 = f32 ? nullptr : s.alloc<unsigned short>(M * C * 2);
    if (s.rc) return s.rc;
    if (f32) {
        s.rc = launch_dilated_conv32(dx, dw, db, dseg, n_seg, (int64_t)M, C, taps, dilation, col, dy, nullptr);
    } else {
        launch_split16(dx, (int64_t)(M * C), 1.0f, 2, C, x16, nullptr);
        s.rc = launch_dilated_conv16(x16, w16.p, w16.out_scale, db, dseg, n_seg, (int64_t)M, C, taps, dilation, dy, nullptr);
    }
    s.sync();
    s.down(out, dy, M * C);
    return s.rc;
}

int pgmi_bench_dilated_conv(int device, int M, int n_seg, int C, int taps, int dilation, int iters, double* ms_per_launch) {
    if (!ms_per_launch || M < 1 || n_seg < 1 || M % n_seg || iters < 1 || C < 32 || C % 32 || C > 8192 || taps < 1 || taps > 15 || !(taps & 1) ||
        dilation < 1) { set_error("bad argument"); return PGMI_EINVAL; }
    OpScope s("dilated conv bench", device);
    if (s.rc) return s.rc;
    const size_t n = (size_t)M * C, K = (size_t)taps * C, blk = std::min(n, (size_t)1 << 22);
    // seeded values of the magnitudes the block sees (GELU outputs, weights ~ 1 / sqrt K); x repeats a 4 M-element block
    std::vector<float> hx(blk), hw((size_t)C * K), hb(C, 0.01f);
    std::vector<int32_t> seg(n_seg + 1);
    uint32_t st = 12345u;
    auto rnd = [&]() { st = st * 1664525u + 1013904223u; return (float)(int32_t)st * (1.0f / 2147483648.0f); };
    for (float& v : hx) v = 1.5f * rnd();
    for (float& v : hw) v = rnd() * 1.7f / sqrtf((float)K);
    for (int i = 0; i <= n_seg; ++i) seg[i] = i * (M / n_seg);
    float* dx = s.alloc<float>(n);
    float* db = s.up(hb);
    int32_t* dseg = s.up(seg);
    float* dy = s.alloc<float>(n);
    unsigned short* x16 = s.alloc<unsigned short>(2 * n);
    const W16 w16 = s.w16(hw.data(), hw.size(), K);
    for (size_t o = 0; o < n && !s.rc; o += blk) s.hip(hipMemcpy(dx + o, hx.data(), std::min(blk, n - o) * 4, hipMemcpyHostToDevice));
    if (s.rc) return s.rc;
    auto launch = [&]() { return launch_dilated_conv16(x16, w16.p, w16.out_scale, db, dseg, n_seg, M, C, taps, dilation, dy, nullptr); };
    launch_split16(dx, (int64_t)n, 1.0f, 2, C, x16, nullptr);
    for (int i = 0; i < 2 && !s.rc; ++i) s.rc = launch();
    const double ms = s.time_ms(launch, iters);
    if (!s.rc) *ms_per_launch = ms;
    return s.rc;
}

int pgmi_op_ln_gelu(int device, int precision, const float* x, const float* w, const float* b, int rows, int D, float eps, float* y) {
    if (!x || !w || !b || !y || rows < 1 || rows > (1 << 20)) { set_error("bad argument"); return PGMI_EINVAL; }
    if (precision != PGMI_PREC_FP32 && precision != PGMI_PREC_F16X3) { set_error("ln_gelu op: precision f16x3 or fp32"); return PGMI_EINVAL; }
    if (D < 32 || D % 32 || D > 5120) { set_error("ln_gelu op: D = %d must be a multiple of 32 in 32 .. 5120", D); return PGMI_EINVAL; }
    OpScope s("ln_gelu op", device);
    const bool f32 = precision == PGMI_PREC_FP32;
    const size_t n = (size_t)rows * D;
    float* dx = s.up(x, n);
    float* dw = s.up(w, (size_t)D);
    float* db = s.up(b, (size_t)D);
    float* dy = f32 ? s.alloc<float>(n) : nullptr;
    unsigned short* y16 = f32 ? nullptr : s.alloc<unsigned short>(2 * n, 0xFF);      // an element the kernel skips shows as NaN
    if (!s.rc) s.rc = f32 ? launch_ln_gelu32(dx, dw, db, rows, D, eps, dy, nullptr) : launch_ln_gelu16(dx, dw, db, rows, D, eps, y16, nullptr);
    s.sync();
    if (f32) s.down(y, dy, n);
    else s.planes(y, y16, (size_t)rows, (size_t)D);
    return s.rc;
}

}  // extern "C"
