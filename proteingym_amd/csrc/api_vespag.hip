// VespaG entries of the C ABI (include/pgmi.h, VespaG section): the packed residue rows of a library of sequences
// through an ESM2 model, the head's handle and blob walk, the head on packed rows, the op entry.  The two kernels that are not GEMMs
// are in vespag.hip.
// Packed rows: the library runs in descending length, in chunks of rows_per_chunk sequences padded to the chunk's longest (kv_len masks
// the <pad> keys, as in pgmi_pppl_run); the chunk's residue rows are run_encoder's keep list, so the last layer's out-projection and
// FFN see no <cls>, <eos> or <pad> row and m->x comes back compacted; emb_layer_norm_after, then launch_packed_scatter puts each row at
// its place in the caller's order.  Every kernel on the way computes a row (the attention: a query) from its own sequence's rows, and
// none picks a summation order from the batch or the pad length; at the shapes of tests/test_gpu_vespag.py (D = 128, T <= 72) a row's
// bits are the same whatever chunk it ran in, which the test asserts.  Larger shapes were not compared bit for bit.
// Head: one GEMM over up to VESPAG_HEAD_ROWS packed rows (f16x3: on their split planes), then the row kernel.
#include "model.h"

namespace pgmi {

constexpr int VESPAG_HEAD_ROWS = 16384, VESPAG_OUT = 20;

// The order, chunks and packed places of a library (host only).
struct RowsPlan {
    std::vector<int32_t> sid;            // sequences in the order they run: descending token length, stable
    std::vector<int32_t> chunk_end;      // chunk i = sid[chunk_end[i - 1] .. chunk_end[i])
    std::vector<int64_t> packed_off;     // [n + 1]: the packed row of sequence n's first residue, in the caller's order
    int64_t tokens = 0, padded = 0;      // tokens of the library; tokens the chunks run (pads included)
};

static RowsPlan plan_rows(const int64_t* seq_off, int64_t n_seq, int cap) {
    RowsPlan p;
    const int J = (int)n_seq;
    auto len_of = [&](int32_t n) { return seq_off[n + 1] - seq_off[n]; };
    p.sid.resize(J);
    for (int j = 0; j < J; ++j) p.sid[j] = j;
    std::stable_sort(p.sid.begin(), p.sid.end(), [&](int32_t a, int32_t b) { return len_of(a) > len_of(b); });
    p.packed_off.resize((size_t)J + 1);
    p.packed_off[0] = 0;
    for (int n = 0; n < J; ++n) p.packed_off[n + 1] = p.packed_off[n] + len_of(n) - 2;
    for (int j0 = 0; j0 < J;) {
        const int64_t T = len_of(p.sid[j0]);
        const int64_t per = std::max<int64_t>(1, cap / roundup32(T));              // rows_per_chunk's rule on `cap` rows
        const int j1 = (int)std::min<int64_t>(J, j0 + per);
        p.chunk_end.push_back(j1);
        p.padded += (j1 - j0) * T;
        j0 = j1;
    }
    p.tokens = seq_off[J];
    return p;
}

static int check_seq_off(const int64_t* seq_off, int64_t n_seq) {
    if (!seq_off || n_seq <= 0 || n_seq > 0x7fffffff) { set_error("bad argument"); return PGMI_EINVAL; }
    if (seq_off[0] != 0) { set_error("seq_off[0] must be 0"); return PGMI_EINVAL; }
    for (int64_t n = 0; n < n_seq; ++n) {
        const int64_t len = seq_off[n + 1] - seq_off[n];
        if (len < 3 || len > (1 << 24)) {
            set_error("packed rows: sequence %lld has %lld tokens (<cls> + at least one residue + <eos>)", (long long)n, (long long)len);
            return PGMI_EINVAL;
        }
    }
    if (seq_off[n_seq] - 2 * n_seq > 0x7fffffff) { set_error("packed rows: %lld residue rows exceed 2^31 - 1", (long long)(seq_off[n_seq] - 2 * n_seq)); return PGMI_EINVAL; }
    return PGMI_OK;
}

// the refusals of a library for `esm`, before any device work
static int check_library(const pgmi_model* esm, const uint8_t* tokens, const int64_t* seq_off, int64_t n_seq) {
    if (!esm || !tokens) { set_error("bad argument"); return PGMI_EINVAL; }
    if (esm->cfg.arch != PGMI_ARCH_ESM2) { set_error("packed rows: the model must be an ESM2 model (arch %d)", esm->cfg.arch); return PGMI_EINVAL; }
    int rc = check_seq_off(seq_off, n_seq);
    if (rc) return rc;
    int64_t Tmax = 0;
    for (int64_t n = 0; n < n_seq; ++n) {
        Tmax = std::max(Tmax, seq_off[n + 1] - seq_off[n]);
        for (int64_t i = seq_off[n]; i < seq_off[n + 1]; ++i)
            if (tokens[i] >= esm->n_token_ids || tokens[i] == PGMI_TOK_PAD) {
                set_error("token id %d invalid at sequence %lld, position %lld", (int)tokens[i], (long long)n, (long long)(i - seq_off[n]));
                return PGMI_EINVAL;
            }
    }
    if (Tmax + 31 > esm->max_rows) { set_error("T=%lld exceeds the ESM2 model's workspace rows %d", (long long)Tmax, esm->max_rows); return PGMI_EINVAL; }
    return PGMI_OK;
}

// Precision fp32 has no fp16 range to leave (check_nonfinite does not read the flag there), but a residue row may still be NaN or inf;
// pgmi_vespag_head refuses such a row on the host, so the packed route refuses it too: the scatter's flag, read as check_nonfinite reads it.
static int fp32_rows_flag(pgmi_model* esm) {
    int32_t flag = 0;
    PGMI_HIP(hipMemcpyAsync(&flag, esm->nonfinite, 4, hipMemcpyDeviceToHost, esm->stream));
    PGMI_HIP(hipStreamSynchronize(esm->stream));
    if (!flag) return PGMI_OK;
    PGMI_HIP(hipMemsetAsync(esm->nonfinite, 0, 4, esm->stream));
    set_error("packed rows: a residue row is not finite in precision fp32");
    return PGMI_EINVAL;
}

// The library's residue rows into d_rows [sum L][D] (device), packed in the caller's order; the library has passed check_library.
static int esm_packed_rows(pgmi_model* esm, const RowsPlan& p, const uint8_t* tokens, const int64_t* seq_off, float* d_rows) {
    hipStream_t st = esm->stream;
    const int D = esm->cfg.embed_dim;
    const bool f32 = esm->cfg.precision == PGMI_PREC_FP32;
    std::vector<int32_t> toks, keep, dst;
    int j0 = 0;
    for (const int j1 : p.chunk_end) {
        const int bc = j1 - j0, T = (int)(seq_off[p.sid[j0] + 1] - seq_off[p.sid[j0]]);
        toks.assign((size_t)bc * T, PGMI_TOK_PAD);
        keep.clear();
        dst.clear();
        for (int b = 0; b < bc; ++b) {
            const int32_t n = p.sid[j0 + b];
            const int len = (int)(seq_off[n + 1] - seq_off[n]);
            for (int i = 0; i < len; ++i) toks[(size_t)b * T + i] = tokens[seq_off[n] + i];
            for (int i = 0; i < len - 2; ++i) {
                keep.push_back(b * T + 1 + i);
                dst.push_back((int32_t)(p.packed_off[n] + i));
            }
        }
        const int R = (int)keep.size();
        PGMI_HIP(hipMemcpyAsync(esm->tokens, toks.data(), toks.size() * 4, hipMemcpyHostToDevice, st));
        PGMI_HIP(hipMemcpyAsync(esm->row_idx, keep.data(), (size_t)R * 4, hipMemcpyHostToDevice, st));
        PGMI_HIP(hipMemcpyAsync(esm->aux_i, dst.data(), (size_t)R * 4, hipMemcpyHostToDevice, st));
        bool compacted = false;
        int rc = run_encoder(esm, bc, T, esm->row_idx, R, &compacted);
        if (rc) { hipStreamSynchronize(st); return rc; }
        const float* src = esm->x;
        if (!compacted) {                                  // PGMI_KEEP_ROWS=0: the full rows; qkv is free after the attention
            launch_gather_rows(esm->x, esm->row_idx, R, D, esm->qkv, st);
            src = esm->qkv;
        }
        {
            ProfScope s(esm, PGMI_K_LAYERNORM, 0, (double)R * D * 8);
            launch_layernorm(src, esm->lna_w, esm->lna_b, R, D, 1e-5f, esm->h, st);
        }
        {
            ProfScope s(esm, PGMI_K_SCORE, 0, (double)R * D * 8);
            launch_packed_scatter(esm->h, esm->aux_i, R, D, d_rows, esm->nonfinite, st);
        }
        PGMI_HIP(hipGetLastError());
        // the end of a chunk: the host arrays are reused by the next one, and a non-finite row ends the call here, not after the library
        if ((rc = f32 ? fp32_rows_flag(esm) : check_nonfinite(esm))) return rc;
        if (esm->prof && (rc = prof_drain(esm))) return rc;
        j0 = j1;
    }
    return PGMI_OK;
}

static int plan_cap(const pgmi_model* esm, int row_cap) { return row_cap > 0 ? std::min(row_cap, esm->max_rows) : esm->max_rows; }

// The head on n <= VESPAG_HEAD_ROWS rows (device, fp32 [n][D]): y [n][20].  a16: [n][D] split elements of scratch (f16x3), hid: [n][H].
// pm gives the precision, the stream, the GEMM variant and the profile.
static int vespag_head_rows(pgmi_model* pm, const float* rows, uint32_t* a16, const float* w1, const W16& w116, const float* b1, const float* w2,
                            const float* b2, const int32_t* wt, int n, int D, int H, float slope, float* hid, float* y) {
    hipStream_t st = pm->stream;
    unsigned short* a = reinterpret_cast<unsigned short*>(a16);
    if (pm->cfg.precision != PGMI_PREC_FP32) {
        ProfScope p(pm, PGMI_K_LAYERNORM, 0, (double)n * D * 8);
        launch_split16(rows, (int64_t)n * D, 1.0f, 2, D, a, st);
    }
    {
        ProfScope p(pm, PGMI_K_GEMM_FC1, 2.0 * n * (double)H * D, 0);
        const int rc = linear(pm, rows, a, w1, w116, b1, nullptr, hid, nullptr, n, H, D, EPI_NONE);
        if (rc) return rc;
    }
    ProfScope p(pm, PGMI_K_HEAD, 2.0 * n * (double)H * VESPAG_OUT, (double)n * (H + VESPAG_OUT) * 4);
    launch_vespag_head(hid, w2, b2, wt, n, H, slope, y, st);
    PGMI_HIP(hipGetLastError());
    return PGMI_OK;
}

static int check_head_dims(int D, int H) {
    if (D < 32 || D % 32 || D > 8192) { set_error("VespaG: input_dim %d must be a multiple of 32 in 32 .. 8192", D); return PGMI_EINVAL; }
    if (H < 32 || H % 32 || H > 768) { set_error("VespaG: hidden %d must be a multiple of 32 in 32 .. 768 (W2 is held in LDS)", H); return PGMI_EINVAL; }
    return PGMI_OK;
}

static int check_wt_cols(const int32_t* wt, int64_t R) {
    for (int64_t r = 0; r < R; ++r)
        if (wt[r] < -1 || wt[r] >= VESPAG_OUT) { set_error("VespaG: wt_cols[%lld] = %d outside -1 .. 19", (long long)r, (int)wt[r]); return PGMI_EINVAL; }
    return PGMI_OK;
}

}  // namespace pgmi

struct pgmi_vespag {
    pgmi_model pm;                       // device, stream, allocation pool and profiling state (pgmi_vespag_profile_model)
    pgmi_vespag_config cfg;
    pgmi_model* esm = nullptr;           // borrowed, with its stream
    int D = 0, H = 0;
    float *w1 = nullptr, *b1 = nullptr, *w2 = nullptr, *b2 = nullptr;
    W16 w116;
    // rows [R][D] packed (landscapes) or one chunk of them (head); y [R][20]; wt [R]; of one head chunk: a16 [rows][D] split, hid [rows][H]
    DevBuf<float> rows, y, hid;
    DevBuf<uint32_t> a16;
    DevBuf<int32_t> wt;
};

namespace pgmi {

static int vespag_check(const pgmi_vespag_config* c) {
    if (!c) { set_error("null config"); return PGMI_EINVAL; }
    if (c->abi_version != PGMI_ABI_VERSION) { set_error("ABI version mismatch: got %d, library is %d", c->abi_version, PGMI_ABI_VERSION); return PGMI_EINVAL; }
    const int rc = check_head_dims(c->input_dim, c->hidden);
    if (rc) return rc;
    if (c->out != VESPAG_OUT) { set_error("VespaG: out = %d, the head has 20 columns", c->out); return PGMI_EINVAL; }
    if (c->precision != PGMI_PREC_FP32 && c->precision != PGMI_PREC_F16X3) { set_error("VespaG runs in precision f16x3 or fp32"); return PGMI_EINVAL; }
    if (!std::isfinite(c->negative_slope)) { set_error("VespaG: negative_slope is not finite"); return PGMI_EINVAL; }
    return PGMI_OK;
}

static int64_t vespag_count(const pgmi_vespag_config* c) {
    const int64_t D = c->input_dim, H = c->hidden;
    return H * D + H + VESPAG_OUT * H + VESPAG_OUT;
}

// the head over R packed rows already in m->rows (wt_cols uploaded to m->wt), in chunks; y_host [R][20]
static int vespag_head_packed(pgmi_vespag* m, int64_t R, float* y_host) {
    const size_t D = m->D, H = m->H, C = (size_t)std::min<int64_t>(R, VESPAG_HEAD_ROWS);
    const bool split = m->cfg.precision != PGMI_PREC_FP32;
    int rc = reserve_all(&m->pm, m->y, (size_t)R * VESPAG_OUT, m->hid, C * H, m->a16, split ? C * D : 0);
    if (rc) return rc;
    for (int64_t r0 = 0; r0 < R; r0 += VESPAG_HEAD_ROWS) {
        const int n = (int)std::min<int64_t>(VESPAG_HEAD_ROWS, R - r0);
        rc = vespag_head_rows(&m->pm, m->rows + (size_t)r0 * D, m->a16, m->w1, m->w116, m->b1, m->w2, m->b2, m->wt + r0, n, (int)D, (int)H,
                              m->cfg.negative_slope, m->hid, m->y + (size_t)r0 * VESPAG_OUT);
        if (rc) return rc;
    }
    PGMI_HIP(hipMemcpyAsync(y_host, m->y, (size_t)R * VESPAG_OUT * 4, hipMemcpyDeviceToHost, m->pm.stream));
    return PGMI_OK;
}

// the end of an entry: the stream, the profile, and the [R][20] landscape on the host -- finite rows can still leave the fp16 range of the
// first Linear's split operand in precision f16x3
static int vespag_finish(pgmi_vespag* m, int rc, const char* what, const float* y_host, int64_t R) {
    rc = side_sync(&m->pm, rc, what);
    if (!rc && m->pm.prof) rc = prof_drain(&m->pm);
    for (int64_t i = 0; !rc && i < R * VESPAG_OUT; ++i)
        if (!std::isfinite(y_host[i])) return overflow_error(m->cfg.precision);
    return rc;
}

}  // namespace pgmi

extern "C" {

int pgmi_op_packed_rows_plan(const int64_t* seq_off, int64_t n_seq, int row_cap, int32_t* order, int32_t* chunk_end, int32_t* n_chunks,
                             int64_t* packed_off) {
    if (!order || !chunk_end || !n_chunks || !packed_off || row_cap <= 0) { set_error("bad argument"); return PGMI_EINVAL; }
    const int rc = check_seq_off(seq_off, n_seq);
    if (rc) return rc;
    const RowsPlan p = plan_rows(seq_off, n_seq, row_cap);
    std::copy(p.sid.begin(), p.sid.end(), order);
    std::copy(p.chunk_end.begin(), p.chunk_end.end(), chunk_end);
    std::copy(p.packed_off.begin(), p.packed_off.end(), packed_off);
    *n_chunks = (int32_t)p.chunk_end.size();
    return PGMI_OK;
}

int pgmi_esm_packed_rows(pgmi_model* esm, const uint8_t* tokens, const int64_t* seq_off, int64_t n_seq, int row_cap, float* rows_host,
                         int64_t* stats) {
    int rc = check_library(esm, tokens, seq_off, n_seq);
    if (rc) return rc;
    PGMI_HIP(hipSetDevice(esm->device));
    const RowsPlan p = plan_rows(seq_off, n_seq, plan_cap(esm, row_cap));
    const size_t n = (size_t)p.packed_off[n_seq] * esm->cfg.embed_dim;
    std::vector<void*> pool;
    float* d_rows = nullptr;
    rc = dev_alloc(pool, &d_rows, n);
    if (!rc) rc = esm_packed_rows(esm, p, tokens, seq_off, d_rows);
    hipError_t e = hipSuccess;
    if (!rc && rows_host) e = hipMemcpyAsync(rows_host, d_rows, n * 4, hipMemcpyDeviceToHost, esm->stream);
    const hipError_t e2 = hipStreamSynchronize(esm->stream);
    for (void* q : pool) hipFree(q);
    if (!rc && (e != hipSuccess || e2 != hipSuccess)) { set_error("packed rows failed: %s", hipGetErrorString(e != hipSuccess ? e : e2)); rc = PGMI_EHIP; }
    if (!rc && stats) { stats[0] = (int64_t)p.chunk_end.size(); stats[1] = p.tokens; stats[2] = p.padded; }
    return rc;
}

int64_t pgmi_vespag_weight_count(const pgmi_vespag_config* cfg) {
    if (vespag_check(cfg)) return -1;
    return vespag_count(cfg);
}

int pgmi_vespag_create(const pgmi_vespag_config* cfg, const float* w, int64_t n_weights, pgmi_model* esm, int device, pgmi_vespag** out) {
    if (!out) { set_error("null out"); return PGMI_EINVAL; }
    *out = nullptr;
    int rc = vespag_check(cfg);
    if (rc) return rc;
    if (esm) {
        if (esm->cfg.arch != PGMI_ARCH_ESM2) { set_error("VespaG: the sequence model must be an ESM2 model (arch %d)", esm->cfg.arch); return PGMI_EINVAL; }
        if (esm->cfg.embed_dim != cfg->input_dim) { set_error("VespaG: input_dim %d differs from the ESM2 model's width %d", cfg->input_dim, esm->cfg.embed_dim); return PGMI_EINVAL; }
        if (esm->cfg.precision != cfg->precision) { set_error("VespaG: precision %d differs from the ESM2 model's %d", cfg->precision, esm->cfg.precision); return PGMI_EINVAL; }
        device = esm->device;
    }
    pgmi_vespag* m = new pgmi_vespag();
    rc = side_open(&m->pm, "VespaG", w, n_weights, vespag_count(cfg), true, device, cfg->precision, esm ? esm->stream : nullptr);
    if (rc) { delete m; return rc; }
    m->cfg = *cfg;
    m->esm = esm;
    m->D = cfg->input_dim; m->H = cfg->hidden;
    const size_t D = m->D, H = m->H;
    BlobCursor c(&m->pm, w, n_weights);
    c.linear(&m->w1, &m->w116, H * D, D);
    c.upload(&m->b1, H);
    c.upload(&m->w2, VESPAG_OUT * H);
    c.upload(&m->b2, VESPAG_OUT);
    rc = c.finish();
    if (rc) { pgmi_vespag_destroy(m); return rc; }
    *out = m;
    return PGMI_OK;
}

void pgmi_vespag_destroy(pgmi_vespag* m) {
    if (!m) return;
    side_release(&m->pm, !m->esm);
    delete m;
}

pgmi_model* pgmi_vespag_profile_model(pgmi_vespag* m) { return m ? &m->pm : nullptr; }

int pgmi_vespag_landscapes(pgmi_vespag* m, const uint8_t* tokens, const int64_t* seq_off, int64_t n_seq, const int32_t* wt_cols, float* y_host,
                           float* rows_host) {
    if (!m || !wt_cols || !y_host) { set_error("bad argument"); return PGMI_EINVAL; }
    pgmi_model* esm = m->esm;
    if (!esm) { set_error("VespaG: no ESM2 model (pgmi_vespag_create was given none): pgmi_vespag_head takes pre-computed rows"); return PGMI_EINVAL; }
    int rc = check_library(esm, tokens, seq_off, n_seq);
    if (rc) return rc;
    const RowsPlan p = plan_rows(seq_off, n_seq, plan_cap(esm, 0));
    const int64_t R = p.packed_off[n_seq];
    if ((rc = check_wt_cols(wt_cols, R))) return rc;
    PGMI_HIP(hipSetDevice(m->pm.device));
    hipStream_t st = m->pm.stream;
    const size_t D = m->D;
    if ((rc = reserve_all(&m->pm, m->rows, (size_t)R * D, m->wt, (size_t)R))) return rc;
    if ((rc = esm_packed_rows(esm, p, tokens, seq_off, m->rows))) return rc;
    PGMI_HIP(hipMemcpyAsync(m->wt, wt_cols, (size_t)R * 4, hipMemcpyHostToDevice, st));
    rc = vespag_head_packed(m, R, y_host);
    if (!rc && rows_host) PGMI_HIP(hipMemcpyAsync(rows_host, m->rows, (size_t)R * D * 4, hipMemcpyDeviceToHost, st));
    return vespag_finish(m, rc, "VespaG landscapes", y_host, R);
}

int pgmi_vespag_head(pgmi_vespag* m, const float* rows_host, const int32_t* wt_cols, int64_t R, float* y_host) {
    if (!m || !rows_host || !wt_cols || !y_host || R <= 0 || R > 0x7fffffff) { set_error("bad argument"); return PGMI_EINVAL; }
    const size_t D = m->D, n = (size_t)R * D;
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(rows_host[i])) { set_error("VespaG: element %zu of row %zu is not finite", i % D, i / D); return PGMI_EINVAL; }
    int rc = check_wt_cols(wt_cols, R);
    if (rc) return rc;
    PGMI_HIP(hipSetDevice(m->pm.device));
    hipStream_t st = m->pm.stream;
    if ((rc = reserve_all(&m->pm, m->rows, n, m->wt, (size_t)R))) return rc;
    PGMI_HIP(hipMemcpyAsync(m->rows, rows_host, n * 4, hipMemcpyHostToDevice, st));
    PGMI_HIP(hipMemcpyAsync(m->wt, wt_cols, (size_t)R * 4, hipMemcpyHostToDevice, st));
    rc = vespag_head_packed(m, R, y_host);
    return vespag_finish(m, rc, "VespaG head", y_host, R);
}

int pgmi_op_vespag_head(int device, int precision, const float* rows, const float* W1, const float* b1, const float* W2, const float* b2,
                        const int32_t* wt_cols, int R, int input_dim, int hidden, float slope, float* y) {
    if (!rows || !W1 || !b1 || !W2 || !b2 || !wt_cols || !y || R < 1 || R > VESPAG_HEAD_ROWS) { set_error("bad argument"); return PGMI_EINVAL; }
    if (precision != PGMI_PREC_FP32 && precision != PGMI_PREC_F16X3) { set_error("vespag head op: precision f16x3 or fp32"); return PGMI_EINVAL; }
    int rc = check_head_dims(input_dim, hidden);
    if (!rc) rc = check_wt_cols(wt_cols, R);
    if (rc) return rc;
    OpScope s("vespag head op", device);
    s.tmp.cfg.precision = precision;                              // what linear() reads; the stream is the default one
    const bool f32 = precision == PGMI_PREC_FP32;
    const size_t D = input_dim, H = hidden;
    float* drows = s.up(rows, (size_t)R * D);
    float* w1 = f32 ? s.up(W1, H * D) : nullptr;
    const W16 w116 = f32 ? W16{} : s.w16(W1, H * D, D);
    float* db1 = s.up(b1, H);
    float* w2 = s.up(W2, VESPAG_OUT * H);
    float* db2 = s.up(b2, (size_t)VESPAG_OUT);
    int32_t* wt = s.up(wt_cols, (size_t)R);
    uint32_t* a16 = f32 ? nullptr : s.alloc<uint32_t>((size_t)R * D);
    float* hid = s.alloc<float>((size_t)R * H);
    float* dy = s.alloc<float>((size_t)R * VESPAG_OUT, 0xFF);     // an element the kernel skips shows as NaN
    if (!s.rc) s.rc = vespag_head_rows(&s.tmp, drows, a16, w1, w116, db1, w2, db2, wt, R, input_dim, hidden, slope, hid, dy);
    s.sync();
    s.down(y, dy, (size_t)R * VESPAG_OUT);
    return s.rc;
}

}  // extern "C"
