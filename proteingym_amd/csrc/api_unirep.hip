// UniRep entries of the C ABI (include/pgmi.h, UniRep section): the folded blob's walk (padding H to Hp = roundup(H, 32), the two
// recurrent weights transposed to the GEMMs' [N][K]), the target's pass that keeps (c, h) after every step, and the step loop over
// chunks of equal-length rows ordered by their join step.  The kernels around the two GEMMs are in mlstm.hip.
// A GEMM output element's sum does not depend on the launch's row count and every other kernel is row-local, so a row started from
// the target's stored state computes, step by step, the bits it would compute from the zero state.
#include "model.h"

namespace pgmi {

constexpr int UR_TOKENS = 26, UR_OUT = 25, UR_WINDOW = 8;      // token ids 0 .. 25; Dense(25); steps per head launch
constexpr long long UR_ROWS_LIMIT = 32768;
static long long g_unirep_max_rows = 0;

int unirep_set_option(const char* name, long long value) {
    if (!strcmp(name, "unirep_max_rows")) { g_unirep_max_rows = std::min(std::max(value, 0LL), UR_ROWS_LIMIT); return PGMI_OK; }
    return PGMI_EINVAL;
}

}  // namespace pgmi

struct pgmi_unirep {
    pgmi_model pm;                       // device, stream, allocation pool and profiling state (pgmi_unirep_profile_model)
    pgmi_unirep_config cfg;
    int H = 0, Hp = 0;
    float *Tmx = nullptr, *Tx = nullptr, *Wd = nullptr, *bd = nullptr;     // [26][Hp], [26][4 Hp], [25][Hp], [25]
    float *wmh32 = nullptr, *wh32 = nullptr;                               // fp32 mode: [Hp][Hp], [4 Hp][Hp] ([out][in])
    W16 wmh16, wh16;
    // the target: inputs ttok [tL], state table entries 0 .. tL (entry j = the state after j steps; entry 0 = zeros), log-prob rows
    int tL = 0;
    std::vector<int32_t> ttok;
    DevBuf<float> ctab, tlp;
    DevBuf<uint32_t> htab;
    // workspace of a chunk
    DevBuf<int32_t> inp, tgt, join;
    DevBuf<float> c, g1, mm, z, hwin, terms, lp, zout;
    DevBuf<uint32_t> hs;                 // the h operand of product 1: split rows or fp32 rows, 4 bytes per unit either way
    size_t win_rows = 0;                 // rows per window slot of hwin
    DevBuf<double> score;
};

namespace pgmi {

static int ur_check(const pgmi_unirep_config* c) {
    if (!c) { set_error("null config"); return PGMI_EINVAL; }
    if (c->abi_version != PGMI_ABI_VERSION) { set_error("ABI version mismatch: got %d, library is %d", c->abi_version, PGMI_ABI_VERSION); return PGMI_EINVAL; }
    if (c->hidden < 1 || c->hidden > 8192) { set_error("UniRep: hidden size %d outside 1 .. 8192", c->hidden); return PGMI_EINVAL; }
    if (c->vocab != UR_TOKENS) { set_error("UniRep: vocabulary must be %d (unirep.py:325), got %d", UR_TOKENS, c->vocab); return PGMI_EINVAL; }
    if (c->precision != PGMI_PREC_FP32 && c->precision != PGMI_PREC_F16X3) {
        set_error("UniRep runs in precision f16x3 or fp32 (bf16 is not parity-gated for a recurrence)");
        return PGMI_EINVAL;
    }
    if (c->max_rows < 0) { set_error("UniRep: negative max_rows"); return PGMI_EINVAL; }
    return PGMI_OK;
}

static int64_t ur_count(const pgmi_unirep_config* c) {
    const int64_t H = c->hidden;
    return UR_TOKENS * H + UR_TOKENS * 4 * H + H * H + H * 4 * H + H * UR_OUT + UR_OUT;
}

static int ur_build(pgmi_unirep* m, const float* w, int64_t n_weights) {
    const size_t H = m->H, Hp = m->Hp;
    BlobCursor c(&m->pm, w, n_weights);
    {   // Tmx [26][H] -> [26][Hp]
        const float* s = c.take(UR_TOKENS * H);
        std::vector<float> t(UR_TOKENS * Hp, 0.0f);
        for (size_t a = 0; a < UR_TOKENS; ++a) memcpy(&t[a * Hp], s + a * H, H * sizeof(float));
        c.upload(&m->Tmx, t);
    }
    {   // Tx [26][4 H] -> [26][4][Hp]
        const float* s = c.take(UR_TOKENS * 4 * H);
        std::vector<float> t(UR_TOKENS * 4 * Hp, 0.0f);
        for (size_t a = 0; a < UR_TOKENS; ++a)
            for (size_t g = 0; g < 4; ++g) memcpy(&t[(a * 4 + g) * Hp], s + a * 4 * H + g * H, H * sizeof(float));
        c.upload(&m->Tx, t);
    }
    {   // wmh [H in][H out] -> [Hp out][Hp in]
        const float* s = c.take(H * H);
        std::vector<float> t(Hp * Hp, 0.0f);
        for (size_t k = 0; k < H; ++k)
            for (size_t n = 0; n < H; ++n) t[n * Hp + k] = s[k * H + n];
        c.linear(&m->wmh32, &m->wmh16, t, Hp);
    }
    {   // wh [H in][4 H out] -> [4][Hp out][Hp in]
        const float* s = c.take(H * 4 * H);
        std::vector<float> t(4 * Hp * Hp, 0.0f);
        for (size_t k = 0; k < H; ++k)
            for (size_t g = 0; g < 4; ++g)
                for (size_t n = 0; n < H; ++n) t[(g * Hp + n) * Hp + k] = s[k * 4 * H + g * H + n];
        c.linear(&m->wh32, &m->wh16, t, Hp);
    }
    {   // Dense kernel [H][25] -> [25][Hp]; bias [25]
        const float* s = c.take(H * UR_OUT);
        std::vector<float> t(UR_OUT * Hp, 0.0f);
        for (size_t k = 0; k < H; ++k)
            for (size_t v = 0; v < UR_OUT; ++v) t[v * Hp + k] = s[k * UR_OUT + v];
        c.upload(&m->Wd, t);
        c.upload(&m->bd, UR_OUT);
    }
    int rc = c.finish();
    // entry 0 of the state table: the zero state (unirep.py:76-79), also what a handle without a target starts from
    if (!rc) rc = reserve_all(&m->pm, m->ctab, Hp, m->htab, Hp);
    if (!rc) {
        PGMI_HIP(hipMemset(m->ctab, 0, Hp * 4));
        PGMI_HIP(hipMemset(m->htab, 0, Hp * 4));
    }
    return rc;
}

static int ur_rows_cap(const pgmi_unirep* m) {
    long long r = m->cfg.max_rows > 0 ? m->cfg.max_rows : 8192;
    if (g_unirep_max_rows > 0) r = g_unirep_max_rows;
    return (int)std::min(std::max(r, 1LL), UR_ROWS_LIMIT);
}

static int ur_workspace(pgmi_unirep* m, size_t R, size_t Lc, bool want_lp, bool want_z) {
    pgmi_model* pm = &m->pm;
    const size_t Hp = m->Hp;
    int rc = reserve_all(pm, m->inp, R * Lc, m->tgt, R * Lc, m->join, R, m->c, R * Hp, m->hs, R * Hp, m->g1, R * Hp, m->mm, R * Hp,
                         m->z, R * 4 * Hp, m->terms, R * Lc, m->score, R);
    if (!rc && R > m->win_rows) {
        rc = m->hwin.reserve(pm, (size_t)UR_WINDOW * R * Hp);
        if (!rc) m->win_rows = R;
    }
    if (!rc && want_lp) rc = m->lp.reserve(pm, R * Lc * UR_OUT);
    if (!rc && want_z) rc = m->zout.reserve(pm, R * 4 * Hp);
    return rc;
}

// One step of rows [0, rows) of the chunk's state (m->c, m->hs): unirep.py:123-131.  tok[r * tok_stride] = row r's input token.
static int ur_step(pgmi_unirep* m, int rows, const int32_t* tok, int tok_stride, float* hwin, float* z_out) {
    pgmi_model* pm = &m->pm;
    hipStream_t st = pm->stream;
    const int Hp = m->Hp;
    const bool f32 = m->cfg.precision == PGMI_PREC_FP32;
    int rc;
    {
        ProfScope p(pm, PGMI_K_GEMM_FC1, 2.0 * rows * (double)m->H * m->H, 0);
        rc = linear(pm, reinterpret_cast<const float*>(m->hs.p), reinterpret_cast<const unsigned short*>(m->hs.p), m->wmh32, m->wmh16, nullptr, nullptr,
                    m->g1, nullptr, rows, Hp, Hp, EPI_NONE);
    }
    if (rc) return rc;
    {
        ProfScope p(pm, PGMI_K_LAYERNORM, 0, (double)rows * Hp * 12);
        launch_mlstm_m(m->g1, m->Tmx, tok, tok_stride, rows, Hp, f32 ? nullptr : reinterpret_cast<unsigned short*>(m->mm.p),
                       f32 ? m->mm : nullptr, st);
    }
    {
        ProfScope p(pm, PGMI_K_GEMM_FC2, 2.0 * rows * (double)m->H * 4 * m->H, 0);
        rc = linear(pm, m->mm, reinterpret_cast<const unsigned short*>(m->mm.p), m->wh32, m->wh16, nullptr, nullptr, m->z, nullptr, rows, 4 * Hp, Hp,
                    EPI_NONE);
    }
    if (rc) return rc;
    {
        ProfScope p(pm, PGMI_K_ATTENTION, 0, (double)rows * Hp * 36);
        MlstmGate a;
        a.z = m->z; a.Tx = m->Tx; a.tok = tok; a.tok_stride = tok_stride; a.c = m->c;
        if (f32) a.h32 = reinterpret_cast<float*>(m->hs.p); else a.h16 = reinterpret_cast<unsigned short*>(m->hs.p);
        a.hwin = hwin; a.z_out = z_out; a.rows = rows; a.Hp = Hp;
        launch_mlstm_gate(a, st);
    }
    return PGMI_OK;
}

// A chunk of n rows of Lc steps each, ordered by join (ascending): host arrays inp / tgt [n][Lc], join [n].  Row r runs the steps
// join[r] .. Lc - 1 from entry join[r] of the state table; its terms before that come from the target's rows.  scores (nullable)
// [n]; lp_host (nullable) [n][Lc][25] (rows from the zero state only); record: a one-row chunk from the zero state that fills the
// table's entries 1 .. Lc and the target's log-probability rows.
static int ur_chunk(pgmi_unirep* m, const int32_t* inp, const int32_t* tgt, const int32_t* join, int n, int Lc, double* scores,
                    float* lp_host, bool record, int64_t* rowsteps) {
    pgmi_model* pm = &m->pm;
    hipStream_t st = pm->stream;
    const size_t Hp = m->Hp;
    const bool want_lp = lp_host || record;
    int rc = ur_workspace(m, (size_t)n, (size_t)Lc, want_lp, false);
    if (rc) return rc;
    const size_t nt = (size_t)n * Lc;
    PGMI_HIP(hipMemcpyAsync(m->inp, inp, nt * 4, hipMemcpyHostToDevice, st));
    PGMI_HIP(hipMemcpyAsync(m->tgt, tgt, nt * 4, hipMemcpyHostToDevice, st));
    PGMI_HIP(hipMemcpyAsync(m->join, join, (size_t)n * 4, hipMemcpyHostToDevice, st));
    {
        ProfScope p(pm, PGMI_K_EMBED, 0, 0);
        launch_mlstm_init(m->ctab, m->htab, join[n - 1] > 0 ? m->tlp : nullptr, m->tgt, m->join, n, (int)Hp, Lc, m->c, m->hs, m->terms, st);
    }
    const size_t slot = m->win_rows * Hp;
    int act = 0, w0 = -1;
    for (int t = join[0]; t < Lc; ++t) {
        while (act < n && join[act] <= t) ++act;             // rows with join <= t: a leading range of the chunk
        if (w0 < 0) w0 = t;
        rc = ur_step(m, act, m->inp + t, Lc, m->hwin + (size_t)(t % UR_WINDOW) * slot, nullptr);
        if (rc) return rc;
        if (rowsteps) *rowsteps += act;
        if (record) {
            PGMI_HIP(hipMemcpyAsync(m->ctab + (size_t)(t + 1) * Hp, m->c, Hp * 4, hipMemcpyDeviceToDevice, st));
            PGMI_HIP(hipMemcpyAsync(m->htab + (size_t)(t + 1) * Hp, m->hs, Hp * 4, hipMemcpyDeviceToDevice, st));
        }
        if ((t + 1) % UR_WINDOW == 0 || t == Lc - 1) {
            ProfScope p(pm, PGMI_K_HEAD, 2.0 * (t + 1 - w0) * act * (double)m->H * UR_OUT, 0);
            launch_mlstm_head(m->hwin, slot, UR_WINDOW, m->Wd, m->bd, m->tgt, m->join, Lc, w0, t + 1 - w0, act, (int)Hp, m->terms,
                              want_lp ? m->lp : nullptr, st);
            w0 = -1;
        }
        if (pm->prof && (t & 31) == 31) { rc = prof_drain(pm); if (rc) return rc; }
    }
    {
        ProfScope p(pm, PGMI_K_SCORE, 0, 0);
        launch_mlstm_score(m->terms, m->tgt, n, Lc, m->score, st);
    }
    PGMI_HIP(hipGetLastError());
    if (record) PGMI_HIP(hipMemcpyAsync(m->tlp, m->lp, nt * UR_OUT * 4, hipMemcpyDeviceToDevice, st));
    if (lp_host) PGMI_HIP(hipMemcpyAsync(lp_host, m->lp, nt * UR_OUT * 4, hipMemcpyDeviceToHost, st));
    if (scores) PGMI_HIP(hipMemcpyAsync(scores, m->score, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    // the chunk's host arrays and the workspace are reused by the next chunk: wait for the copies
    return side_sync(pm, PGMI_OK, "UniRep step loop");
}

static int ur_check_tokens(const int32_t* tok, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (tok[i] < 0 || tok[i] >= UR_TOKENS) { set_error("UniRep: token %d at element %zu (0 .. 25 are valid)", (int)tok[i], i); return PGMI_EINVAL; }
    return PGMI_OK;
}

}  // namespace pgmi

extern "C" {

int64_t pgmi_unirep_weight_count(const pgmi_unirep_config* cfg) {
    if (ur_check(cfg)) return -1;
    return ur_count(cfg);
}

int pgmi_unirep_model_create(const pgmi_unirep_config* cfg, const float* w, int64_t n_weights, int device, pgmi_unirep** out) {
    if (!out) { set_error("null out"); return PGMI_EINVAL; }
    *out = nullptr;
    int rc = ur_check(cfg);
    if (rc) return rc;
    pgmi_unirep* m = new pgmi_unirep();
    rc = side_open(&m->pm, "UniRep", w, n_weights, ur_count(cfg), true, device, cfg->precision, nullptr);
    if (rc) { delete m; return rc; }
    m->cfg = *cfg;
    m->H = cfg->hidden;
    m->Hp = roundup32(cfg->hidden);
    rc = ur_build(m, w, n_weights);
    if (rc) { pgmi_unirep_destroy(m); return rc; }
    *out = m;
    return PGMI_OK;
}

void pgmi_unirep_destroy(pgmi_unirep* m) {
    if (!m) return;
    side_release(&m->pm, true);
    delete m;
}

pgmi_model* pgmi_unirep_profile_model(pgmi_unirep* m) { return m ? &m->pm : nullptr; }

int pgmi_unirep_set_target(pgmi_unirep* m, const int32_t* tokens, int L) {
    if (!m) { set_error("null model"); return PGMI_EINVAL; }
    m->tL = 0;
    m->ttok.clear();
    if (L == 0) return PGMI_OK;                          // clears the target
    if (!tokens || L < 0 || L > (1 << 20)) { set_error("UniRep: bad target (L = %d)", L); return PGMI_EINVAL; }
    int rc = ur_check_tokens(tokens, (size_t)L + 1);
    if (rc) return rc;
    PGMI_HIP(hipSetDevice(m->pm.device));
    pgmi_model* pm = &m->pm;
    const size_t Hp = m->Hp;
    rc = reserve_all(pm, m->ctab, (size_t)(L + 1) * Hp, m->htab, (size_t)(L + 1) * Hp, m->tlp, (size_t)L * UR_OUT);
    if (rc) return rc;
    PGMI_HIP(hipMemsetAsync(m->ctab, 0, Hp * 4, pm->stream));
    PGMI_HIP(hipMemsetAsync(m->htab, 0, Hp * 4, pm->stream));
    const int32_t join0 = 0;
    rc = ur_chunk(m, tokens, tokens + 1, &join0, 1, L, nullptr, nullptr, true, nullptr);
    if (rc) return rc;
    m->ttok.assign(tokens, tokens + L + 1);
    m->tL = L;
    return PGMI_OK;
}

int pgmi_unirep_token_logprobs(pgmi_unirep* m, const int32_t* tokens, int L, float* out) {
    if (!m || !tokens || !out || L < 1 || L > (1 << 20)) { set_error("bad argument"); return PGMI_EINVAL; }
    int rc = ur_check_tokens(tokens, (size_t)L);
    if (rc) return rc;
    PGMI_HIP(hipSetDevice(m->pm.device));
    std::vector<int32_t> tgt((size_t)L, 1);              // the terms are not read
    const int32_t join0 = 0;
    return ur_chunk(m, tokens, tgt.data(), &join0, 1, L, nullptr, out, false, nullptr);
}

int pgmi_unirep_sequence_nll(pgmi_unirep* m, const int32_t* tokens, const int64_t* offsets, int64_t n, int from_scratch, double* out,
                             int64_t* out_rowsteps) {
    if (!m || !tokens || !offsets || !out || n <= 0 || n > (1LL << 31) - 1) { set_error("bad argument"); return PGMI_EINVAL; }
    if (offsets[0] != 0) { set_error("UniRep: offsets[0] must be 0"); return PGMI_EINVAL; }
    for (int64_t i = 0; i < n; ++i) {
        const int64_t len = offsets[i + 1] - offsets[i];
        if (len < 2 || len > (1 << 20)) { set_error("UniRep: sequence %lld has %lld tokens (start + at least one residue)", (long long)i, (long long)len); return PGMI_EINVAL; }
    }
    int rc = ur_check_tokens(tokens, (size_t)offsets[n]);
    if (rc) return rc;
    PGMI_HIP(hipSetDevice(m->pm.device));
    // join step = residues shared with the target from the left (0 without a target, from scratch, or under another first token)
    std::vector<int32_t> len(n), join(n, 0);
    std::vector<int64_t> order(n);
    for (int64_t i = 0; i < n; ++i) {
        const int32_t* v = tokens + offsets[i];
        len[i] = (int32_t)(offsets[i + 1] - offsets[i] - 1);
        order[i] = i;
        if (from_scratch || m->tL == 0 || v[0] != m->ttok[0]) continue;
        const int lim = std::min(len[i], m->tL);
        int p = 0;
        while (p < lim && v[1 + p] == m->ttok[1 + p]) ++p;
        join[i] = p;
    }
    std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) {
        return len[a] != len[b] ? len[a] < len[b] : join[a] < join[b];
    });
    const int cap = ur_rows_cap(m);
    int64_t steps = 0;
    std::vector<int32_t> inp, tgt, cj;
    std::vector<double> sc;
    for (int64_t i0 = 0; i0 < n;) {
        const int Lc = len[order[i0]];
        int64_t i1 = i0;
        while (i1 < n && i1 - i0 < cap && len[order[i1]] == Lc) ++i1;
        const int nc = (int)(i1 - i0);
        inp.resize((size_t)nc * Lc); tgt.resize((size_t)nc * Lc); cj.resize(nc); sc.resize(nc);
        for (int r = 0; r < nc; ++r) {
            const int32_t* v = tokens + offsets[order[i0 + r]];
            memcpy(&inp[(size_t)r * Lc], v, (size_t)Lc * 4);
            memcpy(&tgt[(size_t)r * Lc], v + 1, (size_t)Lc * 4);
            cj[r] = join[order[i0 + r]];
        }
        rc = ur_chunk(m, inp.data(), tgt.data(), cj.data(), nc, Lc, sc.data(), nullptr, false, &steps);
        if (rc) return rc;
        for (int r = 0; r < nc; ++r) out[order[i0 + r]] = sc[r];
        i0 = i1;
    }
    if (out_rowsteps) *out_rowsteps = steps;
    return PGMI_OK;
}

int pgmi_op_mlstm_step(pgmi_unirep* m, const float* h_prev, const float* c_prev, const int32_t* tokens, int rows, float* h, float* c,
                       float* z) {
    if (!m || !h_prev || !c_prev || !tokens || !h || !c || !z || rows < 1 || rows > UR_ROWS_LIMIT) { set_error("bad argument"); return PGMI_EINVAL; }
    int rc = ur_check_tokens(tokens, (size_t)rows);
    if (rc) return rc;
    PGMI_HIP(hipSetDevice(m->pm.device));
    hipStream_t st = m->pm.stream;
    const size_t H = m->H, Hp = m->Hp, R = rows;
    rc = ur_workspace(m, R, 1, false, true);
    if (rc) return rc;
    std::vector<float> hp(R * Hp, 0.0f), cp(R * Hp, 0.0f);
    for (size_t r = 0; r < R; ++r) {
        memcpy(&hp[r * Hp], h_prev + r * H, H * 4);
        memcpy(&cp[r * Hp], c_prev + r * H, H * 4);
    }
    PGMI_HIP(hipMemcpyAsync(m->inp, tokens, R * 4, hipMemcpyHostToDevice, st));
    PGMI_HIP(hipMemcpyAsync(m->c, cp.data(), R * Hp * 4, hipMemcpyHostToDevice, st));
    if (m->cfg.precision == PGMI_PREC_FP32) PGMI_HIP(hipMemcpyAsync(m->hs, hp.data(), R * Hp * 4, hipMemcpyHostToDevice, st));
    else {   // the operand form the gate kernel writes between steps: split rows
        PGMI_HIP(hipMemcpyAsync(m->g1, hp.data(), R * Hp * 4, hipMemcpyHostToDevice, st));
        launch_split16(m->g1, (int64_t)(R * Hp), 1.0f, 2, (int)Hp, reinterpret_cast<unsigned short*>(m->hs.p), st);
    }
    rc = ur_step(m, rows, m->inp, 1, m->hwin, m->zout);
    if (rc) return rc;
    PGMI_HIP(hipGetLastError());
    PGMI_HIP(hipMemcpyAsync(h, m->hwin, R * Hp * 4, hipMemcpyDeviceToHost, st));
    PGMI_HIP(hipMemcpyAsync(c, m->c, R * Hp * 4, hipMemcpyDeviceToHost, st));
    PGMI_HIP(hipMemcpyAsync(z, m->zout, R * 4 * Hp * 4, hipMemcpyDeviceToHost, st));
    PGMI_HIP(hipStreamSynchronize(st));
    return PGMI_OK;
}

}  // extern "C"
