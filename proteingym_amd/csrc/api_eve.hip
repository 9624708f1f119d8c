// EVE / DeepSequence entries of the C ABI (include/pgmi.h, EVE section): the blob walk in state_dict() order, the encoder, one
// Monte-Carlo sample of the ELBO (sampled decoder weights once per sample, then row chunks through latent -> hidden layers -> final
// GEMM -> reduction), the noise seam (injected tensors / the generator's tensors) and the production loop with fp64 accumulators.
// The kernels are in eve.hip; every GEMM is launch_gemm_f32, whose K must be a multiple of 32: every operand's K (and every
// activation's row pitch) is rounded up to 32 with zeros, so the padded columns add exact zeros to the sums.
#include "model.h"

namespace pgmi {

static long long g_eve_max_rows = 0, g_eve_fixed_sample = -1, g_eve_prior_batch = 0;

int eve_set_option(const char* name, long long value) {
    if (!strcmp(name, "eve_max_rows")) { g_eve_max_rows = value > 0 ? value : 0; return PGMI_OK; }
    if (!strcmp(name, "eve_fixed_sample")) { g_eve_fixed_sample = value; return PGMI_OK; }
    if (!strcmp(name, "eve_prior_batch")) { g_eve_prior_batch = value > 0 ? value : 0; return PGMI_OK; }
    return PGMI_EINVAL;
}

struct EveLinear {           // deterministic Linear, operand [Np][Kp] zero-padded, bias [Np]
    float *w = nullptr, *b = nullptr;
    int N = 0, K = 0;
};
struct EveBayes {            // sampled Linear: mean / sd in the reference's element order, sampled operand [Np][Kp], bias [Np]
    float *w_mean = nullptr, *w_sd = nullptr, *b_mean = nullptr, *b_sd = nullptr, *w = nullptr, *b = nullptr;
    int N = 0, K = 0;
};
// device copies of one call's injected noise (nullptr everywhere: the generator)
struct EveInj {
    const float* z_eps = nullptr;
    const uint8_t* keep[PGMI_EVE_MAX_LAYERS + 1] = {nullptr};
    const float* w_eps[PGMI_EVE_MAX_LAYERS] = {nullptr};
    const float* b_eps[PGMI_EVE_MAX_LAYERS] = {nullptr};
    const float *wout = nullptr, *bout = nullptr, *conv = nullptr, *sparsity = nullptr, *temp = nullptr;
};

}  // namespace pgmi

struct pgmi_eve {
    pgmi_model pm;                       // device, stream, allocation pool and profiling state (pgmi_eve_profile_model)
    pgmi_eve_config cfg;
    int L = 0, N = 0, z = 0, ldz = 0, H = 0, Hp = 0, C = 0, Ht = 0, wmax = 0;
    uint32_t keep24 = 0;
    float scale = 1.0f;
    float *w0t = nullptr, *b0 = nullptr;             // encoder layer 0: transposed weight [20 L][E0p], bias [E0p]
    std::vector<EveLinear> enc;                      // encoder layers 1 .., then fc_mean | fc_log_var as one [2 z] layer
    std::vector<EveBayes> dec;
    float *wout_mean = nullptr, *wout_sd = nullptr, *bout_mean = nullptr, *bout_sd = nullptr, *conv_mean = nullptr, *conv_sd = nullptr,
          *sp_mean = nullptr, *sp_sd = nullptr, *t_mean = nullptr, *t_sd = nullptr;
    float *wfinal = nullptr, *bout = nullptr, *temp = nullptr;       // sampled: [20 L][Hp], [20 L], [1]
    // workspace (grow-only)
    DevBuf<uint8_t> res;
    DevBuf<float> mulv, ha, hb, logits;
    DevBuf<float> out3;       // elbo | bce | kld, [3][M]
    DevBuf<double> acc;       // [M][3]
    // pgmi_eve_log_prior: hidden vectors [2][EVE_PRIOR_S][wmax], the final kernel's partial sums, accumulators [20 L][3]
    DevBuf<float> pr_h, pr_partial;
    DevBuf<double> pr_acc;
};

namespace pgmi {

static int eve_check(const pgmi_eve_config* c) {
    if (!c) { set_error("null config"); return PGMI_EINVAL; }
    if (c->abi_version != PGMI_ABI_VERSION) { set_error("ABI version mismatch: got %d, library is %d", c->abi_version, PGMI_ABI_VERSION); return PGMI_EINVAL; }
    if (c->alphabet != 20) { set_error("EVE alphabet must be 20, got %d", c->alphabet); return PGMI_EINVAL; }
    if (c->seq_len <= 0 || c->z_dim <= 0) { set_error("EVE: non-positive seq_len / z_dim"); return PGMI_EINVAL; }
    if (c->n_enc < 1 || c->n_enc > PGMI_EVE_MAX_LAYERS || c->n_dec < 1 || c->n_dec > PGMI_EVE_MAX_LAYERS) {
        set_error("EVE: 1 .. %d layers per stack, got %d / %d", PGMI_EVE_MAX_LAYERS, c->n_enc, c->n_dec);
        return PGMI_EINVAL;
    }
    for (int i = 0; i < c->n_enc; ++i) if (c->enc_sizes[i] <= 0) { set_error("EVE: encoder size %d is not positive", i); return PGMI_EINVAL; }
    for (int i = 0; i < c->n_dec; ++i) if (c->dec_sizes[i] <= 0) { set_error("EVE: decoder size %d is not positive", i); return PGMI_EINVAL; }
    if (c->conv_depth < 0 || c->conv_depth % 4 != 0 || c->conv_depth > 1024) { set_error("EVE: conv_depth %d must be 0 or a multiple of 4 up to 1024", c->conv_depth); return PGMI_EINVAL; }
    if (c->sparsity_tiles < 0 || (c->sparsity_tiles > 0 && c->dec_sizes[c->n_dec - 1] % c->sparsity_tiles != 0)) {
        set_error("EVE: sparsity_tiles %d must divide the last hidden size %d", c->sparsity_tiles, c->dec_sizes[c->n_dec - 1]);
        return PGMI_EINVAL;
    }
    const int acts[3] = {c->enc_act, c->dec_first_act, c->dec_last_act};
    for (int a : acts) if (a < PGMI_EVE_ACT_RELU || a > PGMI_EVE_ACT_LINEAR) { set_error("EVE: unknown activation id %d", a); return PGMI_EINVAL; }
    if (!(c->dropout_p >= 0.0f && c->dropout_p < 1.0f)) { set_error("EVE: dropout_p must be in [0, 1)"); return PGMI_EINVAL; }
    if (c->precision != PGMI_PREC_FP32) { set_error("EVE runs in precision fp32 only"); return PGMI_EINVAL; }
    return PGMI_OK;
}

static int64_t eve_count(const pgmi_eve_config* c) {
    const int64_t L = c->seq_len, z = c->z_dim, H = c->dec_sizes[c->n_dec - 1], C = c->conv_depth ? c->conv_depth : 20;
    int64_t n = 0, in = 20 * L;
    for (int i = 0; i < c->n_enc; ++i) { n += (int64_t)c->enc_sizes[i] * in + c->enc_sizes[i]; in = c->enc_sizes[i]; }
    n += 2 * (z * in + z);
    if (c->sparsity_tiles) n += 2 * (H / c->sparsity_tiles) * L;
    n += 2 * C * L * H + 2 * 20 * L;
    if (c->temperature) n += 2;
    in = z;
    for (int i = 0; i < c->n_dec; ++i) { n += 2 * ((int64_t)c->dec_sizes[i] * in + c->dec_sizes[i]); in = c->dec_sizes[i]; }
    if (c->conv_depth) n += 2 * 20 * C;
    return n;
}

// [N][K] -> zero-padded [roundup32(N)][roundup32(K)]
static std::vector<float> pad_matrix(const float* w, int N, int K) {
    const int Np = roundup32(N), Kp = roundup32(K);
    std::vector<float> o((size_t)Np * Kp, 0.0f);
    for (int n = 0; n < N; ++n) memcpy(&o[(size_t)n * Kp], w + (size_t)n * K, (size_t)K * sizeof(float));
    return o;
}
static std::vector<float> pad_vector(const float* b, int N) {
    std::vector<float> o((size_t)roundup32(N), 0.0f);
    memcpy(o.data(), b, (size_t)N * sizeof(float));
    return o;
}
static std::vector<float> sd_of(const float* log_var, size_t n) {
    std::vector<float> o(n);
    for (size_t i = 0; i < n; ++i) o[i] = expf(0.5f * log_var[i]);
    return o;
}
static int zeros_dev(std::vector<void*>& pool, float** p, size_t n) {
    int rc = dev_alloc(pool, p, n);
    if (rc) return rc;
    PGMI_HIP(hipMemset(*p, 0, n * sizeof(float)));
    return PGMI_OK;
}

static int eve_build(pgmi_eve* m, const float* w, int64_t n_weights) {
    const pgmi_eve_config& c = m->cfg;
    std::vector<void*>& pool = m->pm.allocs;
    BlobCursor b(&m->pm, w, n_weights);
    auto zeros = [&](float** dst, size_t n) { if (!b.rc) b.rc = zeros_dev(pool, dst, n); };
    const int L = c.seq_len, z = c.z_dim, H = c.dec_sizes[c.n_dec - 1], C = c.conv_depth ? c.conv_depth : 20;
    m->L = L; m->N = 20 * L; m->z = z; m->ldz = roundup32(2 * z); m->H = H; m->Hp = roundup32(H); m->C = C;
    m->Ht = c.sparsity_tiles ? H / c.sparsity_tiles : 0;
    m->keep24 = c.dropout_p > 0.0f ? (uint32_t)lrint((1.0 - (double)c.dropout_p) * 16777216.0) : 0;
    m->scale = (float)(1.0 / (1.0 - (double)c.dropout_p));
    m->wmax = roundup32(z);
    // encoder layer 0, transposed: W0t[col][n]
    {
        const int E0 = c.enc_sizes[0], E0p = roundup32(E0);
        const float* w0 = b.take((size_t)E0 * m->N);
        std::vector<float> t((size_t)m->N * E0p, 0.0f);
        for (int n = 0; n < E0; ++n)
            for (int k = 0; k < m->N; ++k) t[(size_t)k * E0p + n] = w0[(size_t)n * m->N + k];
        b.upload(&m->w0t, t);
        b.upload(&m->b0, pad_vector(b.take(E0), E0));
        m->wmax = std::max(m->wmax, E0p);
    }
    int in = c.enc_sizes[0];
    for (int i = 1; i < c.n_enc; ++i) {
        EveLinear l;
        l.N = c.enc_sizes[i]; l.K = in;
        b.upload(&l.w, pad_matrix(b.take((size_t)l.N * in), l.N, in));
        b.upload(&l.b, pad_vector(b.take(l.N), l.N));
        m->enc.push_back(l);
        m->wmax = std::max(m->wmax, roundup32(l.N));
        in = l.N;
    }
    {   // fc_mean | fc_log_var as one layer of 2 z columns
        const float *wm = b.take((size_t)z * in), *bm = b.take(z), *wl = b.take((size_t)z * in), *bl = b.take(z);
        std::vector<float> wz((size_t)2 * z * in), bz((size_t)2 * z);
        memcpy(wz.data(), wm, (size_t)z * in * sizeof(float));
        memcpy(wz.data() + (size_t)z * in, wl, (size_t)z * in * sizeof(float));
        memcpy(bz.data(), bm, (size_t)z * sizeof(float));
        memcpy(bz.data() + z, bl, (size_t)z * sizeof(float));
        EveLinear l;
        l.N = 2 * z; l.K = in;
        b.upload(&l.w, pad_matrix(wz.data(), 2 * z, in));
        b.upload(&l.b, pad_vector(bz.data(), 2 * z));
        m->enc.push_back(l);
    }
    if (c.sparsity_tiles) {
        const size_t n = (size_t)m->Ht * L;
        b.upload(&m->sp_mean, n);
        b.upload(&m->sp_sd, sd_of(b.take(n), n));
    }
    {
        const size_t n = (size_t)C * L * H;
        b.upload(&m->wout_mean, n);
        b.upload(&m->wout_sd, sd_of(b.take(n), n));
        b.upload(&m->bout_mean, m->N);
        b.upload(&m->bout_sd, sd_of(b.take(m->N), m->N));
    }
    if (c.temperature) {
        b.upload(&m->t_mean, 1);
        b.upload(&m->t_sd, sd_of(b.take(1), 1));
    }
    m->dec.resize(c.n_dec);
    in = z;
    for (int i = 0; i < c.n_dec; ++i) {
        EveBayes& l = m->dec[i];
        l.N = c.dec_sizes[i]; l.K = in;
        b.upload(&l.w_mean, (size_t)l.N * in);
        b.upload(&l.b_mean, l.N);
        zeros(&l.w, (size_t)roundup32(l.N) * roundup32(in));
        zeros(&l.b, roundup32(l.N));
        m->wmax = std::max(m->wmax, roundup32(l.N));
        in = l.N;
    }
    in = z;
    for (int i = 0; i < c.n_dec; ++i) {
        EveBayes& l = m->dec[i];
        b.upload(&l.w_sd, sd_of(b.take((size_t)l.N * in), (size_t)l.N * in));
        b.upload(&l.b_sd, sd_of(b.take(l.N), l.N));
        in = l.N;
    }
    if (c.conv_depth) {
        b.upload(&m->conv_mean, (size_t)20 * C);
        b.upload(&m->conv_sd, sd_of(b.take((size_t)20 * C), (size_t)20 * C));
    }
    zeros(&m->wfinal, (size_t)m->N * m->Hp);
    zeros(&m->bout, m->N);
    zeros(&m->temp, 1);
    return b.finish();
}

static int eve_rows_per_chunk(const pgmi_eve* m, int M) {
    long long rows = std::max<long long>(1, (256ll << 20) / ((long long)m->N * 4));
    if (g_eve_max_rows > 0) rows = std::min(rows, g_eve_max_rows);
    return (int)std::min<long long>(rows, M);
}

static int eve_check_call(pgmi_eve* m, const uint8_t* residues, int M) {
    if (!m || !residues || M <= 0) { set_error("bad argument"); return PGMI_EINVAL; }
    PGMI_HIP(hipSetDevice(m->pm.device));
    return PGMI_OK;
}

// residues -> device; encoder -> mulv [M][ldz] (mu | log_var)
static int eve_encode(pgmi_eve* m, const uint8_t* residues, int M) {
    pgmi_model* pm = &m->pm;
    hipStream_t st = pm->stream;
    const int per = std::min(M, 4096);
    int rc = reserve_all(pm, m->res, (size_t)M * m->L, m->mulv, (size_t)M * m->ldz, m->ha, (size_t)per * m->wmax, m->hb, (size_t)per * m->wmax);
    if (rc) return rc;
    PGMI_HIP(hipMemcpyAsync(m->res, residues, (size_t)M * m->L, hipMemcpyHostToDevice, st));
    const int act = m->cfg.enc_act;
    for (int r0 = 0; r0 < M; r0 += per) {
        const int mc = std::min(per, M - r0);
        ProfScope p(pm, PGMI_K_HEAD, 0, 0);
        float *cur = m->ha, *nxt = m->hb;
        launch_eve_gather(m->res + (size_t)r0 * m->L, m->w0t, m->b0, mc, m->L, roundup32(m->cfg.enc_sizes[0]), act, cur, st);
        for (size_t i = 0; i < m->enc.size(); ++i) {
            const EveLinear& l = m->enc[i];
            const bool last = i + 1 == m->enc.size();
            float* dst = last ? m->mulv + (size_t)r0 * m->ldz : nxt;
            rc = launch_gemm_f32(cur, l.w, l.b, nullptr, dst, mc, roundup32(l.N), roundup32(l.K), EPI_NONE, st);
            if (rc) return rc;
            if (!last) {
                launch_eve_act(dst, mc, l.N, roundup32(l.N), act, 0, 1.0f, 0, 0, 0, 0, nullptr, 0, st);
                std::swap(cur, nxt);
            }
        }
    }
    PGMI_HIP(hipGetLastError());
    return PGMI_OK;
}

// the decoder's operands of one sample
static int eve_sample_weights(pgmi_eve* m, uint64_t seed, uint32_t sample, const EveInj& inj) {
    pgmi_model* pm = &m->pm;
    hipStream_t st = pm->stream;
    ProfScope p(pm, PGMI_K_EMBED, 0, (double)m->C * m->L * m->H * 8 + (double)m->N * m->Hp * 4);
    for (size_t i = 0; i < m->dec.size(); ++i) {
        const EveBayes& l = m->dec[i];
        launch_eve_sample(l.w_mean, l.w_sd, (int64_t)l.N * l.K, l.K, roundup32(l.K), seed, sample, PGMI_EVE_T_W + (int)i, inj.w_eps[i], l.w, st);
        launch_eve_sample(l.b_mean, l.b_sd, l.N, l.N, roundup32(l.N), seed, sample, PGMI_EVE_T_B + (int)i, inj.b_eps[i], l.b, st);
    }
    launch_eve_sample_final(m->wout_mean, m->wout_sd, m->conv_mean, m->conv_sd, m->sp_mean, m->sp_sd, m->L, m->H, m->Hp, m->C, m->Ht,
                            m->cfg.conv_depth != 0, seed, sample, inj.wout, inj.conv, inj.sparsity, m->wfinal, st);
    launch_eve_sample(m->bout_mean, m->bout_sd, m->N, m->N, m->N, seed, sample, PGMI_EVE_T_BOUT, inj.bout, m->bout, st);
    if (m->cfg.temperature) launch_eve_sample(m->t_mean, m->t_sd, 1, 1, 1, seed, sample, PGMI_EVE_T_TEMP, inj.temp, m->temp, st);
    PGMI_HIP(hipGetLastError());
    return PGMI_OK;
}

// rows [r0, r0 + mc) of the call through the sampled decoder; the call's row i is assay row row_base + i
static int eve_rows(pgmi_eve* m, int r0, int mc, int64_t row_base, uint64_t seed, uint32_t sample, const EveInj& inj, float* elbo, float* bce,
                    float* kld, double* acc, int first) {
    pgmi_model* pm = &m->pm;
    hipStream_t st = pm->stream;
    const pgmi_eve_config& c = m->cfg;
    float *cur = m->ha, *nxt = m->hb;
    {
        double fl = 0;
        for (const EveBayes& l : m->dec) fl += 2.0 * mc * l.N * l.K;
        ProfScope p(pm, PGMI_K_GEMM_FC1, fl, 0);
        launch_eve_latent(m->mulv, m->ldz, r0, mc, m->z, roundup32(m->z), m->keep24, m->scale, seed, sample, row_base + r0, inj.z_eps, inj.keep[0],
                          r0, cur, st);
        for (size_t i = 0; i < m->dec.size(); ++i) {
            const EveBayes& l = m->dec[i];
            int rc = launch_gemm_f32(cur, l.w, l.b, nullptr, nxt, mc, roundup32(l.N), roundup32(l.K), EPI_NONE, st);
            if (rc) return rc;
            launch_eve_act(nxt, mc, l.N, roundup32(l.N), i + 1 == m->dec.size() ? c.dec_last_act : c.dec_first_act, m->keep24, m->scale, seed, sample,
                           PGMI_EVE_T_KEEP + 1 + (int)i, row_base + r0, inj.keep[i + 1], r0, st);
            std::swap(cur, nxt);
        }
    }
    {
        ProfScope p(pm, PGMI_K_GEMM_FC2, 2.0 * mc * m->N * m->H, 0);
        int rc = launch_gemm_f32(cur, m->wfinal, m->bout, nullptr, m->logits, mc, m->N, m->Hp, EPI_NONE, st);
        if (rc) return rc;
    }
    {
        ProfScope p(pm, PGMI_K_SCORE, 0, (double)mc * m->N * 4);
        launch_eve_elbo(m->logits, m->res, m->mulv, m->ldz, m->z, c.temperature ? m->temp : nullptr, mc, m->L, r0, elbo, bce, kld, acc, first, st);
    }
    PGMI_HIP(hipGetLastError());
    return PGMI_OK;
}

static int eve_workspace(pgmi_eve* m, int M, int per) {
    return reserve_all(&m->pm, m->ha, (size_t)per * m->wmax, m->hb, (size_t)per * m->wmax, m->logits, (size_t)per * m->N, m->out3, (size_t)3 * M,
                       m->acc, (size_t)3 * M);
}

template <typename T>
static int inj_upload(std::vector<void*>& pool, const T** dst, const T* host, size_t n, const char* what) {
    if (!host) { set_error("injected noise: %s is NULL", what); return PGMI_EINVAL; }
    T* d = nullptr;
    int rc = dev_upload(pool, &d, host, n);
    *dst = d;
    return rc;
}

static int eve_upload_noise(pgmi_eve* m, const pgmi_eve_noise* nz, int M, std::vector<void*>& pool, EveInj* inj, bool keeps = true) {
    const pgmi_eve_config& c = m->cfg;
    const bool drop = keeps && m->keep24 != 0;
    int rc = inj_upload(pool, &inj->z_eps, (const float*)nz->z_eps, (size_t)M * m->z, "z_eps");
    if (!rc && drop) rc = inj_upload(pool, &inj->keep[0], (const uint8_t*)nz->keep[0], (size_t)M * m->z, "keep[0]");
    for (int i = 0; i < c.n_dec && !rc; ++i) {
        const EveBayes& l = m->dec[i];
        rc = inj_upload(pool, &inj->w_eps[i], (const float*)nz->w_eps[i], (size_t)l.N * l.K, "w_eps");
        if (!rc) rc = inj_upload(pool, &inj->b_eps[i], (const float*)nz->b_eps[i], (size_t)l.N, "b_eps");
        if (!rc && drop) rc = inj_upload(pool, &inj->keep[i + 1], (const uint8_t*)nz->keep[i + 1], (size_t)M * l.N, "keep");
    }
    if (!rc) rc = inj_upload(pool, &inj->wout, (const float*)nz->wout_eps, (size_t)m->C * m->L * m->H, "wout_eps");
    if (!rc) rc = inj_upload(pool, &inj->bout, (const float*)nz->bout_eps, (size_t)m->N, "bout_eps");
    if (!rc && c.conv_depth) rc = inj_upload(pool, &inj->conv, (const float*)nz->conv_eps, (size_t)20 * m->C, "conv_eps");
    if (!rc && c.sparsity_tiles) rc = inj_upload(pool, &inj->sparsity, (const float*)nz->sparsity_eps, (size_t)m->Ht * m->L, "sparsity_eps");
    if (!rc && c.temperature) rc = inj_upload(pool, &inj->temp, (const float*)nz->temp_eps, 1, "temp_eps");
    return rc;
}

}  // namespace pgmi

extern "C" {

int64_t pgmi_eve_weight_count(const pgmi_eve_config* cfg) {
    if (eve_check(cfg)) return -1;
    return eve_count(cfg);
}

int pgmi_eve_create(const pgmi_eve_config* cfg, const float* w, int64_t n_weights, int device, pgmi_eve** out) {
    if (!out) { set_error("null out"); return PGMI_EINVAL; }
    *out = nullptr;
    int rc = eve_check(cfg);
    if (rc) return rc;
    pgmi_eve* m = new pgmi_eve();
    rc = side_open(&m->pm, "EVE", w, n_weights, eve_count(cfg), false, device, cfg->precision, nullptr);
    if (rc) { delete m; return rc; }
    m->cfg = *cfg;
    rc = eve_build(m, w, n_weights);
    if (rc) { pgmi_eve_destroy(m); return rc; }
    *out = m;
    return PGMI_OK;
}

void pgmi_eve_destroy(pgmi_eve* m) {
    if (!m) return;
    side_release(&m->pm, true);
    delete m;
}

pgmi_model* pgmi_eve_profile_model(pgmi_eve* m) { return m ? &m->pm : nullptr; }

int pgmi_eve_encode(pgmi_eve* m, const uint8_t* residues, int M, float* mu, float* log_var) {
    int rc = eve_check_call(m, residues, M);
    if (rc) return rc;
    if (!mu || !log_var) { set_error("bad argument"); return PGMI_EINVAL; }
    rc = eve_encode(m, residues, M);
    if (rc) return rc;
    const size_t z = m->z;
    PGMI_HIP(hipMemcpy2DAsync(mu, z * 4, m->mulv, (size_t)m->ldz * 4, z * 4, M, hipMemcpyDeviceToHost, m->pm.stream));
    PGMI_HIP(hipMemcpy2DAsync(log_var, z * 4, m->mulv + z, (size_t)m->ldz * 4, z * 4, M, hipMemcpyDeviceToHost, m->pm.stream));
    PGMI_HIP(hipStreamSynchronize(m->pm.stream));
    return PGMI_OK;
}

int pgmi_eve_elbo(pgmi_eve* m, const uint8_t* residues, int M, int64_t row_base, uint64_t seed, int sample, const pgmi_eve_noise* injected,
                  float* elbo, float* bce, float* kld) {
    int rc = eve_check_call(m, residues, M);
    if (rc) return rc;
    if (row_base < 0 || sample < 0) { set_error("bad argument"); return PGMI_EINVAL; }
    const int per = eve_rows_per_chunk(m, M);
    rc = eve_encode(m, residues, M);
    if (!rc) rc = eve_workspace(m, M, per);
    if (rc) return rc;
    std::vector<void*> pool;
    EveInj inj;
    if (injected) rc = eve_upload_noise(m, injected, M, pool, &inj);
    if (!rc) rc = eve_sample_weights(m, seed, (uint32_t)sample, inj);
    for (int r0 = 0; r0 < M && !rc; r0 += per)
        rc = eve_rows(m, r0, std::min(per, M - r0), row_base, seed, (uint32_t)sample, inj, m->out3, m->out3 + M, m->out3 + 2 * (size_t)M,
                      nullptr, 0);
    hipStream_t st = m->pm.stream;
    if (!rc && elbo && hipMemcpyAsync(elbo, m->out3, (size_t)M * 4, hipMemcpyDeviceToHost, st) != hipSuccess) rc = PGMI_EHIP;
    if (!rc && bce && hipMemcpyAsync(bce, m->out3 + M, (size_t)M * 4, hipMemcpyDeviceToHost, st) != hipSuccess) rc = PGMI_EHIP;
    if (!rc && kld && hipMemcpyAsync(kld, m->out3 + 2 * (size_t)M, (size_t)M * 4, hipMemcpyDeviceToHost, st) != hipSuccess) rc = PGMI_EHIP;
    rc = side_sync(&m->pm, rc, "EVE sample");
    for (void* p : pool) hipFree(p);
    return rc;
}

int pgmi_eve_noise_fill(pgmi_eve* m, uint64_t seed, int sample, int64_t row_base, int M, pgmi_eve_noise* out) {
    if (!m || !out || M <= 0 || row_base < 0 || sample < 0) { set_error("bad argument"); return PGMI_EINVAL; }
    PGMI_HIP(hipSetDevice(m->pm.device));
    hipStream_t st = m->pm.stream;
    const uint32_t j = (uint32_t)sample;
    // one tensor at a time through a device buffer of the largest one
    size_t big = std::max((size_t)m->C * m->L * m->H, (size_t)M * std::max(m->wmax, m->z));
    for (const EveBayes& l : m->dec) big = std::max(big, (size_t)l.N * l.K);
    float* d = nullptr;
    std::vector<void*> pool;
    int rc = dev_alloc(pool, &d, big);
    if (rc) return rc;
    auto normal = [&](float* host, int tensor, uint64_t e0, size_t n) {
        if (!host || rc) return;
        launch_eve_fill_normal(seed, j, tensor, e0, (int64_t)n, d, st);
        if (hipMemcpyAsync(host, d, n * 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) { set_error("noise_fill: copy failed"); rc = PGMI_EHIP; }
    };
    auto keep = [&](uint8_t* host, int tensor, uint64_t e0, size_t n) {
        if (!host || rc) return;
        launch_eve_fill_keep(seed, j, tensor, e0, (int64_t)n, m->keep24, reinterpret_cast<uint8_t*>(d), st);
        if (hipMemcpyAsync(host, d, n, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) { set_error("noise_fill: copy failed"); rc = PGMI_EHIP; }
    };
    normal(out->z_eps, PGMI_EVE_T_Z, (uint64_t)row_base * m->z, (size_t)M * m->z);
    keep(out->keep[0], PGMI_EVE_T_KEEP, (uint64_t)row_base * m->z, (size_t)M * m->z);
    for (size_t i = 0; i < m->dec.size(); ++i) {
        const EveBayes& l = m->dec[i];
        normal(out->w_eps[i], PGMI_EVE_T_W + (int)i, 0, (size_t)l.N * l.K);
        normal(out->b_eps[i], PGMI_EVE_T_B + (int)i, 0, (size_t)l.N);
        keep(out->keep[i + 1], PGMI_EVE_T_KEEP + 1 + (int)i, (uint64_t)row_base * l.N, (size_t)M * l.N);
    }
    normal(out->wout_eps, PGMI_EVE_T_WOUT, 0, (size_t)m->C * m->L * m->H);
    normal(out->bout_eps, PGMI_EVE_T_BOUT, 0, (size_t)m->N);
    if (m->cfg.conv_depth) normal(out->conv_eps, PGMI_EVE_T_CONV, 0, (size_t)20 * m->C);
    if (m->cfg.sparsity_tiles) normal(out->sparsity_eps, PGMI_EVE_T_SPARSITY, 0, (size_t)m->Ht * m->L);
    if (m->cfg.temperature) normal(out->temp_eps, PGMI_EVE_T_TEMP, 0, 1);
    hipStreamSynchronize(st);
    for (void* p : pool) hipFree(p);
    return rc;
}

int pgmi_eve_evol_indices(pgmi_eve* m, const uint8_t* residues, int M, int num_samples, uint64_t seed, double* mean_elbo, double* std_elbo) {
    int rc = eve_check_call(m, residues, M);
    if (rc) return rc;
    if (num_samples <= 0 || !mean_elbo) { set_error("bad argument"); return PGMI_EINVAL; }
    const int per = eve_rows_per_chunk(m, M);
    rc = eve_encode(m, residues, M);
    if (!rc) rc = eve_workspace(m, M, per);
    if (rc) return rc;
    const EveInj none{};
    for (int j = 0; j < num_samples && !rc; ++j) {
        const uint32_t sample = g_eve_fixed_sample >= 0 ? (uint32_t)g_eve_fixed_sample : (uint32_t)j;
        rc = eve_sample_weights(m, seed, sample, none);
        for (int r0 = 0; r0 < M && !rc; r0 += per)
            rc = eve_rows(m, r0, std::min(per, M - r0), 0, seed, sample, none, nullptr, nullptr, nullptr, m->acc, j == 0);
        // profiling events are per launch group: drain them before they pile up over thousands of samples
        if (!rc && m->pm.prof && (j & 63) == 63) rc = prof_drain(&m->pm);
    }
    if (rc) { hipStreamSynchronize(m->pm.stream); return rc; }
    std::vector<double> a((size_t)3 * M);
    PGMI_HIP(hipMemcpyAsync(a.data(), m->acc, a.size() * 8, hipMemcpyDeviceToHost, m->pm.stream));
    PGMI_HIP(hipStreamSynchronize(m->pm.stream));
    const double n = num_samples;
    for (int i = 0; i < M; ++i) {
        const double shift = a[3 * (size_t)i], s = a[3 * (size_t)i + 1], ss = a[3 * (size_t)i + 2];
        mean_elbo[i] = shift + s / n;
        if (std_elbo) std_elbo[i] = num_samples > 1 ? sqrt(std::max(0.0, (ss - s * s / n) / (n - 1))) : 0.0;
    }
    return PGMI_OK;
}

}  // extern "C"

namespace pgmi {

// samples [j0, j0 + S) of a log-prior call: latent -> sampled hidden layers -> fused final layer -> log-softmax into the accumulators
static int eve_prior_group(pgmi_eve* m, uint64_t seed, int j0, int S, const EveInj* inj /* S structs or nullptr */) {
    pgmi_model* pm = &m->pm;
    hipStream_t st = pm->stream;
    const pgmi_eve_config& c = m->cfg;
    auto ptrs = [&](auto field) {
        EvePriorPtrs p;
        for (int s = 0; s < S && inj; ++s) p.p[s] = field(inj[s]);
        return p;
    };
    float *cur = m->pr_h, *nxt = m->pr_h + (size_t)EVE_PRIOR_S * m->wmax;
    {
        double fl = 0;
        for (const EveBayes& l : m->dec) fl += 2.0 * S * l.N * l.K;
        ProfScope p(pm, PGMI_K_GEMM_FC1, fl, 0);
        launch_eve_prior_latent(m->mulv, m->z, m->wmax, seed, (uint32_t)j0, ptrs([](const EveInj& i) { return i.z_eps; }), S, cur, st);
        for (size_t i = 0; i < m->dec.size(); ++i) {
            const EveBayes& l = m->dec[i];
            launch_eve_prior_hidden(l.w_mean, l.w_sd, l.b_mean, l.b_sd, l.N, l.K, seed, (uint32_t)j0, PGMI_EVE_T_W + (int)i, PGMI_EVE_T_B + (int)i,
                                    ptrs([i](const EveInj& x) { return x.w_eps[i]; }), ptrs([i](const EveInj& x) { return x.b_eps[i]; }), S, cur,
                                    m->wmax, i + 1 == m->dec.size() ? c.dec_last_act : c.dec_first_act, nxt, m->wmax, st);
            std::swap(cur, nxt);
        }
    }
    {
        ProfScope p(pm, PGMI_K_GEMM_FC2, 2.0 * S * m->N * m->H, (double)m->C * m->L * m->H * 8);
        launch_eve_prior_final(m->wout_mean, m->wout_sd, m->conv_mean, m->conv_sd, m->sp_mean, m->sp_sd, m->L, m->H, m->C, m->Ht,
                               c.conv_depth != 0, seed, (uint32_t)j0, ptrs([](const EveInj& i) { return i.wout; }),
                               ptrs([](const EveInj& i) { return i.conv; }), ptrs([](const EveInj& i) { return i.sparsity; }), S, cur, m->wmax,
                               m->pr_partial, st);
    }
    {
        ProfScope p(pm, PGMI_K_SCORE, 0, 0);
        launch_eve_prior_finish(m->pr_partial, S, m->bout_mean, m->bout_sd, c.temperature ? m->t_mean : nullptr, m->t_sd, seed, (uint32_t)j0,
                                ptrs([](const EveInj& i) { return i.bout; }), ptrs([](const EveInj& i) { return i.temp; }), m->L, m->H, j0,
                                m->pr_acc, st);
    }
    PGMI_HIP(hipGetLastError());
    return PGMI_OK;
}

}  // namespace pgmi

extern "C" int pgmi_eve_log_prior(pgmi_eve* m, const uint8_t* residues, int num_samples, uint64_t seed, const pgmi_eve_noise* injected,
                                  double* mean_logp, double* std_logp) {
    using namespace pgmi;
    int rc = eve_check_call(m, residues, 1);
    if (rc) return rc;
    if (num_samples <= 0 || !mean_logp) { set_error("bad argument"); return PGMI_EINVAL; }
    if (m->H < 20) { set_error("EVE log-prior: the last hidden size must be at least 20, got %d", m->H); return PGMI_EINVAL; }
    const int smax = eve_prior_max_samples(m->C, m->cfg.conv_depth != 0);
    if (smax < 1) { set_error("EVE log-prior: conv_depth %d does not fit the final kernel's LDS", m->C); return PGMI_EINVAL; }
    pgmi_model* pm = &m->pm;
    hipStream_t st = pm->stream;
    rc = eve_encode(m, residues, 1);
    if (!rc) rc = reserve_all(pm, m->pr_h, (size_t)2 * EVE_PRIOR_S * m->wmax,
                              m->pr_partial, (size_t)EVE_PRIOR_S * eve_prior_blocks(m->L, m->H) * eve_prior_kmax(m->H), m->pr_acc, (size_t)3 * m->N);
    if (rc) return rc;
    // "eve_prior_batch" samples at a time (default: what one launch serves), each batch in launches of at most smax samples
    const int batch = g_eve_prior_batch > 0 ? (int)std::min<long long>(g_eve_prior_batch, num_samples) : smax;
    int groups = 0;
    for (int j0 = 0; j0 < num_samples && !rc; j0 += batch) {
        const int j1 = std::min(num_samples, j0 + batch);
        for (int k0 = j0; k0 < j1 && !rc; k0 += smax) {
            const int S = std::min(smax, j1 - k0);
            if (injected) {
                std::vector<void*> pool;
                EveInj inj[EVE_PRIOR_S];
                for (int s = 0; s < S && !rc; ++s) rc = eve_upload_noise(m, injected + k0 + s, 1, pool, &inj[s], false);
                if (!rc) rc = eve_prior_group(m, seed, k0, S, inj);
                rc = side_sync(pm, rc, "EVE log-prior");
                for (void* p : pool) hipFree(p);
            } else {
                rc = eve_prior_group(m, seed, k0, S, nullptr);
            }
            if (!rc && pm->prof && (++groups & 63) == 63) rc = prof_drain(pm);
        }
    }
    if (rc) { hipStreamSynchronize(st); return rc; }
    std::vector<double> a((size_t)3 * m->N);
    PGMI_HIP(hipMemcpyAsync(a.data(), m->pr_acc, a.size() * 8, hipMemcpyDeviceToHost, st));
    PGMI_HIP(hipStreamSynchronize(st));
    const double n = num_samples;
    for (int i = 0; i < m->N; ++i) {
        const double shift = a[3 * (size_t)i], s = a[3 * (size_t)i + 1], ss = a[3 * (size_t)i + 2];
        mean_logp[i] = shift + s / n;
        if (std_logp) std_logp[i] = num_samples > 1 ? sqrt(std::max(0.0, (ss - s * s / n) / (n - 1))) : 0.0;
    }
    return PGMI_OK;
}
