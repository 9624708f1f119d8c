// ESM3 (proteingym/baselines/evoscale/esm/models/esm3.py, layers/{blocks,geom_attention,transformer_stack}.py): model creation, the
// bound window structure, the input embedding and block 0's geometric attention branch.  The plain blocks are ESM C's: the walk
// below sets on Layer exactly what create_esmc (api_esmc.hip) sets, and the forward behind pgmi_token_logprobs / pgmi_masked_logprobs is
// run_encoder / run_head (api_esm.hip).
//
// Input embedding (esm3.py:100-155).  With the defaults of ESM3.forward and ESM3.logits every track but sequence and structure is a
// per-token constant: ss8 and sasa at their pad rows (index 0), the function track at its padding row and the residue annotations at
// the EmbeddingBag's padding index (both zero), average_plddt = 1, per_res_plddt = p in {0, 1}.  create_esm3 folds
//     c[p] = plddt_projection(rbf16(1)) + structure_per_res_plddt_projection(rbf16(p)) + ss8_embed[0] + sasa_embed[0]
// in fp32, in the reference's left-to-right order, and the embedding kernel adds sequence row, structure-token row and c[p].
//
// Block 0 (blocks.py:150-162): x += attn(x) / s; x += geom_attn(x) / s; x += ffn(x) / s.  geom_branch: LayerNorm without bias into the
// split operand, proj [15 Hv, D] on the f16x3 GEMM into fp32 rows (m->qkv, free after the attention), the geometric attention kernel
// (geom_attention.hip) over the window's frames into fp32 rows of Kp = roundup(3 Hv, 32) columns (m->h), split into the GEMM operand
// (m->g16), and out_proj [D, Kp] with the residual and 1/s on its out_scale.
#include "model.h"

namespace pgmi {

namespace {
constexpr int kStructVocab = 4096 + 5;     // esm3.py:87
constexpr int kRbfBins = 16;

int kp_of(int v_heads) { return (3 * v_heads + 31) / 32 * 32; }

// misc.py:55-65 with v_min 0, v_max 1, 16 bins, in fp32
void rbf16(float v, float* out) {
    const float std_ = 1.0f / kRbfBins;
    for (int i = 0; i < kRbfBins; ++i) {
        const float centre = (float)i / (float)(kRbfBins - 1);
        const float z = (v - centre) / std_;
        out[i] = expf(-(z * z));
    }
}
}  // namespace

int esm3_check(const pgmi_config* c, int v_heads) {
    const int Hv = v_heads, D = c->embed_dim, F = c->ffn_dim;
    if (Hv <= 0 || Hv % 4) { set_error("ESM3: v_heads %d must be a positive multiple of 4", Hv); return PGMI_EINVAL; }
    if (15 * Hv > 3 * D || kp_of(Hv) > D || kp_of(Hv) > F) {
        set_error("ESM3: v_heads %d too wide for embed_dim %d / ffn_dim %d (15 v_heads <= 3 D, roundup(3 v_heads, 32) <= min(D, F))", Hv, D, F);
        return PGMI_EINVAL;
    }
    return PGMI_OK;
}

int64_t esm3_weight_count(const pgmi_config* c, int v_heads) {
    const int64_t D = c->embed_dim, F = c->ffn_dim, V = c->vocab, Hv = v_heads;
    const int64_t layer = 2 * D + 3 * D * D + 2 * D + D * D + 2 * D + 2 * F * D + D * F;
    const int64_t geom = 2 * Hv + D + 15 * Hv * D + D * 3 * Hv;
    const int64_t embed = V * D + 2 * (D * kRbfBins + D) + (int64_t)kStructVocab * D + 11 * D + 19 * D;
    return embed + (int64_t)c->layers * layer + geom + D + (D * D + D) + 2 * D + (V * D + V);
}

// Weight blob: include/pgmi.h (PGMI_ARCH_ESM3).
int create_esm3(pgmi_model* m, const pgmi_config* cfg, const float* w, int64_t n_weights, int v_heads) {
    const size_t D = cfg->embed_dim, F = cfg->ffn_dim, V = cfg->vocab, Hv = v_heads, Kp = kp_of(v_heads);
    const float inv_s = 1.0f / sqrtf((float)cfg->layers / 36.0f);      // transformer_stack.py:50
    BlobCursor c(m, w, n_weights);
    c.upload(&m->embed_tokens, V * D);
    {
        const float *pw = c.take(D * kRbfBins), *pb = c.take(D), *sw = c.take(D * kRbfBins), *sb = c.take(D);
        c.upload(&m->e3_struct_embed, (size_t)kStructVocab * D);
        const float *ss8 = c.take(11 * D), *sasa = c.take(19 * D);     // row 0 of each: SS8_PAD_TOKEN = SASA_PAD_TOKEN = 0
        float r1[kRbfBins], rp[kRbfBins];
        rbf16(1.0f, r1);
        std::vector<float> cst(2 * D);
        for (int p = 0; p < 2; ++p) {
            rbf16((float)p, rp);
            for (size_t d = 0; d < D; ++d) {
                float a = 0.f, b = 0.f;
                for (int i = 0; i < kRbfBins; ++i) { a += pw[d * kRbfBins + i] * r1[i]; b += sw[d * kRbfBins + i] * rp[i]; }
                cst[p * D + d] = (((a + pb[d]) + (b + sb[d])) + ss8[d]) + sasa[d];
            }
        }
        c.upload(&m->e3_const, cst.data(), 2 * D);
    }
    m->layers.resize(cfg->layers);
    std::vector<float> qw(D);
    for (int l = 0; l < cfg->layers; ++l) {
        Layer& L = m->layers[l];
        c.upload(&L.ln1_w, D);
        c.upload(&L.ln1_b, D);
        c.w16(&L.wqkv16, 3 * D * D, D);
        const float* q = c.take(D);                                    // 1/sqrt(64) folded into q_ln's weight: exact
        for (size_t i = 0; i < D; ++i) qw[i] = q[i] * 0.125f;
        c.upload(&L.q_ln, qw.data(), D);
        c.upload(&L.k_ln, D);
        c.w16(&L.wo16, D * D, D);
        if (l == 0) {                                                  // transformer_stack.py:32: n_layers_geom = 1
            // F.softplus (beta 1, threshold 20) of the per-head scales, in fp32
            const float *ds = c.take(Hv), *rs = c.take(Hv);
            std::vector<float> wd(Hv), wr(Hv);
            for (size_t h = 0; h < Hv; ++h) {
                wd[h] = ds[h] > 20.0f ? ds[h] : log1pf(expf(ds[h]));
                wr[h] = rs[h] > 20.0f ? rs[h] : log1pf(expf(rs[h]));
            }
            c.upload(&L.g_wdist, wd.data(), Hv);
            c.upload(&L.g_wrot, wr.data(), Hv);
            c.upload(&L.g_norm_w, D);
            c.w16(&L.g_proj16, 15 * Hv * D, D);
            const float* wo = c.take(D * 3 * Hv);
            std::vector<float> wop(D * Kp, 0.0f);                      // zero columns for the K padding
            for (size_t o = 0; o < D; ++o)
                for (size_t i = 0; i < 3 * Hv; ++i) wop[o * Kp + i] = wo[o * 3 * Hv + i];
            c.w16(&L.g_out16, wop.data(), D * Kp, Kp);
            L.g_out16.out_scale *= inv_s;
        }
        c.upload(&L.ln2_w, D);
        c.upload(&L.ln2_b, D);
        c.w16(&L.w116, 2 * F * D, D);
        c.w16(&L.w216, D * F, F);
        L.wo16.out_scale *= inv_s;
        L.w216.out_scale *= inv_s;
    }
    c.upload(&m->lna_w, D);
    m->lna_b = m->zeros;                                               // transformer_stack.py:62: LayerNorm without bias
    c.w16(&m->hd16, D * D, D);
    c.upload(&m->hd_b, D);
    c.upload(&m->hln_w, D);
    c.upload(&m->hln_b, D);
    c.upload(&m->head_w, V * D);
    c.upload(&m->head_b, V);
    m->fc1_epi = EPI_SWIGLU;
    m->fc1_cols = 2 * (int)F;
    m->e3_vheads = v_heads;
    m->e3_Kp = (int)Kp;
    return c.finish();
}

int esm3_embed(pgmi_model* m, int B, int T) {
    if (m->e3_T == 0) { set_error("ESM3: no window structure bound (pgmi_esm3_set_structure)"); return PGMI_EINVAL; }
    if (T != m->e3_T) { set_error("ESM3: T=%d but the bound window has %d tokens", T, m->e3_T); return PGMI_EINVAL; }
    launch_esm3_embed(m->tokens, m->e3_stok, m->e3_plddt, m->embed_tokens, m->e3_struct_embed, m->e3_const, B * T, T, m->cfg.embed_dim,
                      m->x, m->stream);
    return PGMI_OK;
}

int geom_branch(pgmi_model* m, const Layer& L, int B, int T) {
    const int M = B * T, D = m->cfg.embed_dim, Hv = m->e3_vheads, Kp = m->e3_Kp;
    hipStream_t s = m->stream;
    int rc;
    { ProfScope p(m, PGMI_K_LAYERNORM, 0, 2.0 * M * D * 4);
      launch_layernorm16(m->x, L.g_norm_w, m->zeros, M, D, 1e-5f, m->h16, 1, s); }                // geom_attention.py:38: no bias
    { ProfScope p(m, PGMI_K_GEMM_QKV, 2.0 * M * 15 * Hv * D, 0);
      if ((rc = linear(m, nullptr, m->h16, nullptr, L.g_proj16, nullptr, nullptr, m->qkv, nullptr, M, 15 * Hv, D, EPI_NONE))) return rc; }
    { ProfScope p(m, PGMI_K_GEOM, 30.0 * M * T * Hv, (double)M * (15 * Hv + Kp) * 4);
      GeomAttLaunch g;
      g.proj = m->qkv, g.pitch = 15 * Hv;
      g.rot = m->e3_rot, g.trans = m->e3_trans, g.mask = m->e3_mask;
      g.w_rot = L.g_wrot, g.w_dist = L.g_wdist;
      g.B = B, g.S = T, g.H = Hv;
      g.out = m->h, g.opitch = Kp;
      g.stream = s;
      if ((rc = launch_geom_attention(g))) return rc;
      launch_split16(m->h, (int64_t)M * Kp, 1.0f, 2, Kp, m->g16, s); }
    { ProfScope p(m, PGMI_K_GEMM_OUT, 2.0 * M * D * Kp, 0);
      if ((rc = linear(m, nullptr, m->g16, nullptr, L.g_out16, nullptr, m->x, m->x, nullptr, M, D, Kp, EPI_NONE))) return rc; }
    return PGMI_OK;
}

}  // namespace pgmi

extern "C" {

int64_t pgmi_esm3_weight_count(const pgmi_config* cfg, int v_heads) {
    if (!cfg || cfg->layers <= 0 || cfg->embed_dim <= 0 || cfg->ffn_dim <= 0 || v_heads <= 0) return -1;
    return esm3_weight_count(cfg, v_heads);
}

int pgmi_esm3_model_create(const pgmi_config* cfg, int v_heads, const float* weights, int64_t n_weights, int device, pgmi_model** out) {
    if (cfg && cfg->arch != PGMI_ARCH_ESM3) {
        if (out) *out = nullptr;
        set_error("pgmi_esm3_model_create: arch must be PGMI_ARCH_ESM3");
        return PGMI_EINVAL;
    }
    return model_create(cfg, weights, n_weights, device, out, v_heads);
}

int pgmi_esm3_set_structure(pgmi_model* m, const int32_t* structure_tokens, const int32_t* plddt, const float* rot, const float* trans,
                            const int32_t* frame_mask, int T) {
    if (!m || m->cfg.arch != PGMI_ARCH_ESM3) { set_error("pgmi_esm3_set_structure: not an ESM3 model"); return PGMI_EINVAL; }
    if (!structure_tokens || !plddt || !rot || !trans || !frame_mask || T <= 0) { set_error("bad argument"); return PGMI_EINVAL; }
    if (T + 31 > m->max_rows) { set_error("T=%d exceeds workspace rows %d", T, m->max_rows); return PGMI_EINVAL; }
    bool framed = false;
    for (int t = 0; t < T; ++t) {
        if (structure_tokens[t] < 0 || structure_tokens[t] >= kStructVocab) { set_error("structure token %d out of range at %d", structure_tokens[t], t); return PGMI_EINVAL; }
        framed = framed || frame_mask[t] != 0;
    }
    for (int i = 0; i < 12 * T; ++i) {
        const float v = i < 9 * T ? rot[i] : trans[i - 9 * T];
        if (!std::isfinite(v)) { set_error("non-finite frame value (frameless tokens carry the mean frame or the identity)"); return PGMI_EINVAL; }
    }
    PGMI_HIP(hipSetDevice(m->device));
    PGMI_HIP(hipStreamSynchronize(m->stream));               // no forward is reading the previous window
    if ((size_t)T > m->e3_cap) {
        const size_t cap = std::max<size_t>(T, 1024);
        int rc = dev_alloc(m->allocs, &m->e3_stok, cap);
        if (!rc) rc = dev_alloc(m->allocs, &m->e3_plddt, cap);
        if (!rc) rc = dev_alloc(m->allocs, &m->e3_mask, cap);
        if (!rc) rc = dev_alloc(m->allocs, &m->e3_rot, cap * 9);
        if (!rc) rc = dev_alloc(m->allocs, &m->e3_trans, cap * 3);
        if (rc) { m->e3_cap = 0; m->e3_T = 0; return rc; }
        m->e3_cap = cap;
    }
    m->e3_T = 0;
    PGMI_HIP(hipMemcpy(m->e3_stok, structure_tokens, (size_t)T * 4, hipMemcpyHostToDevice));
    PGMI_HIP(hipMemcpy(m->e3_plddt, plddt, (size_t)T * 4, hipMemcpyHostToDevice));
    PGMI_HIP(hipMemcpy(m->e3_mask, frame_mask, (size_t)T * 4, hipMemcpyHostToDevice));
    PGMI_HIP(hipMemcpy(m->e3_rot, rot, (size_t)T * 9 * 4, hipMemcpyHostToDevice));
    PGMI_HIP(hipMemcpy(m->e3_trans, trans, (size_t)T * 3 * 4, hipMemcpyHostToDevice));
    m->e3_T = T;
    m->e3_framed = framed;
    return PGMI_OK;
}

}  // extern "C"
