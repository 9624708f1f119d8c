// C ABI of libpgmi.so (include/pgmi.h): errors, configuration and token checks, weight split, model create / destroy, options and
// profiling.  The per-architecture weight walks live in api_esm / api_esmc / api_saprot / api_tranception / api_progen2 / api_gpt / api_msa.hip, the
// layer loops in api_esm.hip (encoder; SaProt's entries on it in api_saprot.hip), api_gpt.hip (decoder) and api_msa.hip.
#include "model.h"

namespace pgmi {

static thread_local char g_err[1024] = "";
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int prof_drain(pgmi_model* m) {
    if (m->events_used == 0) return PGMI_OK;
    PGMI_HIP(hipStreamSynchronize(m->stream));
    for (size_t i = 0; i < m->events_used; ++i) {
        float ms = 0.f;
        PGMI_HIP(hipEventElapsedTime(&ms, m->events[i].start, m->events[i].stop));
        m->prof_ms[m->events[i].cls] += ms;
    }
    m->events_used = 0;
    return PGMI_OK;
}

int check_cfg(const pgmi_config* c) {
    if (!c) { set_error("null config"); return PGMI_EINVAL; }
    if (c->abi_version != PGMI_ABI_VERSION) { set_error("ABI version mismatch: got %d, library is %d", c->abi_version, PGMI_ABI_VERSION); return PGMI_EINVAL; }
    if (c->arch != PGMI_ARCH_ESM1B && c->arch != PGMI_ARCH_ESM2 && c->arch != PGMI_ARCH_TRANCEPTION && c->arch != PGMI_ARCH_MSA &&
        c->arch != PGMI_ARCH_PROGEN2 && c->arch != PGMI_ARCH_GPT && c->arch != PGMI_ARCH_ESMC && c->arch != PGMI_ARCH_SAPROT &&
        c->arch != PGMI_ARCH_POET && c->arch != PGMI_ARCH_PROGEN3 && c->arch != PGMI_ARCH_ESM3 && c->arch != PGMI_ARCH_ESMIF1 &&
        c->arch != PGMI_ARCH_MULAN) { set_error("unknown arch %d", c->arch); return PGMI_EINVAL; }
    if (c->layers <= 0 || c->embed_dim <= 0 || c->heads <= 0 || c->ffn_dim <= 0) { set_error("non-positive model dimension"); return PGMI_EINVAL; }
    if (c->arch == PGMI_ARCH_ESMIF1) return if1_check(c, c->embed_dim);      // the encoder width is checked at creation
    if (esmc_blocks(c->arch)) {
        // the QK-LayerNorm prep pass holds a q / k row of D <= 2048 in registers; FC1's SwiGLU epilogue pairs 32-column blocks
        if (c->precision != PGMI_PREC_F16X3) { set_error("ESM C is available in precision f16x3 only"); return PGMI_EINVAL; }
        if (c->embed_dim % 32 || c->embed_dim != c->heads * kHeadDim) { set_error("ESM C needs head_dim 64 and d %% 32 == 0 (embed_dim %d, heads %d)", c->embed_dim, c->heads); return PGMI_EINVAL; }
        if (c->embed_dim > 2048) { set_error("ESM C: embed_dim %d above the 2048 this build supports", c->embed_dim); return PGMI_EINVAL; }
        if (c->ffn_dim % 32) { set_error("ESM C: the SwiGLU hidden width %d must be a multiple of 32", c->ffn_dim); return PGMI_EINVAL; }
        if (c->vocab != PGMI_ESMC_VOCAB) { set_error("ESM C vocab must be %d", PGMI_ESMC_VOCAB); return PGMI_EINVAL; }
        return PGMI_OK;
    }
    {
        // head_dim 64 natively; smaller head dims (ESM2 8M/35M/150M: 16/24/32) run zero-padded to 64 lanes per head;
        // head_dim 128 (ESM2-15B: pretrained.py:387-394) as two 64-lane slot groups per head (see pgmi_model_create)
        const int dh = c->embed_dim / c->heads;
        // ProGen2: any even head_dim up to 256, zero-padded to one (<= 64), two (<= 128) or four (<= 256) slot groups per head
        // (api_progen2.hip)
        const bool pg2 = c->arch == PGMI_ARCH_PROGEN2;
        // causal decoder: ESM2's layout (RITA XL: head_dim 128)
        const bool esm_layout = c->arch == PGMI_ARCH_ESM1B || c->arch == PGMI_ARCH_ESM2 || c->arch == PGMI_ARCH_GPT || c->arch == PGMI_ARCH_SAPROT ||
                                c->arch == PGMI_ARCH_MULAN;
        const bool pg3 = c->arch == PGMI_ARCH_PROGEN3;        // what the causal attention runs: 64, 128 and ProGen2's padded 80 / 96 / 256
        if (pg3 && (c->embed_dim % c->heads || (dh != 64 && dh != 80 && dh != 96 && dh != 128 && dh != 256))) {
            set_error("unsupported head_dim %d (embed_dim %d / heads %d): ProGen3 runs head dims 64, 80, 96, 128 and 256", dh, c->embed_dim, c->heads);
            return PGMI_EINVAL;
        }
        const bool poet = c->arch == PGMI_ARCH_POET;          // interleaved rotary pairs in one slot group: even head dims up to 64
        if (poet && c->embed_dim % c->heads == 0 && dh > kHeadDim) {
            set_error("unsupported head_dim %d (embed_dim %d / heads %d): PoET's prefix attention runs even head dims up to 64", dh, c->embed_dim, c->heads);
            return PGMI_EINVAL;
        }
        const bool ok = c->embed_dim % c->heads == 0 &&
                        (dh == kHeadDim || (dh < kHeadDim && dh % 2 == 0 && (esm_layout || poet)) || (dh == 2 * kHeadDim && esm_layout) ||
                         (pg2 && dh % 2 == 0 && dh <= 4 * kHeadDim) || pg3);
        if (pg2 && !ok && c->embed_dim % c->heads == 0 && dh > 4 * kHeadDim) {
            set_error("unsupported head_dim %d (embed_dim %d / heads %d): ProGen2 runs even head dims up to 256", dh, c->embed_dim, c->heads);
            return PGMI_EINVAL;
        }
        if (!ok) { set_error("unsupported head_dim %d (embed_dim %d / heads %d): this build supports head_dim 64, even head dims below 64 and head_dim 128 (ESM)", dh, c->embed_dim, c->heads); return PGMI_EINVAL; }
    }
    if (c->embed_dim % 32 || c->ffn_dim % 32) { set_error("embed_dim and ffn_dim must be multiples of 32"); return PGMI_EINVAL; }
    if (c->arch == PGMI_ARCH_TRANCEPTION) {
        if (c->vocab != 25) { set_error("Tranception vocab must be 25"); return PGMI_EINVAL; }
        if (c->heads % 4) { set_error("Invalid number of heads. Tranception requires the number of heads to be a multiple of 4."); return PGMI_EINVAL; }
        if (c->precision != PGMI_PREC_F16X3) { set_error("Tranception is available in precision f16x3 only"); return PGMI_EINVAL; }
        if (c->max_positions <= 0) { set_error("Tranception needs max_positions = n_ctx"); return PGMI_EINVAL; }
    } else if (c->arch == PGMI_ARCH_PROGEN2) {
        if (c->vocab != PGMI_PG2_VOCAB) { set_error("ProGen2 vocab must be %d", PGMI_PG2_VOCAB); return PGMI_EINVAL; }
        // modeling_progen.py:157-168 splits the fused projection into mp_num = 8 blocks of whole heads
        if (c->heads % 8) { set_error("ProGen2 needs the number of heads to be a multiple of 8 (mp_num = 8), got %d", c->heads); return PGMI_EINVAL; }
        if (c->precision != PGMI_PREC_F16X3) { set_error("ProGen2 is available in precision f16x3 only"); return PGMI_EINVAL; }
        if (c->max_positions <= 0) { set_error("ProGen2 needs max_positions = n_positions"); return PGMI_EINVAL; }
    } else if (c->arch == PGMI_ARCH_GPT) {
        if (c->vocab < 2) { set_error("causal decoder vocab must be at least 2, got %d", c->vocab); return PGMI_EINVAL; }
        if (c->precision != PGMI_PREC_F16X3) { set_error("the causal decoder (RITA / ProtGPT2) is available in precision f16x3 only"); return PGMI_EINVAL; }
        if (c->max_positions <= 0) { set_error("the causal decoder needs max_positions = n_positions / max_seq_len"); return PGMI_EINVAL; }
    } else if (c->arch == PGMI_ARCH_SAPROT) {
        if (c->vocab != PGMI_SAPROT_VOCAB) { set_error("SaProt vocab must be %d (5 specials + 21 x 21 residue tokens)", PGMI_SAPROT_VOCAB); return PGMI_EINVAL; }
        if (c->max_positions != 0) { set_error("SaProt has rotary positions: max_positions must be 0"); return PGMI_EINVAL; }
    } else if (c->arch == PGMI_ARCH_MULAN) {
        if (c->vocab != PGMI_VOCAB && c->vocab != PGMI_SAPROT_VOCAB) { set_error("MULAN vocab must be %d (ESM2's alphabet) or %d (SaProt's)", PGMI_VOCAB, PGMI_SAPROT_VOCAB); return PGMI_EINVAL; }
        if (c->max_positions != 0) { set_error("MULAN has rotary positions: max_positions must be 0"); return PGMI_EINVAL; }
    } else if (c->arch == PGMI_ARCH_POET) {
        if (c->vocab <= PGMI_POET_TOK_MASK || c->vocab > kWave) { set_error("PoET vocab must be in [%d, 64], got %d", PGMI_POET_TOK_MASK + 1, c->vocab); return PGMI_EINVAL; }
        if (c->precision != PGMI_PREC_F16X3) { set_error("PoET is available in precision f16x3 only"); return PGMI_EINVAL; }
        if (c->max_positions < 0) { set_error("PoET: max_positions is the largest prompt in tokens (0: no prompt)"); return PGMI_EINVAL; }
    } else if (c->arch == PGMI_ARCH_PROGEN3) {
        if (c->vocab <= kWave) { set_error("ProGen3 vocab must be above 64 (the wide LM head), got %d", c->vocab); return PGMI_EINVAL; }
        if (c->precision != PGMI_PREC_F16X3) { set_error("ProGen3 is available in precision f16x3 only"); return PGMI_EINVAL; }
        if (c->max_positions <= 0) { set_error("ProGen3 needs max_positions = the rotary table's rows"); return PGMI_EINVAL; }
    } else if (c->vocab != PGMI_VOCAB) { set_error("vocab must be %d", PGMI_VOCAB); return PGMI_EINVAL; }
    if (c->arch == PGMI_ARCH_ESM1B && c->max_positions <= 0) { set_error("ESM-1b arch needs max_positions"); return PGMI_EINVAL; }
    if (c->arch == PGMI_ARCH_MSA) {
        if (c->max_positions <= 0) { set_error("MSA Transformer needs max_positions"); return PGMI_EINVAL; }
        if (c->embed_dim != c->heads * kHeadDim) { set_error("MSA Transformer: head_dim must be 64"); return PGMI_EINVAL; }
        if (c->precision != PGMI_PREC_F16X3) { set_error("MSA Transformer is available in precision f16x3 only"); return PGMI_EINVAL; }
    }
    if (c->precision != PGMI_PREC_FP32 && c->precision != PGMI_PREC_F16X3 && c->precision != PGMI_PREC_BF16) { set_error("unknown precision %d", c->precision); return PGMI_EINVAL; }
    // f16x3: K tiles of 32 (checked above); the bf16 GEMM's K tile is 64
    if (c->precision == PGMI_PREC_BF16 && (c->embed_dim % 64 || c->ffn_dim % 64)) { set_error("precision bf16 needs embed_dim and ffn_dim to be multiples of 64"); return PGMI_EINVAL; }
    return PGMI_OK;
}

// trailing-only padding, at least one real token per sequence
int check_tokens(const int32_t* tokens, int B, int T, int n_ids) {
    for (int b = 0; b < B; ++b) {
        const int32_t* t = tokens + (size_t)b * T;
        bool seen_pad = false;
        if (t[0] == PGMI_TOK_PAD) { set_error("sequence %d is empty (all <pad>)", b); return PGMI_EINVAL; }
        for (int i = 0; i < T; ++i) {
            if (t[i] < 0 || t[i] >= n_ids) { set_error("token id %d out of range at [%d,%d]", t[i], b, i); return PGMI_EINVAL; }
            if (t[i] == PGMI_TOK_PAD) seen_pad = true;
            else if (seen_pad) { set_error("interior <pad> at [%d,%d]: only trailing padding is supported", b, i); return PGMI_EINVAL; }
        }
    }
    return PGMI_OK;
}

// token ids inside [0, V)
int check_vocab(const int32_t* tokens, int B, int T, int V) {
    for (int b = 0; b < B; ++b)
        for (int t = 0; t < T; ++t) {
            const int tk = tokens[(size_t)b * T + t];
            if (tk < 0 || tk >= V) { set_error("token id %d out of range at [%d,%d]", tk, b, t); return PGMI_EINVAL; }
        }
    return PGMI_OK;
}

int env_int(const char* name, int dflt) {
    const char* v = getenv(name);
    return v ? atoi(v) : dflt;
}

// Upload a Linear weight [n_elems] as 16-bit planes.  f16x3: W*2^s with 2^s chosen so that
// max|W|*2^s lies in [8192, 16384): hi stays far below fp16's 65504 and lo = fp16(W' - hi) stays in
// the normal range for every element within 2^-15 of the largest.  bf16: one plane, no scaling.
int make_w16(std::vector<void*>& pool, const float* host, size_t n, size_t K, int precision, hipStream_t s, W16* out) {
    float mx = 0.f;
    for (size_t i = 0; i < n; ++i) mx = std::max(mx, fabsf(host[i]));
    float scale = 1.0f;
    const int planes = (precision == PGMI_PREC_F16X3) ? 2 : 1;
    if (precision == PGMI_PREC_F16X3 && mx > 0.f && std::isfinite(mx)) scale = exp2f(floorf(log2f(16384.0f / mx)));
    float* tmp = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&tmp), n * sizeof(float));
    if (e != hipSuccess) { set_error("hipMalloc failed: %s", hipGetErrorString(e)); return PGMI_ENOMEM; }
    int rc = dev_alloc(pool, &out->p, n * planes);
    if (rc) { hipFree(tmp); return rc; }
    e = hipMemcpy(tmp, host, n * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        launch_split16(tmp, (int64_t)n, scale, precision == PGMI_PREC_BF16 ? 1 : 0, (int)K, out->p, s);
        e = hipStreamSynchronize(s);
    }
    hipFree(tmp);
    if (e != hipSuccess) { set_error("weight split failed: %s", hipGetErrorString(e)); return PGMI_EHIP; }
    out->out_scale = 1.0f / scale;
    return PGMI_OK;
}

// y = epi(in W^T + b) (+ residual).  fp32 mode: in32 -> fp32 out.  16-bit modes: in16 planes ->
// either fp32 out (out32) or 16-bit planes (out16).
int linear(pgmi_model* m, const float* in32, const unsigned short* in16, const float* W32, const W16& w16, const float* bias,
           const float* residual, float* out32, unsigned short* out16, int M, int N, int K, int epi) {
    if (m->cfg.precision == PGMI_PREC_FP32)
        return launch_gemm_f32(in32, W32, bias, residual, out32, M, N, K, epi, m->stream);
    GemmLaunch g;
    g.A = in16; g.W = w16.p; g.out_scale = w16.out_scale;
    g.bias = bias; g.residual = residual;
    g.out32 = out32; g.out16 = out16;
    g.M = M; g.N = N; g.K = K;
    g.epilogue = epi; g.bf = m->cfg.precision == PGMI_PREC_BF16; g.variant = m->gemm_variant; g.stream = m->stream;
    return launch_gemm16(g);
}

// The fused QKV projection of m->h16 (M rows, sequences of T) into the attention operands m->qk16 / m->vt16: f16x3, no rotary; the
// caller sets what differs (bf, the rotary tables).  Da = H * 64 attention lanes.
GemmLaunch qkv_launch(pgmi_model* m, const W16& w16, const float* bias, int M, int Da, int K, int T, int H) {
    GemmLaunch g;
    g.A = m->h16; g.W = w16.p; g.out_scale = w16.out_scale;
    g.bias = bias;
    g.out16 = m->qk16;
    g.M = M; g.N = 3 * Da; g.K = K;
    g.variant = m->gemm_variant; g.stream = m->stream;
    g.qkv.vt16 = m->vt16; g.qkv.vt_plane = m->vt16_plane; g.qkv.qk_plane = m->qk16_plane;
    g.qkv.T = T; g.qkv.H = H;
    return g;
}

// A launch of attention_prefix.hip over the uploaded segments of pl: the q planes in m->qk16, split context rows into m->h16.  The
// caller sets what differs: qkv / pos and the rotary tables of a prep pass, the own planes and their pitch, the prefix planes and P.
PrefixAttLaunch prefix_launch(pgmi_model* m, const SegPlan& pl) {
    PrefixAttLaunch a;
    a.seg_off = pl.d_seg_off; a.ent_seg = pl.d_ent_seg; a.ent_tile = pl.d_ent_tile;
    a.n_seg = pl.n_seg(); a.n_ent = pl.n_ent(); a.H = m->cfg.heads;
    a.q16 = m->qk16; a.q_plane = (size_t)m->max_rows * m->Da;
    a.out = ATT_OUT_SPLIT; a.ctx16 = m->h16; a.stream = m->stream;
    return a;
}

int alloc_prefix_cache(pgmi_model* m) {
    PrefixCache& c = m->pfx;
    c.pitch = ((size_t)m->cfg.max_positions + 31) / 32 * 32;
    c.plane = (size_t)m->Da * c.pitch;
    c.cap = (size_t)m->max_rows;
    int rc = PGMI_OK;
    if (c.pitch) {
        const size_t n = (size_t)m->cfg.layers * 4 * c.plane;
        rc = dev_alloc(m->allocs, &c.planes, n);
        if (!rc) PGMI_HIP(hipMemset(c.planes, 0, n * sizeof(unsigned short)));
    }
    if (!rc) rc = dev_alloc(m->allocs, &c.meta, PrefixCache::meta_ints(c.cap));
    if (!rc) rc = dev_alloc(m->allocs, &m->gpt_sum, c.cap);
    return rc;
}

// fp16 range check for the 16-bit modes: the vocabulary kernel raises the flag when a computed
// log-probability is NaN/inf (an activation exceeded fp16's 65504 upstream).
int check_nonfinite(pgmi_model* m) {
    if (m->cfg.precision == PGMI_PREC_FP32) return PGMI_OK;
    int32_t flag = 0;
    PGMI_HIP(hipMemcpyAsync(&flag, m->nonfinite, 4, hipMemcpyDeviceToHost, m->stream));
    PGMI_HIP(hipStreamSynchronize(m->stream));
    if (flag) {
        PGMI_HIP(hipMemsetAsync(m->nonfinite, 0, 4, m->stream));
        set_error("non-finite log-probabilities: an activation left the fp16/bf16 range in precision mode %d; "
                  "re-run with precision fp32", m->cfg.precision);
        return PGMI_EOVERFLOW;
    }
    return PGMI_OK;
}

// Pad keys (t >= T inside the last 32-key tile) are never written by the fused QKV epilogue: they must hold finite data (their
// softmax weight is exactly 0).  The V^T planes are cleared whenever the batch shape changes (precision fp32 has none).
int reset_pad_keys(pgmi_model* m, int B, int T) {
    if (!m->vt16 || (B == m->last_B && T == m->last_T)) return PGMI_OK;
    PGMI_HIP(hipMemsetAsync(m->vt16, 0, m->vt16_plane * 2 * sizeof(unsigned short), m->stream));
    m->last_B = B;
    m->last_T = T;
    return PGMI_OK;
}

}  // namespace pgmi

extern "C" {

int pgmi_abi_version(void) { return PGMI_ABI_VERSION; }

const char* pgmi_last_error(void) { return g_err; }

int pgmi_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int64_t pgmi_weight_count(const pgmi_config* c) {
    if (!c || c->layers <= 0 || c->embed_dim <= 0 || c->ffn_dim <= 0) return -1;
    const int64_t D = c->embed_dim, F = c->ffn_dim, V = c->vocab;
    if (c->arch == PGMI_ARCH_TRANCEPTION) {
        const int64_t conv = 3 * ((64 * 3 + 64) + (64 * 5 + 64) + (64 * 7 + 64));
        return V * D + (int64_t)c->layers * (2 * D + (D * 3 * D + 3 * D) + conv + (D * D + D) + 2 * D + (D * F + F) + (F * D + D)) + 2 * D + V * D;
    }
    if (c->arch == PGMI_ARCH_PROGEN2)        // include/pgmi.h: the ProGen2 blob
        return V * D + (int64_t)c->layers * (2 * D + 3 * D * D + D * D + (F * D + F) + (D * F + D)) + 2 * D + V * D + V;
    if (c->arch == PGMI_ARCH_GPT) return -1;      // the blob depends on pos_kind: pgmi_gpt_weight_count
    if (c->arch == PGMI_ARCH_POET) return -1;     // the blob depends on final_norm: pgmi_poet_weight_count
    if (c->arch == PGMI_ARCH_PROGEN3) return -1;  // the blob depends on pgmi_pg3_params: pgmi_pg3_weight_count
    if (c->arch == PGMI_ARCH_ESM3) return -1;     // the blob depends on v_heads: pgmi_esm3_weight_count
    if (c->arch == PGMI_ARCH_ESMIF1) return -1;   // the blob depends on the encoder width: pgmi_esmif1_weight_count
    if (c->arch == PGMI_ARCH_ESMC) return esmc_weight_count(c);
    if (c->arch == PGMI_ARCH_MULAN) return -1;    // ESM2's blob and the adapter's: pgmi_mulan_weight_count
    if (c->arch == PGMI_ARCH_MSA) {
        const int64_t attn = 2 * D + 4 * (D * D + D);
        return V * D + (int64_t)(c->max_positions + 2) * D + 1024 * D + 2 * D +
               (int64_t)c->layers * (2 * attn + 2 * D + (F * D + F) + (D * F + D)) + 2 * D + (D * D + D) + 2 * D + V;
    }
    int64_t n = V * D;
    if (c->arch == PGMI_ARCH_ESM1B) n += (int64_t)(c->max_positions + 2) * D;
    if (c->emb_layer_norm_before) n += 2 * D;
    n += (int64_t)c->layers * (2 * D + 4 * (D * D + D) + 2 * D + (F * D + F) + (D * F + D));
    n += 2 * D + (D * D + D) + 2 * D + V;
    return n;
}

int pgmi_model_create(const pgmi_config* cfg, const float* w, int64_t n_weights, int device, pgmi_model** out) {
    if (cfg && cfg->arch == PGMI_ARCH_PROGEN2) {
        if (out) *out = nullptr;
        set_error("ProGen2 models are created with pgmi_pg2_model_create (it takes rotary_dim)");
        return PGMI_EINVAL;
    }
    if (cfg && cfg->arch == PGMI_ARCH_GPT) {
        if (out) *out = nullptr;
        set_error("causal decoder models are created with pgmi_gpt_model_create (it takes pos_kind)");
        return PGMI_EINVAL;
    }
    if (cfg && cfg->arch == PGMI_ARCH_SAPROT) {
        if (out) *out = nullptr;
        set_error("SaProt models are created with pgmi_saprot_model_create (it takes the tokenizer's <mask> id)");
        return PGMI_EINVAL;
    }
    if (cfg && cfg->arch == PGMI_ARCH_MULAN) {
        if (out) *out = nullptr;
        set_error("MULAN models are created with pgmi_mulan_model_create (it takes the <mask> id and the vocabulary's groups)");
        return PGMI_EINVAL;
    }
    if (cfg && cfg->arch == PGMI_ARCH_POET) {
        if (out) *out = nullptr;
        set_error("PoET models are created with pgmi_poet_model_create (it takes final_norm)");
        return PGMI_EINVAL;
    }
    if (cfg && cfg->arch == PGMI_ARCH_PROGEN3) {
        if (out) *out = nullptr;
        set_error("ProGen3 models are created with pgmi_pg3_model_create (it takes pgmi_pg3_params)");
        return PGMI_EINVAL;
    }
    if (cfg && cfg->arch == PGMI_ARCH_ESM3) {
        if (out) *out = nullptr;
        set_error("ESM3 models are created with pgmi_esm3_model_create (it takes v_heads)");
        return PGMI_EINVAL;
    }
    if (cfg && cfg->arch == PGMI_ARCH_ESMIF1) {
        if (out) *out = nullptr;
        set_error("ESM-IF1 decoders are created with pgmi_esmif1_model_create (it takes the encoder width)");
        return PGMI_EINVAL;
    }
    return model_create(cfg, w, n_weights, device, out, 0);
}

}  // extern "C"

namespace pgmi {

// Workspace of max_rows token rows, shared by every forward of the model.
static int alloc_workspace(pgmi_model* m) {
    const pgmi_config& c = m->cfg;
    const size_t R = m->max_rows, D = c.embed_dim, V = c.vocab, Da = m->Da;
    const size_t F = c.arch == PGMI_ARCH_MULAN ? std::max<size_t>(c.ffn_dim, 4 * D) : c.ffn_dim;   // MULAN's adapter layer: 4 D
    const size_t Dw = std::max(D, Da);                   // h / h16 hold LN output [.,D] and attention context [.,Da]
    const bool f32mode = c.precision == PGMI_PREC_FP32;
    int rc = PGMI_OK;
    auto alloc = [&](auto** p, size_t n) { if (!rc) rc = dev_alloc(m->allocs, p, n); };
    alloc(&m->x, R * D);
    alloc(&m->h, R * Dw);
    alloc(&m->qkv, R * 3 * Da);
    alloc(&m->g, R * (f32mode ? std::max(F, D) : D));
    if (!f32mode) {
        const size_t planes = c.precision == PGMI_PREC_F16X3 ? 2 : 1;
        m->h16_plane = R * Dw;
        m->g16_plane = R * F;
        alloc(&m->h16, m->h16_plane * planes);
        alloc(&m->g16, m->g16_plane * planes);
    }
    alloc(&m->nonfinite, (size_t)1);
    if (!f32mode) {                                      // (bf16 mode: its attention runs on the split-fp16 operands as well)
        m->qk16_plane = R * 2 * Da;
        m->vt16_plane = R * Da;
        alloc(&m->qk16, m->qk16_plane * 2);
        alloc(&m->vt16, m->vt16_plane * 2);
    }
    if (c.arch == PGMI_ARCH_MSA) {
        alloc(&m->xt, R * D);
        alloc(&m->msa_kv_len, (size_t)2048);
    }
    // the wide causal-decoder head writes its full rows per head chunk (api_gpt.hip): R * V would be ~20 GB at V = 50 257
    alloc(&m->lp, ((c.arch == PGMI_ARCH_GPT || c.arch == PGMI_ARCH_PROGEN3) && V > kWave ? (size_t)m->gpt_head_rows : R) * V);
    alloc(&m->denom, R);
    alloc(&m->tokens, R);
    alloc(&m->pos_idx, R);
    alloc(&m->kv_len, R);
    alloc(&m->row_idx, R);
    alloc(&m->aux_i, R);
    if (rc) return rc;
    PGMI_HIP(hipMemset(m->nonfinite, 0, 4));
    if (m->vt16) PGMI_HIP(hipMemset(m->vt16, 0, m->vt16_plane * 2 * sizeof(unsigned short)));
    return PGMI_OK;
}

// pgmi_model_create, pgmi_pg2_model_create and pgmi_gpt_model_create; arch_arg is ProGen2's rotary_dim or the causal decoder's
// pos_kind, SaProt's and MULAN's <mask> id, PoET's final_norm, ESM3's v_heads, ESM-IF1's encoder width (0 for every other arch); pg3: ProGen3's parameters
int model_create(const pgmi_config* cfg, const float* w, int64_t n_weights, int device, pgmi_model** out, int arch_arg,
                 const pgmi_pg3_params* pg3) {
    if (!out) { set_error("null out"); return PGMI_EINVAL; }
    *out = nullptr;
    int rc = check_cfg(cfg);
    if (rc) return rc;
    if (cfg->arch == PGMI_ARCH_PROGEN3 && (rc = pg3_check(cfg, pg3))) return rc;
    if (cfg->arch == PGMI_ARCH_ESM3 && (rc = esm3_check(cfg, arch_arg))) return rc;
    if (cfg->arch == PGMI_ARCH_ESMIF1 && (rc = if1_check(cfg, arch_arg))) return rc;
    const int64_t need = cfg->arch == PGMI_ARCH_GPT ? gpt_weight_count(cfg, arch_arg)
                         : cfg->arch == PGMI_ARCH_PROGEN3 ? pg3_weight_count(cfg, pg3)
                         : cfg->arch == PGMI_ARCH_POET ? poet_weight_count(cfg, arch_arg)
                         : cfg->arch == PGMI_ARCH_ESM3 ? esm3_weight_count(cfg, arch_arg)
                         : cfg->arch == PGMI_ARCH_ESMIF1 ? if1_weight_count(cfg, arch_arg)
                         : cfg->arch == PGMI_ARCH_MULAN ? mulan_weight_count(cfg) : pgmi_weight_count(cfg);
    if (need < 0) { set_error("causal decoder pos_kind %d: must be PGMI_GPT_POS_ROTARY or PGMI_GPT_POS_LEARNED", arch_arg); return PGMI_EINVAL; }
    if (!w || n_weights != need) {
        set_error("weight blob has %lld elements, config needs %lld", (long long)n_weights, (long long)need);
        return PGMI_EINVAL;
    }
    const int ndev = pgmi_device_count();
    if (ndev <= 0) { set_error("no HIP device visible (libpgmi has no CPU fallback)"); return PGMI_ENODEV; }
    if (device < 0 || device >= ndev) { set_error("device %d out of range (%d visible)", device, ndev); return PGMI_EINVAL; }
    PGMI_HIP(hipSetDevice(device));
    pgmi_model* m = new pgmi_model();
    m->cfg = *cfg;
    m->device = device;
    if (hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking) != hipSuccess) { set_error("hipStreamCreate failed"); delete m; return PGMI_EHIP; }
    m->dh = cfg->embed_dim / cfg->heads;
    m->rot_halves = m->dh > 2 * kHeadDim ? 4 : m->dh > kHeadDim ? 2 : 1;     // 4: ProGen2 head dims above 128 (check_cfg)
    m->Hs = cfg->heads * m->rot_halves;
    m->Da = m->Hs * kHeadDim;
    m->ln_eps = cfg->ln_eps > 0.f ? cfg->ln_eps : 1e-5f;
    m->max_rows = std::max(cfg->max_rows > 0 ? cfg->max_rows : 98304, 2048);
    const size_t V = cfg->vocab;
    const std::vector<float> zeros(std::max({3 * (size_t)m->Da, (V + 63) / 64 * 64, (size_t)cfg->embed_dim, V, (size_t)cfg->heads}), 0.0f);
    rc = dev_upload(m->allocs, &m->zeros, zeros.data(), zeros.size());
    m->fc1_cols = cfg->ffn_dim;                          // ESM C's SwiGLU FC1: 2 ffn_dim (create_esmc)
    if (!rc) switch (cfg->arch) {
        case PGMI_ARCH_TRANCEPTION: rc = create_tranception(m, cfg, w, n_weights); break;
        case PGMI_ARCH_MSA: rc = create_msa(m, cfg, w, n_weights); break;
        case PGMI_ARCH_PROGEN2: rc = create_progen2(m, cfg, w, n_weights, arch_arg); break;
        case PGMI_ARCH_GPT: rc = create_gpt(m, cfg, w, n_weights, arch_arg); break;
        case PGMI_ARCH_ESMC: rc = create_esmc(m, cfg, w, n_weights); break;
        case PGMI_ARCH_SAPROT: rc = create_saprot(m, cfg, w, n_weights, arch_arg); break;
        case PGMI_ARCH_MULAN: rc = create_mulan(m, cfg, w, n_weights, arch_arg); break;
        case PGMI_ARCH_POET: rc = create_poet(m, cfg, w, n_weights, arch_arg); break;
        case PGMI_ARCH_PROGEN3: rc = create_progen3(m, cfg, w, n_weights, pg3); break;
        case PGMI_ARCH_ESM3: rc = create_esm3(m, cfg, w, n_weights, arch_arg); break;
        case PGMI_ARCH_ESMIF1: rc = create_esmif1(m, cfg, w, n_weights, arch_arg); break;
        default: rc = create_esm(m, cfg, w, n_weights);
    }
    if (!rc) rc = alloc_workspace(m);
    if (rc) { pgmi_model_destroy(m); return rc; }
    m->keep_rows = env_int("PGMI_KEEP_ROWS", 1);
    gemm_options_from_env();                             // the GEMM launchers' test hooks: read here, not per launch
    m->gemm_variant = env_int("PGMI_GEMM_VARIANT", 0);   // tuning only (gemm_f16.hip gemm_group_m); below 1000 = the product configuration
    *out = m;
    return PGMI_OK;
}

}  // namespace pgmi

namespace pgmi {

int side_open(pgmi_model* pm, const char* name, const float* w, int64_t n_weights, int64_t want, bool scan_finite, int device, int precision,
              hipStream_t lend) {
    if (!w || n_weights != want) {
        set_error("%s weight blob has %lld elements, config needs %lld", name, (long long)n_weights, (long long)want);
        return PGMI_EINVAL;
    }
    for (int64_t i = 0; scan_finite && i < n_weights; ++i)
        if (!std::isfinite(w[i])) { set_error("%s: weight blob element %lld is not finite", name, (long long)i); return PGMI_EINVAL; }
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) { set_error("no HIP device (libpgmi has no CPU fallback)"); return PGMI_ENODEV; }
    if (device < 0 || device >= n_dev) { set_error("device %d out of range (%d visible)", device, n_dev); return PGMI_EINVAL; }
    PGMI_HIP(hipSetDevice(device));
    gemm_options_from_env();
    pm->device = device;
    pm->cfg.precision = precision;                       // what BlobCursor and linear() read
    if (lend) pm->stream = lend;
    else if (hipStreamCreate(&pm->stream) != hipSuccess) { set_error("hipStreamCreate failed"); return PGMI_EHIP; }
    return PGMI_OK;
}

int side_sync(pgmi_model* pm, int rc, const char* what) {
    const hipError_t e1 = hipGetLastError(), e2 = hipStreamSynchronize(pm->stream);
    if (!rc && (e1 != hipSuccess || e2 != hipSuccess)) {
        set_error("%s failed: %s", what, hipGetErrorString(e1 != hipSuccess ? e1 : e2));
        rc = PGMI_EHIP;
    }
    return rc;
}

int overflow_error(int precision) {
    set_error("non-finite log-probabilities%s", precision == PGMI_PREC_F16X3
              ? ": an activation left the fp16 range in precision f16x3; re-run with precision fp32" : "");
    return PGMI_EOVERFLOW;
}

void side_release(pgmi_model* pm, bool own_stream) {
    hipSetDevice(pm->device);
    if (pm->stream) hipStreamSynchronize(pm->stream);
    for (ProfEvent& e : pm->events) { hipEventDestroy(e.start); hipEventDestroy(e.stop); }
    for (void* p : pm->allocs) hipFree(p);
    if (pm->stream && own_stream) hipStreamDestroy(pm->stream);
}

}  // namespace pgmi

extern "C" {

void pgmi_model_destroy(pgmi_model* m) {
    if (!m) return;
    hipSetDevice(m->device);
    if (m->stream) hipStreamSynchronize(m->stream);
    for (pgmi_assay* a : m->assays) {           // assays outliving their model become inert handles
        for (void* p : a->allocs) hipFree(p);
        a->allocs.clear();
        a->m = nullptr;
    }
    m->assays.clear();
    for (pgmi_pppl* q : m->pppls) {
        for (void* p : q->allocs) hipFree(p);
        q->allocs.clear();
        q->m = nullptr;
    }
    m->pppls.clear();
    for (auto& e : m->events) { hipEventDestroy(e.start); hipEventDestroy(e.stop); }
    if (m->moe.counts_host) hipHostFree(m->moe.counts_host);
    for (void* p : m->allocs) hipFree(p);
    if (m->stream) hipStreamDestroy(m->stream);
    delete m;
}

int pgmi_model_device(const pgmi_model* m) { return m ? m->device : -1; }

int pgmi_set_option(const char* name, int64_t value) {
    if (!name) { set_error("null option name"); return PGMI_EINVAL; }
    int rc = gemm_set_option(name, (long long)value);
    if (rc) rc = att_set_option(name, (long long)value);
    if (rc) rc = eve_set_option(name, (long long)value);
    if (rc) rc = mpnn_set_option(name, (long long)value);
    if (rc) rc = unirep_set_option(name, (long long)value);
    if (rc) rc = s2f_set_option(name, (long long)value);
    if (rc) rc = prosst_set_option(name, (long long)value);
    if (rc) set_error("unknown option '%s' (gemm_half_tail, gemm_max_rows, att_xcd_local, att_v3, eve_max_rows, eve_fixed_sample, eve_prior_batch, mpnn_max_rows, unirep_max_rows, s2f_max_rows, prosst_max_rows, prosst_share_layer0)", name);
    return rc;
}

int pgmi_synchronize(pgmi_model* m) {
    if (!m) { set_error("null model"); return PGMI_EINVAL; }
    PGMI_HIP(hipStreamSynchronize(m->stream));
    return PGMI_OK;
}

int pgmi_profile_enable(pgmi_model* m, int on) {
    if (!m) { set_error("null model"); return PGMI_EINVAL; }
    int rc = prof_drain(m);
    m->prof = on != 0;
    return rc;
}

int pgmi_profile_reset(pgmi_model* m) {
    if (!m) { set_error("null model"); return PGMI_EINVAL; }
    int rc = prof_drain(m);
    for (int i = 0; i < PGMI_K_COUNT; ++i) { m->prof_ms[i] = 0; m->prof_n[i] = 0; m->prof_flops[i] = 0; m->prof_bytes[i] = 0; }
    return rc;
}

int pgmi_profile_get(pgmi_model* m, int k, double* ms, int64_t* launches, double* flops, double* bytes) {
    if (!m || k < 0 || k >= PGMI_K_COUNT) { set_error("bad argument"); return PGMI_EINVAL; }
    int rc = prof_drain(m);
    if (rc) return rc;
    if (ms) *ms = m->prof_ms[k];
    if (launches) *launches = m->prof_n[k];
    if (flops) *flops = m->prof_flops[k];
    if (bytes) *bytes = m->prof_bytes[k];
    return PGMI_OK;
}

}  // extern "C"
