// Single-op and timing entries of include/pgmi.h (numerics tests against torch ops; interleaved A/B of launch parameters).  Every entry
// that touches the device checks its arguments, then makes an OpScope (model.h): the device, the pool, the transfers and the timer.
#include "model.h"

// The op entries' GEMMs on their own buffers: f16x3, no epilogue, no output yet -- the caller sets what differs
static GemmLaunch op_gemm(const unsigned short* a16, const W16& w16, const float* bias, int M, int N, int K, int variant) {
    GemmLaunch g;
    g.A = a16; g.W = w16.p; g.out_scale = w16.out_scale;
    g.bias = bias;
    g.M = M; g.N = N; g.K = K;
    g.variant = variant;
    return g;
}

// The attention operands of M rows of width Da: q | k planes qk16 [2][M][2 Da] and V^T planes vt16 [2][M / T][Da][roundup32(T)]
struct QkvPlanes {
    unsigned short *qk16 = nullptr, *vt16 = nullptr;
    size_t qk_plane = 0, vt_plane = 0;
};

// X [M][K] through the fused QKV projection into `o`, as the layer loops run it: the activation split, the weight planes of W [3 Da][K],
// the f16x3 GEMM with H slot groups per token on sequences of T rows.  cos_t / sin_t (device, or neither): rotary with rot_halves table
// rows per token.
static void op_qkv_project(OpScope& s, const float* X, const float* W, const float* bias, size_t M, size_t Da, int K, const QkvPlanes& o,
                           int T, int H, const float* cos_t = nullptr, const float* sin_t = nullptr, int rot_halves = 1) {
    float* dx = s.up(X, M * K);
    float* db = s.up(bias, 3 * Da);
    unsigned short* a16 = s.alloc<unsigned short>(M * K * 2);
    const W16 w16 = s.w16(W, 3 * Da * K, (size_t)K);
    if (s.rc) return;
    gemm_options_from_env();
    launch_split16(dx, (int64_t)(M * K), 1.0f, 2, K, a16, nullptr);
    GemmLaunch g = op_gemm(a16, w16, db, (int)M, 3 * (int)Da, K, env_int("PGMI_GEMM_VARIANT", 0));
    g.out16 = o.qk16;
    g.qkv.vt16 = o.vt16; g.qkv.vt_plane = o.vt_plane; g.qkv.qk_plane = o.qk_plane;
    g.qkv.cos_t = cos_t; g.qkv.sin_t = sin_t; g.qkv.rotary = cos_t != nullptr;
    g.qkv.T = T; g.qkv.H = H; g.qkv.rot_halves = rot_halves;
    s.rc = launch_gemm16(g);
}

// two row-major planes of n halfs (hi, then lo) back as fp32
static void op_fetch_flat(OpScope& s, float* host, const unsigned short* dev16, size_t n) {
    std::vector<unsigned short> h(s.rc ? 0 : 2 * n);
    s.down(h.data(), dev16, h.size());
    for (size_t i = 0; i < n && !s.rc; ++i) host[i] = rebuild_split(h[i], h[n + i]);
}

// the V^T planes [B][D][Tp] of sequences of T keys back as fp32 rows v [B][T][D]
static void op_fetch_vt(OpScope& s, float* v, const unsigned short* vt16, int B, int T, size_t D) {
    const size_t Tp = roundup32((size_t)T), plane = (size_t)B * Tp * D;
    std::vector<unsigned short> h(s.rc ? 0 : 2 * plane);
    s.down(h.data(), vt16, h.size());
    for (int b = 0; b < B && !s.rc; ++b)
        for (int t = 0; t < T; ++t) {
            const int tk = t & 31, pos = (t & ~31) + ((tk & 0x13) | ((tk & 4) << 1) | ((tk & 8) >> 1));   // keys with bits 2, 3 swapped
            for (size_t c = 0; c < D; ++c) {
                const size_t o = ((size_t)b * D + c) * Tp + pos;
                v[((size_t)b * T + t) * D + c] = rebuild_split(h[o], h[plane + o]);
            }
        }
}

// PoET's prefix attention (cross = false: x = own rows q | k | v [R][3 Da], cached = the prefix's k | v rows, P >= 0 of them) and
// ESM-IF1's cross-attention (cross = true: x = q rows [R][Da], cached = the memory's k | v rows, P > 0) through attention_prefix.hip's
// launchers: the cached planes are filled by the prep pass over one segment of P rows, as pgmi_poet_set_prompt and
// pgmi_esmif1_set_memory fill theirs.  What the kernels must write themselves starts as 0xFF bytes (NaN): an operand element or a
// context row they skip shows.
static int op_cached_attention(const char* what, int device, bool cross, const float* x, const int32_t* seg_off, int n_seg,
                               const float* cached, int P, int heads, int split, float* ctx) {
    std::vector<int32_t> ent_seg, ent_tile, pseg{0, P}, pent_seg, pent_tile;
    for (int b = 0; b < n_seg; ++b) {
        const int len = seg_off[b + 1] - seg_off[b];
        if (len <= 0) { set_error("segment %d is empty", b); return PGMI_EINVAL; }
        for (int j = 0; j * 32 < len; ++j) { ent_seg.push_back(b); ent_tile.push_back(j); }
    }
    for (int j = 0; j * 32 < P; ++j) { pent_seg.push_back(0); pent_tile.push_back(j); }
    OpScope s(what, device);
    const size_t R = (size_t)seg_off[n_seg], Da = (size_t)heads * kHeadDim, pitch = ent_seg.size() * 32, ppitch = pent_seg.size() * 32;
    std::vector<float> pq((size_t)P * 3 * Da, 0.0f);            // the cached rows as q | k | v with a zero q block
    for (size_t t = 0; t < (size_t)P; ++t) memcpy(&pq[t * 3 * Da + Da], cached + t * 2 * Da, 2 * Da * sizeof(float));
    const float* dx = s.up(x, R * (cross ? 1 : 3) * Da);
    PrefixAttLaunch a;
    a.seg_off = s.up(seg_off, (size_t)n_seg + 1); a.ent_seg = s.up(ent_seg); a.ent_tile = s.up(ent_tile);
    a.n_seg = n_seg; a.n_ent = (int)ent_seg.size(); a.H = heads;
    a.q16 = s.alloc<unsigned short>(2 * R * Da, cross ? 0xFF : -1); a.q_plane = R * Da;
    if (!cross) {
        a.qkv = dx;
        a.k16 = s.alloc<unsigned short>(2 * Da * pitch, 0xFF); a.vt16 = s.alloc<unsigned short>(2 * Da * pitch, 0xFF); a.pitch = pitch;
    }
    a.ppitch = ppitch; a.P = P;
    a.out = split ? ATT_OUT_SPLIT : ATT_OUT_F32;
    a.ctx = s.alloc<float>(R * Da, 0xFF); a.ctx16 = s.alloc<unsigned short>(2 * R * Da, 0xFF);
    if (P > 0) {
        PrefixAttLaunch p;
        p.qkv = s.up(pq); p.seg_off = s.up(pseg); p.ent_seg = s.up(pent_seg); p.ent_tile = s.up(pent_tile);
        p.n_seg = 1; p.n_ent = (int)pent_seg.size(); p.H = heads;
        p.q16 = s.alloc<unsigned short>(2 * (size_t)P * Da); p.q_plane = (size_t)P * Da;
        p.k16 = s.alloc<unsigned short>(2 * Da * ppitch, 0xFF); p.vt16 = s.alloc<unsigned short>(2 * Da * ppitch, 0xFF); p.pitch = ppitch;
        a.pk16 = p.k16; a.pvt16 = p.vt16;
        if (!s.rc) s.rc = launch_prefix_prep(p);
    }
    if (!s.rc) s.rc = cross ? launch_cross_q_prep(dx, R, heads, a.q16, R * Da, nullptr) : launch_prefix_prep(a);
    if (!s.rc) s.rc = cross ? launch_cross_attention(a) : launch_prefix_attention(a);
    s.sync();
    if (split) s.planes(ctx, a.ctx16, R, Da);
    else s.down(ctx, a.ctx, R * Da);
    return s.rc;
}

extern "C" {

// ---- single-op entry points for the numerics tests -------------------------------------------
int pgmi_op_layernorm(int device, const float* x, const float* w, const float* b, int rows, int D, float eps, float* y) {
    if (!x || !w || !b || !y || rows <= 0 || D <= 0 || D % 4) { set_error("bad argument"); return PGMI_EINVAL; }
    OpScope s("layernorm op", device);
    const size_t n = (size_t)rows * D;
    float* dx = s.up(x, n);
    float* dw = s.up(w, (size_t)D);
    float* db = s.up(b, (size_t)D);
    float* dy = s.alloc<float>(n);
    if (s.rc) return s.rc;
    launch_layernorm(dx, dw, db, rows, D, eps, dy, nullptr);
    s.sync();
    s.down(y, dy, n);
    return s.rc;
}

int pgmi_op_rmsnorm(int device, const float* x, const float* w, int rows, int D, float eps, float* y) {
    if (!x || !w || !y || rows <= 0 || D <= 0) { set_error("bad argument"); return PGMI_EINVAL; }
    if (D % 32) { set_error("rmsnorm op: D = %d is not a multiple of 32 (the K-interleaved operand)", D); return PGMI_EINVAL; }
    OpScope s("rmsnorm op", device);
    float* dx = s.up(x, (size_t)rows * D);
    float* dw = s.up(w, (size_t)D);
    unsigned short* y16 = s.alloc<unsigned short>((size_t)rows * D * 2, 0xFF);     // an element the kernel skips shows as NaN
    if (!s.rc) s.rc = launch_rmsnorm16(dx, dw, rows, D, eps, y16, nullptr);
    s.sync();
    s.planes(y, y16, (size_t)rows, (size_t)D);
    return s.rc;
}

// ProGen3's feed-forward block (api_progen3.hip pg3_ffn without the norm) on rows taken as they are: the router kernel splits them and
// routes them, then moe_ffn (or, for one expert, dense_ffn) adds the block's output into a zeroed x.
int pgmi_op_moe(int device, const float* h, const float* gate, const float* w1, const float* w3, const float* w2, int M, int D, int F,
                int E, int top_k, int gated, float* out, int32_t* ids, float* weights) {
    if (!h || !w1 || !w2 || !out || (gated && !w3) || (E > 1 && !gate) || M <= 0 || D <= 0 || F <= 0) { set_error("bad argument"); return PGMI_EINVAL; }
    if (D % 32 || F % 32) { set_error("moe op: D = %d and F = %d must be multiples of 32", D, F); return PGMI_EINVAL; }
    if (E < 1 || E > kWave || top_k < 1 || top_k > E) { set_error("moe op: %d experts, top-%d: 1 .. 64 experts, 1 <= top_k <= experts", E, top_k); return PGMI_EINVAL; }
    OpScope s("moe op", device);
    pgmi_model& tmp = s.tmp;                                     // the stream (default), the GEMM variant and no profile
    const size_t FD = (size_t)F * D;
    float* dh = s.up(h, (size_t)M * D);
    float* dg = E > 1 ? s.up(gate, (size_t)E * D) : nullptr;
    float* dx = s.alloc<float>((size_t)M * D, 0x00);
    unsigned short* h16 = s.alloc<unsigned short>((size_t)M * D * 2);
    unsigned short* g16 = E == 1 ? s.alloc<unsigned short>((size_t)M * F * 2) : nullptr;
    if (!s.rc) s.rc = moe_ws_alloc(s.pool, &tmp.moe, (size_t)M, 1, D, F, E, top_k, gated);
    std::vector<W16> ew1(E), ew2(E);
    std::vector<float> fc1(gated ? 2 * FD : 0);
    for (int e = 0; e < E && !s.rc; ++e) {
        if (gated) {
            pack_swiglu(w1 + e * FD, w3 + e * FD, (size_t)F, (size_t)D, fc1.data());
            ew1[e] = s.w16(fc1.data(), fc1.size(), (size_t)D);
        } else ew1[e] = s.w16(w1 + e * FD, FD, (size_t)D);
        ew2[e] = s.w16(w2 + e * FD, FD, (size_t)F);
    }
    if (s.rc) return s.rc;
    gemm_options_from_env();
    tmp.gemm_variant = env_int("PGMI_GEMM_VARIANT", 0);
    MoeRoute r;
    if (E > 1) { r.gate = dg; r.E = E; r.top_k = top_k; r.ids = tmp.moe.ids; r.wts = tmp.moe.wts; }
    s.rc = launch_rmsnorm_route(dh, nullptr, M, D, 0.0f, h16, r, nullptr);
    if (!s.rc) s.rc = E == 1 ? dense_ffn(&tmp, tmp.moe, ew1[0], ew2[0], h16, g16, M, D, F, gated, dx)
                             : moe_ffn(&tmp, tmp.moe, ew1, ew2, h16, tmp.moe.ids, tmp.moe.wts, M, D, F, E, top_k, gated, dx);
    s.sync();
    s.down(out, dx, (size_t)M * D);
    if (E > 1 && ids) s.down(ids, tmp.moe.ids, (size_t)M * top_k);
    if (E > 1 && weights) s.down(weights, tmp.moe.wts, (size_t)M * top_k);
    return s.rc;
}

int pgmi_op_gemm(int device, int precision, const float* A, const float* W, const float* bias, const float* residual,
                 int M, int N, int K, int epilogue, float* C) {
    if (!A || !W || !C || M <= 0 || N <= 0 || K <= 0) { set_error("bad argument"); return PGMI_EINVAL; }
    if (precision != PGMI_PREC_FP32 && precision != PGMI_PREC_F16X3 && precision != PGMI_PREC_BF16) { set_error("unknown precision %d", precision); return PGMI_EINVAL; }
    OpScope s("gemm op", device);
    if (s.rc) return s.rc;
    // epilogue: EPI_* in the low byte; + 256 (f16x3 only, no residual, N % 32 == 0): run the SPLIT-PLANE output epilogue and return its
    // planes rebuilt as fp32 (tests: a row's bits through the half- and full-height items)
    const int epi = epilogue & 255;
    const bool split_planes = (epilogue & 256) != 0, f32 = precision == PGMI_PREC_FP32, bf = precision == PGMI_PREC_BF16;
    // EPI_SWIGLU: f16x3 split-plane output only (N % 64 == 0); C is then [M, N / 2]
    if (epi == EPI_SWIGLU && (!split_planes || precision != PGMI_PREC_F16X3 || (N % 64))) {
        set_error("SwiGLU GEMM op: precision f16x3 with the split-plane output (epilogue 4 + 256), N %% 64 == 0");
        return PGMI_EINVAL;
    }
    if (epi == EPI_RELU && precision != PGMI_PREC_F16X3) {       // the ReLU epilogue exists in the f16x3 kernels only (ESM-IF1's decoder)
        set_error("ReLU GEMM op: precision f16x3 only");
        return PGMI_EINVAL;
    }
    if (split_planes && (f32 || residual || (N % (precision == PGMI_PREC_F16X3 ? 32 : 4)))) {
        set_error("16-bit-plane GEMM op: f16x3 (N %% 32 == 0) or bf16 (N %% 4 == 0), no residual");
        return PGMI_EINVAL;
    }
    const size_t MN = (size_t)M * N;
    float* dA = s.up(A, (size_t)M * K);
    float* dW = f32 ? s.up(W, (size_t)N * K) : nullptr;
    float* dB = bias ? s.up(bias, (size_t)N) : nullptr;
    float* dR = residual ? s.up(residual, MN) : nullptr;
    float* dC = split_planes ? nullptr : s.alloc<float>(MN);
    unsigned short* c16 = split_planes ? s.alloc<unsigned short>(MN * 2) : nullptr;
    unsigned short* a16 = f32 ? nullptr : s.alloc<unsigned short>((size_t)M * K * (bf ? 1 : 2));
    const W16 w16 = f32 ? W16() : s.w16(W, (size_t)N * K, (size_t)K, precision);
    if (s.rc) return s.rc;
    gemm_options_from_env();                             // a model-less entry of the tests: the hooks are read per call here
    if (f32) {
        s.rc = launch_gemm_f32(dA, dW, dB, dR, dC, M, N, K, epi, nullptr);
    } else {
        launch_split16(dA, (int64_t)M * K, 1.0f, bf ? 1 : 2, K, a16, nullptr);
        GemmLaunch g = op_gemm(a16, w16, dB, M, N, K, env_int("PGMI_GEMM_VARIANT", 0));
        g.epilogue = epi; g.bf = bf;
        if (split_planes) g.out16 = c16;                 // the split-plane epilogue: the next GEMM's operand
        else { g.residual = dR; g.out32 = dC; }
        s.rc = launch_gemm16(g);
    }
    s.sync();
    if (!split_planes) s.down(C, dC, MN);
    else if (bf) s.bf16_plane(C, c16, MN);
    else s.planes(C, c16, (size_t)M, (size_t)(epi == EPI_SWIGLU ? N / 2 : N));     // the output columns
    return s.rc;
}

int pgmi_bench_gemm_ab(int device, int precision, int M, int N, int K, int epilogue, int split_out, const int* variants,
                       int n_variants, int rounds, int iters, double* ms_out) {
    if (M <= 0 || N <= 0 || K <= 0 || iters <= 0 || rounds <= 0 || n_variants <= 0 || !variants || !ms_out) { set_error("bad argument"); return PGMI_EINVAL; }
    OpScope s("bench", device);
    if (s.rc) return s.rc;
    gemm_options_from_env();
    const bool f32 = precision == PGMI_PREC_FP32, bf = precision == PGMI_PREC_BF16;
    // split_out 2: fp32 output with the in-place residual of the out-projection / FC2 (x += ...); 3: the fused QKV epilogue
    // (attention operands; N = 3 D, sequences of 288 tokens when M allows)
    const bool fused_qkv = split_out == 3 && !f32 && !bf;
    if (fused_qkv && (N % 3 || (N / 3) % 64)) { set_error("fused QKV bench needs N = 3 D, D %% 64 == 0"); return PGMI_EINVAL; }
    std::vector<float> hA((size_t)M * K), hW((size_t)N * K), hb(N);
    unsigned int st = 12345u;
    auto rnd = [&]() { st = st * 1664525u + 1013904223u; return ((st >> 8) * (1.0f / 8388608.0f)) - 1.0f; };
    for (auto& v : hA) v = rnd();
    for (auto& v : hW) v = rnd() * 0.03f;
    for (auto& v : hb) v = rnd();
    const int planes = bf ? 1 : 2, Tq = (M % 288 == 0) ? 288 : M;
    const size_t MN = (size_t)M * N;
    float* dA = s.up(hA);
    float* dB = s.up(hb);
    float* dW = f32 ? s.up(hW) : nullptr;
    float* dC = f32 || (split_out != 1 && split_out != 3) ? s.alloc<float>(MN) : nullptr;
    unsigned short* a16 = f32 ? nullptr : s.alloc<unsigned short>((size_t)M * K * planes);
    unsigned short* c16 = !f32 && split_out == 1 ? s.alloc<unsigned short>(MN * planes) : nullptr;
    const W16 w16 = f32 ? W16() : s.w16(hW.data(), hW.size(), (size_t)K, precision);
    QkvPlanes o;
    if (fused_qkv) {
        o.qk_plane = (size_t)M * 2 * (N / 3);
        o.vt_plane = (size_t)(M / Tq) * (N / 3) * roundup32((size_t)Tq);
        o.qk16 = s.alloc<unsigned short>(o.qk_plane * 2);
        o.vt16 = s.alloc<unsigned short>(o.vt_plane * 2);
    }
    if (s.rc) return s.rc;
    if (!f32) launch_split16(dA, (int64_t)M * K, 1.0f, bf ? 1 : 2, K, a16, nullptr);
    auto run = [&](int var) -> int {
        if (f32) return launch_gemm_f32(dA, dW, dB, split_out == 2 ? dC : nullptr, dC, M, N, K, epilogue, nullptr);
        GemmLaunch g = op_gemm(a16, w16, dB, M, N, K, var);
        if (fused_qkv) {
            g.out16 = o.qk16;
            g.qkv.vt16 = o.vt16; g.qkv.vt_plane = o.vt_plane; g.qkv.qk_plane = o.qk_plane;
            g.qkv.T = Tq; g.qkv.H = N / 3 / kHeadDim;
            return launch_gemm16(g);
        }
        g.epilogue = epilogue; g.bf = bf;
        if (split_out == 2) g.residual = dC;
        if (split_out == 1) g.out16 = c16; else g.out32 = dC;
        return launch_gemm16(g);
    };
    auto variant = [&](int v) { return variants[v] >= 0 ? variants[v] : env_int("PGMI_GEMM_VARIANT", 0); };
    std::vector<std::vector<double>> samples(n_variants);
    for (int v = 0; v < n_variants && !s.rc; ++v) s.rc = run(variant(v));     // warm-up
    for (int r = 0; r < rounds; ++r)
        for (int v = 0; v < n_variants; ++v)                       // interleaved rounds: variants see the same clocks / temperature
            samples[v].push_back(s.time_ms([&]() { return run(variant(v)); }, iters));
    s.sync();
    for (int v = 0; v < n_variants && !s.rc; ++v) {
        std::sort(samples[v].begin(), samples[v].end());
        ms_out[v] = samples[v][samples[v].size() / 2];             // median over the rounds
    }
    return s.rc;
}

int pgmi_bench_gemm(int device, int precision, int M, int N, int K, int epilogue, int split_out, int variant,
                    int iters, double* ms_per_launch) {
    return pgmi_bench_gemm_ab(device, precision, M, N, K, epilogue, split_out, &variant, 1, 1, iters, ms_per_launch);
}

int pgmi_op_qkln_prep(int device, const float* qkv, const float* q_w, const float* k_w, int B, int T, int H, int iters, float* qk,
                      float* v, double* ms) {
    if (!qkv || !q_w || !k_w || B <= 0 || T <= 0 || H <= 0 || H * kHeadDim > 2048 || iters < 0 || (iters > 0 && !ms)) { set_error("bad argument"); return PGMI_EINVAL; }
    OpScope s("qkln prep op", device);
    const size_t D = (size_t)H * kHeadDim, M = (size_t)B * T, qk_plane = M * 2 * D, vt_plane = (size_t)B * roundup32((size_t)T) * D;
    float* dq = s.up(qkv, M * 3 * D);
    float* dqw = s.up(q_w, D);
    float* dkw = s.up(k_w, D);
    unsigned short* qk16 = s.alloc<unsigned short>(qk_plane * 2);
    unsigned short* vt16 = s.alloc<unsigned short>(vt_plane * 2);
    if (!s.rc) s.rc = upload_rotate_half(&s.tmp, T);     // head_dim 64: ESM2's rotate-half tables
    auto launch = [&]() {
        return launch_qkln_prep(dq, dqw, dkw, 1e-5f, s.tmp.rot_cos, s.tmp.rot_sin, B, T, H, qk16, qk_plane, vt16, vt_plane, nullptr);
    };
    if (!s.rc) s.rc = launch();
    if (!s.rc && iters > 0) *ms = s.time_ms(launch, iters);
    s.sync();
    if (qk) op_fetch_flat(s, qk, qk16, qk_plane);
    if (v) op_fetch_vt(s, v, vt16, B, T, D);
    return s.rc;
}

int pgmi_op_attention(int device, int precision, const float* qkv, const int32_t* kv_len, int B, int T, int H,
                      int rotary, float* ctx) {
    if (!qkv || !ctx || B <= 0 || T <= 0 || H <= 0) { set_error("bad argument"); return PGMI_EINVAL; }
    OpScope s("attention op", device);
    const size_t D = (size_t)H * kHeadDim, M = (size_t)B * T;
    const bool f16 = precision == PGMI_PREC_F16X3;
    float* dq = s.up(qkv, M * 3 * D);
    int32_t* dl = kv_len ? s.up(kv_len, (size_t)B) : nullptr;
    float* dc = s.alloc<float>(M * D);
    AttLaunch a;
    a.qk_plane = M * 2 * D, a.vt_plane = (size_t)B * roundup32((size_t)T) * D;
    a.qk16 = f16 ? s.alloc<unsigned short>(a.qk_plane * 2) : nullptr;
    a.vt16 = f16 ? s.alloc<unsigned short>(a.vt_plane * 2) : nullptr;
    s.tmp.cfg.arch = PGMI_ARCH_ESM2;
    if (!s.rc && rotary) s.rc = ensure_rotary(&s.tmp, T);
    if (s.rc) return s.rc;
    if (f16) {
        a.B = B, a.T = T, a.H = H;
        a.kv_len = dl;
        a.out = ATT_OUT_F32, a.ctx = dc;
        a.qkv = dq, a.cos_t = s.tmp.rot_cos, a.sin_t = s.tmp.rot_sin, a.rotary = rotary;
        s.rc = launch_attention_f16x3_v2(a);
    } else {
        if (rotary) launch_rotary(dq, s.tmp.rot_cos, s.tmp.rot_sin, B * T, T, H, nullptr);
        s.rc = launch_attention_f32(dq, dl, B, T, H, dc, nullptr);
    }
    s.sync();
    s.down(ctx, dc, M * D);
    return s.rc;
}

// The attention of one decoder layer (run_decoder, api_gpt.hip) in slot space, through the launchers and the argument pattern it uses.
// Fused form (X, W, bias): split the activations, make the weight planes, the fused QKV projection with H = heads * lanes / 64 slot groups
// and rot_halves = lanes / 64, then the causal attention on its operands.  Conv form (qkv, conv): fp32 rows into the attention's
// depth-wise-convolution prep pass.  Shapes are the launchers' to refuse; only what the uploads themselves need is checked here.
int pgmi_op_causal_attention(int device, int lanes, const float* X, const float* W, const float* bias, int K, const float* qkv,
                             const float* conv, const float* rot_cos, const float* rot_sin, const float* slopes, int B, int T,
                             int heads, float* ctx) {
    const bool fused = X && W && bias && !qkv && !conv, conv_form = qkv && conv && !X && !W && !bias && !rot_cos && !rot_sin;
    if ((!fused && !conv_form) || !slopes || !ctx || B <= 0 || T <= 0 || heads <= 0 || lanes <= 0 || !rot_cos != !rot_sin) { set_error("bad argument"); return PGMI_EINVAL; }
    // the activation / weight split writes K-interleaved rows (ki_off) before any launcher sees K: whole groups of 32 only
    if (fused && (K <= 0 || K % 32)) { set_error("causal attention op: K = %d is not a positive multiple of 32", K); return PGMI_EINVAL; }
    OpScope s("causal attention op", device);
    const size_t M = (size_t)B * T, Da = (size_t)heads * lanes, n_rot = (size_t)T * std::max(lanes / kHeadDim, 1) * kHeadDim;
    QkvPlanes o;
    o.qk_plane = M * 2 * Da, o.vt_plane = (size_t)B * roundup32((size_t)T) * Da;
    o.qk16 = s.alloc<unsigned short>(o.qk_plane * 2);
    o.vt16 = s.alloc<unsigned short>(o.vt_plane * 2, 0x00);          // pad keys: finite (reset_pad_keys)
    AttLaunch a;
    a.qk16 = o.qk16, a.qk_plane = o.qk_plane, a.vt16 = o.vt16, a.vt_plane = o.vt_plane;
    a.B = B, a.T = T, a.H = heads, a.head_dim = lanes;
    a.slopes = s.up(slopes, (size_t)heads);
    a.out = ATT_OUT_SPLIT, a.ctx16 = s.alloc<unsigned short>(M * Da * 2);
    if (fused) {                                                    // the operands carry the rotary already
        const float* dcos = rot_cos ? s.up(rot_cos, n_rot) : nullptr;
        const float* dsin = rot_sin ? s.up(rot_sin, n_rot) : nullptr;
        op_qkv_project(s, X, W, bias, M, Da, K, o, T, (int)(Da / kHeadDim), dcos, dsin, lanes / kHeadDim);
    } else {
        a.qkv = s.up(qkv, M * 3 * Da), a.conv = s.up(conv, (size_t)3 * 4 * kHeadDim * 8);
    }
    if (!s.rc) s.rc = launch_attention_f16x3_v2(a);
    s.sync();
    s.planes(ctx, a.ctx16, M, Da);                                  // the context planes (K-interleaved rows of Da) rebuilt as fp32
    return s.rc;
}

// PoET's prefix attention through launch_prefix_prep / launch_prefix_attention (attention_prefix.hip): the prefix planes are filled by the
// prep pass over one segment of P rows (as pgmi_poet_set_prompt fills the cache), the own planes by the prep pass over the segments.
int pgmi_op_prefix_attention(int device, const float* qkv, const int32_t* seg_off, int n_seg, const float* prefix_kv, int P, int heads,
                             int split, float* ctx) {
    if (!qkv || !seg_off || !ctx || n_seg <= 0 || heads <= 0 || P < 0 || (P > 0 && !prefix_kv) || seg_off[0] != 0) { set_error("bad argument"); return PGMI_EINVAL; }
    return op_cached_attention("prefix attention op", device, false, qkv, seg_off, n_seg, prefix_kv, P, heads, split, ctx);
}

// ESM-IF1's cross-attention through launch_cross_q_prep / launch_cross_attention (attention_prefix.hip): the memory planes are filled by
// the prep pass over one segment of S rows (as pgmi_esmif1_set_memory fills a layer's planes).
int pgmi_op_cross_attention(int device, const float* q, const int32_t* seg_off, int n_seg, const float* mem_kv, int S, int heads,
                            int split, float* ctx) {
    if (!q || !seg_off || !ctx || !mem_kv || n_seg <= 0 || heads <= 0 || S <= 0 || seg_off[0] != 0) { set_error("bad argument"); return PGMI_EINVAL; }
    return op_cached_attention("cross attention op", device, true, q, seg_off, n_seg, mem_kv, S, heads, split, ctx);
}

// The chunks pack_chunk cuts a batch of B packed sequences into for a workspace of max_rows rows, as score_packed walks them (host
// only: no device is touched): out_b1[i] = the end of chunk i, *out_n = the number of chunks.
int pgmi_op_packed_chunks(const int32_t* lens, int B, int drop_last, int same_length, int max_rows, int32_t* out_b1, int32_t* out_n) {
    if (!lens || !out_b1 || !out_n || B <= 0 || max_rows <= 0) { set_error("bad argument"); return PGMI_EINVAL; }
    const int lo = drop_last ? 2 : 1;
    for (int b = 0; b < B; ++b)
        if (lens[b] < lo) { set_error("row %d of this call: length %d below %d", b, lens[b], lo); return PGMI_EINVAL; }
    *out_n = 0;
    for (int b0 = 0; b0 < B;) {
        const PackedChunk ch = pack_chunk(lens, b0, B, drop_last != 0, same_length != 0, max_rows, own_pitch(max_rows));
        if (ch.b1 == b0) { set_error("row %d of this call: %d tokens exceed the workspace of %d rows", b0, lens[b0], max_rows); return PGMI_EINVAL; }
        out_b1[(*out_n)++] = b0 = ch.b1;
    }
    return PGMI_OK;
}

// The K splits run_msa's rule picks for an alignment of R x C tokens and H heads (host only: no device is touched).
int pgmi_op_tied_row_splits(int R, int C, int H) {
    if (R <= 0 || C <= 0 || H <= 0) { set_error("bad argument"); return PGMI_EINVAL; }
    return tied_row_splits(R, C, H);
}

// The tied row attention of one MSA Transformer layer (run_msa, api_msa.hip) through launch_tied_row_attention with run_msa's aliasing:
// the q planes and the context planes are one buffer.  Every buffer the kernels write or are meant to ignore starts as 0xFF bytes (NaN in
// fp32 and in fp16): the stale workspace of an earlier, wider alignment.  What the launcher refuses is refused before any allocation.
int pgmi_op_tied_row_attention(int device, const float* qkv, int R, int C, int H, int splits, float* ctx, float* probs) {
    if (!qkv || !ctx || R <= 0 || C <= 0 || H <= 0 || splits < 0) { set_error("bad argument"); return PGMI_EINVAL; }
    const int S = splits ? splits : tied_row_splits(R, C, H);
    const int refused = tied_row_check(R, C, H, S);
    if (refused) return refused;
    OpScope s("tied row attention op", device);
    const size_t M = (size_t)R * C, D = (size_t)H * kHeadDim, Kp = (size_t)tied_row_kp(C);
    TiedRowLaunch t;
    t.qkv = s.up(qkv, M * 3 * D), t.R = R, t.C = C, t.H = H, t.S = S;
    t.qctx16 = s.alloc<unsigned short>(M * D * 2, 0xFF), t.k16 = s.alloc<unsigned short>(M * D * 2);
    t.part = s.alloc<float>((size_t)H * S * C * Kp, 0xFF), t.p = s.alloc<float>((size_t)H * C * Kp, 0xFF);
    t.vt = s.alloc<float>((size_t)H * R * kHeadDim * Kp, 0xFF);
    if (!s.rc) s.rc = launch_tied_row_attention(t);
    s.sync();
    s.planes(ctx, t.qctx16, M, D);                               // the context planes (K-interleaved rows of D) rebuilt as fp32
    if (probs) s.planes(probs, reinterpret_cast<const unsigned short*>(t.p), (size_t)H * C, Kp);   // the P planes: rows (h, i) of Kp columns
    return s.rc;
}

// The column attention of one MSA Transformer layer (run_msa's column block): the activation split, the fused QKV projection without
// rotary on sequences of R rows, V^T planes zeroed first (pad keys must be finite), then the dense attention with B = C, T = R, a device
// kv_len of C entries equal to R and the split-plane context, which starts as 0xFF bytes.
int pgmi_op_column_attention(int device, const float* X, const float* W, const float* bias, int K, int R, int C, int H, float* ctx) {
    if (!X || !W || !bias || !ctx || R <= 0 || C <= 0 || H <= 0) { set_error("bad argument"); return PGMI_EINVAL; }
    // the activation / weight split writes K-interleaved rows (ki_off) before any launcher sees K: whole groups of 32 only
    if (K <= 0 || K % 32) { set_error("column attention op: K = %d is not a positive multiple of 32", K); return PGMI_EINVAL; }
    OpScope s("column attention op", device);
    const size_t M = (size_t)C * R, D = (size_t)H * kHeadDim;
    const std::vector<int32_t> kv((size_t)C, R);
    QkvPlanes o;
    o.qk_plane = M * 2 * D, o.vt_plane = (size_t)C * roundup32((size_t)R) * D;
    o.qk16 = s.alloc<unsigned short>(o.qk_plane * 2);
    o.vt16 = s.alloc<unsigned short>(o.vt_plane * 2, 0x00);
    AttLaunch a;
    a.qk16 = o.qk16, a.qk_plane = o.qk_plane, a.vt16 = o.vt16, a.vt_plane = o.vt_plane;
    a.B = C, a.T = R, a.H = H;
    a.kv_len = s.up(kv);
    a.out = ATT_OUT_SPLIT, a.ctx16 = s.alloc<unsigned short>(M * D * 2, 0xFF);
    op_qkv_project(s, X, W, bias, M, D, K, o, R, H);
    if (!s.rc) s.rc = launch_attention_f16x3_v2(a);
    s.sync();
    s.planes(ctx, a.ctx16, M, D);
    return s.rc;
}

// The attention of one encoder layer (run_encoder, api_esm.hip) in slot space, through the launchers and the argument pattern it uses: the
// activation split, the weight planes, the fused QKV projection with H = heads * lanes / 64 slot groups and rot_halves = lanes / 64 (f16x3
// whatever `out` is), then the dense attention on its operands with the device kv_len and the requested context kind.  V^T planes are zeroed
// first (reset_pad_keys); the q | k planes and the context start as 0xFF bytes (NaN): an element the kernels skip shows.  Shapes are the
// launchers' to refuse; only what the uploads themselves need is checked here, before the device is touched.
int pgmi_op_dense_attention(int device, int lanes, const float* X, const float* W, const float* bias, int K, const float* rot_cos,
                            const float* rot_sin, const int32_t* kv_len, int B, int T, int heads, int out, float* ctx, float* qk, float* v) {
    if (!X || !W || !bias || !ctx || B <= 0 || T <= 0 || heads <= 0) { set_error("bad argument"); return PGMI_EINVAL; }
    if (!rot_cos != !rot_sin) { set_error("dense attention op: rot_cos and rot_sin go together (both, or neither for no rotary)"); return PGMI_EINVAL; }
    if (lanes != 64 && lanes != 128) { set_error("dense attention op: lanes = %d is neither 64 nor 128", lanes); return PGMI_EINVAL; }
    // the activation / weight split writes K-interleaved rows (ki_off) before any launcher sees K: whole groups of 32 only
    if (K <= 0 || K % 32) { set_error("dense attention op: K = %d is not a positive multiple of 32", K); return PGMI_EINVAL; }
    for (int b = 0; kv_len && b < B; ++b)
        if (kv_len[b] < 1 || kv_len[b] > T) { set_error("dense attention op: kv_len[%d] = %d is outside [1, %d]", b, kv_len[b], T); return PGMI_EINVAL; }
    OpScope s("dense attention op", device);
    const size_t M = (size_t)B * T, Da = (size_t)heads * lanes, n_rot = (size_t)T * (lanes / kHeadDim) * kHeadDim;
    QkvPlanes o;
    o.qk_plane = M * 2 * Da, o.vt_plane = (size_t)B * roundup32((size_t)T) * Da;
    o.qk16 = s.alloc<unsigned short>(o.qk_plane * 2, 0xFF);
    o.vt16 = s.alloc<unsigned short>(o.vt_plane * 2, 0x00);          // pad keys: finite (reset_pad_keys)
    AttLaunch a;
    a.qk16 = o.qk16, a.qk_plane = o.qk_plane, a.vt16 = o.vt16, a.vt_plane = o.vt_plane;
    a.B = B, a.T = T, a.H = heads, a.head_dim = lanes;
    a.kv_len = kv_len ? s.up(kv_len, (size_t)B) : nullptr;
    // the context: M Da fp32 values, M Da hi | lo pairs or M Da bf16 values -- one buffer of the largest of the three context kinds
    a.out = (AttOut)out, a.ctx = s.alloc<float>(M * Da, 0xFF), a.ctx16 = reinterpret_cast<unsigned short*>(a.ctx);
    const float* dcos = rot_cos ? s.up(rot_cos, n_rot) : nullptr;
    const float* dsin = rot_sin ? s.up(rot_sin, n_rot) : nullptr;
    op_qkv_project(s, X, W, bias, M, Da, K, o, T, (int)(Da / kHeadDim), dcos, dsin, lanes / kHeadDim);
    if (!s.rc) s.rc = launch_attention_f16x3_v2(a);
    s.sync();
    if (out == ATT_OUT_F32) s.down(ctx, a.ctx, M * Da);
    if (out == ATT_OUT_SPLIT) s.planes(ctx, a.ctx16, M, Da);         // the context planes (K-interleaved rows of Da) rebuilt as fp32
    if (out == ATT_OUT_BF16) s.bf16_plane(ctx, a.ctx16, M * Da);
    if (qk) op_fetch_flat(s, qk, o.qk16, o.qk_plane);
    if (v) op_fetch_vt(s, v, o.vt16, B, T, Da);
    return s.rc;
}

// ESM3's geometric attention kernel (geom_attention.hip) through the launcher the model and the structure tokenizer use.
int pgmi_op_geom_attention(int device, const float* proj, const float* rot, const float* trans, const int32_t* frame_mask,
                           int per_row_frames, const float* w_rot, const float* w_dist, int B, int S, int H, float* out) {
    if (!proj || !rot || !trans || !frame_mask || !w_rot || !w_dist || !out || B <= 0 || S <= 0 || H <= 0) { set_error("bad argument"); return PGMI_EINVAL; }
    OpScope s("geometric attention op", device);
    const size_t rows = (size_t)B * S, nf = per_row_frames ? rows : (size_t)S;
    GeomAttLaunch g;
    g.proj = s.up(proj, rows * 15 * H), g.pitch = 15 * H;
    g.rot = s.up(rot, nf * 9), g.trans = s.up(trans, nf * 3), g.mask = s.up(frame_mask, nf), g.per_row_frames = per_row_frames != 0;
    g.w_rot = s.up(w_rot, (size_t)H), g.w_dist = s.up(w_dist, (size_t)H);
    g.B = B, g.S = S, g.H = H;
    g.out = s.alloc<float>(rows * 3 * H, 0xFF), g.opitch = 3 * H;     // an element the kernel skips shows as NaN
    if (!s.rc) s.rc = launch_geom_attention(g);
    s.sync();
    s.down(out, g.out, rows * 3 * H);
    return s.rc;
}

int pgmi_op_geom_key_tile(int S) { return geom_key_tile(S); }

}  // extern "C"

// ---- the scoring tail (elementwise.hip): log-softmax heads and per-sequence sums on their own buffers ----------------------------------
// Every output is allocated with kOutGuard spare values behind it and starts as 0xFF bytes (NaN): an element the kernel skips shows as
// NaN on the host, and a guard value the kernel touched fails the call.  *nonfinite is the device flag after the launch (zero before).
static constexpr size_t kOutGuard = 64;                          // one row of the narrow head at its widest
static float* out_alloc(OpScope& s, size_t n) { return s.alloc<float>(n + kOutGuard, 0xFF); }
static int32_t* flag_alloc(OpScope& s) { return s.alloc<int32_t>(1, 0x00); }
static void out_fetch(OpScope& s, const float* d, size_t n, float* host) {
    uint32_t guard[kOutGuard];
    s.down(host, d, n);
    s.down(guard, reinterpret_cast<const uint32_t*>(d + n), kOutGuard);
    for (size_t i = 0; i < kOutGuard && !s.rc; ++i)
        if (guard[i] != 0xFFFFFFFFu) { set_error("%s: the kernel wrote %zu values past the end of its output", s.what, i + 1); s.rc = PGMI_EHIP; }
}

extern "C" {

int pgmi_op_vocab_logsoftmax(int device, const float* h, const float* E, const float* bias, int rows, int D, int V, float* out,
                             int32_t* nonfinite) {
    if (!h || !E || !bias || !out || !nonfinite || rows <= 0 || D <= 0) { set_error("bad argument"); return PGMI_EINVAL; }
    if (V < 1 || V > 64) { set_error("narrow log-softmax op: V = %d is outside 1 .. 64 (lane v owns logit v)", V); return PGMI_EINVAL; }
    OpScope s("narrow log-softmax op", device);
    const size_t n_out = (size_t)rows * V;
    float* dh = s.up(h, (size_t)rows * D);
    float* dE = s.up(E, (size_t)V * D);
    float* db = s.up(bias, (size_t)V);
    float* dout = out_alloc(s, n_out);
    int32_t* dflag = flag_alloc(s);
    if (s.rc) return s.rc;
    launch_vocab_logsoftmax(dh, dE, db, rows, D, V, dout, dflag, nullptr);
    s.sync();
    out_fetch(s, dout, n_out, out);
    s.down(nonfinite, dflag, 1);
    return s.rc;
}

int pgmi_op_wide_logsoftmax(int device, const float* logits, int ldl, int rows, int V, const int32_t* tgt, float* out,
                            int32_t* nonfinite) {
    if (!logits || !out || !nonfinite || rows <= 0 || V <= 0 || ldl <= 0) { set_error("bad argument"); return PGMI_EINVAL; }
    if (ldl % 4 || ldl < V) { set_error("wide log-softmax op: ldl = %d must be a multiple of 4 and at least V = %d", ldl, V); return PGMI_EINVAL; }
    for (int r = 0; tgt && r < rows; ++r)
        if (tgt[r] < 0 || tgt[r] >= V) { set_error("wide log-softmax op: tgt[%d] = %d is outside [0, %d)", r, tgt[r], V); return PGMI_EINVAL; }
    OpScope s("wide log-softmax op", device);
    const size_t n_out = tgt ? (size_t)rows : (size_t)rows * V;
    float* dl = s.up(logits, (size_t)rows * ldl);
    int32_t* dt = tgt ? s.up(tgt, (size_t)rows) : nullptr;
    float* dout = out_alloc(s, n_out);
    int32_t* dflag = flag_alloc(s);
    if (s.rc) return s.rc;
    launch_wide_logsoftmax(dl, ldl, rows, V, dt, dout, dflag, nullptr);
    s.sync();
    out_fetch(s, dout, n_out, out);
    s.down(nonfinite, dflag, 1);
    return s.rc;
}

int pgmi_op_group_logsoftmax(int device, const float* h, const float* E, const float* bias, int rows, int D, int V, int first, int groups,
                             int width, float* full, float* group, int32_t* nonfinite) {
    if (!h || !E || !bias || !nonfinite || rows <= 0 || D <= 0 || V <= 0 || first < 0 || groups <= 0 || width <= 0) { set_error("bad argument"); return PGMI_EINVAL; }
    if (!full && !group) { set_error("grouped log-softmax op: neither `full` nor `group` is asked for"); return PGMI_EINVAL; }
    const int refused = group_logsoftmax_check(D, V, first, groups, width);
    if (refused) return refused;
    OpScope s("grouped log-softmax op", device);
    const size_t n_full = (size_t)rows * V, n_group = (size_t)rows * groups;
    float* dh = s.up(h, (size_t)rows * D);
    float* dE = s.up(E, (size_t)V * D);
    float* db = s.up(bias, (size_t)V);
    float* dfull = full ? out_alloc(s, n_full) : nullptr;
    float* dgroup = group ? out_alloc(s, n_group) : nullptr;
    int32_t* dflag = flag_alloc(s);
    if (!s.rc) s.rc = launch_group_logsoftmax(dh, dE, db, rows, D, V, first, groups, width, dfull, dgroup, dflag, nullptr);
    s.sync();
    if (full) out_fetch(s, dfull, n_full, full);
    if (group) out_fetch(s, dgroup, n_group, group);
    s.down(nonfinite, dflag, 1);
    return s.rc;
}

// The range checks of every index the two kernels form are made here, on the host, so that no input can make a kernel read outside the
// buffers this entry allocates.  Dense form: sequence b owns the rows b T .. b T + T - 1.  Ragged form: sequence b owns the T - seq_p[b]
// packed rows from seq_off[b] on and reads the first seq_p[b] rows of its root, a sequence that owns all its T rows.
int pgmi_op_seq_loglik(int device, const float* lp, const int32_t* tokens, int B, int T, int V, const int32_t* lens, const int32_t* seq_off,
                       const int32_t* seq_p, const int32_t* seq_root, int n_lp_rows, const float* prior, int n_prior_rows,
                       const int32_t* a0, const int32_t* row0, const int32_t* n, const int32_t* flip, float alpha, const float* eve,
                       float beta, int eve_fallback, float* out) {
    if (!lp || !tokens || !out || B <= 0 || T <= 0 || V <= 0 || n_lp_rows <= 0) { set_error("bad argument"); return PGMI_EINVAL; }
    if (!lens && (!seq_off || !seq_p || !seq_root)) { set_error("sequence sum op: neither `lens` (dense) nor seq_off / seq_p / seq_root (ragged)"); return PGMI_EINVAL; }
    if (eve && !prior) { set_error("sequence sum op: an EVE table without a retrieval prior"); return PGMI_EINVAL; }
    if (prior && (!a0 || !row0 || !n || !flip || n_prior_rows <= 0)) { set_error("bad argument"); return PGMI_EINVAL; }
    for (int i = 0; i < n_lp_rows; ++i)
        if (tokens[i] < 0 || tokens[i] >= V) { set_error("sequence sum op: token %d = %d is outside [0, %d)", i, tokens[i], V); return PGMI_EINVAL; }
    if (lens) {
        if ((int64_t)B * T != n_lp_rows) { set_error("sequence sum op: dense form with %d rows for B = %d, T = %d", n_lp_rows, B, T); return PGMI_EINVAL; }
        for (int b = 0; b < B; ++b)
            if (lens[b] < 0 || lens[b] > T) { set_error("sequence sum op: lens[%d] = %d is outside [0, %d]", b, lens[b], T); return PGMI_EINVAL; }
    } else {
        for (int b = 0; b < B; ++b) {
            const int64_t p = seq_p[b], off = seq_off[b], root = seq_root[b];
            const bool ok = p >= 0 && p <= T && off >= 0 && off + (T - p) <= n_lp_rows && root >= 0 && root < B && seq_p[root] == 0 &&
                            seq_off[root] >= 0 && (int64_t)seq_off[root] + T <= n_lp_rows;
            if (!ok) { set_error("sequence sum op: ragged sequence %d (offset %d, first own token %d, root %d) leaves the %d packed rows", b, seq_off[b], seq_p[b], seq_root[b], n_lp_rows); return PGMI_EINVAL; }
        }
    }
    for (int b = 0; prior && b < B; ++b) {
        if (n[b] < 0) { set_error("sequence sum op: prior window %d has n = %d", b, n[b]); return PGMI_EINVAL; }
        if (n[b] == 0) continue;
        if (a0[b] < 0 || row0[b] < 0 || (int64_t)a0[b] + n[b] > T - 1 || (int64_t)row0[b] + n[b] > n_prior_rows) {
            set_error("sequence sum op: prior window %d (a0 %d, row0 %d, n %d) leaves the %d targets or the %d prior rows", b, a0[b], row0[b], n[b], T - 1, n_prior_rows);
            return PGMI_EINVAL;
        }
    }
    OpScope s("sequence sum op", device);
    const size_t nB = (size_t)B;
    float* dlp = s.up(lp, (size_t)n_lp_rows * V);
    int32_t* dtok = s.up(tokens, (size_t)n_lp_rows);
    int32_t* dlens = lens ? s.up(lens, nB) : nullptr;
    int32_t *doff = lens ? nullptr : s.up(seq_off, nB), *dp = lens ? nullptr : s.up(seq_p, nB), *droot = lens ? nullptr : s.up(seq_root, nB);
    float* dprior = prior ? s.up(prior, (size_t)n_prior_rows * V) : nullptr;
    int32_t *da0 = prior ? s.up(a0, nB) : nullptr, *drow0 = prior ? s.up(row0, nB) : nullptr;
    int32_t *dn = prior ? s.up(n, nB) : nullptr, *dflip = prior ? s.up(flip, nB) : nullptr;
    float* deve = eve ? s.up(eve, (size_t)n_prior_rows * V) : nullptr;
    float* dout = out_alloc(s, nB);
    if (s.rc) return s.rc;
    if (lens) launch_seq_loglik(dlp, dtok, dlens, B, T, V, dprior, da0, drow0, dn, dflip, alpha, deve, beta, eve_fallback, dout, nullptr);
    else launch_seq_loglik_ragged(dlp, dtok, doff, dp, droot, B, T, V, dprior, da0, drow0, dn, dflip, alpha, deve, beta, eve_fallback, dout, nullptr);
    s.sync();
    out_fetch(s, dout, nB, out);
    return s.rc;
}

}  // extern "C"
