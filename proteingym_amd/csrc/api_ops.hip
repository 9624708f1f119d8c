// Single-op and timing entries of include/pgmi.h (numerics tests against torch ops; interleaved A/B of launch parameters).
#include "model.h"

// a value of the split fp16 planes (common.h split_act) back as fp32: hi + lo 2^-11
static inline float rebuild_split(unsigned short h, unsigned short l) {
    _Float16 a, b;
    memcpy(&a, &h, 2); memcpy(&b, &l, 2);
    return (float)a + (float)b * (1.0f / kLoScale);
}

extern "C" {

// ---- single-op entry points for the numerics tests -------------------------------------------
int pgmi_op_layernorm(int device, const float* x, const float* w, const float* b, int rows, int D, float eps, float* y) {
    if (!x || !w || !b || !y || rows <= 0 || D <= 0 || D % 4) { set_error("bad argument"); return PGMI_EINVAL; }
    if (pgmi_device_count() <= 0) { set_error("no HIP device visible"); return PGMI_ENODEV; }
    PGMI_HIP(hipSetDevice(device));
    std::vector<void*> pool;
    float *dx, *dw, *db, *dy;
    int rc = 0;
    if ((rc = dev_upload(pool, &dx, x, (size_t)rows * D)) || (rc = dev_upload(pool, &dw, w, (size_t)D)) ||
        (rc = dev_upload(pool, &db, b, (size_t)D)) || (rc = dev_alloc(pool, &dy, (size_t)rows * D))) {
        for (void* p : pool) hipFree(p);
        return rc;
    }
    launch_layernorm(dx, dw, db, rows, D, eps, dy, nullptr);
    hipError_t e = hipMemcpy(y, dy, (size_t)rows * D * 4, hipMemcpyDeviceToHost);
    for (void* p : pool) hipFree(p);
    if (e != hipSuccess) { set_error("layernorm op failed: %s", hipGetErrorString(e)); return PGMI_EHIP; }
    return PGMI_OK;
}

int pgmi_op_rmsnorm(int device, const float* x, const float* w, int rows, int D, float eps, float* y) {
    if (!x || !w || !y || rows <= 0 || D <= 0) { set_error("bad argument"); return PGMI_EINVAL; }
    if (D % 32) { set_error("rmsnorm op: D = %d is not a multiple of 32 (the K-interleaved operand)", D); return PGMI_EINVAL; }
    if (pgmi_device_count() <= 0) { set_error("no HIP device visible"); return PGMI_ENODEV; }
    PGMI_HIP(hipSetDevice(device));
    std::vector<void*> pool;
    auto cleanup = [&]() { for (void* p : pool) hipFree(p); };
    float *dx = nullptr, *dw = nullptr;
    unsigned short* y16 = nullptr;
    int rc = 0;
    if ((rc = dev_upload(pool, &dx, x, (size_t)rows * D)) || (rc = dev_upload(pool, &dw, w, (size_t)D)) ||
        (rc = dev_alloc(pool, &y16, (size_t)rows * D * 2))) {
        cleanup();
        return rc;
    }
    hipError_t e = hipMemset(y16, 0xFF, (size_t)rows * D * 2 * sizeof(unsigned short));     // an element the kernel skips shows as NaN
    if (e == hipSuccess) rc = launch_rmsnorm16(dx, dw, rows, D, eps, y16, nullptr);
    std::vector<unsigned short> h(rc ? 0 : (size_t)rows * D * 2);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (!rc && e == hipSuccess) e = hipMemcpy(h.data(), y16, h.size() * 2, hipMemcpyDeviceToHost);
    cleanup();
    if (rc) return rc;
    if (e != hipSuccess) { set_error("rmsnorm op failed: %s", hipGetErrorString(e)); return PGMI_EHIP; }
    for (size_t m = 0; m < (size_t)rows; ++m)
        for (int n = 0; n < D; ++n) {
            const size_t o = ki_off(m, n, D);
            y[m * D + n] = rebuild_split(h[o], h[o + 32]);
        }
    return PGMI_OK;
}

// ProGen3's feed-forward block (api_progen3.hip pg3_ffn without the norm) on rows taken as they are: the router kernel splits them and
// routes them, then moe_ffn (or, for one expert, dense_ffn) adds the block's output into a zeroed x.
int pgmi_op_moe(int device, const float* h, const float* gate, const float* w1, const float* w3, const float* w2, int M, int D, int F,
                int E, int top_k, int gated, float* out, int32_t* ids, float* weights) {
    if (!h || !w1 || !w2 || !out || (gated && !w3) || (E > 1 && !gate) || M <= 0 || D <= 0 || F <= 0) { set_error("bad argument"); return PGMI_EINVAL; }
    if (D % 32 || F % 32) { set_error("moe op: D = %d and F = %d must be multiples of 32", D, F); return PGMI_EINVAL; }
    if (E < 1 || E > kWave || top_k < 1 || top_k > E) { set_error("moe op: %d experts, top-%d: 1 .. 64 experts, 1 <= top_k <= experts", E, top_k); return PGMI_EINVAL; }
    if (pgmi_device_count() <= 0) { set_error("no HIP device visible"); return PGMI_ENODEV; }
    PGMI_HIP(hipSetDevice(device));
    gemm_options_from_env();
    pgmi_model tmp;                                              // the stream (default), the GEMM variant and no profile
    tmp.gemm_variant = env_int("PGMI_GEMM_VARIANT", 0);
    std::vector<void*>& pool = tmp.allocs;
    auto cleanup = [&]() {
        if (tmp.moe.counts_host) hipHostFree(tmp.moe.counts_host);
        for (void* p : pool) hipFree(p);
        pool.clear();
    };
    float *dh = nullptr, *dg = nullptr, *dx = nullptr;
    unsigned short *h16 = nullptr, *g16 = nullptr;
    const size_t FD = (size_t)F * D;
    int rc = 0;
    if ((rc = dev_upload(pool, &dh, h, (size_t)M * D)) || (E > 1 && (rc = dev_upload(pool, &dg, gate, (size_t)E * D))) ||
        (rc = dev_alloc(pool, &dx, (size_t)M * D)) || (rc = dev_alloc(pool, &h16, (size_t)M * D * 2)) ||
        (E == 1 && (rc = dev_alloc(pool, &g16, (size_t)M * F * 2))) || (rc = moe_ws_alloc(pool, &tmp.moe, (size_t)M, 1, D, F, E, top_k, gated))) {
        cleanup();
        return rc;
    }
    std::vector<W16> ew1(E), ew2(E);
    std::vector<float> fc1(gated ? 2 * FD : 0);
    for (int e = 0; e < E && !rc; ++e) {
        if (gated) {
            pack_swiglu(w1 + e * FD, w3 + e * FD, (size_t)F, (size_t)D, fc1.data());
            rc = make_w16(pool, fc1.data(), fc1.size(), (size_t)D, PGMI_PREC_F16X3, nullptr, &ew1[e]);
        } else rc = make_w16(pool, w1 + e * FD, FD, (size_t)D, PGMI_PREC_F16X3, nullptr, &ew1[e]);
        if (!rc) rc = make_w16(pool, w2 + e * FD, FD, (size_t)F, PGMI_PREC_F16X3, nullptr, &ew2[e]);
    }
    hipError_t er = rc ? hipSuccess : hipMemset(dx, 0, (size_t)M * D * 4);
    if (!rc && er == hipSuccess) {
        MoeRoute r;
        if (E > 1) { r.gate = dg; r.E = E; r.top_k = top_k; r.ids = tmp.moe.ids; r.wts = tmp.moe.wts; }
        rc = launch_rmsnorm_route(dh, nullptr, M, D, 0.0f, h16, r, nullptr);
        if (!rc) rc = E == 1 ? dense_ffn(&tmp, tmp.moe, ew1[0], ew2[0], h16, g16, M, D, F, gated, dx)
                             : moe_ffn(&tmp, tmp.moe, ew1, ew2, h16, tmp.moe.ids, tmp.moe.wts, M, D, F, E, top_k, gated, dx);
    }
    if (er == hipSuccess) er = hipDeviceSynchronize();
    if (!rc && er == hipSuccess) er = hipMemcpy(out, dx, (size_t)M * D * 4, hipMemcpyDeviceToHost);
    if (!rc && er == hipSuccess && E > 1 && ids) er = hipMemcpy(ids, tmp.moe.ids, (size_t)M * top_k * 4, hipMemcpyDeviceToHost);
    if (!rc && er == hipSuccess && E > 1 && weights) er = hipMemcpy(weights, tmp.moe.wts, (size_t)M * top_k * 4, hipMemcpyDeviceToHost);
    cleanup();
    if (rc) return rc;
    if (er != hipSuccess) { set_error("moe op failed: %s", hipGetErrorString(er)); return PGMI_EHIP; }
    return PGMI_OK;
}

// The op entries' GEMMs on their own buffers: f16x3, no epilogue, no output yet -- the caller sets what differs
static GemmLaunch op_gemm(const unsigned short* a16, const W16& w16, const float* bias, int M, int N, int K, int variant) {
    GemmLaunch g;
    g.A = a16; g.W = w16.p; g.out_scale = w16.out_scale;
    g.bias = bias;
    g.M = M; g.N = N; g.K = K;
    g.variant = variant;
    return g;
}

int pgmi_op_gemm(int device, int precision, const float* A, const float* W, const float* bias, const float* residual,
                 int M, int N, int K, int epilogue, float* C) {
    if (!A || !W || !C || M <= 0 || N <= 0 || K <= 0) { set_error("bad argument"); return PGMI_EINVAL; }
    if (precision != PGMI_PREC_FP32 && precision != PGMI_PREC_F16X3 && precision != PGMI_PREC_BF16) { set_error("unknown precision %d", precision); return PGMI_EINVAL; }
    if (pgmi_device_count() <= 0) { set_error("no HIP device visible"); return PGMI_ENODEV; }
    PGMI_HIP(hipSetDevice(device));
    gemm_options_from_env();                             // a model-less entry of the tests: the hooks are read per call here
    std::vector<void*> pool;
    float *dA, *dW = nullptr, *dB = nullptr, *dR = nullptr, *dC;
    int rc = 0;
    if ((rc = dev_upload(pool, &dA, A, (size_t)M * K)) ||
        (precision == PGMI_PREC_FP32 && (rc = dev_upload(pool, &dW, W, (size_t)N * K))) ||
        (bias && (rc = dev_upload(pool, &dB, bias, (size_t)N))) ||
        (residual && (rc = dev_upload(pool, &dR, residual, (size_t)M * N))) ||
        (rc = dev_alloc(pool, &dC, (size_t)M * N))) {
        for (void* p : pool) hipFree(p);
        return rc;
    }
    // epilogue: EPI_* in the low byte; + 256 (f16x3 only, no residual, N % 32 == 0): run the SPLIT-PLANE output epilogue and return its
    // planes rebuilt as fp32 (tests: a row's bits through the half- and full-height items)
    const int epi = epilogue & 255;
    const bool split_planes = (epilogue & 256) != 0;
    // EPI_SWIGLU: f16x3 split-plane output only (N % 64 == 0); C is then [M, N / 2]
    if (epi == EPI_SWIGLU && (!split_planes || precision != PGMI_PREC_F16X3 || (N % 64))) {
        for (void* p : pool) hipFree(p);
        set_error("SwiGLU GEMM op: precision f16x3 with the split-plane output (epilogue 4 + 256), N %% 64 == 0");
        return PGMI_EINVAL;
    }
    if (epi == EPI_RELU && precision != PGMI_PREC_F16X3) {       // the ReLU epilogue exists in the f16x3 kernels only (ESM-IF1's decoder)
        for (void* p : pool) hipFree(p);
        set_error("ReLU GEMM op: precision f16x3 only");
        return PGMI_EINVAL;
    }
    if (split_planes && (precision == PGMI_PREC_FP32 || residual || (N % (precision == PGMI_PREC_F16X3 ? 32 : 4)))) {
        for (void* p : pool) hipFree(p);
        set_error("16-bit-plane GEMM op: f16x3 (N %% 32 == 0) or bf16 (N %% 4 == 0), no residual");
        return PGMI_EINVAL;
    }
    if (precision == PGMI_PREC_FP32) {
        rc = launch_gemm_f32(dA, dW, dB, dR, dC, M, N, K, epi, nullptr);
    } else {
        const bool bf = precision == PGMI_PREC_BF16;
        const int planes = bf ? 1 : 2;
        W16 w16;
        unsigned short* a16 = nullptr;
        rc = make_w16(pool, W, (size_t)N * K, (size_t)K, precision, nullptr, &w16);
        if (!rc) rc = dev_alloc(pool, &a16, (size_t)M * K * planes);
        if (!rc) {
            launch_split16(dA, (int64_t)M * K, 1.0f, bf ? 1 : 2, K, a16, nullptr);
            GemmLaunch g = op_gemm(a16, w16, dB, M, N, K, env_int("PGMI_GEMM_VARIANT", 0));
            g.epilogue = epi; g.bf = bf;
            if (split_planes) {
                // the split-plane epilogue (the next GEMM's operand): run it, then rebuild fp32 = hi + lo 2^-11 from the K-interleaved planes
                unsigned short* c16 = nullptr;
                const int No = epi == EPI_SWIGLU ? N / 2 : N;              // output columns
                rc = dev_alloc(pool, &c16, (size_t)M * N * 2);
                g.out16 = c16;
                if (!rc) rc = launch_gemm16(g);
                if (!rc) {
                    std::vector<unsigned short> h((size_t)M * N * 2);
                    hipError_t e2 = hipMemcpy(h.data(), c16, h.size() * 2, hipMemcpyDeviceToHost);
                    if (e2 != hipSuccess) { set_error("gemm op failed: %s", hipGetErrorString(e2)); rc = PGMI_EHIP; }
                    for (size_t m = 0; m < (size_t)M && !rc && bf; ++m)           // bf16 plane, row-major
                        for (int n = 0; n < N; ++n) {
                            const unsigned int u = (unsigned int)h[m * N + n] << 16;
                            memcpy(&C[m * N + n], &u, 4);
                        }
                    for (size_t m = 0; m < (size_t)M && !rc && !bf; ++m)
                        for (int n = 0; n < No; ++n) {
                            const size_t o = ki_off(m, n, No);
                            C[m * No + n] = rebuild_split(h[o], h[o + 32]);
                        }
                }
                for (void* p : pool) hipFree(p);
                return rc;
            }
            g.residual = dR; g.out32 = dC;
            rc = launch_gemm16(g);
        }
    }
    hipError_t e = hipMemcpy(C, dC, (size_t)M * N * 4, hipMemcpyDeviceToHost);
    for (void* p : pool) hipFree(p);
    if (rc) return rc;
    if (e != hipSuccess) { set_error("gemm op failed: %s", hipGetErrorString(e)); return PGMI_EHIP; }
    return PGMI_OK;
}

int pgmi_bench_gemm_ab(int device, int precision, int M, int N, int K, int epilogue, int split_out, const int* variants,
                       int n_variants, int rounds, int iters, double* ms_out) {
    if (M <= 0 || N <= 0 || K <= 0 || iters <= 0 || rounds <= 0 || n_variants <= 0 || !variants || !ms_out) { set_error("bad argument"); return PGMI_EINVAL; }
    if (pgmi_device_count() <= 0) { set_error("no HIP device visible"); return PGMI_ENODEV; }
    PGMI_HIP(hipSetDevice(device));
    gemm_options_from_env();
    std::vector<void*> pool;
    auto cleanup = [&]() { for (void* p : pool) hipFree(p); };
    std::vector<float> hA((size_t)M * K), hW((size_t)N * K), hb(N);
    unsigned int st = 12345u;
    auto rnd = [&]() { st = st * 1664525u + 1013904223u; return ((st >> 8) * (1.0f / 8388608.0f)) - 1.0f; };
    for (auto& v : hA) v = rnd();
    for (auto& v : hW) v = rnd() * 0.03f;
    for (auto& v : hb) v = rnd();
    float *dA, *dW = nullptr, *dB, *dC = nullptr;
    unsigned short *a16 = nullptr, *c16 = nullptr;
    int rc = 0;
    if ((rc = dev_upload(pool, &dA, hA.data(), hA.size())) || (rc = dev_upload(pool, &dB, hb.data(), hb.size()))) { cleanup(); return rc; }
    hipEvent_t e0, e1;
    PGMI_HIP(hipEventCreate(&e0));
    PGMI_HIP(hipEventCreate(&e1));
    const bool f32 = precision == PGMI_PREC_FP32;
    const bool bf = precision == PGMI_PREC_BF16;
    const int planes = bf ? 1 : 2;
    W16 w16;
    if (f32) {
        if ((rc = dev_upload(pool, &dW, hW.data(), hW.size())) || (rc = dev_alloc(pool, &dC, (size_t)M * N))) { cleanup(); return rc; }
    } else {
        if ((rc = make_w16(pool, hW.data(), hW.size(), (size_t)K, precision, nullptr, &w16)) ||
            (rc = dev_alloc(pool, &a16, (size_t)M * K * planes))) { cleanup(); return rc; }
        launch_split16(dA, (int64_t)M * K, 1.0f, bf ? 1 : 2, K, a16, nullptr);
        if (split_out == 1) rc = dev_alloc(pool, &c16, (size_t)M * N * planes);
        else if (split_out != 3) rc = dev_alloc(pool, &dC, (size_t)M * N);
        if (rc) { cleanup(); return rc; }
    }
    // split_out 2: fp32 output with the in-place residual of the out-projection / FC2 (x += ...); 3: the fused QKV epilogue
    // (attention operands; N = 3 D, sequences of 288 tokens when M allows)
    const bool fused_qkv = split_out == 3 && !f32 && !bf;
    const int Tq = (M % 288 == 0) ? 288 : M;
    unsigned short *qk16 = nullptr, *vt16 = nullptr;
    size_t qk_plane = 0, vt_plane = 0;
    if (fused_qkv) {
        if (N % 3 || (N / 3) % 64) { set_error("fused QKV bench needs N = 3 D, D %% 64 == 0"); cleanup(); return PGMI_EINVAL; }
        const size_t Tp = (size_t)(Tq + 31) / 32 * 32;
        qk_plane = (size_t)M * 2 * (N / 3);
        vt_plane = (size_t)(M / Tq) * (N / 3) * Tp;
        if ((rc = dev_alloc(pool, &qk16, qk_plane * 2)) || (rc = dev_alloc(pool, &vt16, vt_plane * 2))) { cleanup(); return rc; }
    }
    auto run = [&](int var) -> int {
        if (f32) return launch_gemm_f32(dA, dW, dB, split_out == 2 ? dC : nullptr, dC, M, N, K, epilogue, nullptr);
        GemmLaunch g = op_gemm(a16, w16, dB, M, N, K, var);
        if (fused_qkv) {
            g.out16 = qk16;
            g.qkv.vt16 = vt16; g.qkv.vt_plane = vt_plane; g.qkv.qk_plane = qk_plane;
            g.qkv.T = Tq; g.qkv.H = N / 3 / kHeadDim;
            return launch_gemm16(g);
        }
        g.epilogue = epilogue; g.bf = bf;
        if (split_out == 2) g.residual = dC;
        if (split_out == 1) g.out16 = c16; else g.out32 = dC;
        return launch_gemm16(g);
    };
    std::vector<std::vector<double>> samples(n_variants);
    for (int v = 0; v < n_variants && !rc; ++v) rc = run(variants[v] >= 0 ? variants[v] : env_int("PGMI_GEMM_VARIANT", 0));   // warm-up
    for (int r = 0; r < rounds && !rc; ++r)
        for (int v = 0; v < n_variants && !rc; ++v) {              // interleaved rounds: variants see the same clocks / temperature
            const int var = variants[v] >= 0 ? variants[v] : env_int("PGMI_GEMM_VARIANT", 0);
            hipEventRecord(e0, nullptr);
            for (int i = 0; i < iters && !rc; ++i) rc = run(var);
            hipEventRecord(e1, nullptr);
            hipError_t e = hipEventSynchronize(e1);
            float ms = 0.f;
            if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
            if (e != hipSuccess) { set_error("bench failed: %s", hipGetErrorString(e)); rc = PGMI_EHIP; }
            samples[v].push_back(ms / iters);
        }
    if (!rc)
        for (int v = 0; v < n_variants; ++v) {
            std::sort(samples[v].begin(), samples[v].end());
            ms_out[v] = samples[v][samples[v].size() / 2];         // median over the rounds
        }
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    cleanup();
    return rc;
}

int pgmi_bench_gemm(int device, int precision, int M, int N, int K, int epilogue, int split_out, int variant,
                    int iters, double* ms_per_launch) {
    return pgmi_bench_gemm_ab(device, precision, M, N, K, epilogue, split_out, &variant, 1, 1, iters, ms_per_launch);
}

int pgmi_op_qkln_prep(int device, const float* qkv, const float* q_w, const float* k_w, int B, int T, int H, int iters, float* qk,
                      float* v, double* ms) {
    if (!qkv || !q_w || !k_w || B <= 0 || T <= 0 || H <= 0 || H * kHeadDim > 2048 || iters < 0 || (iters > 0 && !ms)) { set_error("bad argument"); return PGMI_EINVAL; }
    if (pgmi_device_count() <= 0) { set_error("no HIP device visible"); return PGMI_ENODEV; }
    PGMI_HIP(hipSetDevice(device));
    const size_t D = (size_t)H * kHeadDim, M = (size_t)B * T, Tp = (size_t)(T + 31) / 32 * 32;
    std::vector<void*> pool;
    auto cleanup = [&]() { for (void* p : pool) hipFree(p); };
    float *dq = nullptr, *dqw = nullptr, *dkw = nullptr;
    unsigned short *qk16 = nullptr, *vt16 = nullptr;
    int rc = 0;
    if ((rc = dev_upload(pool, &dq, qkv, M * 3 * D)) || (rc = dev_upload(pool, &dqw, q_w, D)) || (rc = dev_upload(pool, &dkw, k_w, D)) ||
        (rc = dev_alloc(pool, &qk16, M * 2 * D * 2)) || (rc = dev_alloc(pool, &vt16, (size_t)B * Tp * D * 2))) {
        cleanup();
        return rc;
    }
    pgmi_model tmp;                                      // head_dim 64: ESM2's rotate-half tables
    rc = upload_rotate_half(&tmp, T);
    auto launch = [&]() {
        return launch_qkln_prep(dq, dqw, dkw, 1e-5f, tmp.rot_cos, tmp.rot_sin, B, T, H, qk16, M * 2 * D, vt16, (size_t)B * Tp * D, nullptr);
    };
    if (!rc) rc = launch();
    if (!rc && iters > 0) {
        hipEvent_t e0, e1;
        PGMI_HIP(hipEventCreate(&e0));
        PGMI_HIP(hipEventCreate(&e1));
        hipEventRecord(e0, nullptr);
        for (int i = 0; i < iters && !rc; ++i) rc = launch();
        hipEventRecord(e1, nullptr);
        hipEventSynchronize(e1);
        float t = 0.f;
        hipEventElapsedTime(&t, e0, e1);
        *ms = (double)t / iters;
        hipEventDestroy(e0);
        hipEventDestroy(e1);
    }
    hipDeviceSynchronize();
    std::vector<unsigned short> hq(qk ? M * 2 * D * 2 : 0), hv(v ? (size_t)B * Tp * D * 2 : 0);
    hipError_t e = hipSuccess;
    if (!rc && qk) e = hipMemcpy(hq.data(), qk16, hq.size() * 2, hipMemcpyDeviceToHost);
    if (!rc && v && e == hipSuccess) e = hipMemcpy(hv.data(), vt16, hv.size() * 2, hipMemcpyDeviceToHost);
    for (void* p : tmp.allocs) hipFree(p);
    cleanup();
    if (rc) return rc;
    if (e != hipSuccess) { set_error("qkln prep op failed: %s", hipGetErrorString(e)); return PGMI_EHIP; }
    if (qk)
        for (size_t i = 0; i < M * 2 * D; ++i) qk[i] = rebuild_split(hq[i], hq[M * 2 * D + i]);
    if (v) {
        const size_t vp = (size_t)B * Tp * D;
        for (int b = 0; b < B; ++b)
            for (int t = 0; t < T; ++t) {
                const int tk = t & 31, pos = (t & ~31) + ((tk & 0x13) | ((tk & 4) << 1) | ((tk & 8) >> 1));   // keys with bits 2, 3 swapped
                for (size_t c = 0; c < D; ++c) {
                    const size_t o = ((size_t)b * H * kHeadDim + c) * Tp + pos;
                    v[((size_t)b * T + t) * D + c] = rebuild_split(hv[o], hv[vp + o]);
                }
            }
    }
    return PGMI_OK;
}

int pgmi_op_attention(int device, int precision, const float* qkv, const int32_t* kv_len, int B, int T, int H,
                      int rotary, float* ctx) {
    if (!qkv || !ctx || B <= 0 || T <= 0 || H <= 0) { set_error("bad argument"); return PGMI_EINVAL; }
    if (pgmi_device_count() <= 0) { set_error("no HIP device visible"); return PGMI_ENODEV; }
    PGMI_HIP(hipSetDevice(device));
    std::vector<void*> pool;
    float *dq, *dc;
    int32_t* dl = nullptr;
    const size_t D = (size_t)H * kHeadDim;
    int rc = 0;
    if ((rc = dev_upload(pool, &dq, qkv, (size_t)B * T * 3 * D)) || (kv_len && (rc = dev_upload(pool, &dl, kv_len, (size_t)B))) ||
        (rc = dev_alloc(pool, &dc, (size_t)B * T * D))) {
        for (void* p : pool) hipFree(p);
        return rc;
    }
    pgmi_model tmp;
    tmp.cfg.arch = PGMI_ARCH_ESM2;
    if (rotary) rc = ensure_rotary(&tmp, T);
    if (!rc && precision == PGMI_PREC_F16X3) {
        const size_t Tp = (size_t)(T + 31) / 32 * 32;
        unsigned short *qk = nullptr, *vt = nullptr;
        rc = dev_alloc(pool, &qk, (size_t)B * T * 2 * D * 2);
        if (!rc) rc = dev_alloc(pool, &vt, (size_t)B * Tp * D * 2);
        AttLaunch a;
        a.qk16 = qk, a.qk_plane = (size_t)B * T * 2 * D, a.vt16 = vt, a.vt_plane = (size_t)B * Tp * D;
        a.B = B, a.T = T, a.H = H;
        a.kv_len = dl;
        a.out = ATT_OUT_F32, a.ctx = dc;
        a.qkv = dq, a.cos_t = tmp.rot_cos, a.sin_t = tmp.rot_sin, a.rotary = rotary;
        if (!rc) rc = launch_attention_f16x3_v2(a);
    } else if (!rc) {
        if (rotary) launch_rotary(dq, tmp.rot_cos, tmp.rot_sin, B * T, T, H, nullptr);
        rc = launch_attention_f32(dq, dl, B, T, H, dc, nullptr);
    }
    hipDeviceSynchronize();
    for (void* p : tmp.allocs) hipFree(p);
    hipError_t e = hipMemcpy(ctx, dc, (size_t)B * T * D * 4, hipMemcpyDeviceToHost);
    for (void* p : pool) hipFree(p);
    if (rc) return rc;
    if (e != hipSuccess) { set_error("attention op failed: %s", hipGetErrorString(e)); return PGMI_EHIP; }
    return PGMI_OK;
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
    if (pgmi_device_count() <= 0) { set_error("no HIP device visible"); return PGMI_ENODEV; }
    PGMI_HIP(hipSetDevice(device));
    gemm_options_from_env();
    const size_t M = (size_t)B * T, Da = (size_t)heads * lanes, Tp = (size_t)(T + 31) / 32 * 32, Hs = Da / kHeadDim;
    const int halves = lanes / kHeadDim, rotary = rot_cos != nullptr;
    const size_t qk_plane = M * 2 * Da, vt_plane = (size_t)B * Tp * Da;
    std::vector<void*> pool;
    auto cleanup = [&]() { for (void* p : pool) hipFree(p); };
    float *dx = nullptr, *db = nullptr, *dq = nullptr, *dconv = nullptr, *dcos = nullptr, *dsin = nullptr, *dsl = nullptr;
    unsigned short *a16 = nullptr, *qk16 = nullptr, *vt16 = nullptr, *c16 = nullptr;
    int rc = 0;
    if ((rc = dev_upload(pool, &dsl, slopes, (size_t)heads)) || (rc = dev_alloc(pool, &qk16, qk_plane * 2)) ||
        (rc = dev_alloc(pool, &vt16, vt_plane * 2)) || (rc = dev_alloc(pool, &c16, M * Da * 2)) ||
        (fused && ((rc = dev_upload(pool, &dx, X, M * K)) || (rc = dev_upload(pool, &db, bias, 3 * Da)) || (rc = dev_alloc(pool, &a16, M * K * 2)))) ||
        (rotary && ((rc = dev_upload(pool, &dcos, rot_cos, (size_t)T * std::max(halves, 1) * kHeadDim)) ||
                    (rc = dev_upload(pool, &dsin, rot_sin, (size_t)T * std::max(halves, 1) * kHeadDim)))) ||
        (conv_form && ((rc = dev_upload(pool, &dq, qkv, M * 3 * Da)) || (rc = dev_upload(pool, &dconv, conv, (size_t)3 * 4 * kHeadDim * 8))))) {
        cleanup();
        return rc;
    }
    hipError_t e = hipMemset(vt16, 0, vt_plane * 2 * sizeof(unsigned short));      // pad keys: finite (reset_pad_keys)
    if (e != hipSuccess) { cleanup(); set_error("causal attention op failed: %s", hipGetErrorString(e)); return PGMI_EHIP; }
    if (fused) {
        W16 w16;
        rc = make_w16(pool, W, 3 * Da * K, (size_t)K, PGMI_PREC_F16X3, nullptr, &w16);
        if (!rc) {
            launch_split16(dx, (int64_t)(M * K), 1.0f, 2, K, a16, nullptr);
            GemmLaunch g = op_gemm(a16, w16, db, (int)M, 3 * (int)Da, K, env_int("PGMI_GEMM_VARIANT", 0));
            g.out16 = qk16;
            g.qkv.vt16 = vt16; g.qkv.vt_plane = vt_plane; g.qkv.qk_plane = qk_plane;
            g.qkv.cos_t = dcos; g.qkv.sin_t = dsin; g.qkv.rotary = rotary;
            g.qkv.T = T; g.qkv.H = (int)Hs; g.qkv.rot_halves = halves;
            rc = launch_gemm16(g);
        }
    }
    AttLaunch a;
    a.qk16 = qk16, a.qk_plane = qk_plane, a.vt16 = vt16, a.vt_plane = vt_plane;
    a.B = B, a.T = T, a.H = heads, a.head_dim = lanes;
    a.slopes = dsl;
    a.out = ATT_OUT_SPLIT, a.ctx16 = c16;
    a.qkv = dq, a.conv = dconv;             // conv form only (the fused form's operands carry the rotary already)
    if (!rc) rc = launch_attention_f16x3_v2(a);
    std::vector<unsigned short> h(rc ? 0 : M * Da * 2);
    e = hipDeviceSynchronize();
    if (!rc && e == hipSuccess) e = hipMemcpy(h.data(), c16, h.size() * 2, hipMemcpyDeviceToHost);
    cleanup();
    if (rc) return rc;
    if (e != hipSuccess) { set_error("causal attention op failed: %s", hipGetErrorString(e)); return PGMI_EHIP; }
    for (size_t m = 0; m < M; ++m)                               // the context planes (K-interleaved rows of Da) rebuilt as fp32
        for (size_t n = 0; n < Da; ++n) {
            const size_t o = ki_off(m, (int)n, (int)Da);
            ctx[m * Da + n] = rebuild_split(h[o], h[o + 32]);
        }
    return PGMI_OK;
}

// PoET's prefix attention through launch_prefix_prep / launch_prefix_attention (attention_prefix.hip): the prefix planes are filled by the
// prep pass over one segment of P rows (as pgmi_poet_set_prompt fills the cache), the own planes by the prep pass over the segments.
int pgmi_op_prefix_attention(int device, const float* qkv, const int32_t* seg_off, int n_seg, const float* prefix_kv, int P, int heads,
                             int split, float* ctx) {
    if (!qkv || !seg_off || !ctx || n_seg <= 0 || heads <= 0 || P < 0 || (P > 0 && !prefix_kv) || seg_off[0] != 0) { set_error("bad argument"); return PGMI_EINVAL; }
    std::vector<int32_t> ent_seg, ent_tile, pseg{0, P}, pent_seg, pent_tile;
    for (int b = 0; b < n_seg; ++b) {
        const int len = seg_off[b + 1] - seg_off[b];
        if (len <= 0) { set_error("segment %d is empty", b); return PGMI_EINVAL; }
        for (int j = 0; j * 32 < len; ++j) { ent_seg.push_back(b); ent_tile.push_back(j); }
    }
    for (int j = 0; j * 32 < P; ++j) { pent_seg.push_back(0); pent_tile.push_back(j); }
    if (pgmi_device_count() <= 0) { set_error("no HIP device visible"); return PGMI_ENODEV; }
    PGMI_HIP(hipSetDevice(device));
    const size_t R = (size_t)seg_off[n_seg], Da = (size_t)heads * kHeadDim, pitch = ent_seg.size() * 32, ppitch = pent_seg.size() * 32;
    std::vector<float> pq((size_t)P * 3 * Da, 0.0f);            // the prefix rows as q | k | v with a zero q block
    for (size_t t = 0; t < (size_t)P; ++t) memcpy(&pq[t * 3 * Da + Da], prefix_kv + t * 2 * Da, 2 * Da * sizeof(float));
    std::vector<void*> pool;
    auto cleanup = [&]() { for (void* p : pool) hipFree(p); };
    float *dq = nullptr, *dpq = nullptr, *dctx = nullptr;
    int32_t *d_off = nullptr, *d_es = nullptr, *d_et = nullptr, *dp_off = nullptr, *dp_es = nullptr, *dp_et = nullptr;
    unsigned short *q16 = nullptr, *k16 = nullptr, *vt16 = nullptr, *pq16 = nullptr, *pk16 = nullptr, *pvt16 = nullptr, *c16 = nullptr;
    int rc = 0;
    if ((rc = dev_upload(pool, &dq, qkv, R * 3 * Da)) || (rc = dev_upload(pool, &d_off, seg_off, (size_t)n_seg + 1)) ||
        (rc = dev_upload(pool, &d_es, ent_seg.data(), ent_seg.size())) || (rc = dev_upload(pool, &d_et, ent_tile.data(), ent_tile.size())) ||
        (rc = dev_alloc(pool, &q16, 2 * R * Da)) || (rc = dev_alloc(pool, &k16, 2 * Da * pitch)) || (rc = dev_alloc(pool, &vt16, 2 * Da * pitch)) ||
        (rc = dev_alloc(pool, &c16, 2 * R * Da)) || (rc = dev_alloc(pool, &dctx, R * Da)) ||
        (P > 0 && ((rc = dev_upload(pool, &dpq, pq.data(), pq.size())) || (rc = dev_upload(pool, &dp_off, pseg.data(), pseg.size())) ||
                   (rc = dev_upload(pool, &dp_es, pent_seg.data(), pent_seg.size())) || (rc = dev_upload(pool, &dp_et, pent_tile.data(), pent_tile.size())) ||
                   (rc = dev_alloc(pool, &pq16, 2 * (size_t)P * Da)) || (rc = dev_alloc(pool, &pk16, 2 * Da * ppitch)) ||
                   (rc = dev_alloc(pool, &pvt16, 2 * Da * ppitch))))) {
        cleanup();
        return rc;
    }
    // what the kernels must write themselves starts as 0xFF bytes (NaN): an operand element or a context row they skip shows
    hipError_t e = hipMemset(k16, 0xFF, 2 * Da * pitch * 2);
    if (e == hipSuccess) e = hipMemset(vt16, 0xFF, 2 * Da * pitch * 2);
    if (e == hipSuccess) e = hipMemset(c16, 0xFF, 2 * R * Da * 2);
    if (e == hipSuccess) e = hipMemset(dctx, 0xFF, R * Da * 4);
    if (e == hipSuccess && P > 0) e = hipMemset(pk16, 0xFF, 2 * Da * ppitch * 2);
    if (e == hipSuccess && P > 0) e = hipMemset(pvt16, 0xFF, 2 * Da * ppitch * 2);
    if (e != hipSuccess) { cleanup(); set_error("prefix attention op failed: %s", hipGetErrorString(e)); return PGMI_EHIP; }
    if (P > 0) {
        PrefixAttLaunch p;
        p.qkv = dpq; p.seg_off = dp_off; p.ent_seg = dp_es; p.ent_tile = dp_et; p.n_seg = 1; p.n_ent = (int)pent_seg.size(); p.H = heads;
        p.q16 = pq16; p.q_plane = (size_t)P * Da; p.k16 = pk16; p.vt16 = pvt16; p.pitch = ppitch;
        rc = launch_prefix_prep(p);
    }
    PrefixAttLaunch a;
    a.qkv = dq; a.seg_off = d_off; a.ent_seg = d_es; a.ent_tile = d_et; a.n_seg = n_seg; a.n_ent = (int)ent_seg.size(); a.H = heads;
    a.q16 = q16; a.q_plane = R * Da; a.k16 = k16; a.vt16 = vt16; a.pitch = pitch;
    a.pk16 = pk16; a.pvt16 = pvt16; a.ppitch = ppitch; a.P = P;
    a.out = split ? ATT_OUT_SPLIT : ATT_OUT_F32; a.ctx = dctx; a.ctx16 = c16;
    if (!rc) rc = launch_prefix_prep(a);
    if (!rc) rc = launch_prefix_attention(a);
    std::vector<unsigned short> h(rc || !split ? 0 : R * Da * 2);
    e = hipDeviceSynchronize();
    if (!rc && e == hipSuccess) e = split ? hipMemcpy(h.data(), c16, h.size() * 2, hipMemcpyDeviceToHost) : hipMemcpy(ctx, dctx, R * Da * 4, hipMemcpyDeviceToHost);
    cleanup();
    if (rc) return rc;
    if (e != hipSuccess) { set_error("prefix attention op failed: %s", hipGetErrorString(e)); return PGMI_EHIP; }
    if (split)
        for (size_t m = 0; m < R; ++m)
            for (size_t n = 0; n < Da; ++n) {
                const size_t o = ki_off(m, (int)n, (int)Da);
                ctx[m * Da + n] = rebuild_split(h[o], h[o + 32]);
            }
    return PGMI_OK;
}

// ESM-IF1's cross-attention through launch_cross_q_prep / launch_cross_attention (attention_prefix.hip): the memory planes are filled by
// the prep pass over one segment of S rows (as pgmi_esmif1_set_memory fills a layer's planes).
int pgmi_op_cross_attention(int device, const float* q, const int32_t* seg_off, int n_seg, const float* mem_kv, int S, int heads,
                            int split, float* ctx) {
    if (!q || !seg_off || !ctx || !mem_kv || n_seg <= 0 || heads <= 0 || S <= 0 || seg_off[0] != 0) { set_error("bad argument"); return PGMI_EINVAL; }
    std::vector<int32_t> ent_seg, ent_tile, pseg{0, S}, pent_seg, pent_tile;
    for (int b = 0; b < n_seg; ++b) {
        const int len = seg_off[b + 1] - seg_off[b];
        if (len <= 0) { set_error("segment %d is empty", b); return PGMI_EINVAL; }
        for (int j = 0; j * 32 < len; ++j) { ent_seg.push_back(b); ent_tile.push_back(j); }
    }
    for (int j = 0; j * 32 < S; ++j) { pent_seg.push_back(0); pent_tile.push_back(j); }
    if (pgmi_device_count() <= 0) { set_error("no HIP device visible"); return PGMI_ENODEV; }
    PGMI_HIP(hipSetDevice(device));
    const size_t R = (size_t)seg_off[n_seg], Da = (size_t)heads * kHeadDim, ppitch = pent_seg.size() * 32;
    std::vector<float> pq((size_t)S * 3 * Da, 0.0f);            // the memory rows as q | k | v with a zero q block
    for (size_t t = 0; t < (size_t)S; ++t) memcpy(&pq[t * 3 * Da + Da], mem_kv + t * 2 * Da, 2 * Da * sizeof(float));
    std::vector<void*> pool;
    auto cleanup = [&]() { for (void* p : pool) hipFree(p); };
    float *dq = nullptr, *dpq = nullptr, *dctx = nullptr;
    int32_t *d_off = nullptr, *d_es = nullptr, *d_et = nullptr, *dp_off = nullptr, *dp_es = nullptr, *dp_et = nullptr;
    unsigned short *q16 = nullptr, *pq16 = nullptr, *pk16 = nullptr, *pvt16 = nullptr, *c16 = nullptr;
    int rc = 0;
    if ((rc = dev_upload(pool, &dq, q, R * Da)) || (rc = dev_upload(pool, &d_off, seg_off, (size_t)n_seg + 1)) ||
        (rc = dev_upload(pool, &d_es, ent_seg.data(), ent_seg.size())) || (rc = dev_upload(pool, &d_et, ent_tile.data(), ent_tile.size())) ||
        (rc = dev_alloc(pool, &q16, 2 * R * Da)) || (rc = dev_alloc(pool, &c16, 2 * R * Da)) || (rc = dev_alloc(pool, &dctx, R * Da)) ||
        (rc = dev_upload(pool, &dpq, pq.data(), pq.size())) || (rc = dev_upload(pool, &dp_off, pseg.data(), pseg.size())) ||
        (rc = dev_upload(pool, &dp_es, pent_seg.data(), pent_seg.size())) || (rc = dev_upload(pool, &dp_et, pent_tile.data(), pent_tile.size())) ||
        (rc = dev_alloc(pool, &pq16, 2 * (size_t)S * Da)) || (rc = dev_alloc(pool, &pk16, 2 * Da * ppitch)) ||
        (rc = dev_alloc(pool, &pvt16, 2 * Da * ppitch))) {
        cleanup();
        return rc;
    }
    // what the kernels must write themselves starts as 0xFF bytes (NaN): an operand element or a context row they skip shows
    hipError_t e = hipMemset(q16, 0xFF, 2 * R * Da * 2);
    if (e == hipSuccess) e = hipMemset(c16, 0xFF, 2 * R * Da * 2);
    if (e == hipSuccess) e = hipMemset(dctx, 0xFF, R * Da * 4);
    if (e == hipSuccess) e = hipMemset(pk16, 0xFF, 2 * Da * ppitch * 2);
    if (e == hipSuccess) e = hipMemset(pvt16, 0xFF, 2 * Da * ppitch * 2);
    if (e != hipSuccess) { cleanup(); set_error("cross attention op failed: %s", hipGetErrorString(e)); return PGMI_EHIP; }
    PrefixAttLaunch p;
    p.qkv = dpq; p.seg_off = dp_off; p.ent_seg = dp_es; p.ent_tile = dp_et; p.n_seg = 1; p.n_ent = (int)pent_seg.size(); p.H = heads;
    p.q16 = pq16; p.q_plane = (size_t)S * Da; p.k16 = pk16; p.vt16 = pvt16; p.pitch = ppitch;
    rc = launch_prefix_prep(p);
    PrefixAttLaunch a;
    a.seg_off = d_off; a.ent_seg = d_es; a.ent_tile = d_et; a.n_seg = n_seg; a.n_ent = (int)ent_seg.size(); a.H = heads;
    a.q16 = q16; a.q_plane = R * Da;
    a.pk16 = pk16; a.pvt16 = pvt16; a.ppitch = ppitch; a.P = S;
    a.out = split ? ATT_OUT_SPLIT : ATT_OUT_F32; a.ctx = dctx; a.ctx16 = c16;
    if (!rc) rc = launch_cross_q_prep(dq, R, heads, q16, R * Da, nullptr);
    if (!rc) rc = launch_cross_attention(a);
    std::vector<unsigned short> h(rc || !split ? 0 : R * Da * 2);
    e = hipDeviceSynchronize();
    if (!rc && e == hipSuccess) e = split ? hipMemcpy(h.data(), c16, h.size() * 2, hipMemcpyDeviceToHost) : hipMemcpy(ctx, dctx, R * Da * 4, hipMemcpyDeviceToHost);
    cleanup();
    if (rc) return rc;
    if (e != hipSuccess) { set_error("cross attention op failed: %s", hipGetErrorString(e)); return PGMI_EHIP; }
    if (split)
        for (size_t m = 0; m < R; ++m)
            for (size_t n = 0; n < Da; ++n) {
                const size_t o = ki_off(m, (int)n, (int)Da);
                ctx[m * Da + n] = rebuild_split(h[o], h[o + 32]);
            }
    return PGMI_OK;
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
    int rc = tied_row_check(R, C, H, S);
    if (rc) return rc;
    if (pgmi_device_count() <= 0) { set_error("no HIP device visible"); return PGMI_ENODEV; }
    PGMI_HIP(hipSetDevice(device));
    const size_t M = (size_t)R * C, D = (size_t)H * kHeadDim, Kp = (size_t)tied_row_kp(C);
    const size_t n_part = (size_t)H * S * C * Kp, n_p = (size_t)H * C * Kp, n_vt = (size_t)H * R * kHeadDim * Kp;
    std::vector<void*> pool;
    auto cleanup = [&]() { for (void* p : pool) hipFree(p); };
    float *dq = nullptr, *part = nullptr, *pp = nullptr, *vt = nullptr;
    unsigned short *qctx16 = nullptr, *k16 = nullptr;
    if ((rc = dev_upload(pool, &dq, qkv, M * 3 * D)) || (rc = dev_alloc(pool, &qctx16, M * D * 2)) || (rc = dev_alloc(pool, &k16, M * D * 2)) ||
        (rc = dev_alloc(pool, &part, n_part)) || (rc = dev_alloc(pool, &pp, n_p)) || (rc = dev_alloc(pool, &vt, n_vt))) {
        cleanup();
        return rc;
    }
    hipError_t e = hipMemset(part, 0xFF, n_part * 4);
    if (e == hipSuccess) e = hipMemset(pp, 0xFF, n_p * 4);
    if (e == hipSuccess) e = hipMemset(vt, 0xFF, n_vt * 4);
    if (e == hipSuccess) e = hipMemset(qctx16, 0xFF, M * D * 2 * sizeof(unsigned short));
    if (e != hipSuccess) { cleanup(); set_error("tied row attention op failed: %s", hipGetErrorString(e)); return PGMI_EHIP; }
    TiedRowLaunch t;
    t.qkv = dq, t.R = R, t.C = C, t.H = H, t.S = S;
    t.qctx16 = qctx16, t.k16 = k16;
    t.part = part, t.p = pp, t.vt = vt;
    rc = launch_tied_row_attention(t);
    std::vector<unsigned short> h(rc ? 0 : M * D * 2), hp(rc || !probs ? 0 : n_p * 2);
    e = hipDeviceSynchronize();
    if (!rc && e == hipSuccess) e = hipMemcpy(h.data(), qctx16, h.size() * 2, hipMemcpyDeviceToHost);
    if (!rc && probs && e == hipSuccess) e = hipMemcpy(hp.data(), pp, hp.size() * 2, hipMemcpyDeviceToHost);
    cleanup();
    if (rc) return rc;
    if (e != hipSuccess) { set_error("tied row attention op failed: %s", hipGetErrorString(e)); return PGMI_EHIP; }
    for (size_t m = 0; m < M; ++m)                               // the context planes (K-interleaved rows of D) rebuilt as fp32
        for (size_t n = 0; n < D; ++n) {
            const size_t o = ki_off(m, (int)n, (int)D);
            ctx[m * D + n] = rebuild_split(h[o], h[o + 32]);
        }
    if (probs)                                                   // the P planes: rows (h, i) of Kp columns
        for (size_t r = 0; r < (size_t)H * C; ++r)
            for (size_t j = 0; j < Kp; ++j) {
                const size_t o = ki_off(r, (int)j, (int)Kp);
                probs[r * Kp + j] = rebuild_split(hp[o], hp[o + 32]);
            }
    return PGMI_OK;
}

// The column attention of one MSA Transformer layer (run_msa's column block): the activation split, the fused QKV projection without
// rotary on sequences of R rows, V^T planes zeroed first (pad keys must be finite), then the dense attention with B = C, T = R, a device
// kv_len of C entries equal to R and the split-plane context, which starts as 0xFF bytes.
int pgmi_op_column_attention(int device, const float* X, const float* W, const float* bias, int K, int R, int C, int H, float* ctx) {
    if (!X || !W || !bias || !ctx || R <= 0 || C <= 0 || H <= 0) { set_error("bad argument"); return PGMI_EINVAL; }
    // the activation / weight split writes K-interleaved rows (ki_off) before any launcher sees K: whole groups of 32 only
    if (K <= 0 || K % 32) { set_error("column attention op: K = %d is not a positive multiple of 32", K); return PGMI_EINVAL; }
    if (pgmi_device_count() <= 0) { set_error("no HIP device visible"); return PGMI_ENODEV; }
    PGMI_HIP(hipSetDevice(device));
    gemm_options_from_env();
    const size_t M = (size_t)C * R, D = (size_t)H * kHeadDim, Tp = (size_t)(R + 31) / 32 * 32;
    const size_t qk_plane = M * 2 * D, vt_plane = (size_t)C * Tp * D;
    std::vector<void*> pool;
    auto cleanup = [&]() { for (void* p : pool) hipFree(p); };
    const std::vector<int32_t> kv((size_t)C, R);
    float *dx = nullptr, *db = nullptr;
    int32_t* dl = nullptr;
    unsigned short *a16 = nullptr, *qk16 = nullptr, *vt16 = nullptr, *c16 = nullptr;
    int rc = 0;
    if ((rc = dev_upload(pool, &dx, X, M * K)) || (rc = dev_upload(pool, &db, bias, 3 * D)) || (rc = dev_upload(pool, &dl, kv.data(), kv.size())) ||
        (rc = dev_alloc(pool, &a16, M * K * 2)) || (rc = dev_alloc(pool, &qk16, qk_plane * 2)) || (rc = dev_alloc(pool, &vt16, vt_plane * 2)) ||
        (rc = dev_alloc(pool, &c16, M * D * 2))) {
        cleanup();
        return rc;
    }
    hipError_t e = hipMemset(vt16, 0, vt_plane * 2 * sizeof(unsigned short));
    if (e == hipSuccess) e = hipMemset(c16, 0xFF, M * D * 2 * sizeof(unsigned short));
    if (e != hipSuccess) { cleanup(); set_error("column attention op failed: %s", hipGetErrorString(e)); return PGMI_EHIP; }
    W16 w16;
    rc = make_w16(pool, W, 3 * D * K, (size_t)K, PGMI_PREC_F16X3, nullptr, &w16);
    if (!rc) {
        launch_split16(dx, (int64_t)(M * K), 1.0f, 2, K, a16, nullptr);
        GemmLaunch g = op_gemm(a16, w16, db, (int)M, 3 * (int)D, K, env_int("PGMI_GEMM_VARIANT", 0));
        g.out16 = qk16;
        g.qkv.vt16 = vt16; g.qkv.vt_plane = vt_plane; g.qkv.qk_plane = qk_plane;
        g.qkv.T = R; g.qkv.H = H;
        rc = launch_gemm16(g);
    }
    AttLaunch a;
    a.qk16 = qk16, a.qk_plane = qk_plane, a.vt16 = vt16, a.vt_plane = vt_plane;
    a.B = C, a.T = R, a.H = H;
    a.kv_len = dl;
    a.out = ATT_OUT_SPLIT, a.ctx16 = c16;
    if (!rc) rc = launch_attention_f16x3_v2(a);
    std::vector<unsigned short> h(rc ? 0 : M * D * 2);
    e = hipDeviceSynchronize();
    if (!rc && e == hipSuccess) e = hipMemcpy(h.data(), c16, h.size() * 2, hipMemcpyDeviceToHost);
    cleanup();
    if (rc) return rc;
    if (e != hipSuccess) { set_error("column attention op failed: %s", hipGetErrorString(e)); return PGMI_EHIP; }
    for (size_t m = 0; m < M; ++m)
        for (size_t n = 0; n < D; ++n) {
            const size_t o = ki_off(m, (int)n, (int)D);
            ctx[m * D + n] = rebuild_split(h[o], h[o + 32]);
        }
    return PGMI_OK;
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
    if (pgmi_device_count() <= 0) { set_error("no HIP device visible"); return PGMI_ENODEV; }
    PGMI_HIP(hipSetDevice(device));
    gemm_options_from_env();
    const size_t M = (size_t)B * T, Da = (size_t)heads * lanes, Tp = (size_t)(T + 31) / 32 * 32, Hs = Da / kHeadDim;
    const int halves = lanes / kHeadDim, rotary = rot_cos != nullptr;
    const size_t qk_plane = M * 2 * Da, vt_plane = (size_t)B * Tp * Da;
    std::vector<void*> pool;
    auto cleanup = [&]() { for (void* p : pool) hipFree(p); };
    float *dx = nullptr, *db = nullptr, *dcos = nullptr, *dsin = nullptr, *dc = nullptr;
    int32_t* dl = nullptr;
    unsigned short *a16 = nullptr, *qk16 = nullptr, *vt16 = nullptr;
    int rc = 0;
    // dc: M Da fp32 values, M Da hi | lo pairs or M Da bf16 values -- one buffer of the largest of the three context kinds
    if ((rc = dev_upload(pool, &dx, X, M * K)) || (rc = dev_upload(pool, &db, bias, 3 * Da)) || (kv_len && (rc = dev_upload(pool, &dl, kv_len, (size_t)B))) ||
        (rotary && ((rc = dev_upload(pool, &dcos, rot_cos, (size_t)T * halves * kHeadDim)) || (rc = dev_upload(pool, &dsin, rot_sin, (size_t)T * halves * kHeadDim)))) ||
        (rc = dev_alloc(pool, &a16, M * K * 2)) || (rc = dev_alloc(pool, &qk16, qk_plane * 2)) || (rc = dev_alloc(pool, &vt16, vt_plane * 2)) ||
        (rc = dev_alloc(pool, &dc, M * Da))) {
        cleanup();
        return rc;
    }
    hipError_t e = hipMemset(vt16, 0, vt_plane * 2 * sizeof(unsigned short));      // pad keys: finite (reset_pad_keys)
    if (e == hipSuccess) e = hipMemset(qk16, 0xFF, qk_plane * 2 * sizeof(unsigned short));
    if (e == hipSuccess) e = hipMemset(dc, 0xFF, M * Da * sizeof(float));
    if (e != hipSuccess) { cleanup(); set_error("dense attention op failed: %s", hipGetErrorString(e)); return PGMI_EHIP; }
    W16 w16;
    rc = make_w16(pool, W, 3 * Da * K, (size_t)K, PGMI_PREC_F16X3, nullptr, &w16);
    if (!rc) {
        launch_split16(dx, (int64_t)(M * K), 1.0f, 2, K, a16, nullptr);
        GemmLaunch g = op_gemm(a16, w16, db, (int)M, 3 * (int)Da, K, env_int("PGMI_GEMM_VARIANT", 0));
        g.out16 = qk16;
        g.qkv.vt16 = vt16; g.qkv.vt_plane = vt_plane; g.qkv.qk_plane = qk_plane;
        g.qkv.cos_t = dcos; g.qkv.sin_t = dsin; g.qkv.rotary = rotary;
        g.qkv.T = T; g.qkv.H = (int)Hs; g.qkv.rot_halves = halves;
        rc = launch_gemm16(g);
    }
    AttLaunch a;
    a.qk16 = qk16, a.qk_plane = qk_plane, a.vt16 = vt16, a.vt_plane = vt_plane;
    a.B = B, a.T = T, a.H = heads, a.head_dim = lanes;
    a.kv_len = dl;
    a.out = (AttOut)out, a.ctx = dc, a.ctx16 = reinterpret_cast<unsigned short*>(dc);
    if (!rc) rc = launch_attention_f16x3_v2(a);
    std::vector<float> hc(rc ? 0 : M * Da);
    std::vector<unsigned short> hq(rc || !qk ? 0 : qk_plane * 2), hv(rc || !v ? 0 : vt_plane * 2);
    e = hipDeviceSynchronize();
    if (!rc && e == hipSuccess) e = hipMemcpy(hc.data(), dc, hc.size() * sizeof(float), hipMemcpyDeviceToHost);
    if (!rc && qk && e == hipSuccess) e = hipMemcpy(hq.data(), qk16, hq.size() * 2, hipMemcpyDeviceToHost);
    if (!rc && v && e == hipSuccess) e = hipMemcpy(hv.data(), vt16, hv.size() * 2, hipMemcpyDeviceToHost);
    cleanup();
    if (rc) return rc;
    if (e != hipSuccess) { set_error("dense attention op failed: %s", hipGetErrorString(e)); return PGMI_EHIP; }
    const unsigned short* h16 = reinterpret_cast<const unsigned short*>(hc.data());
    if (out == ATT_OUT_F32) memcpy(ctx, hc.data(), M * Da * sizeof(float));
    for (size_t m = 0; m < M && out == ATT_OUT_SPLIT; ++m)       // the context planes (K-interleaved rows of Da) rebuilt as fp32
        for (size_t n = 0; n < Da; ++n) {
            const size_t o = ki_off(m, (int)n, (int)Da);
            ctx[m * Da + n] = rebuild_split(h16[o], h16[o + 32]);
        }
    for (size_t i = 0; i < M * Da && out == ATT_OUT_BF16; ++i) {  // one bf16 plane, row-major
        const unsigned int u = (unsigned int)h16[i] << 16;
        memcpy(&ctx[i], &u, 4);
    }
    if (qk)
        for (size_t i = 0; i < qk_plane; ++i) qk[i] = rebuild_split(hq[i], hq[qk_plane + i]);
    if (v)
        for (int b = 0; b < B; ++b)
            for (int t = 0; t < T; ++t) {
                const int tk = t & 31, pos = (t & ~31) + ((tk & 0x13) | ((tk & 4) << 1) | ((tk & 8) >> 1));   // keys with bits 2, 3 swapped
                for (size_t c = 0; c < Da; ++c) {
                    const size_t o = ((size_t)b * Da + c) * Tp + pos;
                    v[((size_t)b * T + t) * Da + c] = rebuild_split(hv[o], hv[vt_plane + o]);
                }
            }
    return PGMI_OK;
}

// ESM3's geometric attention kernel (geom_attention.hip) through the launcher the model and the structure tokenizer use.
int pgmi_op_geom_attention(int device, const float* proj, const float* rot, const float* trans, const int32_t* frame_mask,
                           int per_row_frames, const float* w_rot, const float* w_dist, int B, int S, int H, float* out) {
    if (!proj || !rot || !trans || !frame_mask || !w_rot || !w_dist || !out || B <= 0 || S <= 0 || H <= 0) { set_error("bad argument"); return PGMI_EINVAL; }
    if (pgmi_device_count() <= 0) { set_error("no HIP device visible"); return PGMI_ENODEV; }
    PGMI_HIP(hipSetDevice(device));
    const size_t rows = (size_t)B * S, nf = per_row_frames ? rows : (size_t)S;
    std::vector<void*> pool;
    auto cleanup = [&]() { for (void* p : pool) hipFree(p); };
    float *dp = nullptr, *dr = nullptr, *dt = nullptr, *dwr = nullptr, *dwd = nullptr, *dout = nullptr;
    int32_t* dm = nullptr;
    int rc = 0;
    if ((rc = dev_upload(pool, &dp, proj, rows * 15 * H)) || (rc = dev_upload(pool, &dr, rot, nf * 9)) || (rc = dev_upload(pool, &dt, trans, nf * 3)) ||
        (rc = dev_upload(pool, &dm, frame_mask, nf)) || (rc = dev_upload(pool, &dwr, w_rot, (size_t)H)) || (rc = dev_upload(pool, &dwd, w_dist, (size_t)H)) ||
        (rc = dev_alloc(pool, &dout, rows * 3 * H))) {
        cleanup();
        return rc;
    }
    hipError_t e = hipMemset(dout, 0xFF, rows * 3 * H * sizeof(float));         // an element the kernel skips shows as NaN
    GeomAttLaunch g;
    g.proj = dp, g.pitch = 15 * H;
    g.rot = dr, g.trans = dt, g.mask = dm, g.per_row_frames = per_row_frames != 0;
    g.w_rot = dwr, g.w_dist = dwd;
    g.B = B, g.S = S, g.H = H;
    g.out = dout, g.opitch = 3 * H;
    if (e == hipSuccess) rc = launch_geom_attention(g);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (!rc && e == hipSuccess) e = hipMemcpy(out, dout, rows * 3 * H * sizeof(float), hipMemcpyDeviceToHost);
    cleanup();
    if (rc) return rc;
    if (e != hipSuccess) { set_error("geometric attention op failed: %s", hipGetErrorString(e)); return PGMI_EHIP; }
    return PGMI_OK;
}

int pgmi_op_geom_key_tile(int S) { return geom_key_tile(S); }

// ---- the scoring tail (elementwise.hip): log-softmax heads and per-sequence sums on their own buffers ----------------------------------
// Every output is allocated with kOutGuard spare values behind it and starts as 0xFF bytes (NaN): an element the kernel skips shows as
// NaN on the host, and a guard value the kernel touched fails the call.  *nonfinite is the device flag after the launch (zero before).
static constexpr size_t kOutGuard = 64;                          // one row of the narrow head at its widest
static int out_alloc(std::vector<void*>& pool, float** p, size_t n) {
    int rc = dev_alloc(pool, p, n + kOutGuard);
    if (rc) return rc;
    PGMI_HIP(hipMemset(*p, 0xFF, (n + kOutGuard) * sizeof(float)));
    return PGMI_OK;
}
static int out_fetch(const float* d, size_t n, float* host, const char* what) {
    uint32_t guard[kOutGuard];
    PGMI_HIP(hipMemcpy(host, d, n * sizeof(float), hipMemcpyDeviceToHost));
    PGMI_HIP(hipMemcpy(guard, d + n, sizeof(guard), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < kOutGuard; ++i)
        if (guard[i] != 0xFFFFFFFFu) { set_error("%s op: the kernel wrote %zu values past the end of its output", what, i + 1); return PGMI_EHIP; }
    return PGMI_OK;
}
static int flag_alloc(std::vector<void*>& pool, int32_t** p) {
    int rc = dev_alloc(pool, p, (size_t)1);
    if (rc) return rc;
    PGMI_HIP(hipMemset(*p, 0, 4));
    return PGMI_OK;
}
static int op_finish(hipError_t e, const char* what) {
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) { set_error("%s op failed: %s", what, hipGetErrorString(e)); return PGMI_EHIP; }
    return PGMI_OK;
}

int pgmi_op_vocab_logsoftmax(int device, const float* h, const float* E, const float* bias, int rows, int D, int V, float* out,
                             int32_t* nonfinite) {
    if (!h || !E || !bias || !out || !nonfinite || rows <= 0 || D <= 0) { set_error("bad argument"); return PGMI_EINVAL; }
    if (V < 1 || V > 64) { set_error("narrow log-softmax op: V = %d is outside 1 .. 64 (lane v owns logit v)", V); return PGMI_EINVAL; }
    if (pgmi_device_count() <= 0) { set_error("no HIP device visible"); return PGMI_ENODEV; }
    PGMI_HIP(hipSetDevice(device));
    std::vector<void*> pool;
    auto cleanup = [&]() { for (void* p : pool) hipFree(p); };
    float *dh = nullptr, *dE = nullptr, *db = nullptr, *dout = nullptr;
    int32_t* dflag = nullptr;
    const size_t n_out = (size_t)rows * V;
    int rc = 0;
    if ((rc = dev_upload(pool, &dh, h, (size_t)rows * D)) || (rc = dev_upload(pool, &dE, E, (size_t)V * D)) ||
        (rc = dev_upload(pool, &db, bias, (size_t)V)) || (rc = out_alloc(pool, &dout, n_out)) || (rc = flag_alloc(pool, &dflag))) {
        cleanup();
        return rc;
    }
    launch_vocab_logsoftmax(dh, dE, db, rows, D, V, dout, dflag, nullptr);
    rc = op_finish(hipDeviceSynchronize(), "narrow log-softmax");
    if (!rc) rc = out_fetch(dout, n_out, out, "narrow log-softmax");
    if (!rc) rc = op_finish(hipMemcpy(nonfinite, dflag, 4, hipMemcpyDeviceToHost), "narrow log-softmax");
    cleanup();
    return rc;
}

int pgmi_op_wide_logsoftmax(int device, const float* logits, int ldl, int rows, int V, const int32_t* tgt, float* out,
                            int32_t* nonfinite) {
    if (!logits || !out || !nonfinite || rows <= 0 || V <= 0 || ldl <= 0) { set_error("bad argument"); return PGMI_EINVAL; }
    if (ldl % 4 || ldl < V) { set_error("wide log-softmax op: ldl = %d must be a multiple of 4 and at least V = %d", ldl, V); return PGMI_EINVAL; }
    for (int r = 0; tgt && r < rows; ++r)
        if (tgt[r] < 0 || tgt[r] >= V) { set_error("wide log-softmax op: tgt[%d] = %d is outside [0, %d)", r, tgt[r], V); return PGMI_EINVAL; }
    if (pgmi_device_count() <= 0) { set_error("no HIP device visible"); return PGMI_ENODEV; }
    PGMI_HIP(hipSetDevice(device));
    std::vector<void*> pool;
    auto cleanup = [&]() { for (void* p : pool) hipFree(p); };
    float *dl = nullptr, *dout = nullptr;
    int32_t *dt = nullptr, *dflag = nullptr;
    const size_t n_out = tgt ? (size_t)rows : (size_t)rows * V;
    int rc = 0;
    if ((rc = dev_upload(pool, &dl, logits, (size_t)rows * ldl)) || (tgt && (rc = dev_upload(pool, &dt, tgt, (size_t)rows))) ||
        (rc = out_alloc(pool, &dout, n_out)) || (rc = flag_alloc(pool, &dflag))) {
        cleanup();
        return rc;
    }
    launch_wide_logsoftmax(dl, ldl, rows, V, dt, dout, dflag, nullptr);
    rc = op_finish(hipDeviceSynchronize(), "wide log-softmax");
    if (!rc) rc = out_fetch(dout, n_out, out, "wide log-softmax");
    if (!rc) rc = op_finish(hipMemcpy(nonfinite, dflag, 4, hipMemcpyDeviceToHost), "wide log-softmax");
    cleanup();
    return rc;
}

int pgmi_op_group_logsoftmax(int device, const float* h, const float* E, const float* bias, int rows, int D, int V, int first, int groups,
                             int width, float* full, float* group, int32_t* nonfinite) {
    if (!h || !E || !bias || !nonfinite || rows <= 0 || D <= 0 || V <= 0 || first < 0 || groups <= 0 || width <= 0) { set_error("bad argument"); return PGMI_EINVAL; }
    if (!full && !group) { set_error("grouped log-softmax op: neither `full` nor `group` is asked for"); return PGMI_EINVAL; }
    int rc = group_logsoftmax_check(D, V, first, groups, width);
    if (rc) return rc;
    if (pgmi_device_count() <= 0) { set_error("no HIP device visible"); return PGMI_ENODEV; }
    PGMI_HIP(hipSetDevice(device));
    std::vector<void*> pool;
    auto cleanup = [&]() { for (void* p : pool) hipFree(p); };
    float *dh = nullptr, *dE = nullptr, *db = nullptr, *dfull = nullptr, *dgroup = nullptr;
    int32_t* dflag = nullptr;
    const size_t n_full = (size_t)rows * V, n_group = (size_t)rows * groups;
    if ((rc = dev_upload(pool, &dh, h, (size_t)rows * D)) || (rc = dev_upload(pool, &dE, E, (size_t)V * D)) ||
        (rc = dev_upload(pool, &db, bias, (size_t)V)) || (full && (rc = out_alloc(pool, &dfull, n_full))) ||
        (group && (rc = out_alloc(pool, &dgroup, n_group))) || (rc = flag_alloc(pool, &dflag))) {
        cleanup();
        return rc;
    }
    rc = launch_group_logsoftmax(dh, dE, db, rows, D, V, first, groups, width, dfull, dgroup, dflag, nullptr);
    if (!rc) rc = op_finish(hipDeviceSynchronize(), "grouped log-softmax");
    if (!rc && full) rc = out_fetch(dfull, n_full, full, "grouped log-softmax");
    if (!rc && group) rc = out_fetch(dgroup, n_group, group, "grouped log-softmax");
    if (!rc) rc = op_finish(hipMemcpy(nonfinite, dflag, 4, hipMemcpyDeviceToHost), "grouped log-softmax");
    cleanup();
    return rc;
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
    if (pgmi_device_count() <= 0) { set_error("no HIP device visible"); return PGMI_ENODEV; }
    PGMI_HIP(hipSetDevice(device));
    std::vector<void*> pool;
    auto cleanup = [&]() { for (void* p : pool) hipFree(p); };
    float *dlp = nullptr, *dprior = nullptr, *deve = nullptr, *dout = nullptr;
    int32_t *dtok = nullptr, *dlens = nullptr, *doff = nullptr, *dp = nullptr, *droot = nullptr, *da0 = nullptr, *drow0 = nullptr, *dn = nullptr, *dflip = nullptr;
    const size_t nB = (size_t)B;
    int rc = 0;
    if ((rc = dev_upload(pool, &dlp, lp, (size_t)n_lp_rows * V)) || (rc = dev_upload(pool, &dtok, tokens, (size_t)n_lp_rows)) ||
        (lens && (rc = dev_upload(pool, &dlens, lens, nB))) ||
        (!lens && ((rc = dev_upload(pool, &doff, seq_off, nB)) || (rc = dev_upload(pool, &dp, seq_p, nB)) || (rc = dev_upload(pool, &droot, seq_root, nB)))) ||
        (prior && ((rc = dev_upload(pool, &dprior, prior, (size_t)n_prior_rows * V)) || (rc = dev_upload(pool, &da0, a0, nB)) ||
                   (rc = dev_upload(pool, &drow0, row0, nB)) || (rc = dev_upload(pool, &dn, n, nB)) || (rc = dev_upload(pool, &dflip, flip, nB)))) ||
        (eve && (rc = dev_upload(pool, &deve, eve, (size_t)n_prior_rows * V))) || (rc = out_alloc(pool, &dout, nB))) {
        cleanup();
        return rc;
    }
    if (lens) launch_seq_loglik(dlp, dtok, dlens, B, T, V, dprior, da0, drow0, dn, dflip, alpha, deve, beta, eve_fallback, dout, nullptr);
    else launch_seq_loglik_ragged(dlp, dtok, doff, dp, droot, B, T, V, dprior, da0, drow0, dn, dflip, alpha, deve, beta, eve_fallback, dout, nullptr);
    rc = op_finish(hipDeviceSynchronize(), "sequence sum");
    if (!rc) rc = out_fetch(dout, nB, out, "sequence sum");
    cleanup();
    return rc;
}


}  // extern "C"
