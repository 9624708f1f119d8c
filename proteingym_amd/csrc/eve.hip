// EVE / DeepSequence Bayesian-VAE scoring kernels (proteingym/baselines/EVE/EVE/VAE_model.py:165-181, VAE_decoder.py:112-167,
// VAE_encoder.py:69-88).  One Monte-Carlo sample j of the ELBO is: noise -> sampled decoder weights (once per sample, shared by every
// row of the assay) -> per-row latent + dropout -> hidden layers -> logits -> per-row BCE + KLD.  The GEMMs are the fp32 launcher
// (gemm_f32.hip); everything around them lives here:
//   eve_gather_kernel        encoder layer 0 as a gather over the one-hot's non-zeros (residues uint8 [M][L], 255 = no letter)
//   eve_act_kernel           activation (+ dropout with the 1/(1-p) scale) in place on a GEMM's rows
//   eve_latent_kernel        z = exp(lv / 2) eps + mu, dropout, zero K padding
//   eve_sample_kernel        W = sd eps + mean into a zero-padded [Np][Kp] GEMM operand (hidden weights, every bias, temperature)
//   eve_sample_final_kernel  W_final: sampled W_out contracted with the sampled conv weight in registers, sparsity gate, and the
//                            reference's flat views ([C L, H] read as [L H, C]; [L H, 20] read as [H, L, 20] and as [20 L, H])
//   eve_elbo_kernel          per row: 20-way log-sum-exp per position, BCE-with-logits of the log-probabilities, KLD, fp64 sums
//   eve_fill_*_kernel        the generator's noise as tensors (pgmi_eve_noise_fill)
//   eve_prior_*_kernel       the log-prior of ONE row over many samples (pgmi_eve_log_prior): latent, sampled hidden layers as
//                            matrix-vector products, the final layer fused with its sampler (W_final never exists in memory), and the
//                            log-softmax with its fp64 accumulators; up to EVE_PRIOR_S samples per launch share one read of the means
//                            and standard deviations
// Noise: counter-based Philox4x32-10.  key = seed; counter = (element / 4 low, element / 4 high, sample j, tensor id); the four
// outputs of a counter serve elements 4 b .. 4 b + 3 of the tensor: normals by Box-Muller in fp32 (outputs 0,1 -> elements 0,1;
// outputs 2,3 -> elements 2,3), dropout keeps by output < (1 - p) 2^24 on the top 24 bits.  Per-row tensors are indexed by the row's
// GLOBAL index in the assay, so a row's draw does not depend on the launch or chunk it is in.  Every kernel takes its noise either from
// the generator or from an injected tensor (same arithmetic after the draw: the two give the same bits for the same noise).
// Compiled with -ffp-contract=off (build_native.py): the draw and its use round the same way at every call site.
#include "common.h"

namespace pgmi {

struct EveRng {
    uint32_t k0, k1, sample;
};

__device__ __forceinline__ void philox4x32_10(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t out[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

__device__ __forceinline__ void eve_bits4(const EveRng& g, int tensor, uint64_t block, uint32_t out[4]) {
    philox4x32_10(g.k0, g.k1, (uint32_t)block, (uint32_t)(block >> 32), g.sample, (uint32_t)tensor, out);
}

// Box-Muller: u1 in (0, 1) and u2 in [0, 1) from the top 24 bits, exact in fp32
__device__ __forceinline__ void box_muller(uint32_t a, uint32_t b, float& n0, float& n1) {
    const float u1 = ((float)(a >> 8) + 0.5f) * 5.9604644775390625e-08f;
    const float u2 = (float)(b >> 8) * 5.9604644775390625e-08f;
    const float r = sqrtf(-2.0f * logf(u1));
    float s, c;
    sincosf(6.283185307179586f * u2, &s, &c);
    n0 = r * c;
    n1 = r * s;
}

__device__ __forceinline__ void eve_normal4(const EveRng& g, int tensor, uint64_t block, float n[4]) {
    uint32_t b[4];
    eve_bits4(g, tensor, block, b);
    box_muller(b[0], b[1], n[0], n[1]);
    box_muller(b[2], b[3], n[2], n[3]);
}

__device__ __forceinline__ float eve_normal(const EveRng& g, int tensor, uint64_t e) {
    float n[4];
    eve_normal4(g, tensor, e >> 2, n);
    const int i = (int)(e & 3);
    return i == 0 ? n[0] : i == 1 ? n[1] : i == 2 ? n[2] : n[3];
}

__device__ __forceinline__ bool eve_keep(const EveRng& g, int tensor, uint64_t e, uint32_t keep24) {
    uint32_t b[4];
    eve_bits4(g, tensor, e >> 2, b);
    const int i = (int)(e & 3);
    const uint32_t x = i == 0 ? b[0] : i == 1 ? b[1] : i == 2 ? b[2] : b[3];
    return (x >> 8) < keep24;
}

__device__ __forceinline__ float eve_act(float x, int act) {
    switch (act) {
        case PGMI_EVE_ACT_RELU: return x > 0.0f ? x : 0.0f;
        case PGMI_EVE_ACT_TANH: return tanhf(x);
        case PGMI_EVE_ACT_SIGMOID: return 1.0f / (1.0f + expf(-x));
        case PGMI_EVE_ACT_ELU: return x > 0.0f ? x : expm1f(x);
        default: return x;
    }
}

// ---- encoder layer 0 ------------------------------------------------------------------------------------------------------------
// out[m][n] = act(b[n] + sum_l W0t[20 l + res[m][l]][n]); W0t [20 L][ld] is the transposed first-layer weight, columns >= N zero.
// One block per row; the residues sit in LDS, a thread owns columns n = tid, tid + 256, ...; positions are added in order.
__global__ __launch_bounds__(256) void eve_gather_kernel(const uint8_t* __restrict__ res, const float* __restrict__ W0t,
                                                         const float* __restrict__ b, int L, int A, int ld, int act, float* __restrict__ out) {
    extern __shared__ int eve_cols[];
    const int m = blockIdx.x;
    for (int l = threadIdx.x; l < L; l += blockDim.x) {
        const int r = res[(size_t)m * L + l];
        eve_cols[l] = r < A ? l * A + r : -1;
    }
    __syncthreads();
    for (int n = threadIdx.x; n < ld; n += blockDim.x) {
        float acc = b[n];
        for (int l = 0; l < L; ++l) {
            const int c = eve_cols[l];
            if (c >= 0) acc += W0t[(size_t)c * ld + n];
        }
        out[(size_t)m * ld + n] = eve_act(acc, act);
    }
}

// ---- activation + dropout, in place ---------------------------------------------------------------------------------------------
// x [rows][ld]; columns < n: x = keep ? act(x) * scale : 0 (keep24 == 0: no dropout).  Generator element: (row_base + r) * n + c of
// `tensor`; injected keep [.][n] is indexed by the call's local row inj_row0 + r.
__global__ __launch_bounds__(256) void eve_act_kernel(float* __restrict__ x, int rows, int n, int ld, int act, uint32_t keep24, float scale,
                                                      EveRng g, int tensor, int64_t row_base, const uint8_t* __restrict__ inj, int64_t inj_row0) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)rows * n) return;
    const int r = (int)(i / n), c = (int)(i % n);
    float v = eve_act(x[(size_t)r * ld + c], act);
    if (keep24) {
        const bool keep = inj ? inj[(size_t)(inj_row0 + r) * n + c] != 0 : eve_keep(g, tensor, (uint64_t)(row_base + r) * n + c, keep24);
        v = keep ? v * scale : 0.0f;
    }
    x[(size_t)r * ld + c] = v;
}

// ---- latent ---------------------------------------------------------------------------------------------------------------------
// mulv [.][ldz]: mu in columns [0, z), log_var in [z, 2 z) of row mulv_row0 + r.  h [rows][ld]: dropout(exp(lv / 2) eps + mu), 0 past z.
__global__ __launch_bounds__(256) void eve_latent_kernel(const float* __restrict__ mulv, int ldz, int64_t mulv_row0, int rows, int z, int ld,
                                                         uint32_t keep24, float scale, EveRng g, int64_t row_base,
                                                         const float* __restrict__ inj_eps, const uint8_t* __restrict__ inj_keep,
                                                         int64_t inj_row0, float* __restrict__ h) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)rows * ld) return;
    const int r = (int)(i / ld), c = (int)(i % ld);
    float v = 0.0f;
    if (c < z) {
        const float* row = mulv + (size_t)(mulv_row0 + r) * ldz;
        const uint64_t e = (uint64_t)(row_base + r) * z + c;
        const float eps = inj_eps ? inj_eps[(size_t)(inj_row0 + r) * z + c] : eve_normal(g, PGMI_EVE_T_Z, e);
        v = expf(0.5f * row[z + c]) * eps + row[c];
        if (keep24) {
            const bool keep = inj_keep ? inj_keep[(size_t)(inj_row0 + r) * z + c] != 0 : eve_keep(g, PGMI_EVE_T_KEEP, e, keep24);
            v = keep ? v * scale : 0.0f;
        }
    }
    h[i] = v;
}

// ---- sampled operand: out[(e / K) * Kp + e % K] = sd[e] * eps[e] + mean[e], e < n ---------------------------------------------------
// One thread per Philox counter (4 elements).  The padding of `out` is zeroed once at creation and never written.
__global__ __launch_bounds__(256) void eve_sample_kernel(const float* __restrict__ mean, const float* __restrict__ sd, int64_t n, int K, int Kp,
                                                         EveRng g, int tensor, const float* __restrict__ inj, float* __restrict__ out) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b * 4 >= n) return;
    float eps[4];
    if (!inj) eve_normal4(g, tensor, (uint64_t)b, eps);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t e = b * 4 + i;
        if (e >= n) break;
        const float ev = inj ? inj[e] : eps[i];
        out[(e / K) * Kp + e % K] = sd[e] * ev + mean[e];
    }
}

// ---- W_final --------------------------------------------------------------------------------------------------------------------
// Thread r < L H owns row r of W_out's flat memory read as [L H][C]: it samples those C values (C % 4 == 0: one counter per 4),
// contracts them with the sampled conv weight (flat [20][C] read as [C][20], in LDS: conv_s[c * 20 + a]) into 20 values in registers
// (CONV false: C == 20 and the values are the output), multiplies by the sparsity gate of (h', l') = (r / L, r % L), and writes flat
// elements f = 20 r + a of the product to W_final[f / H][f % H] (row pitch Hp; pad columns stay zero).
template <bool CONV>
__global__ __launch_bounds__(256) void eve_sample_final_kernel(const float* __restrict__ w_mean, const float* __restrict__ w_sd,
                                                               const float* __restrict__ c_mean, const float* __restrict__ c_sd,
                                                               const float* __restrict__ s_mean, const float* __restrict__ s_sd,
                                                               int L, int H, int Hp, int C, int Ht, EveRng g, const float* __restrict__ inj_w,
                                                               const float* __restrict__ inj_c, const float* __restrict__ inj_s,
                                                               float* __restrict__ out) {
    constexpr int A = 20;
    extern __shared__ float conv_s[];
    if (CONV) {
        for (int i = threadIdx.x; i < A * C; i += blockDim.x) {
            const float ev = inj_c ? inj_c[i] : eve_normal(g, PGMI_EVE_T_CONV, (uint64_t)i);
            conv_s[i] = c_sd[i] * ev + c_mean[i];
        }
        __syncthreads();
    }
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= (int64_t)L * H) return;
    float acc[A];
#pragma unroll
    for (int a = 0; a < A; ++a) acc[a] = 0.0f;
    const int64_t base = r * C;
    if (CONV) {
        for (int c = 0; c < C; c += 4) {
            float eps[4];
            if (inj_w) { const f32x4 t = *reinterpret_cast<const f32x4*>(inj_w + base + c); eps[0] = t[0]; eps[1] = t[1]; eps[2] = t[2]; eps[3] = t[3]; }
            else eve_normal4(g, PGMI_EVE_T_WOUT, (uint64_t)(base + c) >> 2, eps);
            const f32x4 mu = *reinterpret_cast<const f32x4*>(w_mean + base + c);
            const f32x4 sg = *reinterpret_cast<const f32x4*>(w_sd + base + c);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float v = sg[i] * eps[i] + mu[i];
                const float* cv = conv_s + (c + i) * A;
#pragma unroll
                for (int a = 0; a < A; ++a) acc[a] += v * cv[a];
            }
        }
    } else {
#pragma unroll
        for (int c = 0; c < A; c += 4) {
            float eps[4];
            if (inj_w) { const f32x4 t = *reinterpret_cast<const f32x4*>(inj_w + base + c); eps[0] = t[0]; eps[1] = t[1]; eps[2] = t[2]; eps[3] = t[3]; }
            else eve_normal4(g, PGMI_EVE_T_WOUT, (uint64_t)(base + c) >> 2, eps);
            const f32x4 mu = *reinterpret_cast<const f32x4*>(w_mean + base + c);
            const f32x4 sg = *reinterpret_cast<const f32x4*>(w_sd + base + c);
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[c + i] = sg[i] * eps[i] + mu[i];
        }
    }
    if (Ht > 0) {
        const int hq = (int)(r / L), l = (int)(r % L);
        const int64_t e = (int64_t)(hq % Ht) * L + l;
        const float ev = inj_s ? inj_s[e] : eve_normal(g, PGMI_EVE_T_SPARSITY, (uint64_t)e);
        const float gate = 1.0f / (1.0f + expf(-(s_sd[e] * ev + s_mean[e])));
#pragma unroll
        for (int a = 0; a < A; ++a) acc[a] *= gate;
    }
    const int64_t f0 = r * A;
    int64_t n = f0 / H;
    int k = (int)(f0 % H);
#pragma unroll
    for (int a = 0; a < A; ++a) {
        out[n * Hp + k] = acc[a];
        if (++k == H) { k = 0; ++n; }
    }
}

// ---- ELBO of a row --------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// One wave per row of logits [rows][20 L] (read once, 5 x 16 B per position).  Per position: x = t * logit (t = log(1 + exp(temp)) when
// temp != nullptr), lse over the 20 letters, sum_a log1p(exp(x_a - lse)) - (x_target - lse); a residue >= 20 has no target term.  The
// per-lane sums (positions lane, lane + 64, ...) and the KLD terms are added across the wave in double, in a fixed order.
// Row r of the launch is row loc0 + r of the call (res, mulv, elbo / bce / kld, acc).  acc [.][3] doubles: shift, sum of (elbo -
// shift), sum of (elbo - shift)^2; first != 0 sets shift = elbo and zeroes the sums.
__global__ __launch_bounds__(256) void eve_elbo_kernel(const float* __restrict__ logits, const uint8_t* __restrict__ res,
                                                       const float* __restrict__ mulv, int ldz, int z, const float* __restrict__ temp,
                                                       int rows, int L, int64_t loc0, float* __restrict__ elbo, float* __restrict__ bce,
                                                       float* __restrict__ kld, double* __restrict__ acc, int first) {
    constexpr int A = 20;
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int64_t row = loc0 + r;
    const float t = temp ? logf(1.0f + expf(temp[0])) : 1.0f;
    const float* lg = logits + (size_t)r * A * L;
    const uint8_t* rs = res + (size_t)row * L;
    float part = 0.0f;
    for (int l = lane; l < L; l += 64) {
        float x[A];
#pragma unroll
        for (int q = 0; q < A / 4; ++q) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(lg + (size_t)l * A + 4 * q);
            x[4 * q] = v[0]; x[4 * q + 1] = v[1]; x[4 * q + 2] = v[2]; x[4 * q + 3] = v[3];
        }
        if (temp) {
#pragma unroll
            for (int a = 0; a < A; ++a) x[a] *= t;
        }
        float mx = x[0];
#pragma unroll
        for (int a = 1; a < A; ++a) mx = fmaxf(mx, x[a]);
        float se = 0.0f;
#pragma unroll
        for (int a = 0; a < A; ++a) se += expf(x[a] - mx);
        const float lse = mx + logf(se);
        float s = 0.0f;
        const int tgt = rs[l];
#pragma unroll
        for (int a = 0; a < A; ++a) {
            const float lp = x[a] - lse;
            s += log1pf(expf(lp));
            if (a == tgt) s -= lp;
        }
        part += s;
    }
    const float* mv = mulv + (size_t)row * ldz;
    float kp = 0.0f;
    for (int c = lane; c < z; c += 64) {
        const float mu = mv[c], lv = mv[z + c];
        kp += 1.0f + lv - mu * mu - expf(lv);
    }
    const double b = wave_sum((double)part);
    const double k = -0.5 * wave_sum((double)kp);
    if (lane == 0) {
        const float e = (float)-(b + k);
        if (elbo) elbo[row] = e;
        if (bce) bce[row] = (float)b;
        if (kld) kld[row] = (float)k;
        if (acc) {
            double* a3 = acc + (size_t)row * 3;
            if (first) { a3[0] = (double)e; a3[1] = 0.0; a3[2] = 0.0; }
            else { const double d = (double)e - a3[0]; a3[1] += d; a3[2] += d * d; }
        }
    }
}

// ---- log-prior of one row (pgmi_eve_log_prior) ------------------------------------------------------------------------------------
// A launch serves S <= EVE_PRIOR_S consecutive samples: sample s of the launch draws with the counter's sample word g.sample + s (the
// words pgmi_eve_elbo(row_base = 0, sample) uses), or reads the injected tensor inj.p[s].  No dropout: the reference's model is in eval().
// Every sum below has one order, set by the shapes alone: a sample's bits do not depend on S or on its place in the launch.
static __device__ __forceinline__ EveRng eve_rng_plus(EveRng g, int s) { g.sample += (uint32_t)s; return g; }

// h[s][c] = exp(lv / 2) eps + mu for c < z (row 0 of mulv), 0 up to ld
__global__ __launch_bounds__(256) void eve_prior_latent_kernel(const float* __restrict__ mulv, int z, int ld, EveRng g, EvePriorPtrs inj, int S,
                                                               float* __restrict__ h) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S * ld) return;
    const int s = i / ld, c = i % ld;
    float v = 0.0f;
    if (c < z) {
        const float eps = inj.p[s] ? inj.p[s][c] : eve_normal(eve_rng_plus(g, s), PGMI_EVE_T_Z, (uint64_t)c);
        v = expf(0.5f * mulv[z + c]) * eps + mulv[c];
    }
    h[i] = v;
}

// y[s][n] = act(sum_k (sd eps + mean)[n][k] x[s][k] + (sd eps + mean)[n]): one wave per output n, grid (ceil(N / 4), S).  A lane owns
// the Philox counters b_lo + lane, b_lo + lane + 64, ... of the row's elements [n K, (n + 1) K) (a counter's elements outside the row
// belong to its neighbours) and adds its terms in that order; the 64 lane sums go through one xor butterfly.
__global__ __launch_bounds__(256) void eve_prior_hidden_kernel(const float* __restrict__ w_mean, const float* __restrict__ w_sd,
                                                               const float* __restrict__ b_mean, const float* __restrict__ b_sd, int N, int K,
                                                               EveRng g, int tw, int tb, EvePriorPtrs inj_w, EvePriorPtrs inj_b,
                                                               const float* __restrict__ x, int ldx, int act, float* __restrict__ y, int ldy) {
    const int lane = threadIdx.x & 63, s = blockIdx.y;
    const int n = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (n >= N) return;
    const EveRng gs = eve_rng_plus(g, s);
    const float* iw = inj_w.p[s];
    const float* xs = x + (size_t)s * ldx;
    const int64_t e0 = (int64_t)n * K, e1 = e0 + K;
    float part = 0.0f;
    for (int64_t b = (e0 >> 2) + lane; b <= ((e1 - 1) >> 2); b += 64) {
        float eps[4];
        if (!iw) eve_normal4(gs, tw, (uint64_t)b, eps);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t e = b * 4 + i;
            if (e >= e0 && e < e1) {
                const float ev = iw ? iw[e] : eps[i];
                part += (w_sd[e] * ev + w_mean[e]) * xs[e - e0];
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
    if (lane == 0) {
        const float ev = inj_b.p[s] ? inj_b.p[s][n] : eve_normal(gs, tb, (uint64_t)n);
        y[(size_t)s * ldy + n] = eve_act(part + (b_sd[n] * ev + b_mean[n]), act);
    }
}

// The final layer of one row, fused with its sampler.  Thread t < 256 of sample group gi (threads 256 gi + t; samples S gi .. S gi + S - 1
// of the launch's ns) owns row r = 256 block + t < L H of W_out's flat [L H][C] view exactly as in eve_sample_final_kernel (same draws,
// same contraction, same gate).  The groups of a block walk the same rows' means and standard deviations together, so one read from
// memory serves the launch's samples; each sample has its own conv weight (LDS), gate and hidden vector h[s].  The 20 values are flat
// elements f = 20 r + a of W_final read as [20 L][H]: they meet h[s][f % H] and belong to logit f / H.  With H >= 20 a thread's
// elements touch at most two logits: s0 sums those of logit (20 r) / H, s1 those after the wrap.  Per block (256 rows = 5120 flat
// elements) and logit n, one wave adds the threads' sums of [max(n H, F0), min((n + 1) H, F1)) -- lane i takes threads t_lo + i, + 64,
// ... in order, then one xor butterfly -- into partial[s][block][n - n0], n0 = F0 / H: a logit whose terms straddle blocks is
// finished, in block order, by eve_prior_finish_kernel.  No atomics.
template <bool CONV, int S>
__global__ __launch_bounds__(512) void eve_prior_final_kernel(const float* __restrict__ w_mean, const float* __restrict__ w_sd,
                                                              const float* __restrict__ c_mean, const float* __restrict__ c_sd,
                                                              const float* __restrict__ s_mean, const float* __restrict__ s_sd, int L, int H,
                                                              int C, int Ht, EveRng g, EvePriorPtrs inj_w, EvePriorPtrs inj_c,
                                                              EvePriorPtrs inj_s, int ns, const float* __restrict__ h, int ldh,
                                                              float* __restrict__ partial, int kmax) {
    constexpr int A = 20;
    extern __shared__ float prior_lds[];
    float* conv_s = prior_lds;                                  // [ns][C][20] (CONV)
    float* red = prior_lds + (CONV ? ns * A * C : 0);           // [ns][256][2]
    const int tid = threadIdx.x & 255, sb = (threadIdx.x >> 8) * S;
    if (CONV) {
        for (int i = threadIdx.x; i < ns * A * C; i += blockDim.x) {
            const int s = i / (A * C), e = i % (A * C);
            const float ev = inj_c.p[s] ? inj_c.p[s][e] : eve_normal(eve_rng_plus(g, s), PGMI_EVE_T_CONV, (uint64_t)e);
            conv_s[i] = c_sd[e] * ev + c_mean[e];
        }
        __syncthreads();
    }
    const int64_t LH = (int64_t)L * H, rb = (int64_t)blockIdx.x * 256, r = rb + tid;
    float s0[S], s1[S];
#pragma unroll
    for (int s = 0; s < S; ++s) s0[s] = s1[s] = 0.0f;
    if (r < LH) {
        float acc[S][A];
#pragma unroll
        for (int s = 0; s < S; ++s)
#pragma unroll
            for (int a = 0; a < A; ++a) acc[s][a] = 0.0f;
        const int64_t base = r * C;
        if (CONV) {
            // the next counter's mean / sd are in flight while this one's draws are computed
            f32x4 mu = *reinterpret_cast<const f32x4*>(w_mean + base), sg = *reinterpret_cast<const f32x4*>(w_sd + base);
            for (int c = 0; c < C; c += 4) {
                const int cn = c + 4 < C ? c + 4 : c;
                const f32x4 mu_n = *reinterpret_cast<const f32x4*>(w_mean + base + cn);
                const f32x4 sg_n = *reinterpret_cast<const f32x4*>(w_sd + base + cn);
#pragma unroll
                for (int s = 0; s < S; ++s) {
                    if (sb + s >= ns) continue;
                    const float* iw = inj_w.p[sb + s];
                    float eps[4];
                    if (iw) { const f32x4 t = *reinterpret_cast<const f32x4*>(iw + base + c); eps[0] = t[0]; eps[1] = t[1]; eps[2] = t[2]; eps[3] = t[3]; }
                    else eve_normal4(eve_rng_plus(g, sb + s), PGMI_EVE_T_WOUT, (uint64_t)(base + c) >> 2, eps);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float v = sg[i] * eps[i] + mu[i];
                        const float* cv = conv_s + (sb + s) * A * C + (c + i) * A;
#pragma unroll
                        for (int a = 0; a < A; ++a) acc[s][a] += v * cv[a];
                    }
                }
                mu = mu_n; sg = sg_n;
            }
        } else {
#pragma unroll
            for (int c = 0; c < A; c += 4) {
                const f32x4 mu = *reinterpret_cast<const f32x4*>(w_mean + base + c);
                const f32x4 sg = *reinterpret_cast<const f32x4*>(w_sd + base + c);
#pragma unroll
                for (int s = 0; s < S; ++s) {
                    if (sb + s >= ns) continue;
                    const float* iw = inj_w.p[sb + s];
                    float eps[4];
                    if (iw) { const f32x4 t = *reinterpret_cast<const f32x4*>(iw + base + c); eps[0] = t[0]; eps[1] = t[1]; eps[2] = t[2]; eps[3] = t[3]; }
                    else eve_normal4(eve_rng_plus(g, sb + s), PGMI_EVE_T_WOUT, (uint64_t)(base + c) >> 2, eps);
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[s][c + i] = sg[i] * eps[i] + mu[i];
                }
            }
        }
        if (Ht > 0) {
            const int hq = (int)(r / L), l = (int)(r % L);
            const int64_t e = (int64_t)(hq % Ht) * L + l;
            const float sm = s_mean[e], ss = s_sd[e];
#pragma unroll
            for (int s = 0; s < S; ++s) {
                if (sb + s >= ns) continue;
                const float ev = inj_s.p[sb + s] ? inj_s.p[sb + s][e] : eve_normal(eve_rng_plus(g, sb + s), PGMI_EVE_T_SPARSITY, (uint64_t)e);
                const float gate = 1.0f / (1.0f + expf(-(ss * ev + sm)));
#pragma unroll
                for (int a = 0; a < A; ++a) acc[s][a] *= gate;
            }
        }
        const int k0 = (int)((r * A) % H);
#pragma unroll
        for (int s = 0; s < S; ++s) {
            if (sb + s >= ns) continue;
            const float* hs = h + (size_t)(sb + s) * ldh;
#pragma unroll
            for (int a = 0; a < A; ++a) {
                const int k = k0 + a;
                const bool wrap = k >= H;
                const float p = acc[s][a] * hs[wrap ? k - H : k];
                if (wrap) s1[s] += p; else s0[s] += p;
            }
        }
    }
#pragma unroll
    for (int s = 0; s < S; ++s) {
        if (sb + s >= ns) continue;
        red[((sb + s) * 256 + tid) * 2] = s0[s];
        red[((sb + s) * 256 + tid) * 2 + 1] = s1[s];
    }
    __syncthreads();
    const int64_t nrows = LH - rb < 256 ? LH - rb : 256;
    const int64_t F0 = rb * A, F1 = F0 + nrows * A, n0 = F0 / H;
    const int cnt = (int)((F1 - 1) / H - n0) + 1;
    const int lane = threadIdx.x & 63;
    for (int q = threadIdx.x >> 6; q < cnt; q += blockDim.x >> 6) {
        const int64_t n = n0 + q;
        const int64_t lo = n * H > F0 ? n * H : F0, hi = ((n + 1) * H < F1 ? (n + 1) * H : F1) - 1;
        const int t_lo = (int)(lo / A - rb), t_hi = (int)(hi / A - rb);
        for (int s = 0; s < ns; ++s) {
            float v = 0.0f;
            for (int t = t_lo + lane; t <= t_hi; t += 64) v += red[(s * 256 + t) * 2 + (((rb + t) * A) / H == n ? 0 : 1)];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
            if (lane == 0) partial[((size_t)s * gridDim.x + blockIdx.x) * kmax + q] = v;
        }
    }
}

// Thread l < L finishes position l for the S samples in order: logit 20 l + a = its blocks' partial sums in block order + the sampled
// bias, times log(1 + exp(temperature)); log-softmax over the 20 letters as in eve_elbo_kernel; acc [20 L][3] doubles: the first
// sample's value, sum and sum of squares of (logp - that), added in sample order (sample0 + s == 0 starts them).
__global__ __launch_bounds__(64) void eve_prior_finish_kernel(const float* __restrict__ partial, int nblocks, int kmax, int S,
                                                              const float* __restrict__ b_mean, const float* __restrict__ b_sd,
                                                              const float* __restrict__ t_mean, const float* __restrict__ t_sd, EveRng g,
                                                              EvePriorPtrs inj_b, EvePriorPtrs inj_t, int L, int H, int sample0,
                                                              double* __restrict__ acc) {
    constexpr int A = 20;
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= L) return;
    for (int s = 0; s < S; ++s) {
        const EveRng gs = eve_rng_plus(g, s);
        float t = 1.0f;
        if (t_mean) {
            const float ev = inj_t.p[s] ? inj_t.p[s][0] : eve_normal(gs, PGMI_EVE_T_TEMP, 0);
            t = logf(1.0f + expf(t_sd[0] * ev + t_mean[0]));
        }
        float x[A];
#pragma unroll
        for (int a = 0; a < A; ++a) {
            const int64_t n = (int64_t)l * A + a;
            const int64_t b_lo = n * H / (256 * A), b_hi = ((n + 1) * H - 1) / (256 * A);
            float sum = 0.0f;
            for (int64_t b = b_lo; b <= b_hi; ++b) sum += partial[((size_t)s * nblocks + b) * kmax + (n - b * (256 * A) / H)];
            const float ev = inj_b.p[s] ? inj_b.p[s][n] : eve_normal(gs, PGMI_EVE_T_BOUT, (uint64_t)n);
            x[a] = sum + (b_sd[n] * ev + b_mean[n]);
            if (t_mean) x[a] *= t;
        }
        float mx = x[0];
#pragma unroll
        for (int a = 1; a < A; ++a) mx = fmaxf(mx, x[a]);
        float se = 0.0f;
#pragma unroll
        for (int a = 0; a < A; ++a) se += expf(x[a] - mx);
        const float lse = mx + logf(se);
#pragma unroll
        for (int a = 0; a < A; ++a) {
            double* a3 = acc + ((size_t)l * A + a) * 3;
            const double lp = (double)(x[a] - lse);
            if (sample0 + s == 0) { a3[0] = lp; a3[1] = 0.0; a3[2] = 0.0; }
            else { const double d = lp - a3[0]; a3[1] += d; a3[2] += d * d; }
        }
    }
}

// ---- the generator's noise as tensors -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void eve_fill_normal_kernel(EveRng g, int tensor, uint64_t e0, int64_t n, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = eve_normal(g, tensor, e0 + (uint64_t)i);
}
__global__ __launch_bounds__(256) void eve_fill_keep_kernel(EveRng g, int tensor, uint64_t e0, int64_t n, uint32_t keep24, uint8_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = eve_keep(g, tensor, e0 + (uint64_t)i, keep24) ? 1 : 0;
}

// ---- launchers --------------------------------------------------------------------------------------------------------------------
static inline unsigned eve_blocks(int64_t n) { return (unsigned)((n + 255) / 256); }

static inline EveRng eve_rng(uint64_t seed, uint32_t sample) { return EveRng{(uint32_t)seed, (uint32_t)(seed >> 32), sample}; }

void launch_eve_gather(const uint8_t* res, const float* W0t, const float* b, int rows, int L, int ld, int act, float* out, hipStream_t s) {
    hipLaunchKernelGGL(eve_gather_kernel, dim3(rows), dim3(256), (size_t)L * sizeof(int), s, res, W0t, b, L, 20, ld, act, out);
}

void launch_eve_act(float* x, int rows, int n, int ld, int act, uint32_t keep24, float scale, uint64_t seed, uint32_t sample, int tensor,
                    int64_t row_base, const uint8_t* inj, int64_t inj_row0, hipStream_t s) {
    hipLaunchKernelGGL(eve_act_kernel, dim3(eve_blocks((int64_t)rows * n)), dim3(256), 0, s, x, rows, n, ld, act, keep24, scale,
                       eve_rng(seed, sample), tensor, row_base, inj, inj_row0);
}

void launch_eve_latent(const float* mulv, int ldz, int64_t mulv_row0, int rows, int z, int ld, uint32_t keep24, float scale, uint64_t seed,
                       uint32_t sample, int64_t row_base, const float* inj_eps, const uint8_t* inj_keep, int64_t inj_row0, float* h,
                       hipStream_t s) {
    hipLaunchKernelGGL(eve_latent_kernel, dim3(eve_blocks((int64_t)rows * ld)), dim3(256), 0, s, mulv, ldz, mulv_row0, rows, z, ld, keep24,
                       scale, eve_rng(seed, sample), row_base, inj_eps, inj_keep, inj_row0, h);
}

void launch_eve_sample(const float* mean, const float* sd, int64_t n, int K, int Kp, uint64_t seed, uint32_t sample, int tensor,
                       const float* inj, float* out, hipStream_t s) {
    hipLaunchKernelGGL(eve_sample_kernel, dim3(eve_blocks((n + 3) / 4)), dim3(256), 0, s, mean, sd, n, K, Kp, eve_rng(seed, sample), tensor,
                       inj, out);
}

void launch_eve_sample_final(const float* w_mean, const float* w_sd, const float* c_mean, const float* c_sd, const float* s_mean,
                             const float* s_sd, int L, int H, int Hp, int C, int Ht, bool conv, uint64_t seed, uint32_t sample,
                             const float* inj_w, const float* inj_c, const float* inj_s, float* out, hipStream_t s) {
    const dim3 grid(eve_blocks((int64_t)L * H)), block(256);
    if (conv)
        hipLaunchKernelGGL(eve_sample_final_kernel<true>, grid, block, (size_t)20 * C * sizeof(float), s, w_mean, w_sd, c_mean, c_sd, s_mean,
                           s_sd, L, H, Hp, C, Ht, eve_rng(seed, sample), inj_w, inj_c, inj_s, out);
    else
        hipLaunchKernelGGL(eve_sample_final_kernel<false>, grid, block, 0, s, w_mean, w_sd, c_mean, c_sd, s_mean, s_sd, L, H, Hp, C, Ht,
                           eve_rng(seed, sample), inj_w, inj_c, inj_s, out);
}

void launch_eve_elbo(const float* logits, const uint8_t* res, const float* mulv, int ldz, int z, const float* temp, int rows, int L,
                     int64_t loc0, float* elbo, float* bce, float* kld, double* acc, int first, hipStream_t s) {
    hipLaunchKernelGGL(eve_elbo_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, logits, res, mulv, ldz, z, temp, rows, L, loc0, elbo, bce, kld,
                       acc, first);
}

void launch_eve_fill_normal(uint64_t seed, uint32_t sample, int tensor, uint64_t e0, int64_t n, float* out, hipStream_t s) {
    if (n > 0) hipLaunchKernelGGL(eve_fill_normal_kernel, dim3(eve_blocks(n)), dim3(256), 0, s, eve_rng(seed, sample), tensor, e0, n, out);
}

void launch_eve_fill_keep(uint64_t seed, uint32_t sample, int tensor, uint64_t e0, int64_t n, uint32_t keep24, uint8_t* out, hipStream_t s) {
    if (n > 0) hipLaunchKernelGGL(eve_fill_keep_kernel, dim3(eve_blocks(n)), dim3(256), 0, s, eve_rng(seed, sample), tensor, e0, n, keep24, out);
}

void launch_eve_prior_latent(const float* mulv, int z, int ld, uint64_t seed, uint32_t sample, const EvePriorPtrs& inj, int S, float* h,
                             hipStream_t s) {
    hipLaunchKernelGGL(eve_prior_latent_kernel, dim3(eve_blocks((int64_t)S * ld)), dim3(256), 0, s, mulv, z, ld, eve_rng(seed, sample), inj, S, h);
}

void launch_eve_prior_hidden(const float* w_mean, const float* w_sd, const float* b_mean, const float* b_sd, int N, int K, uint64_t seed,
                             uint32_t sample, int tw, int tb, const EvePriorPtrs& inj_w, const EvePriorPtrs& inj_b, int S, const float* x,
                             int ldx, int act, float* y, int ldy, hipStream_t s) {
    hipLaunchKernelGGL(eve_prior_hidden_kernel, dim3((N + 3) / 4, S), dim3(256), 0, s, w_mean, w_sd, b_mean, b_sd, N, K, eve_rng(seed, sample),
                       tw, tb, inj_w, inj_b, x, ldx, act, y, ldy);
}

int eve_prior_blocks(int L, int H) { return (int)eve_blocks((int64_t)L * H); }
int eve_prior_kmax(int H) { return (256 * 20 - 1) / H + 2; }
// samples one launch of the final kernel can serve: per sample its conv weight (20 C floats) and its reduction buffer (512 floats)
// take dynamic LDS, kept within 48 KB per block; 0 = none
int eve_prior_max_samples(int C, bool conv) {
    const int fit = conv ? (48 * 1024 / 4) / (20 * C + 512) : EVE_PRIOR_S;
    return fit < EVE_PRIOR_S ? fit : EVE_PRIOR_S;
}

void launch_eve_prior_final(const float* w_mean, const float* w_sd, const float* c_mean, const float* c_sd, const float* s_mean,
                            const float* s_sd, int L, int H, int C, int Ht, bool conv, uint64_t seed, uint32_t sample,
                            const EvePriorPtrs& inj_w, const EvePriorPtrs& inj_c, const EvePriorPtrs& inj_s, int S, const float* h, int ldh,
                            float* partial, hipStream_t s) {
    // 1 or 2 samples: one group of 256 threads; 3 or 4: two groups of two samples (the second sample of the last group may be absent)
    const dim3 grid(eve_prior_blocks(L, H)), block(S > 2 ? 512 : 256);
    const size_t lds = ((conv ? (size_t)S * 20 * C : 0) + (size_t)S * 512) * sizeof(float);
    const EveRng g = eve_rng(seed, sample);
    const int kmax = eve_prior_kmax(H);
#define PGMI_EVE_PRIOR_LAUNCH(CONV, N)                                                                                                   \
    hipLaunchKernelGGL((eve_prior_final_kernel<CONV, N>), grid, block, lds, s, w_mean, w_sd, c_mean, c_sd, s_mean, s_sd, L, H, C, Ht, g, \
                       inj_w, inj_c, inj_s, S, h, ldh, partial, kmax)
    if (conv) { if (S == 1) PGMI_EVE_PRIOR_LAUNCH(true, 1); else PGMI_EVE_PRIOR_LAUNCH(true, 2); }
    else { if (S == 1) PGMI_EVE_PRIOR_LAUNCH(false, 1); else PGMI_EVE_PRIOR_LAUNCH(false, 2); }
#undef PGMI_EVE_PRIOR_LAUNCH
}

void launch_eve_prior_finish(const float* partial, int S, const float* b_mean, const float* b_sd, const float* t_mean, const float* t_sd,
                             uint64_t seed, uint32_t sample, const EvePriorPtrs& inj_b, const EvePriorPtrs& inj_t, int L, int H, int sample0,
                             double* acc, hipStream_t s) {
    hipLaunchKernelGGL(eve_prior_finish_kernel, dim3((L + 63) / 64), dim3(64), 0, s, partial, eve_prior_blocks(L, H), eve_prior_kmax(H), S,
                       b_mean, b_sd, t_mean, t_sd, eve_rng(seed, sample), inj_b, inj_t, L, H, sample0, acc);
}

}  // namespace pgmi
