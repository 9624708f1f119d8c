// ProteinMPNN kernels (include/pgmi.h, ProteinMPNN section).  Hidden width 128 everywhere, fp32 only.
//
// Once per structure (off the hot path, simple kernels; the Linear layers between them are launch_gemm_f32):
//   mpnn_graph_kernel       one workgroup per residue: CA distances to every j with the reference's mask rule (masked pairs pushed to
//                           the row maximum), then the K nearest by (distance ascending, index ascending) through rank counting
//   mpnn_edge_feat_kernel   one workgroup per residue: 25 atom-pair distances (virtual C-beta) x 16 RBFs + the 66-way offset / chain
//                           one-hot as a column pick, Linear(416 -> 128, no bias), LayerNorm
//   mpnn_concat_kernel      [h_V_i | h_E_ik | h_V_j] rows of an encoder layer's two edge MLPs
//   mpnn_edge_sum_kernel    masked sum over a node's K messages / 30 (encoder)
//   mpnn_add_ln_kernel      LayerNorm(a + (b + kb bias) / div) * row mask: every row-local stage of both stacks
// Per batch of mutants (the hot path):
//   mpnn_dec_edge_kernel    one wave per (mutant, node): gathers the hoisted tables into pre = W1 x, GELU, the 128 x 128 GEMM with W2
//                           on v_mfma_f32_16x16x4_f32 (W2 resident in LDS for the block's whole tile loop), GELU, sum over the K rows.
//                           pre and the [B,L,K,128] activations live in registers only.
//   mpnn_head_kernel        W_out, log-softmax over 21, -log p[S] per row
//   mpnn_score_kernel       per mutant: masked mean of the rows' NLL in fp64, fixed order
#include <algorithm>

#include "common.h"

namespace pgmi {

constexpr int MH = 128;             // hidden width
constexpr int MPNN_FEAT = 416;      // 16 positional + 25 x 16 RBF
constexpr int MPNN_EG = 16;         // edges per pass of the feature kernel

__device__ __forceinline__ float mpnn_gelu(float x) { return x * 0.5f * (1.0f + erff(x * 0.70710678118654752440f)); }

// ---- graph ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mpnn_graph_kernel(const float* __restrict__ X, const float* __restrict__ mask, int L, int K,
                                                         int32_t* __restrict__ E_idx, float* __restrict__ D_nb) {
    extern __shared__ float d[];          // [L]
    __shared__ float red[4];
    const int i = blockIdx.x, tid = threadIdx.x;
    const float cx = X[(size_t)i * 12 + 3], cy = X[(size_t)i * 12 + 4], cz = X[(size_t)i * 12 + 5], mi = mask[i];
    float mx = 0.0f;
    for (int j = tid; j < L; j += 256) {
        const float dx = X[(size_t)j * 12 + 3] - cx, dy = X[(size_t)j * 12 + 4] - cy, dz = X[(size_t)j * 12 + 5] - cz;
        const float D = mi * mask[j] * sqrtf(dx * dx + dy * dy + dz * dz + 1e-6f);
        d[j] = D;
        mx = fmaxf(mx, D);
    }
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    if ((tid & 63) == 0) red[tid >> 6] = mx;
    __syncthreads();
    const float dmax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    for (int j = tid; j < L; j += 256) d[j] = d[j] + (1.0f - mi * mask[j]) * dmax;
    __syncthreads();
    // rank of j among the row = entries that come before it in (distance, index) order
    for (int j = tid; j < L; j += 256) {
        const float dj = d[j];
        int cnt = 0;
        for (int t = 0; t < L; ++t) {
            const float dt = d[t];
            cnt += (dt < dj || (dt == dj && t < j)) ? 1 : 0;
        }
        if (cnt < K) {
            E_idx[(size_t)i * K + cnt] = j;
            D_nb[(size_t)i * K + cnt] = dj;
        }
    }
}

// atoms of one residue: N, CA, C, O and the virtual C-beta
__device__ __forceinline__ void mpnn_atoms(const float* __restrict__ x, float a[5][3]) {
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int c = 0; c < 3; ++c) a[t][c] = x[t * 3 + c];
    float b[3], cc[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) { b[c] = a[1][c] - a[0][c]; cc[c] = a[2][c] - a[1][c]; }
    const float n[3] = {b[1] * cc[2] - b[2] * cc[1], b[2] * cc[0] - b[0] * cc[2], b[0] * cc[1] - b[1] * cc[0]};
#pragma unroll
    for (int c = 0; c < 3; ++c) a[4][c] = -0.58273431f * n[c] + 0.56802827f * b[c] - 0.54067466f * cc[c] + a[1][c];
}

// (atom of i, atom of j) of the 25 distance blocks in the reference's order; block 0 is the neighbour distance itself
__constant__ int8_t kPairA[25] = {1, 0, 2, 3, 4, 1, 1, 1, 1, 0, 0, 0, 4, 4, 3, 0, 2, 3, 4, 2, 3, 4, 2, 3, 2};
__constant__ int8_t kPairB[25] = {1, 0, 2, 3, 4, 0, 2, 3, 4, 2, 3, 4, 2, 3, 2, 1, 1, 1, 1, 0, 0, 0, 4, 4, 3};

__global__ __launch_bounds__(256) void mpnn_edge_feat_kernel(const float* __restrict__ X, const int32_t* __restrict__ ridx,
                                                             const int32_t* __restrict__ chain, const int32_t* __restrict__ E_idx,
                                                             const float* __restrict__ D_nb, const float* __restrict__ Wpos,
                                                             const float* __restrict__ bpos, const float* __restrict__ Wt,
                                                             const float* __restrict__ ln_w, const float* __restrict__ ln_b, int L, int K,
                                                             float* __restrict__ E) {
    __shared__ float feat[MPNN_EG][MPNN_FEAT];
    __shared__ float emb[MPNN_EG][MH];
    const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float ai[5][3];
    mpnn_atoms(X + (size_t)i * 12, ai);
    const float step = 20.0f / 15.0f;
    for (int k0 = 0; k0 < K; k0 += MPNN_EG) {
        const int ne = min(MPNN_EG, K - k0);
        {   // positional / chain feature: one (edge, feature) per thread
            const int e = tid >> 4, f = tid & 15;
            if (e < ne) {
                const int j = E_idx[(size_t)i * K + k0 + e];
                const int same = chain[i] == chain[j];
                int dd = ridx[i] - ridx[j] + 32;
                dd = max(0, min(64, dd));
                dd = same ? dd : 65;
                feat[e][f] = Wpos[f * 66 + dd] + bpos[f];
            }
        }
        for (int it = tid; it < MPNN_EG * 25; it += 256) {
            const int e = it / 25, p = it % 25;
            if (e >= ne) continue;
            const int j = E_idx[(size_t)i * K + k0 + e];
            float D;
            if (p == 0) {
                D = D_nb[(size_t)i * K + k0 + e];
            } else {
                float aj[5][3];
                mpnn_atoms(X + (size_t)j * 12, aj);
                const int pa = kPairA[p], pb = kPairB[p];
                float s = 0.0f;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    float va = 0.0f, vb = 0.0f;
#pragma unroll
                    for (int t = 0; t < 5; ++t) { va = (pa == t) ? ai[t][c] : va; vb = (pb == t) ? aj[t][c] : vb; }
                    const float df = va - vb;
                    s += df * df;
                }
                D = sqrtf(s + 1e-6f);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float mu = r < 8 ? 2.0f + step * (float)r : 22.0f - step * (float)(15 - r);
                const float z = (D - mu) / 1.25f;
                feat[e][16 + p * 16 + r] = expf(-(z * z));
            }
        }
        __syncthreads();
        {   // Linear(416 -> 128): thread (column c, half h) serves edges 8 h .. 8 h + 7
            const int c = tid & 127, h = tid >> 7;
            float acc[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] = 0.0f;
            for (int f = 0; f < MPNN_FEAT; ++f) {
                const float w = Wt[(size_t)f * MH + c];
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] = fmaf(w, feat[h * 8 + e][f], acc[e]);
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) emb[h * 8 + e][c] = acc[e];
        }
        __syncthreads();
        for (int e = wave; e < ne; e += 4) {   // LayerNorm: one wave per edge, two columns per lane
            const float x0 = emb[e][lane], x1 = emb[e][lane + 64];
            float s = x0 + x1;
            for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
            const float mean = s * (1.0f / MH);
            const float d0 = x0 - mean, d1 = x1 - mean;
            float v = d0 * d0 + d1 * d1;
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
            const float rstd = 1.0f / sqrtf(v * (1.0f / MH) + 1e-5f);
            float* dst = E + ((size_t)i * K + k0 + e) * MH;
            dst[lane] = d0 * rstd * ln_w[lane] + ln_b[lane];
            dst[lane + 64] = d1 * rstd * ln_w[lane + 64] + ln_b[lane + 64];
        }
        __syncthreads();
    }
}

// ---- encoder helpers -----------------------------------------------------------------------------------------------------------
__global__ void mpnn_concat_kernel(const float* __restrict__ hV, const float* __restrict__ hE, const int32_t* __restrict__ E_idx,
                                   int64_t n_edges, int K, float* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;      // one float4 each: 96 per edge
    if (t >= n_edges * 96) return;
    const int64_t e = t / 96;
    const int c4 = (int)(t % 96);
    const int blk = c4 >> 5, c = (c4 & 31) * 4;
    const float* src = blk == 0 ? hV + (e / K) * MH : blk == 1 ? hE + e * MH : hV + (int64_t)E_idx[e] * MH;
    *reinterpret_cast<f32x4*>(out + e * 384 + blk * MH + c) = *reinterpret_cast<const f32x4*>(src + c);
}

__global__ void mpnn_edge_sum_kernel(const float* __restrict__ msg, const float* __restrict__ mask, const int32_t* __restrict__ E_idx,
                                     int L, int K, float* __restrict__ out) {
    const int i = blockIdx.x, c = threadIdx.x;     // 128 threads
    const float mi = mask[i];
    float s = 0.0f;
    for (int k = 0; k < K; ++k) s += mi * mask[E_idx[(size_t)i * K + k]] * msg[((size_t)i * K + k) * MH + c];
    out[(size_t)i * MH + c] = s / 30.0f;
}

// out[r] = LayerNorm(a[r % a_rows] + (b[r] + kb * bias) / div) * rowmask[r % L]; b, bias, rowmask nullable.  One wave per row.
__global__ __launch_bounds__(256) void mpnn_add_ln_kernel(const float* __restrict__ a, int64_t a_rows, const float* __restrict__ b,
                                                          const float* __restrict__ bias, float kb, float div,
                                                          const float* __restrict__ ln_w, const float* __restrict__ ln_b,
                                                          const float* __restrict__ rowmask, int L, int64_t rows, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const float* ar = a + (r % a_rows) * MH;
    float x0 = ar[lane], x1 = ar[lane + 64];
    if (b) {
        float y0 = b[r * MH + lane], y1 = b[r * MH + lane + 64];
        if (bias) { y0 += kb * bias[lane]; y1 += kb * bias[lane + 64]; }
        x0 += y0 / div;
        x1 += y1 / div;
    }
    float s = x0 + x1;
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    const float mean = s * (1.0f / MH);
    const float d0 = x0 - mean, d1 = x1 - mean;
    float v = d0 * d0 + d1 * d1;
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    const float rstd = 1.0f / sqrtf(v * (1.0f / MH) + 1e-5f);
    const float m = rowmask ? rowmask[r % L] : 1.0f;
    out[r * MH + lane] = (d0 * rstd * ln_w[lane] + ln_b[lane]) * m;
    out[r * MH + lane + 64] = (d1 * rstd * ln_w[lane + 64] + ln_b[lane + 64]) * m;
}

// ---- decoder edge kernel -------------------------------------------------------------------------------------------------------
// W2 in LDS, [n][128] with the 16-byte slots of a row XOR-swizzled by n & 15: the 16 lanes of a ds_read_b128 group read 16 rows at
// the same logical slot, which land in 16 different bank slots.
__device__ __forceinline__ int w2_off(int n, int slot) { return n * MH + ((slot ^ (n & 15)) << 2); }

// One wave per (mutant b, node i); RT = 16-row MFMA tiles that cover the node's K edges.  Lane (r = lane & 15, g = lane >> 4) owns
// edge rows 16 rt + r as the A operand; k step (q, e) of the MFMA is input channel 16 q + 4 g + e for both operands, so a lane reads
// its gathers and its W2 fragment as float4.  C layout: column lane & 15, row 4 g + v.
template <int RT>
__global__ __launch_bounds__(256, 2) void mpnn_dec_edge_kernel(const float* __restrict__ Ep, const float* __restrict__ T,
                                                               const float* __restrict__ Penc, const float* __restrict__ AP,
                                                               int64_t ap_bstride, const float* __restrict__ W2,
                                                               const float* __restrict__ b2, const int32_t* __restrict__ E_idx,
                                                               const float* __restrict__ mask, const uint8_t* __restrict__ S,
                                                               const int32_t* __restrict__ rank, int B, int L, int K,
                                                               float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float w2s[MH * MH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, g = lane >> 4;
    for (int f = tid; f < MH * 32; f += 256) {
        const int n = f >> 5, slot = f & 31;
        *reinterpret_cast<f32x4*>(w2s + w2_off(n, slot)) = *reinterpret_cast<const f32x4*>(W2 + n * MH + slot * 4);
    }
    __syncthreads();
    const int tiles_per_b = (L + 3) >> 2;
    const int64_t total = (int64_t)B * tiles_per_b;
    for (int64_t tile = blockIdx.x; tile < total; tile += gridDim.x) {
        const int b = (int)(tile / tiles_per_b);
        const int i = (int)(tile % tiles_per_b) * 4 + wave;
        if (i >= L) continue;                                   // wave-uniform; no barrier inside the tile loop
        const float mi = mask[i];
        const int ri = rank[(size_t)b * L + i];
        const float* ap = AP + (size_t)b * ap_bstride;
        const float* arow = ap + (size_t)i * 256;
        const float *ep[RT], *p1[RT], *p2[RT];
        bool valid[RT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            const int k = rt * 16 + r;
            const int kc = min(k, K - 1);
            const int j = E_idx[(size_t)i * K + kc];
            const bool bw = mi != 0.0f && ri > rank[(size_t)b * L + j];
            ep[rt] = Ep + ((size_t)i * K + kc) * MH;
            p1[rt] = bw ? ap + (size_t)j * 256 + MH : Penc + (size_t)j * MH;
            p2[rt] = T + (bw ? (int)S[(size_t)b * L + j] : 21) * MH;
            valid[rt] = k < K;
        }
        f32x4 acc[RT][8];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int ct = 0; ct < 8; ++ct) acc[rt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
        for (int q = 0; q < 8; ++q) {
            const int c0 = 16 * q + 4 * g;
            const f32x4 av = *reinterpret_cast<const f32x4*>(arow + c0);
            f32x4 a[RT];
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                const f32x4 x = *reinterpret_cast<const f32x4*>(ep[rt] + c0) +
                                (*reinterpret_cast<const f32x4*>(p2[rt] + c0) + *reinterpret_cast<const f32x4*>(p1[rt] + c0));
#pragma unroll
                for (int e = 0; e < 4; ++e) a[rt][e] = valid[rt] ? mpnn_gelu(av[e] + mi * x[e]) : 0.0f;
            }
            f32x4 bf[8];
#pragma unroll
            for (int ct = 0; ct < 8; ++ct) bf[ct] = *reinterpret_cast<const f32x4*>(w2s + w2_off(ct * 16 + r, 4 * q + g));
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                    for (int ct = 0; ct < 8; ++ct)
                        acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[rt][e], bf[ct][e], acc[rt][ct], 0, 0, 0);
        }
        float* dst = out + ((size_t)b * L + i) * MH;
#pragma unroll
        for (int ct = 0; ct < 8; ++ct) {
            const float bias = b2[ct * 16 + r];
            float s = 0.0f;
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int v = 0; v < 4; ++v)
                    if (rt * 16 + 4 * g + v < K) s += mpnn_gelu(acc[rt][ct][v] + bias);
            s += __shfl_xor(s, 16);
            s += __shfl_xor(s, 32);
            if (g == 0) dst[ct * 16 + r] = s;
        }
    }
}

// ---- head ----------------------------------------------------------------------------------------------------------------------
// one wave per row: logits over 21 letters, log-softmax; lp [rows][21] (nullable), nll[r] = -log p[S[r]]
__global__ __launch_bounds__(256) void mpnn_head_kernel(const float* __restrict__ h, const float* __restrict__ W, const float* __restrict__ bias,
                                                        const uint8_t* __restrict__ S, int64_t rows, float* __restrict__ lp,
                                                        float* __restrict__ nll) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const float h0 = h[r * MH + 2 * lane], h1 = h[r * MH + 2 * lane + 1];
    float logit = -INFINITY;
    for (int c = 0; c < 21; ++c) {
        float p = h0 * W[c * MH + 2 * lane] + h1 * W[c * MH + 2 * lane + 1];
        for (int o = 32; o > 0; o >>= 1) p += __shfl_xor(p, o);
        if (lane == c) logit = p + bias[c];
    }
    float mx = logit;
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    float ex = lane < 21 ? expf(logit - mx) : 0.0f;
    for (int o = 32; o > 0; o >>= 1) ex += __shfl_xor(ex, o);
    const float v = logit - mx - logf(ex);
    if (lp && lane < 21) lp[r * 21 + lane] = v;
    const float picked = __shfl(v, (int)S[r]);
    if (nll && lane == 0) nll[r] = -picked;
}

// out[b] = -(sum_i mask_i nll[b, i]) / (sum_i mask_i), fp64, one wave per mutant, lane-strided then butterfly: a fixed order
__global__ __launch_bounds__(64) void mpnn_score_kernel(const float* __restrict__ nll, const float* __restrict__ mask, int L,
                                                        double* __restrict__ out) {
    const int b = blockIdx.x, lane = threadIdx.x;
    double s = 0.0, n = 0.0;
    for (int i = lane; i < L; i += 64) {
        const double m = (double)mask[i];
        s += m * (double)nll[(size_t)b * L + i];
        n += m;
    }
    for (int o = 32; o > 0; o >>= 1) { s += __shfl_xor(s, o); n += __shfl_xor(n, o); }
    if (lane == 0) out[b] = -(s / n);
}

// ---- launchers -----------------------------------------------------------------------------------------------------------------
void launch_mpnn_graph(const float* X, const float* mask, int L, int K, int32_t* E_idx, float* D_nb, hipStream_t s) {
    hipLaunchKernelGGL(mpnn_graph_kernel, dim3(L), dim3(256), (size_t)L * sizeof(float), s, X, mask, L, K, E_idx, D_nb);
}

void launch_mpnn_edge_feat(const float* X, const int32_t* ridx, const int32_t* chain, const int32_t* E_idx, const float* D_nb,
                           const float* Wpos, const float* bpos, const float* Wt, const float* ln_w, const float* ln_b, int L, int K, float* E,
                           hipStream_t s) {
    hipLaunchKernelGGL(mpnn_edge_feat_kernel, dim3(L), dim3(256), 0, s, X, ridx, chain, E_idx, D_nb, Wpos, bpos, Wt, ln_w, ln_b, L, K, E);
}

void launch_mpnn_concat(const float* hV, const float* hE, const int32_t* E_idx, int L, int K, float* out, hipStream_t s) {
    const int64_t n = (int64_t)L * K * 96;
    hipLaunchKernelGGL(mpnn_concat_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, hV, hE, E_idx, (int64_t)L * K, K, out);
}

void launch_mpnn_edge_sum(const float* msg, const float* mask, const int32_t* E_idx, int L, int K, float* out, hipStream_t s) {
    hipLaunchKernelGGL(mpnn_edge_sum_kernel, dim3(L), dim3(MH), 0, s, msg, mask, E_idx, L, K, out);
}

void launch_mpnn_add_ln(const float* a, int64_t a_rows, const float* b, const float* bias, float kb, float div, const float* ln_w,
                        const float* ln_b, const float* rowmask, int L, int64_t rows, float* out, hipStream_t s) {
    hipLaunchKernelGGL(mpnn_add_ln_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, a, a_rows, b, bias, kb, div, ln_w, ln_b,
                       rowmask, L, rows, out);
}

int launch_mpnn_dec_edge(const float* Ep, const float* T, const float* Penc, const float* AP, int64_t ap_bstride, const float* W2,
                         const float* b2, const int32_t* E_idx, const float* mask, const uint8_t* S, const int32_t* rank, int B, int L, int K,
                         float* out, hipStream_t s) {
    // three row tiles are what fits: <3> uses all 256 VGPRs of two waves per SIMD, a fourth tile (K up to 64) would spill to scratch
    if (K < 1 || K > 48 || K > L) { set_error("mpnn: K = %d neighbours outside 1 .. min(48, L)", K); return PGMI_EINVAL; }
    const int64_t total = (int64_t)B * ((L + 3) / 4);
    const dim3 grid((unsigned)std::min<int64_t>(total, 512)), block(256);
#define MPNN_EDGE(RT_) hipLaunchKernelGGL((mpnn_dec_edge_kernel<RT_>), grid, block, 0, s, Ep, T, Penc, AP, ap_bstride, W2, b2, E_idx, mask, S, rank, B, L, K, out)
    switch ((K + 15) / 16) {
        case 1: MPNN_EDGE(1); break;
        case 2: MPNN_EDGE(2); break;
        default: MPNN_EDGE(3); break;
    }
#undef MPNN_EDGE
    PGMI_HIP(hipGetLastError());
    return PGMI_OK;
}

void launch_mpnn_head(const float* h, const float* W, const float* bias, const uint8_t* S, int64_t rows, float* lp, float* nll,
                      hipStream_t s) {
    hipLaunchKernelGGL(mpnn_head_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, h, W, bias, S, rows, lp, nll);
}

void launch_mpnn_score(const float* nll, const float* mask, int B, int L, double* out, hipStream_t s) {
    hipLaunchKernelGGL(mpnn_score_kernel, dim3(B), dim3(64), 0, s, nll, mask, L, out);
}

}  // namespace pgmi
