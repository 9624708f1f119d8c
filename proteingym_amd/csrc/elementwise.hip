// HBM-bound kernels of the ESM forward: masked-window construction, embedding (+token-dropout
// rescale, learned positions), LayerNorm, rotary, row gather/scatter, the vocabulary
// projection + log-softmax on the kept rows, and the per-mutant table lookup.
// One wave64 per row wherever a row reduction is needed (shuffle reductions, no LDS).
#include "common.h"

namespace pgmi {

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// ---- masked windows: compute_fitness.py:490-495 ------------------------------------------
__global__ void make_masked_windows_kernel(const int32_t* __restrict__ wt,
                                           const int32_t* __restrict__ win_start,
                                           const int32_t* __restrict__ mask_rel, int B, int T,
                                           int32_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)B * T) return;
    const int b = (int)(i / T), t = (int)(i % T);
    out[i] = (t == mask_rel[b]) ? PGMI_TOK_MASK : wt[win_start[b] + t];
}
void launch_make_masked_windows(const int32_t* wt, const int32_t* win_start, const int32_t* mask_rel,
                                int B, int T, int32_t* out, hipStream_t s) {
    const int64_t n = (int64_t)B * T;
    hipLaunchKernelGGL(make_masked_windows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s,
                       wt, win_start, mask_rel, B, T, out);
}

__global__ void apply_mask_kernel(int32_t* tokens, const int32_t* __restrict__ mask_pos, int B, int T) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) tokens[(int64_t)b * T + mask_pos[b]] = PGMI_TOK_MASK;
}
void launch_apply_mask(int32_t* tokens, const int32_t* mask_pos, int B, int T, hipStream_t s) {
    hipLaunchKernelGGL(apply_mask_kernel, dim3((B + 255) / 256), dim3(256), 0, s, tokens, mask_pos, B, T);
}

// ---- per-sequence statistics ---------------------------------------------------------------
// scale[b] = 1 or the token-dropout factor (1-0.15*0.8)/(1 - n_mask/n_nonpad)  (esm1.py:125-131);
// the embed kernel applies it as (x*0.88f)/denom, the reference's op order.
// pos_idx[b,t] = cumsum(tok != pad)*(tok != pad) + pad_idx          (modules.py:261-262)
// kv_len[b]    = index of the last non-pad token + 1 (the host only admits trailing padding, so
//                this is the number of valid keys for the attention mask).
// mask_id: the model's <mask> token id (PGMI_TOK_MASK for the ESM alphabet; SaProt's tokenizer has it at 4 and an ordinary residue at 32).
__global__ void seq_stats_kernel(const int32_t* __restrict__ tokens, int B, int T, int token_dropout, int mask_id,
                                 float* __restrict__ denom, int32_t* __restrict__ pos_idx,
                                 int32_t* __restrict__ kv_len) {
    const int b = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (b >= B) return;
    const int32_t* tk = tokens + (int64_t)b * T;
    int running = 0, n_mask = 0, last_valid = -1;
    for (int t0 = 0; t0 < T; t0 += 64) {
        const int t = t0 + lane;
        const int tok = (t < T) ? tk[t] : PGMI_TOK_PAD;
        const int valid = (t < T) && (tok != PGMI_TOK_PAD);
        // inclusive prefix sum of `valid` within the wave
        const unsigned long long bal = __ballot(valid);
        const unsigned long long below = bal & ((lane == 63) ? ~0ull : ((1ull << (lane + 1)) - 1ull));
        const int incl = __popcll(below);
        if (t < T) pos_idx[(int64_t)b * T + t] = valid ? (running + incl + PGMI_TOK_PAD) : PGMI_TOK_PAD;
        running += __popcll(bal);
        n_mask += __popcll(__ballot((t < T) && tok == mask_id));
        if (bal) last_valid = t0 + 63 - __clzll(bal);
    }
    if (lane == 0) {
        float d = 1.0f;
        if (token_dropout) d = 1.0f - (float)n_mask / (float)running;
        denom[b] = d;
        kv_len[b] = last_valid + 1;
    }
}
void launch_seq_stats(const int32_t* tokens, int B, int T, int token_dropout, float* denom,
                      int32_t* pos_idx, int32_t* kv_len, hipStream_t s, int mask_id) {
    hipLaunchKernelGGL(seq_stats_kernel, dim3((B + 3) / 4), dim3(256), 0, s, tokens, B, T, token_dropout, mask_id,
                       denom, pos_idx, kv_len);
}

// ---- embedding: esm1.py:123-139 / esm2.py:83-94 -------------------------------------------
// x = E[tok] (zero for <mask> under token dropout) * 0.88 / denom[b] + Wpos[pos_idx]; pad rows -> 0.
__global__ void embed_kernel(const int32_t* __restrict__ tokens, const float* __restrict__ denom,
                             const int32_t* __restrict__ pos_idx, const float* __restrict__ E,
                             const float* __restrict__ P, int token_dropout, int mask_id, int rows, int T, int D,
                             float* __restrict__ x) {
    const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const int tok = tokens[row];
    const int b = row / T;
    const float dn = denom[b];
    const f32x4* e = reinterpret_cast<const f32x4*>(E + (size_t)tok * D);
    const f32x4* p = P ? reinterpret_cast<const f32x4*>(P + (size_t)pos_idx[row] * D) : nullptr;
    f32x4* xo = reinterpret_cast<f32x4*>(x + (size_t)row * D);
    const bool is_pad = tok == PGMI_TOK_PAD;
    const bool zero_emb = token_dropout && tok == mask_id;
    for (int i = lane; i < D / 4; i += 64) {
        f32x4 v = zero_emb ? f32x4{0.f, 0.f, 0.f, 0.f} : e[i];
        if (token_dropout) {
#pragma unroll
            for (int c = 0; c < 4; ++c) v[c] = (v[c] * 0.88f) / dn;
        }
        if (p) {
            const f32x4 pv = p[i];
#pragma unroll
            for (int c = 0; c < 4; ++c) v[c] += pv[c];
        }
        if (is_pad) v = f32x4{0.f, 0.f, 0.f, 0.f};
        xo[i] = v;
    }
}
void launch_embed(const int32_t* tokens, const float* denom, const int32_t* pos_idx, const float* E,
                  const float* P, int token_dropout, int rows, int T, int D, float* x, hipStream_t s, int mask_id) {
    hipLaunchKernelGGL(embed_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, tokens, denom, pos_idx, E, P,
                       token_dropout, mask_id, rows, T, D, x);
}

// zero the rows of <pad> tokens (esm1.py:138-139), needed after emb_layer_norm_before
__global__ void zero_pad_rows_kernel(const int32_t* __restrict__ tokens, int rows, int D, float* __restrict__ x) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows || tokens[row] != PGMI_TOK_PAD) return;
    for (int i = lane; i < D; i += 64) x[(size_t)row * D + i] = 0.f;
}
void launch_zero_pad_rows(const int32_t* tokens, int rows, int D, float* x, hipStream_t s) {
    hipLaunchKernelGGL(zero_pad_rows_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, tokens, rows, D, x);
}

// ---- LayerNorm (torch.nn.LayerNorm, modules.py:80-81): biased variance, eps inside sqrt ----
// One wave per row, the row held in registers (D <= 64*4*NV), two-pass mean / variance.
// Algorithmic bytes: 2*D*4 per row (read + write); HBM-bound.
// OUTMODE 0: fp32 y;  1: fp16 hi/lo, K-interleaved (f16x3 GEMM operand);  2: bf16 plane
template <int NV, int OUTMODE>
__global__ __launch_bounds__(256) void layernorm_kernel(const float* x,   // may alias y (in place)
                                                        const float* __restrict__ w,
                                                        const float* __restrict__ bsh, int rows, int D,
                                                        float eps, float* y, unsigned short* y16) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const int nv = D >> 2;
    const f32x4* xr = reinterpret_cast<const f32x4*>(x + (size_t)row * D);
    f32x4 v[NV];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = lane + 64 * i;
        v[i] = (c < nv) ? xr[c] : f32x4{0.f, 0.f, 0.f, 0.f};
        s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
    }
    const float mean = wave_sum(s) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = lane + 64 * i;
        if (c < nv) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float d = v[i][k] - mean;
                q += d * d;
            }
        }
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)D + eps);
    const f32x4* wr = reinterpret_cast<const f32x4*>(w);
    const f32x4* br = reinterpret_cast<const f32x4*>(bsh);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = lane + 64 * i;
        if (c < nv) {
            const f32x4 wv = wr[c], bv = br[c];
            f32x4 o;
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = (v[i][k] - mean) * rstd * wv[k] + bv[k];
            if constexpr (OUTMODE == 0) {
                reinterpret_cast<f32x4*>(y + (size_t)row * D)[c] = o;
            } else if constexpr (OUTMODE == 1) {
                typedef _Float16 h4 __attribute__((ext_vector_type(4)));
                h4 hi, lo;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    _Float16 a, b2;
                    split_act(o[k], a, b2);
                    hi[k] = a;
                    lo[k] = b2;
                }
                // K-interleaved GEMM operand (common.h ki_off).  Lanes (2m, 2m+1) hold k..k+3 and k+4..k+7 of one 8-group:
                // the even lane stores the 16 bytes of hi values, the odd lane the 16 bytes of lo values (one exchange of
                // 8 bytes with the neighbour), so 8 lanes write one full 128-byte line with a single store each.
                typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
                typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
                const u32x2 H = __builtin_bit_cast(u32x2, hi), L = __builtin_bit_cast(u32x2, lo);
                const bool odd = lane & 1;
                const unsigned int s0 = odd ? H[0] : L[0], s1 = odd ? H[1] : L[1];
                const unsigned int r0 = __shfl_xor(s0, 1), r1 = __shfl_xor(s1, 1);
                const u32x4 out = odd ? u32x4{r0, r1, L[0], L[1]} : u32x4{H[0], H[1], r0, r1};
                unsigned short* dst = y16 + ki_off((size_t)row, 4 * (c & ~1), D) + (odd ? 32 : 0);
                *reinterpret_cast<u32x4*>(dst) = out;
            } else {
                typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
                unsigned short b[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float ok = o[k];     // copy first: bit_cast of a vector-element lvalue reads element 0
                    unsigned int u = __builtin_bit_cast(unsigned int, ok);
                    u += 0x7fffu + ((u >> 16) & 1u);
                    b[k] = (unsigned short)(u >> 16);
                }
                u32x2 pk;
                pk[0] = b[0] | ((unsigned)b[1] << 16);
                pk[1] = b[2] | ((unsigned)b[3] << 16);
                reinterpret_cast<u32x2*>(y16 + (size_t)row * D)[c] = pk;
            }
        }
    }
}
template <int OUTMODE>
static void launch_ln_mode(const float* x, const float* w, const float* b, int rows, int D, float eps,
                           float* y, unsigned short* y16, hipStream_t s) {
    const dim3 grid((rows + 3) / 4), block(256);
    const int nv = (D / 4 + 63) / 64;
    if (nv <= 1) hipLaunchKernelGGL((layernorm_kernel<1, OUTMODE>), grid, block, 0, s, x, w, b, rows, D, eps, y, y16);
    else if (nv <= 2) hipLaunchKernelGGL((layernorm_kernel<2, OUTMODE>), grid, block, 0, s, x, w, b, rows, D, eps, y, y16);
    else if (nv <= 5) hipLaunchKernelGGL((layernorm_kernel<5, OUTMODE>), grid, block, 0, s, x, w, b, rows, D, eps, y, y16);
    else if (nv <= 10) hipLaunchKernelGGL((layernorm_kernel<10, OUTMODE>), grid, block, 0, s, x, w, b, rows, D, eps, y, y16);
    else hipLaunchKernelGGL((layernorm_kernel<20, OUTMODE>), grid, block, 0, s, x, w, b, rows, D, eps, y, y16);
}
void launch_layernorm(const float* x, const float* w, const float* b, int rows, int D, float eps,
                      float* y, hipStream_t s) {
    launch_ln_mode<0>(x, w, b, rows, D, eps, y, nullptr, s);
}
// mode 1: fp16 hi/lo planes, mode 2: bf16
void launch_layernorm16(const float* x, const float* w, const float* b, int rows, int D, float eps,
                        unsigned short* y16, int mode, hipStream_t s) {
    if (mode == 1) launch_ln_mode<1>(x, w, b, rows, D, eps, nullptr, y16, s);
    else launch_ln_mode<2>(x, w, b, rows, D, eps, nullptr, y16, s);
}

// ---- RMSNorm (ProGen3: x * rsqrt(mean(x^2) + eps) * w, fp32, no bias) into the K-interleaved f16x3 operand; one wave per row ----
template <int NV>
__global__ __launch_bounds__(256) void rmsnorm16_kernel(const float* __restrict__ x, const float* __restrict__ w, int rows, int D,
                                                        float eps, unsigned short* __restrict__ y16) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const int nv = D >> 2;
    const f32x4* xr = reinterpret_cast<const f32x4*>(x + (size_t)row * D);
    f32x4 v[NV];
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = lane + 64 * i;
        v[i] = (c < nv) ? xr[c] : f32x4{0.f, 0.f, 0.f, 0.f};
        q += (v[i][0] * v[i][0] + v[i][1] * v[i][1]) + (v[i][2] * v[i][2] + v[i][3] * v[i][3]);
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)D + eps);
    const f32x4* wr = reinterpret_cast<const f32x4*>(w);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = lane + 64 * i;
        if (c < nv) {
            const f32x4 wv = wr[c];
            f32x4 o;
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = v[i][k] * rstd * wv[k];
            store_split4(o, y16, (size_t)row, c, lane, D);
        }
    }
}
int launch_rmsnorm16(const float* x, const float* w, int rows, int D, float eps, unsigned short* y16, hipStream_t s) {
    // a lane holds at most 20 f32x4 groups; pairs of lanes write 8-column groups of whole 32-column K tiles
    if (rows <= 0 || D <= 0 || D % 32 || D > 5120) { set_error("rmsnorm: D = %d must be a multiple of 32, at most 5120", D); return PGMI_EINVAL; }
    const dim3 grid((rows + 3) / 4), block(256);
    const int nv = (D / 4 + 63) / 64;
    if (nv <= 1) hipLaunchKernelGGL((rmsnorm16_kernel<1>), grid, block, 0, s, x, w, rows, D, eps, y16);
    else if (nv <= 2) hipLaunchKernelGGL((rmsnorm16_kernel<2>), grid, block, 0, s, x, w, rows, D, eps, y16);
    else if (nv <= 5) hipLaunchKernelGGL((rmsnorm16_kernel<5>), grid, block, 0, s, x, w, rows, D, eps, y16);
    else if (nv <= 10) hipLaunchKernelGGL((rmsnorm16_kernel<10>), grid, block, 0, s, x, w, rows, D, eps, y16);
    else hipLaunchKernelGGL((rmsnorm16_kernel<20>), grid, block, 0, s, x, w, rows, D, eps, y16);
    return PGMI_OK;
}

// ---- rotary (rotary_embedding.py:11-20,47-69): half-split rotation of q (already scaled) and k
// qkv [rows, 3*H*64]; tables cos/sin [T, 64] (emb = cat(freqs,freqs)) built on the host in f32
// exactly as the reference does.  One thread handles the pair (d, d+32) of one head.
__global__ void rotary_kernel(float* __restrict__ qkv, const float* __restrict__ cos_t,
                              const float* __restrict__ sin_t, int64_t n, int T, int H, int rh) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;                      // n = rows * 2 * H * 32
    const int d = (int)(i & 31);
    const int64_t j = i >> 5;
    const int h = (int)(j % H);              // 64-lane slot group: a head, or half a head of 128 dims
    const int64_t k2 = j / H;
    const int which = (int)(k2 & 1);         // 0 = q, 1 = k
    const int64_t row = k2 >> 1;
    const int t = (int)(row % T);
    float* p = qkv + row * (size_t)(3 * H * 64) + (size_t)which * H * 64 + h * 64 + d;
    const float x1 = p[0], x2 = p[32];
    const int tr = (t * rh + (h % rh)) * 64;  // table row: one per token, or per (token, slot-group parity) for head_dim 128 (api_esm.hip ensure_rotary)
    const float c1 = cos_t[tr + d], s1 = sin_t[tr + d];
    const float c2 = cos_t[tr + d + 32], s2 = sin_t[tr + d + 32];
    p[0] = x1 * c1 + (-x2) * s1;             // x*cos + rotate_half(x)*sin, first half: -x2
    p[32] = x2 * c2 + x1 * s2;               // second half: +x1
}
void launch_rotary(float* qkv, const float* cos_t, const float* sin_t, int rows, int T, int H, hipStream_t s, int rot_halves) {
    const int64_t n = (int64_t)rows * 2 * H * 32;
    hipLaunchKernelGGL(rotary_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, qkv, cos_t, sin_t, n, T, H, rot_halves);
}

// ---- row gather / scatter -------------------------------------------------------------------
__global__ void gather_rows_kernel(const float* __restrict__ x, const int32_t* __restrict__ idx, int n,
                                   int D, float* __restrict__ y) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= n) return;
    const f32x4* src = reinterpret_cast<const f32x4*>(x + (size_t)idx[row] * D);
    f32x4* dst = reinterpret_cast<f32x4*>(y + (size_t)row * D);
    for (int i = lane; i < D / 4; i += 64) dst[i] = src[i];
}
void launch_gather_rows(const float* x, const int32_t* idx, int n, int D, float* y, hipStream_t s) {
    hipLaunchKernelGGL(gather_rows_kernel, dim3((n + 3) / 4), dim3(256), 0, s, x, idx, n, D, y);
}

// ESM3 (api_esm3.hip): the sequence row plus the window's structure-token row plus the folded per-token constant; D % 4 == 0
__global__ void esm3_embed_kernel(const int32_t* __restrict__ tokens, const int32_t* __restrict__ stok, const int32_t* __restrict__ plddt,
                                  const float* __restrict__ seq_embed, const float* __restrict__ struct_embed, const float* __restrict__ cst,
                                  int n, int T, int D, float* __restrict__ x) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= n) return;
    const int t = row % T;
    const f32x4* a = reinterpret_cast<const f32x4*>(seq_embed + (size_t)tokens[row] * D);
    const f32x4* b = reinterpret_cast<const f32x4*>(struct_embed + (size_t)stok[t] * D);
    const f32x4* c = reinterpret_cast<const f32x4*>(cst + (size_t)(plddt[t] != 0) * D);
    f32x4* dst = reinterpret_cast<f32x4*>(x + (size_t)row * D);
    for (int i = lane; i < D / 4; i += 64) dst[i] = (a[i] + b[i]) + c[i];
}
void launch_esm3_embed(const int32_t* tokens, const int32_t* stok, const int32_t* plddt, const float* seq_embed, const float* struct_embed,
                       const float* cst, int rows, int T, int D, float* x, hipStream_t s) {
    hipLaunchKernelGGL(esm3_embed_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, tokens, stok, plddt, seq_embed, struct_embed, cst, rows, T, D, x);
}

__global__ void strided_index_kernel(int first, int stride, int n, int32_t* __restrict__ idx) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) idx[i] = first + i * stride;
}
void launch_strided_index(int first, int stride, int n, int32_t* idx, hipStream_t s) {
    hipLaunchKernelGGL(strided_index_kernel, dim3((n + 255) / 256), dim3(256), 0, s, first, stride, n, idx);
}

__global__ void scatter_rows_kernel(const float* __restrict__ src, const int32_t* __restrict__ dst_row,
                                    int n, int V, float* __restrict__ table) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * V) return;
    const int rI = i / V, c = i % V;
    table[(size_t)dst_row[rI] * V + c] = src[i];
}
void launch_scatter_rows(const float* src, const int32_t* dst_row, int n, int V, float* table, hipStream_t s) {
    hipLaunchKernelGGL(scatter_rows_kernel, dim3((n * V + 255) / 256), dim3(256), 0, s, src, dst_row, n, V, table);
}

__global__ void row_index_kernel(const int32_t* __restrict__ mask_rel, int B, int T, int32_t* __restrict__ out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) out[b] = b * T + mask_rel[b];
}
void launch_row_index(const int32_t* mask_rel, int B, int T, int32_t* out, hipStream_t s) {
    hipLaunchKernelGGL(row_index_kernel, dim3((B + 255) / 256), dim3(256), 0, s, mask_rel, B, T, out);
}

__global__ void fill_f32_kernel(float* p, int64_t n, float v) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}
void launch_fill_f32(float* p, int64_t n, float v, hipStream_t s) {
    hipLaunchKernelGGL(fill_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, p, n, v);
}

// ---- vocabulary projection + log-softmax (modules.py:327 ; compute_fitness.py:502) ---------
// One wave per row: logits[v] = <h, E[v]> + bias[v] for the 33 symbols, then x - max - log(sum exp).
__global__ __launch_bounds__(256) void vocab_logsoftmax_kernel(const float* __restrict__ h,
                                                               const float* __restrict__ E,
                                                               const float* __restrict__ bias, int rows,
                                                               int D, int V, float* __restrict__ out,
                                                               int32_t* __restrict__ nonfinite) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    // The 33 (25) logits of a row and their log-sum-exp are accumulated in DOUBLE and rounded to fp32 once: the work is negligible
    // (V dot products of D per kept row) and the result carries no rounding of its own on top of the fp32 input row -- a
    // pseudo-ppl score sums ~700 of these values, where a systematic last-place bias of an fp32 log-softmax (values ~ -16: one
    // ulp = 1.9e-6) would add up to 1e-3 (tests/test_gpu_parity_real_width.py).
    const float* hr = h + (size_t)row * D;
    double my_logit = -INFINITY;           // lane v (< V) ends up owning logit v
    for (int v = 0; v < V; ++v) {
        const float* ev = E + (size_t)v * D;
        double acc = 0.0;
        for (int i = lane; i < D; i += 64) acc = fma((double)hr[i], (double)ev[i], acc);
        acc = wave_sum_d(acc);
        if (lane == v) my_logit = acc + (double)bias[v];
    }
    const float mx = wave_max((float)my_logit);
    const double ex = (lane < V) ? exp(my_logit - (double)mx) : 0.0;
    const double lse = log(wave_sum_d(ex));
    const float res = (float)((my_logit - (double)mx) - lse);
    if (lane < V) {
        out[(size_t)row * V + lane] = res;
        if (nonfinite && !(fabsf(res) <= 3.0e38f)) atomicOr(nonfinite, 1);   // NaN/inf: fp16 overflow upstream
    }
}
void launch_vocab_logsoftmax(const float* h, const float* E, const float* bias, int rows, int D, int V,
                             float* out, int32_t* nonfinite, hipStream_t s) {
    hipLaunchKernelGGL(vocab_logsoftmax_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, h, E, bias, rows, D, V, out, nonfinite);
}

// ---- Tranception sequence log-likelihood (one wave per sequence) ------------------------------
// TranceptEVE's second prior (trancepteve/model_pytorch.py:1113-1133): two = (1 - alpha) lp + alpha msa is fused with the EVE row e as
// (1 - beta) two + beta e; a column EVE does not model holds -inf, which either hands the position back to `two` (eve_fallback) or
// goes through the arithmetic as in the reference.
__device__ __forceinline__ float fuse_eve(float two, float e, float beta, int eve_fallback) {
    if (eve_fallback && e == -INFINITY) return two;
    return (1.0f - beta) * two + beta * e;
}
__global__ __launch_bounds__(256) void seq_loglik_kernel(const float* __restrict__ lp, const int32_t* __restrict__ tokens,
                                                         const int32_t* __restrict__ lens, int B, int T, int V,
                                                         const float* __restrict__ prior, const int32_t* __restrict__ a0,
                                                         const int32_t* __restrict__ row0, const int32_t* __restrict__ n,
                                                         const int32_t* __restrict__ flip, float alpha,
                                                         const float* __restrict__ eve, float beta, int eve_fallback,
                                                         float* __restrict__ out) {
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (b >= B) return;
    const int len = lens[b];
    float acc = 0.f;
    for (int t = lane; t < len - 1; t += 64) {
        const int tgt = tokens[(size_t)b * T + t + 1];
        float v = lp[((size_t)b * T + t) * V + tgt];
        if (prior && n[b] > 0 && t >= a0[b] && t < a0[b] + n[b]) {
            const int i = t - a0[b];
            const int row = flip[b] ? row0[b] + (n[b] - 1 - i) : row0[b] + i;
            v = (1.0f - alpha) * v + alpha * prior[(size_t)row * V + tgt];
            if (eve) v = fuse_eve(v, eve[(size_t)row * V + tgt], beta, eve_fallback);
        }
        acc += v;
    }
    acc = wave_sum(acc);
    if (lane == 0) out[b] = acc;
}
// The same reduction over SUFFIX rows (Tranception prefix-shared scoring, common.h AttRagged): sequence b owns the packed rows of its
// tokens seq_p[b] .. T-1 (log-probabilities in lp, ids in tokens, both packed); the rows before seq_p[b] are its root's (the model is
// causal: the same tokens give the same rows).  Same lane partition, same order, same arithmetic as seq_loglik_kernel: with the same
// row values the sum has the same bits.
__global__ __launch_bounds__(256) void seq_loglik_ragged_kernel(const float* __restrict__ lp, const int32_t* __restrict__ tokens,
                                                                const int32_t* __restrict__ seq_off, const int32_t* __restrict__ seq_p,
                                                                const int32_t* __restrict__ seq_root, int B, int T, int V,
                                                                const float* __restrict__ prior, const int32_t* __restrict__ a0,
                                                                const int32_t* __restrict__ row0, const int32_t* __restrict__ n,
                                                                const int32_t* __restrict__ flip, float alpha,
                                                                const float* __restrict__ eve, float beta, int eve_fallback,
                                                                float* __restrict__ out) {
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (b >= B) return;
    const int a = seq_p[b], own0 = seq_off[b] - a, root0 = seq_off[seq_root[b]];
    float acc = 0.f;
    for (int t = lane; t < T - 1; t += 64) {
        const int tgt = tokens[(t + 1 < a) ? root0 + t + 1 : own0 + t + 1];
        float v = lp[(size_t)((t < a) ? root0 + t : own0 + t) * V + tgt];
        if (prior && n[b] > 0 && t >= a0[b] && t < a0[b] + n[b]) {
            const int i = t - a0[b];
            const int row = flip[b] ? row0[b] + (n[b] - 1 - i) : row0[b] + i;
            v = (1.0f - alpha) * v + alpha * prior[(size_t)row * V + tgt];
            if (eve) v = fuse_eve(v, eve[(size_t)row * V + tgt], beta, eve_fallback);
        }
        acc += v;
    }
    acc = wave_sum(acc);
    if (lane == 0) out[b] = acc;
}
void launch_seq_loglik_ragged(const float* lp, const int32_t* tokens, const int32_t* seq_off, const int32_t* seq_p,
                              const int32_t* seq_root, int B, int T, int V, const float* prior, const int32_t* a0,
                              const int32_t* row0, const int32_t* n, const int32_t* flip, float alpha, const float* eve, float beta,
                              int eve_fallback, float* out, hipStream_t s) {
    hipLaunchKernelGGL(seq_loglik_ragged_kernel, dim3((B + 3) / 4), dim3(256), 0, s, lp, tokens, seq_off, seq_p, seq_root, B, T, V,
                       prior, a0, row0, n, flip, alpha, eve, beta, eve_fallback, out);
}
void launch_seq_loglik(const float* lp, const int32_t* tokens, const int32_t* lens, int B, int T, int V,
                       const float* prior, const int32_t* a0, const int32_t* row0, const int32_t* n,
                       const int32_t* flip, float alpha, const float* eve, float beta, int eve_fallback, float* out, hipStream_t s) {
    hipLaunchKernelGGL(seq_loglik_kernel, dim3((B + 3) / 4), dim3(256), 0, s, lp, tokens, lens, B, T, V, prior, a0, row0, n,
                       flip, alpha, eve, beta, eve_fallback, out);
}

// ---- ProGen2 sequence log-likelihood (one wave per sequence) ---------------------------------
// lp holds the log-softmax over the 25 amino-acid columns 5..29 only (compute_fitness.py:67-70); col[b*T + t] is target t's column
// (token id - 5) and n_kept[b] the targets left after the terminal strip (:60-64).  Every row's partial sums run over the same lanes
// in the same order whatever else is in the launch: a sequence gets the same bits in any batch.
__global__ __launch_bounds__(256) void pg2_seq_loglik_kernel(const float* __restrict__ lp, const int32_t* __restrict__ col,
                                                             const int32_t* __restrict__ n_kept, int B, int T, int V,
                                                             float* __restrict__ out) {
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (b >= B) return;
    const int n = n_kept[b];
    double acc = 0.0;
    for (int t = lane; t < n; t += 64) acc += (double)lp[((size_t)b * T + t) * V + col[(size_t)b * T + t]];
    acc = wave_sum_d(acc);
    if (lane == 0) out[b] = (float)acc;
}
void launch_pg2_seq_loglik(const float* lp, const int32_t* col, const int32_t* n_kept, int B, int T, int V, float* out, hipStream_t s) {
    hipLaunchKernelGGL(pg2_seq_loglik_kernel, dim3((B + 3) / 4), dim3(256), 0, s, lp, col, n_kept, B, T, V, out);
}

// ---- label_row (compute_fitness.py:240-250): score = sum_subs f32(lp[mt] - lp[wt]) in double ---
__global__ void score_mutants_kernel(const float* __restrict__ table, int V,
                                     const int32_t* __restrict__ sub_pos,
                                     const int32_t* __restrict__ sub_wt,
                                     const int32_t* __restrict__ sub_mt,
                                     const int64_t* __restrict__ mut_off, int64_t n_mut,
                                     double* __restrict__ scores) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_mut) return;
    double sc = 0.0;
    for (int64_t k = mut_off[i]; k < mut_off[i + 1]; ++k) {
        const float* rowp = table + (size_t)sub_pos[k] * V;
        const float d = rowp[sub_mt[k]] - rowp[sub_wt[k]];
        sc += (double)d;
    }
    scores[i] = sc;
}
void launch_score_mutants(const float* table, int V, const int32_t* sub_pos, const int32_t* sub_wt,
                          const int32_t* sub_mt, const int64_t* mut_off, int64_t n_mut, double* scores,
                          hipStream_t s) {
    if (n_mut <= 0) return;
    hipLaunchKernelGGL(score_mutants_kernel, dim3((unsigned)((n_mut + 255) / 256)), dim3(256), 0, s, table, V,
                       sub_pos, sub_wt, sub_mt, mut_off, n_mut, scores);
}


// ---- pseudo-perplexity rows (compute_fitness.py:258-279), enumerated on the device ----------------------
// A library of variable-length sequences is resident as one byte string tok8 (cls + residues + eos per
// sequence, seq_off[n] .. seq_off[n+1]).  sid[j] lists the sequences of a run in descending token length,
// rp[j] is the number of (sequence, masked position) rows before sid[j] in that order: sequence n with `len`
// tokens (L = len-2 residues) contributes the rows i = 1 .. L-2 (the reference loops i in range(1, len(seq)-1)
// and masks TOKEN i).  Row g of the run = (sid[j], i = 1 + g - rp[j]) with rp[j] <= g < rp[j+1]: one wave per row
// finds j by bisection, then writes the T tokens of the row (<pad> beyond the sequence, <mask> at i), the
// flat index of the masked token and the target token: the reference scores alphabet.get_idx(sequence[i]) =
// token i+1 at masked token i (its off-by-one, reproduced).
__global__ __launch_bounds__(256) void make_pppl_rows_kernel(const uint8_t* __restrict__ tok8, const int64_t* __restrict__ seq_off,
                                                             const int32_t* __restrict__ sid, const int64_t* __restrict__ rp, int J,
                                                             int64_t g0, int bc, int T, int32_t* __restrict__ tokens,
                                                             int32_t* __restrict__ row_idx, int32_t* __restrict__ target) {
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (b >= bc) return;
    const int64_t g = g0 + b;
    int lo = 0, hi = J;                                   // largest j with rp[j] <= g (rp[J] = total rows > g)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (rp[mid] <= g) lo = mid; else hi = mid;
    }
    const int n = sid[lo];
    const int i = 1 + (int)(g - rp[lo]);
    const int64_t o = seq_off[n];
    const int len = (int)(seq_off[n + 1] - o);
    int32_t* out = tokens + (int64_t)b * T;
    for (int t = lane; t < T; t += 64) out[t] = (t == i) ? PGMI_TOK_MASK : (t < len ? (int32_t)tok8[o + t] : PGMI_TOK_PAD);
    if (lane == 0) {
        row_idx[b] = b * T + i;
        target[b] = (int32_t)tok8[o + i + 1];
    }
}
void launch_make_pppl_rows(const uint8_t* tok8, const int64_t* seq_off, const int32_t* sid, const int64_t* rp, int J,
                           int64_t g0, int bc, int T, int32_t* tokens, int32_t* row_idx, int32_t* target, hipStream_t s) {
    hipLaunchKernelGGL(make_pppl_rows_kernel, dim3((bc + 3) / 4), dim3(256), 0, s, tok8, seq_off, sid, rp, J, g0, bc, T,
                       tokens, row_idx, target);
}

// terms[g0 + b] = lp[b, target[b]]   (token_probs[0, i, alphabet.get_idx(sequence[i])], compute_fitness.py:275)
__global__ void pppl_pick_kernel(const float* __restrict__ lp, const int32_t* __restrict__ target, int bc, int V,
                                 float* __restrict__ terms) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < bc) terms[b] = lp[(size_t)b * V + target[b]];
}
void launch_pppl_pick(const float* lp, const int32_t* target, int bc, int V, float* terms, hipStream_t s) {
    hipLaunchKernelGGL(pppl_pick_kernel, dim3((bc + 255) / 256), dim3(256), 0, s, lp, target, bc, V, terms);
}

// out[sid[j] - first] = sum(log_probs): python's left-to-right sum of the f32 terms' double values (:279)
__global__ void pppl_sum_kernel(const float* __restrict__ terms, const int64_t* __restrict__ rp, const int32_t* __restrict__ sid,
                                int J, int64_t first, double* __restrict__ out) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= J) return;
    double acc = 0.0;
    for (int64_t g = rp[j]; g < rp[j + 1]; ++g) acc += (double)terms[g];
    out[sid[j] - first] = acc;
}
void launch_pppl_sum(const float* terms, const int64_t* rp, const int32_t* sid, int J, int64_t first, double* out, hipStream_t s) {
    if (J <= 0) return;
    hipLaunchKernelGGL(pppl_sum_kernel, dim3((J + 127) / 128), dim3(128), 0, s, terms, rp, sid, J, first, out);
}


// ---- causal decoder (api_gpt.hip) -----------------------------------------------------------------------------------------
// x[row] = E[tokens[row]] + P[row % T]: GPT-2's inputs_embeds + position_embeds with position ids 0..T-1 (one wave per row)
__global__ __launch_bounds__(256) void embed_learned_kernel(const int32_t* __restrict__ tokens, const float* __restrict__ E,
                                                            const float* __restrict__ P, int rows, int T, int D, float* __restrict__ x) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const f32x4* e = reinterpret_cast<const f32x4*>(E + (size_t)tokens[row] * D);
    const f32x4* p = reinterpret_cast<const f32x4*>(P + (size_t)(row % T) * D);
    f32x4* xo = reinterpret_cast<f32x4*>(x + (size_t)row * D);
    for (int i = lane; i < D / 4; i += 64) xo[i] = e[i] + p[i];
}
void launch_embed_learned(const int32_t* tokens, const float* E, const float* P, int rows, int T, int D, float* x, hipStream_t s) {
    hipLaunchKernelGGL(embed_learned_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, tokens, E, P, rows, T, D, x);
}

// ESM-IF1's decoder embedding: x[row] = scale * E[tokens[row]] + P[pos[row]] (one wave per row, D % 4 == 0)
__global__ __launch_bounds__(256) void embed_scaled_pos_kernel(const int32_t* __restrict__ tokens, const int32_t* __restrict__ pos,
                                                               const float* __restrict__ E, const float* __restrict__ P, float scale,
                                                               int rows, int D, float* __restrict__ x) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const f32x4* e = reinterpret_cast<const f32x4*>(E + (size_t)tokens[row] * D);
    const f32x4* p = reinterpret_cast<const f32x4*>(P + (size_t)pos[row] * D);
    f32x4* xo = reinterpret_cast<f32x4*>(x + (size_t)row * D);
    for (int i = lane; i < D / 4; i += 64) {
        const f32x4 ev = e[i], pv = p[i];
        f32x4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = fmaf(scale, ev[k], pv[k]);
        xo[i] = o;
    }
}
void launch_embed_scaled_pos(const int32_t* tokens, const int32_t* pos, const float* E, const float* P, float scale, int rows, int D,
                             float* x, hipStream_t s) {
    hipLaunchKernelGGL(embed_scaled_pos_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, tokens, pos, E, P, scale, rows, D, x);
}

// Log-softmax over a wide vocabulary (V > 64: ProtGPT2's 50 257).  One 256-thread workgroup per row of fp32 logits [rows][ldl]
// (ldl % 4 == 0; columns V .. ldl-1 are padding, excluded by index, never by value).  The row is read once: thread i takes the
// float4s i, i + 256, ... and keeps a running max m and s = sum exp(x - m) in double (rescaled when m grows); the 256 (m, s) pairs
// are then combined in a fixed tree order in double.  Every order depends on V alone, so a row's bits do not depend on the other
// rows of the launch.  tgt != nullptr: out[r] = log p(column tgt[r]) (scoring); else out[r * V + c] for every c < V.
// -inf logits follow torch.log_softmax: their columns are -inf, the others what they would be without them; a row of nothing but -inf
// is NaN.  A pair whose m is still -inf has s == 0 (or NaN, from a NaN logit), so lse_merge never forms exp(-inf - -inf).
__device__ __forceinline__ void lse_merge(float& m, double& s, float m2, double s2) {
    const float M = fmaxf(m, m2);
    const double a = s == 0.0 ? 0.0 : s * exp((double)m - (double)M);
    const double b = s2 == 0.0 ? 0.0 : s2 * exp((double)m2 - (double)M);
    m = M;
    s = a + b;
}
__global__ __launch_bounds__(256) void wide_logsoftmax_kernel(const float* __restrict__ logits, int ldl, int V,
                                                              const int32_t* __restrict__ tgt, float* __restrict__ out,
                                                              int32_t* __restrict__ nonfinite) {
    __shared__ float sm[256];
    __shared__ double ss[256];
    const int r = blockIdx.x, tid = threadIdx.x;
    const float* row = logits + (size_t)r * ldl;
    const f32x4* row4 = reinterpret_cast<const f32x4*>(row);
    float m = -INFINITY;
    double s = 0.0;
    for (int i = tid; i < (V + 3) / 4; i += 256) {
        const f32x4 v = row4[i];
        const int c0 = 4 * i;
        float mx = m;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (c0 + k < V) mx = fmaxf(mx, v[k]);
        if (mx > m) {
            s = s == 0.0 ? 0.0 : s * (double)__expf(m - mx);
            m = mx;
        }
        // a -inf logit has probability 0 and adds nothing -- also while m is still -inf, where exp(-inf - m) would be NaN.  (A NaN or
        // +inf logit still makes its term, and so the row, NaN.)  For a finite logit the term is the same instruction on the same operands.
        float e = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (c0 + k < V) e += v[k] == -INFINITY ? 0.0f : __expf(v[k] - m);
        s += (double)e;
    }
    sm[tid] = m;
    ss[tid] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
            float a = sm[tid];
            double b = ss[tid];
            lse_merge(a, b, sm[tid + o], ss[tid + o]);
            sm[tid] = a;
            ss[tid] = b;
        }
        __syncthreads();
    }
    const double lse = (double)sm[0] + log(ss[0]);
    bool bad = false;
    if (tgt) {
        if (tid == 0) {
            const float res = (float)((double)row[tgt[r]] - lse);
            out[r] = res;
            bad = !(fabsf(res) <= 3.0e38f);
        }
    } else {
        for (int c = tid; c < V; c += 256) {
            const float res = (float)((double)row[c] - lse);
            out[(size_t)r * V + c] = res;
            bad |= !(fabsf(res) <= 3.0e38f);
        }
    }
    if (nonfinite && bad) atomicOr(nonfinite, 1);             // NaN/inf: fp16 overflow upstream
}
void launch_wide_logsoftmax(const float* logits, int ldl, int rows, int V, const int32_t* tgt, float* out, int32_t* nonfinite,
                            hipStream_t s) {
    if (rows <= 0) return;
    hipLaunchKernelGGL(wide_logsoftmax_kernel, dim3(rows), dim3(256), 0, s, logits, ldl, V, tgt, out, nonfinite);
}

// out[b] = sum of terms[off[b] .. off[b+1]) in double, left to right: one thread per sequence, so the order is the sequence's own
__global__ void seq_sum_kernel(const float* __restrict__ terms, const int32_t* __restrict__ off, int B, double* __restrict__ out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double acc = 0.0;
    for (int i = off[b]; i < off[b + 1]; ++i) acc += (double)terms[i];
    out[b] = acc;
}
void launch_seq_sum(const float* terms, const int32_t* off, int B, double* out, hipStream_t s) {
    hipLaunchKernelGGL(seq_sum_kernel, dim3((B + 127) / 128), dim3(128), 0, s, terms, off, B, out);
}

// ---- SaProt (api_saprot.hip) ----------------------------------------------------------------------------------------------
// Token rows of the position sets [s0, s0 + bc) of an assay chunk (baselines/saprot/compute_fitness.py:30-36): row b is the wild type wt [T]
// with the tokens at the set's positions set_pos[set_off[s] .. set_off[s + 1]) (ascending) replaced by their masked ids -- the '#'
// amino-acid group with the same structure letter: first + (groups - 1) * width + (id - first) % width; a special token (id < first)
// stays.  keep[e - set_off[s0]] = flat row of entry e: the rows the head reads.  One wave per set; a token looks itself up in the
// set by bisection, so every element of `tokens` is written once.
__global__ __launch_bounds__(256) void saprot_rows_kernel(const int32_t* __restrict__ wt, const int32_t* __restrict__ set_off,
                                                          const int32_t* __restrict__ set_pos, int s0, int bc, int T, int first,
                                                          int groups, int width, int32_t* __restrict__ tokens,
                                                          int32_t* __restrict__ keep) {
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (b >= bc) return;
    const int e0 = set_off[s0], lo0 = set_off[s0 + b], hi0 = set_off[s0 + b + 1];
    int32_t* out = tokens + (int64_t)b * T;
    for (int t = lane; t < T; t += 64) {
        int lo = lo0, hi = hi0;                              // first entry with set_pos >= t
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (set_pos[mid] < t) lo = mid + 1; else hi = mid;
        }
        const int id = wt[t];
        const bool masked = lo < hi0 && set_pos[lo] == t && id >= first;
        out[t] = masked ? first + (groups - 1) * width + (id - first) % width : id;
    }
    for (int e = lo0 + lane; e < hi0; e += 64) keep[e - e0] = b * T + set_pos[e];
}
void launch_saprot_rows(const int32_t* wt, const int32_t* set_off, const int32_t* set_pos, int s0, int bc, int T, int first, int groups,
                        int width, int32_t* tokens, int32_t* keep, hipStream_t s) {
    hipLaunchKernelGGL(saprot_rows_kernel, dim3((bc + 3) / 4), dim3(256), 0, s, wt, set_off, set_pos, s0, bc, T, first, groups, width,
                       tokens, keep);
}

// ---- MULAN (api_mulan.hip) ---------------------------------------------------------------------------------------------------
// The structure adapter's input rows for the position sets [s0, s0 + bc) (mulan/dataset.py:306-314, compute_fitness.py:117-126).  One
// wave per row (b, t): the row looks itself up in its set by bisection, picks its seven values -- 4 for the two end rows and for
// plddt <= 70, -4 in the set, else the stored angles -- and every lane writes y[row][d] = bias[d] + sum_k a_k W[d][k] for its d, in
// fp32, k ascending.  With wt, lane 0 also writes the token (<mask> in the set) and, for a row of the set, its keep entry: every
// entry of the chunk belongs to exactly one row, so keep is written once.
__global__ __launch_bounds__(256) void mulan_rows_kernel(const int32_t* __restrict__ wt, const int32_t* __restrict__ set_off,
                                                         const int32_t* __restrict__ set_pos, int s0, int bc, int T, int mask_id,
                                                         const float* __restrict__ angles, const float* __restrict__ plddt,
                                                         const float* __restrict__ W, const float* __restrict__ bias, int D,
                                                         int32_t* __restrict__ tokens, int32_t* __restrict__ keep, float* __restrict__ y) {
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= (int64_t)bc * T) return;
    const int b = (int)(row / T), t = (int)(row % T);
    const int e0 = set_off[s0], lo0 = set_off[s0 + b], hi0 = set_off[s0 + b + 1];
    int lo = lo0, hi = hi0;                                  // first entry with set_pos >= t
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (set_pos[mid] < t) lo = mid + 1; else hi = mid;
    }
    const bool in_set = lo < hi0 && set_pos[lo] == t;
    float a[7];
    const bool padded = t == 0 || t == T - 1 || plddt[t] <= 70.0f;
#pragma unroll
    for (int k = 0; k < 7; ++k) a[k] = in_set ? -4.0f : padded ? 4.0f : angles[(size_t)t * 7 + k];
    if (wt && lane == 0) {
        tokens[row] = in_set ? mask_id : wt[t];
        if (in_set) keep[lo - e0] = (int32_t)row;
    }
    float* yo = y + (size_t)row * D;
    for (int d = lane; d < D; d += 64) {
        float acc = bias[d];
#pragma unroll
        for (int k = 0; k < 7; ++k) acc = fmaf(a[k], W[(size_t)d * 7 + k], acc);
        yo[d] = acc;
    }
}
void launch_mulan_rows(const int32_t* wt, const int32_t* set_off, const int32_t* set_pos, int s0, int bc, int T, int mask_id,
                       const float* angles, const float* plddt, const float* W, const float* bias, int D, int32_t* tokens, int32_t* keep,
                       float* y, hipStream_t s) {
    const int64_t rows = (int64_t)bc * T;
    hipLaunchKernelGGL(mulan_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, wt, set_off, set_pos, s0, bc, T, mask_id,
                       angles, plddt, W, bias, D, tokens, keep, y);
}

// x = (E[tok] + st[row]), zero for <mask> under token dropout, times 0.88 / denom[b] in embed_kernel's order (model_utils.py:156-176);
// pad rows -> 0.  D % 4 == 0.
__global__ void mulan_embed_kernel(const int32_t* __restrict__ tokens, const float* __restrict__ denom, const float* __restrict__ E,
                                   const float* __restrict__ st, int token_dropout, int mask_id, int rows, int T, int D,
                                   float* __restrict__ x) {
    const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const int tok = tokens[row];
    const float dn = denom[row / T];
    const f32x4* e = reinterpret_cast<const f32x4*>(E + (size_t)tok * D);
    const f32x4* sr = reinterpret_cast<const f32x4*>(st + (size_t)row * D);
    f32x4* xo = reinterpret_cast<f32x4*>(x + (size_t)row * D);
    const bool zero = tok == PGMI_TOK_PAD || (token_dropout && tok == mask_id);
    for (int i = lane; i < D / 4; i += 64) {
        f32x4 v = e[i];
        const f32x4 sv = sr[i];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            v[c] += sv[c];
            if (token_dropout) v[c] = (v[c] * 0.88f) / dn;
        }
        xo[i] = zero ? f32x4{0.f, 0.f, 0.f, 0.f} : v;
    }
}
void launch_mulan_embed(const int32_t* tokens, const float* denom, const float* E, const float* st, int token_dropout, int rows, int T,
                        int D, float* x, hipStream_t s, int mask_id) {
    hipLaunchKernelGGL(mulan_embed_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, tokens, denom, E, st, token_dropout, mask_id, rows, T,
                       D, x);
}

// Vocabulary projection + grouped log-softmax (compute_fitness.py:42-53).  One wave per row of h [rows][D] (D % 4 == 0), V <= 512 logits
// against the tied table E [V][D]:
//   full  [row][V]      (nullable) = logit - lse(row)                                    the log-softmax of all V columns
//   group [row][groups] (nullable) = lse(logits[first + g width .. + width)) - lse(row)  log of the summed probability of group g
// so that group[mt] - group[wt] is the reference's log(sum probs[mt group] / sum probs[wt group]).  The logits and every log-sum-exp
// are accumulated in double and rounded to fp32 once, for the reason given at vocab_logsoftmax_kernel.  The lane holds its share of
// the hidden row in registers (128-bit loads; NV float4 per lane); logit v ends up in slot v / 64 of lane v % 64.  Every sum runs
// over the same lanes in the same order whatever else is in the launch: a row's bits depend on V and D alone.
constexpr int kGroupSlots = 8;
template <int NV>
__global__ __launch_bounds__(256) void group_logsoftmax_kernel(const float* __restrict__ h, const float* __restrict__ E,
                                                               const float* __restrict__ bias, int rows, int D, int V, int first,
                                                               int groups, int width, float* __restrict__ full,
                                                               float* __restrict__ group, int32_t* __restrict__ nonfinite) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const int nv = D >> 2;
    const f32x4* hr = reinterpret_cast<const f32x4*>(h + (size_t)row * D);
    f32x4 x[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = lane + 64 * i;
        x[i] = (c < nv) ? hr[c] : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    double lg[kGroupSlots];
#pragma unroll
    for (int j = 0; j < kGroupSlots; ++j) {
        lg[j] = -INFINITY;
        for (int l = 0; l < 64; ++l) {
            const int v = 64 * j + l;
            if (v >= V) break;                                // uniform over the wave
            const f32x4* ev = reinterpret_cast<const f32x4*>(E + (size_t)v * D);
            double acc = 0.0;
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const int c = lane + 64 * i;
                if (c < nv) {
                    const f32x4 e = ev[c];
#pragma unroll
                    for (int k = 0; k < 4; ++k) acc = fma((double)x[i][k], (double)e[k], acc);
                }
            }
            acc = wave_sum_d(acc);
            if (lane == l) lg[j] = acc + (double)bias[v];
        }
    }
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < kGroupSlots; ++j) mx = fmaxf(mx, (float)lg[j]);
    mx = wave_max(mx);
    double ex = 0.0;
#pragma unroll
    for (int j = 0; j < kGroupSlots; ++j) ex += (64 * j + lane < V) ? exp(lg[j] - (double)mx) : 0.0;
    const double lse = (double)mx + log(wave_sum_d(ex));
    bool bad = false;
    if (full) {
#pragma unroll
        for (int j = 0; j < kGroupSlots; ++j) {
            const int v = 64 * j + lane;
            if (v < V) {
                const float res = (float)(lg[j] - lse);
                full[(size_t)row * V + v] = res;
                bad |= !(fabsf(res) <= 3.0e38f);
            }
        }
    }
    if (group) {
        float mine = 0.f;
        for (int g = 0; g < groups; ++g) {
            const int c0 = first + g * width;
            double val = -INFINITY;                           // this lane's logit inside the group (width <= 64: at most one)
#pragma unroll
            for (int j = 0; j < kGroupSlots; ++j) {
                const int v = 64 * j + lane;
                if (v >= c0 && v < c0 + width && v < V) val = lg[j];
            }
            const float gm = wave_max((float)val);
            const double gs = wave_sum_d(val == -INFINITY ? 0.0 : exp(val - (double)gm));
            const float res = (float)(((double)gm + log(gs)) - lse);
            if (lane == g) mine = res;
        }
        if (lane < groups) {
            group[(size_t)row * groups + lane] = mine;
            bad |= !(fabsf(mine) <= 3.0e38f);
        }
    }
    if (nonfinite && bad) atomicOr(nonfinite, 1);             // NaN/inf: fp16 overflow upstream
}
int group_logsoftmax_check(int D, int V, int first, int groups, int width) {
    const int nv = (D / 4 + 63) / 64;
    if (D % 4 || nv > 10 || V > 64 * kGroupSlots || groups > 64 || width > 64 || first + groups * width > V) {
        set_error("grouped log-softmax: unsupported shape (D %d, V %d, %d groups of %d from column %d)", D, V, groups, width, first);
        return PGMI_EINVAL;
    }
    return PGMI_OK;
}
int launch_group_logsoftmax(const float* h, const float* E, const float* bias, int rows, int D, int V, int first, int groups, int width,
                            float* full, float* group, int32_t* nonfinite, hipStream_t s) {
    if (rows <= 0) return PGMI_OK;
    const int nv = (D / 4 + 63) / 64;
    if (int rc = group_logsoftmax_check(D, V, first, groups, width)) return rc;
    const dim3 grid((rows + 3) / 4), block(256);
#define PGMI_GLS(N) hipLaunchKernelGGL((group_logsoftmax_kernel<N>), grid, block, 0, s, h, E, bias, rows, D, V, first, groups, width, full, group, nonfinite)
    if (nv <= 1) PGMI_GLS(1); else if (nv <= 2) PGMI_GLS(2); else if (nv <= 5) PGMI_GLS(5); else PGMI_GLS(10);
#undef PGMI_GLS
    return PGMI_OK;
}

}  // namespace pgmi
