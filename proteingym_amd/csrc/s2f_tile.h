// The 32-row edge tile of the GVP message kernels (s2f.hip: one node's edges per tile; s3f.hip: two surface points of 16 edges each):
// the dimensions, the vector half of a GVP on the tile and the 272 -> 256 ws product on the fp32 MFMA.  Both kernels gather their
// rows themselves and sum them themselves; what is here sees rows only, so a row's bits are the same in either kernel.
#pragma once

#include "common.h"

namespace pgmi {

constexpr int SS = 256;            // node scalar width
constexpr int SV = 16;             // node vector channels
constexpr int SH0 = 33;            // hidden vector channels of the first message GVP (2 * 16 + 1)

__device__ __forceinline__ float s2f_wave_sum(float x) {
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    return x;
}
__device__ __forceinline__ float s2f_vnorm(const float* v3) {
    return sqrtf(fmaxf(v3[0] * v3[0] + v3[1] * v3[1] + v3[2] * v3[2], 1e-8f));
}

constexpr int FE_M = 32;             // edge rows of a tile: two 16-row MFMA tiles
constexpr int FE_K = SS + SV;        // 272 operand columns of the second and third message GVP: [s | |vh|]
constexpr int FE_LDA = FE_K + 4;     // LDS row stride of the operand tile
constexpr int FE_LDV = SH0 * 3 + 1;  // LDS row stride of the vector tile

constexpr int FE_LDN = SH0 + 3;      // LDS row stride of the first GVP's channel norms
constexpr int FE_SCR = 4 * FE_M * SV; // scratch floats: the norms [FE_M][FE_LDN] of the gather, the gate partials [4][FE_M][16] after it

// The vector half of one GVP on the tile.  In: As[row][0 .. 256) = ws [s | |vh|] + b, Vh[row] = vh [h][3].
// gate = sigmoid(wsv s + bsv) on s before the activation; v = wv vh * gate; s = relu(s) or s, in place.  With nwh [16][16], the next
// GVP's wh: Vh[row] = nwh v and As[row][256 .. 272) = its channel norms, so As[row] is that GVP's operand row.  Without: Vh[row] = v.
// The gate is a [FE_M][256] x [256][16] product on the MFMA: wave w takes columns [64 w, 64 w + 64) and the four partial sums are
// added in wave order.  Everything else is FE_M x 48 outputs, six per thread.
static __device__ __noinline__ void fe_mid(float* As, float* Vh, float* gp, float* wl, const float* __restrict__ wv, const float* __restrict__ wsv,
                                              const float* __restrict__ bsv, const float* __restrict__ nwh, int h, bool relu) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, g = lane >> 4;
    float *wvl = wl, *nwl = wl + SV * SH0, *bl = nwl + SV * SV;  // wv [16][h], nwh [16][16] and bsv [16] in LDS for the loops below
    for (int t = tid; t < SV * h; t += 256) wvl[t] = wv[t];
    if (nwh) nwl[tid] = nwh[tid];
    if (tid < SV) bl[tid] = bsv[tid];
    {
        f32x4 gacc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int c = 64 * wave + 16 * q + 4 * g;
            const f32x4 bf = *reinterpret_cast<const f32x4*>(wsv + r * SS + c);
            const f32x4 a0 = *reinterpret_cast<const f32x4*>(As + r * FE_LDA + c);
            const f32x4 a1 = *reinterpret_cast<const f32x4*>(As + (16 + r) * FE_LDA + c);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                gacc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[e], bf[e], gacc[0], 0, 0, 0);
                gacc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[e], bf[e], gacc[1], 0, 0, 0);
            }
        }
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int v = 0; v < 4; ++v) gp[(wave * FE_M + rt * 16 + 4 * g + v) * SV + r] = gacc[rt][v];
    }
    __syncthreads();
    float out[6];
    int at[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const int idx = tid + 256 * k, row = idx / (SV * 3), t = idx - row * (SV * 3), o = t / 3, d = t - 3 * o;
        at[k] = row * FE_LDV + t;
        const float gate = ((gp[row * SV + o] + gp[(FE_M + row) * SV + o]) + gp[(2 * FE_M + row) * SV + o]) + gp[(3 * FE_M + row) * SV + o] + bl[o];
        float acc = 0.0f;
#pragma unroll 4
        for (int q = 0; q < h; ++q) acc = fmaf(wvl[o * h + q], Vh[row * FE_LDV + q * 3 + d], acc);
        out[k] = acc / (1.0f + expf(-gate));
    }
    if (relu) {
#pragma unroll 4
        for (int row = 0; row < FE_M; ++row) As[row * FE_LDA + tid] = fmaxf(As[row * FE_LDA + tid], 0.0f);
    }
    __syncthreads();                                            // every vh is read
#pragma unroll
    for (int k = 0; k < 6; ++k) Vh[at[k]] = out[k];
    __syncthreads();
    if (!nwh) return;                                           // block-uniform
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const int idx = tid + 256 * k, row = idx / (SV * 3), t = idx - row * (SV * 3), o = t / 3, d = t - 3 * o;
        float acc = 0.0f;
#pragma unroll 4
        for (int q = 0; q < SV; ++q) acc = fmaf(nwl[o * SV + q], Vh[row * FE_LDV + q * 3 + d], acc);
        out[k] = acc;
    }
    __syncthreads();                                            // every v is read
#pragma unroll
    for (int k = 0; k < 6; ++k) Vh[at[k]] = out[k];
    __syncthreads();
    for (int idx = tid; idx < FE_M * SV; idx += 256) {
        const int row = idx / SV, c = idx - row * SV;
        As[row * FE_LDA + SS + c] = s2f_vnorm(Vh + row * FE_LDV + c * 3);
    }
    __syncthreads();
}

// As[FE_M][0 .. 256) <- As[FE_M][0 .. 272) W^T + bias on v_mfma_f32_16x16x4_f32; W [256][ldw] in global memory (L2 resident: every
// block reads the same 0.3 MB).  Wave w owns columns [64 w, 64 w + 64).  Lane (r = lane & 15, g = lane >> 4): k step (q, e) of the
// MFMA is operand column 16 q + 4 g + e for both operands, so a lane reads its A rows and its W rows as float4.  C layout: column
// lane & 15, row 4 g + v.
static __device__ __noinline__ void fe_gemm(float* As, const float* __restrict__ W, int ldw, const float* __restrict__ bias) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
    f32x4 acc[2][4];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) acc[rt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* wrow = W + (size_t)(wave * 64 + r) * ldw + 4 * g;
    const float* arow = As + r * FE_LDA + 4 * g;
    f32x4 a[2], bf[4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) bf[ct] = *reinterpret_cast<const f32x4*>(wrow + (size_t)ct * 16 * ldw);
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) a[rt] = *reinterpret_cast<const f32x4*>(arow + rt * 16 * FE_LDA);
#pragma unroll 1
    for (int q = 0; q < FE_K / 16; ++q) {
        const int qn = min(q + 1, FE_K / 16 - 1);               // the next step's operands load under this step's MFMAs
        f32x4 an[2], bn[4];
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) bn[ct] = *reinterpret_cast<const f32x4*>(wrow + (size_t)ct * 16 * ldw + 16 * qn);
#pragma unroll
        for (int rt = 0; rt < 2; ++rt) an[rt] = *reinterpret_cast<const f32x4*>(arow + rt * 16 * FE_LDA + 16 * qn);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                for (int ct = 0; ct < 4; ++ct)
                    acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[rt][e], bf[ct][e], acc[rt][ct], 0, 0, 0);
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) bf[ct] = bn[ct];
#pragma unroll
        for (int rt = 0; rt < 2; ++rt) a[rt] = an[rt];
    }
    __syncthreads();                                            // every wave has read the operand tile
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
        const int col = wave * 64 + ct * 16 + r;
        const float bc = bias[col];
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int v = 0; v < 4; ++v) As[(rt * 16 + 4 * g + v) * FE_LDA + col] = acc[rt][ct][v] + bc;
    }
    __syncthreads();
}

}  // namespace pgmi
