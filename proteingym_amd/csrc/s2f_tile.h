// The 32-row edge tile of the GVP message kernels (s2f.hip: one node's edges per tile; s3f.hip: two surface points of 16 edges each):
// the dimensions and the LDS of a block, the gather of the rows, the vector half of a GVP on the tile, the 272 -> 256 ws product on the
// fp32 MFMA, and fe_tile, which runs them in order.  A kernel says which edges and which centres its tile holds and sums the rows itself;
// what is here sees rows only, so a row's bits are the same in either kernel.
#pragma once

#include "common.h"

namespace pgmi {

constexpr int SS = S2F_S, SV = S2F_V, SH0 = S2F_H0;   // common.h's dimensions under the names the kernels use

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

// The LDS of a message kernel's block, in each file that has one: the operand tile, the vector tile, the scratch, fe_mid's small
// weights, and fe_rowe[row] = the row's edge, fe_rowe[FE_M + row] = its source node.  Five arrays and not one struct: the compiler then
// knows that they do not overlap.  A kernel that does not call fe_tile gets none of them.
static __shared__ __attribute__((aligned(16))) float fe_As[FE_M * FE_LDA];
static __shared__ float fe_Vh[FE_M * FE_LDV];
static __shared__ float fe_scr[FE_SCR];
static __shared__ float fe_wl[SV * SH0 + SV * SV + SV];
static __shared__ int32_t fe_rowe[2 * FE_M];

// tile rows -> As [FE_M][FE_LDA] = first message GVP's ws output: P_j + Es + P_i + Wn |vh|, and Vh [FE_M][FE_LDV] = its vh (33 channels).
// Row `row` of the tile is edge min(first_edge + row, last_edge): rows past last_edge repeat it and are never summed.  Its centre is node
// centre_lo for rows 0 .. 15 and centre_hi for rows 16 .. 31; TWO = false: every row's centre is centre_lo, which then stays in a register.
// nb = the first node of the masked copy.  The scalar part runs one column per thread over the tile's rows, the column of Wn in registers.
template <bool TWO>
static __device__ __noinline__ void fe_gather(float* As, float* Vh, float* vn, int32_t* rowe, const float* __restrict__ P, const float* __restrict__ VT,
                                              const float* __restrict__ Es, const float* __restrict__ ev, const float* __restrict__ whe,
                                              const float* __restrict__ Wnt, const int32_t* __restrict__ src, int64_t nb, int first_edge,
                                              int last_edge, int centre_lo, int centre_hi) {
    const int tid = threadIdx.x;
    const int64_t nlo = nb + centre_lo, nhi = nb + (TWO ? centre_hi : centre_lo);
    if (tid < FE_M) {
        const int e = min(first_edge + tid, last_edge);
        rowe[tid] = e;
        rowe[FE_M + tid] = src[e];
    }
    __syncthreads();
#pragma unroll 4
    for (int idx = tid; idx < FE_M * SH0 * 3; idx += 256) {
        const int row = idx / (SH0 * 3), t = idx - row * (SH0 * 3), h = t / 3, d = t - 3 * h;
        const int e = rowe[row];
        const int64_t ni = TWO && row >= FE_M / 2 ? nhi : nlo;
        float x = whe[h] * ev[(size_t)e * 3 + d];
        if (VT) x += VT[(nb + rowe[FE_M + row]) * (2 * SH0 * 3) + t] + VT[ni * (2 * SH0 * 3) + SH0 * 3 + t];
        Vh[row * FE_LDV + t] = x;
    }
    __syncthreads();
    for (int idx = tid; idx < FE_M * SH0; idx += 256) {
        const int row = idx / SH0, h = idx - row * SH0;
        vn[row * FE_LDN + h] = s2f_vnorm(Vh + row * FE_LDV + h * 3);
    }
    __syncthreads();
    float wn[SH0];
#pragma unroll
    for (int h = 0; h < SH0; ++h) wn[h] = Wnt[h * SS + tid];
    const float pi0 = P[nlo * 512 + SS + tid], pi1 = TWO ? P[nhi * 512 + SS + tid] : pi0;
#pragma unroll 4
    for (int row = 0; row < FE_M; ++row) {
        const float a = P[(nb + rowe[FE_M + row]) * 512 + tid] + Es[(size_t)rowe[row] * SS + tid] + (row < FE_M / 2 ? pi0 : pi1);
        float n = 0.0f;
#pragma unroll
        for (int h = 0; h < SH0; ++h) n = fmaf(wn[h], vn[row * FE_LDN + h], n);
        As[row * FE_LDA + tid] = a + n;
    }
    __syncthreads();
}

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

// One tile through the three message GVPs of a layer: on return fe_As [FE_M][0 .. 256) and fe_Vh [FE_M][16][3] hold the rows' messages.
// The tile's rows and the gather's operands are fe_gather's; block-uniform, every thread of the block calls it.
template <bool TWO>
__device__ __forceinline__ void fe_tile(const float* __restrict__ P, const float* __restrict__ VT, const float* __restrict__ Es,
                                        const float* __restrict__ ev, const float* __restrict__ whe, const float* __restrict__ Wnt,
                                        const S2fMsgWeights& w, const int32_t* __restrict__ src, int64_t nb, int first_edge, int last_edge,
                                        int centre_lo, int centre_hi) {
    fe_gather<TWO>(fe_As, fe_Vh, fe_scr, fe_rowe, P, VT, Es, ev, whe, Wnt, src, nb, first_edge, last_edge, centre_lo, centre_hi);
    fe_mid(fe_As, fe_Vh, fe_scr, fe_wl, w.wv0, w.wsv0, w.bsv0, w.wh1, SH0, true);
    fe_gemm(fe_As, w.ws1, w.ldw, w.bs1);
    fe_mid(fe_As, fe_Vh, fe_scr, fe_wl, w.wv1, w.wsv1, w.bsv1, w.wh2, SV, true);
    fe_gemm(fe_As, w.ws2, w.ldw, w.bs2);
    fe_mid(fe_As, fe_Vh, fe_scr, fe_wl, w.wv2, w.wsv2, w.bsv2, nullptr, SV, false);
}

}  // namespace pgmi
