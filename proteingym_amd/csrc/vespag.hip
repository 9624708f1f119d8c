// VespaG's two kernels; the first Linear of its head stays on launch_gemm_f32 / launch_gemm16 (api_vespag.hip).
//   packed_scatter_kernel   a chunk's residue rows after emb_layer_norm_after, in the order the chunk ran them, to their place in the
//                           packed [sum L][D] buffer of the caller's order; a non-finite value raises the model's fp16-range flag (one
//                           atomicOr per wave that saw one, as the log-softmax heads do).  dst_row is the only thing that knows both
//                           orders; every source row has its own destination, so no two waves write one address.
//   vespag_head_kernel      per row: LeakyReLU(h) (models/utils.py construct_fnn: nn.LeakyReLU, slope 0.01), the hidden -> 20 product
//                           with W2 in LDS, the bias, and mask_non_mutations (utils/utils.py: exact 0.0 in the wild type's own column;
//                           wt_col -1 leaves the row alone).  fp32, one wave per row, a lane owns the columns k = lane + 64 i of the
//                           hidden row; the 20 sums meet in a butterfly whose order is fixed, so a row's bits depend on nothing but the
//                           row.  No atomics.  The head is about 0.02 % of the encoder's FLOPs per row: it has no MFMA path.
#include "common.h"

namespace pgmi {

namespace {

constexpr int kVespagOut = 20, kVespagRowsPerBlock = 64;

__global__ __launch_bounds__(256) void packed_scatter_kernel(const float* __restrict__ src, const int32_t* __restrict__ dst_row, int n, int D,
                                                            float* __restrict__ out, int32_t* __restrict__ nonfinite) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= n) return;
    const f32x4* s = reinterpret_cast<const f32x4*>(src + (size_t)row * D);
    f32x4* d = reinterpret_cast<f32x4*>(out + (size_t)dst_row[row] * D);
    bool bad = false;
    for (int i = lane; i < D / 4; i += 64) {
        const f32x4 v = s[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) bad |= !(fabsf(v[e]) <= 3.0e38f);       // NaN / inf: fp16 overflow upstream
        d[i] = v;
    }
    if (nonfinite && __any(bad) && lane == 0) atomicOr(nonfinite, 1);
}

__global__ __launch_bounds__(256) void vespag_head_kernel(const float* __restrict__ h, const float* __restrict__ W2, const float* __restrict__ b2,
                                                         const int32_t* __restrict__ wt_col, int rows, int H, float slope,
                                                         float* __restrict__ y) {
    extern __shared__ __attribute__((aligned(16))) float w2s[];              // [20][H]
    for (int i = threadIdx.x; i < kVespagOut * H; i += 256) w2s[i] = W2[i];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r1 = min(rows, (int)(blockIdx.x + 1) * kVespagRowsPerBlock);
    for (int row = blockIdx.x * kVespagRowsPerBlock + wave; row < r1; row += 4) {
        const float* hr = h + (size_t)row * H;
        float acc[kVespagOut];
#pragma unroll
        for (int c = 0; c < kVespagOut; ++c) acc[c] = 0.0f;
        for (int k = lane; k < H; k += 64) {
            const float v = hr[k];
            const float a = v > 0.0f ? v : v * slope;                        // F.leaky_relu: max(0, x) + slope min(0, x)
#pragma unroll
            for (int c = 0; c < kVespagOut; ++c) acc[c] = __builtin_fmaf(a, w2s[c * H + k], acc[c]);
        }
        float mine = 0.0f;
#pragma unroll
        for (int c = 0; c < kVespagOut; ++c) {
            float s = acc[c];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
            if (lane == c) mine = s;
        }
        if (lane < kVespagOut) y[(size_t)row * kVespagOut + lane] = lane == wt_col[row] ? 0.0f : mine + b2[lane];
    }
}

}  // namespace

void launch_packed_scatter(const float* src, const int32_t* dst_row, int n, int D, float* out, int32_t* nonfinite, hipStream_t s) {
    hipLaunchKernelGGL(packed_scatter_kernel, dim3((n + 3) / 4), dim3(256), 0, s, src, dst_row, n, D, out, nonfinite);
}

void launch_vespag_head(const float* h, const float* W2, const float* b2, const int32_t* wt_col, int rows, int H, float slope, float* y,
                        hipStream_t s) {
    const size_t lds = (size_t)kVespagOut * H * sizeof(float);               // H <= 768 (vespag_check): at most 60 KiB
    hipLaunchKernelGGL(vespag_head_kernel, dim3((rows + kVespagRowsPerBlock - 1) / kVespagRowsPerBlock), dim3(256), lds, s, h, W2, b2, wt_col,
                       rows, H, slope, y);
}

}  // namespace pgmi
