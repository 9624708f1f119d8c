// ProtSSN's EGNN layer around its four GEMMs (the layer is proteingym/baselines/protssn/src/module/egnn/
// egnn_pytorch_geometric.py EGNN_Sparse with mlp_num 2, no coordinate update, no norms).  The GEMMs stay on launch_gemm_f32 /
// launch_gemm16 (api_protssn.hip); these kernels write their operands and read their outputs.
//   egnn_edge_rows_kernel   per edge (centre c, neighbour n): SiLU(Pi[n] + Pj[c] + S[e]) -> the W2 product's operand row.  P [L][2 Hp]
//                           holds the per-node tables x Wi^T | x Wj^T of the first edge Linear, S [edges][Hp] the edge share
//                           e We^T + b1: the 2654-wide concatenation of the reference is never formed.  Pad columns (Hp - 5308) are
//                           0 + 0 + 0 and SiLU(0) = 0.
//   egnn_aggregate_kernel   per node i: [x_i | sum over the edges whose neighbour is i, in ascending edge order, of SiLU(msg[e])] ->
//                           the W3 product's operand row.  A CSR by target (built on the host with a stable sort) gives the order, one
//                           thread owns an element: no atomics, and a node nobody selects gets zeros.
//   egnn_silu_rows_kernel   SiLU between W3 and W4 -> the W4 product's operand (fp32 mode; f16x3 uses moe.hip's launch_silu_split)
//   egnn_head_kernel        Linear(D, 20), softmax, log(p + 1e-9) in fp32, one wave per node
// Operand rows are the K-interleaved split planes of common.h (f16x3) or fp32 rows.  Every kernel is element- or row-local, so a
// row's bits do not depend on how many rows a launch has.
#include "common.h"

namespace pgmi {

namespace {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ float egnn_silu(float z) { return z / (1.0f + expf(-z)); }

// eight consecutive columns c .. c + 7 (c % 8 == 0) of operand row `row` of K columns
template <bool SPLIT>
__device__ __forceinline__ void egnn_store8(void* out, size_t row, int c, int K, const float (&v)[8]) {
    if (SPLIT) {
        h8 hi, lo;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            _Float16 a, b;
            split_act(v[k], a, b);
            hi[k] = a;
            lo[k] = b;
        }
        unsigned short* dst = static_cast<unsigned short*>(out) + ki_off(row, c, K);
        *reinterpret_cast<h8*>(dst) = hi;
        *reinterpret_cast<h8*>(dst + 32) = lo;
    } else {
        f32x4* dst = reinterpret_cast<f32x4*>(static_cast<float*>(out) + row * (size_t)K + c);
        dst[0] = f32x4{v[0], v[1], v[2], v[3]};
        dst[1] = f32x4{v[4], v[5], v[6], v[7]};
    }
}

__device__ __forceinline__ void egnn_load8(const float* p, float (&v)[8]) {
    const f32x4 a = reinterpret_cast<const f32x4*>(p)[0], b = reinterpret_cast<const f32x4*>(p)[1];
#pragma unroll
    for (int k = 0; k < 4; ++k) { v[k] = a[k]; v[4 + k] = b[k]; }
}

// one thread per (edge, 8 columns); n8 = edges * Hp / 8
template <bool SPLIT>
__global__ __launch_bounds__(256) void egnn_edge_rows_kernel(const float* __restrict__ P, const float* __restrict__ S,
                                                             const int32_t* __restrict__ centre, const int32_t* __restrict__ nb, int64_t n8,
                                                             int Hp, void* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n8) return;
    const int h8n = Hp / 8;
    const int64_t e = i / h8n;
    const int c = (int)(i % h8n) * 8;
    float a[8], b[8], s[8], v[8];
    egnn_load8(P + (size_t)nb[e] * 2 * Hp + c, a);                  // x_i = x[edge_index[1]]: the neighbour's Wi row
    egnn_load8(P + (size_t)centre[e] * 2 * Hp + Hp + c, b);         // x_j = x[edge_index[0]]: the centre's Wj row
    egnn_load8(S + (size_t)e * Hp + c, s);
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = egnn_silu(__fadd_rn(__fadd_rn(a[k], b[k]), s[k]));
    egnn_store8<SPLIT>(out, (size_t)e, c, Hp, v);
}

// one thread per (node, 8 columns of K = D + hp); n8 = L * K / 8
template <bool SPLIT>
__global__ __launch_bounds__(256) void egnn_aggregate_kernel(const float* __restrict__ x, const float* __restrict__ msg,
                                                             const int32_t* __restrict__ off, const int32_t* __restrict__ eid, int64_t n8, int D,
                                                             int hp, void* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n8) return;
    const int K = D + hp, k8n = K / 8;
    const int64_t node = i / k8n;
    const int c = (int)(i % k8n) * 8;
    float v[8];
    if (c < D) {
        egnn_load8(x + (size_t)node * D + c, v);
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = 0.0f;
        const int j1 = off[node + 1];
        for (int j = off[node]; j < j1; ++j) {
            float t[8];
            egnn_load8(msg + (size_t)eid[j] * hp + (c - D), t);
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = __fadd_rn(v[k], egnn_silu(t[k]));
        }
    }
    egnn_store8<SPLIT>(out, (size_t)node, c, K, v);
}

__global__ __launch_bounds__(256) void egnn_silu_rows_kernel(const float* __restrict__ t, int64_t n8, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n8) return;
    float v[8];
    egnn_load8(t + i * 8, v);
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = egnn_silu(v[k]);
    egnn_store8<false>(out, (size_t)i, 0, 8, v);
}

// one wave per node: logits = W x + b over 20 columns, then log(softmax + 1e-9)
__global__ __launch_bounds__(256) void egnn_head_kernel(const float* __restrict__ x, const float* __restrict__ W, const float* __restrict__ bias,
                                                        int rows, int D, float* __restrict__ lp) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* xr = x + (size_t)row * D;
    float logit[20];
#pragma unroll
    for (int c = 0; c < 20; ++c) {
        float acc = 0.0f;
        for (int k = lane; k < D; k += 64) acc = __builtin_fmaf(xr[k], W[(size_t)c * D + k], acc);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
        logit[c] = acc + bias[c];
    }
    float mx = logit[0];
#pragma unroll
    for (int c = 1; c < 20; ++c) mx = fmaxf(mx, logit[c]);
    float sum = 0.0f, ex[20];
#pragma unroll
    for (int c = 0; c < 20; ++c) { ex[c] = expf(logit[c] - mx); sum += ex[c]; }
    float mine = 0.0f;
#pragma unroll
    for (int c = 0; c < 20; ++c)
        if (lane == c) mine = logf(ex[c] / sum + 1e-9f);
    if (lane < 20) lp[(size_t)row * 20 + lane] = mine;
}

inline unsigned egnn_blocks(int64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

void launch_egnn_edge_rows(const float* P, const float* S, const int32_t* centre, const int32_t* nb, int edges, int Hp, bool split, void* out,
                           hipStream_t s) {
    const int64_t n8 = (int64_t)edges * (Hp / 8);
    if (split) hipLaunchKernelGGL(egnn_edge_rows_kernel<true>, dim3(egnn_blocks(n8)), dim3(256), 0, s, P, S, centre, nb, n8, Hp, out);
    else hipLaunchKernelGGL(egnn_edge_rows_kernel<false>, dim3(egnn_blocks(n8)), dim3(256), 0, s, P, S, centre, nb, n8, Hp, out);
}

void launch_egnn_aggregate(const float* x, const float* msg, const int32_t* off, const int32_t* eid, int L, int D, int hp, bool split, void* out,
                           hipStream_t s) {
    const int64_t n8 = (int64_t)L * ((D + hp) / 8);
    if (split) hipLaunchKernelGGL(egnn_aggregate_kernel<true>, dim3(egnn_blocks(n8)), dim3(256), 0, s, x, msg, off, eid, n8, D, hp, out);
    else hipLaunchKernelGGL(egnn_aggregate_kernel<false>, dim3(egnn_blocks(n8)), dim3(256), 0, s, x, msg, off, eid, n8, D, hp, out);
}

void launch_egnn_silu_rows(const float* t, int rows, int F, float* out, hipStream_t s) {
    const int64_t n8 = (int64_t)rows * (F / 8);
    hipLaunchKernelGGL(egnn_silu_rows_kernel, dim3(egnn_blocks(n8)), dim3(256), 0, s, t, n8, out);
}

void launch_egnn_head(const float* x, const float* W, const float* bias, int rows, int D, float* lp, hipStream_t s) {
    hipLaunchKernelGGL(egnn_head_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, x, W, bias, rows, D, lp);
}

}  // namespace pgmi
