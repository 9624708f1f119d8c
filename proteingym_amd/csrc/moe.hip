// Routed mixture-of-experts block (ProGen3: proteingym/baselines/progen3/progen3/model/moe.py SparseMoeBlock): everything around the
// per-expert GEMMs, which stay on launch_gemm16 (api_progen3.hip moe_ffn).
//   rmsnorm_route_kernel  the layer's second RMSNorm (elementwise.hip rmsnorm16_kernel's arithmetic and operand layout) and, with the
//                         normalised row still in registers, the router: E logits against the fp32 gate, softmax over the
//                         experts, top-k, renormalise.  One wave per row; lane e owns expert e (E <= 64).
//   moe_count / moe_offsets / moe_slots   the token -> expert permutation without atomics: per block of 1024 (row, k) entries the count
//                         per expert (ballots), an exclusive scan over the blocks per expert, segment offsets padded to the GEMM's row
//                         tile, and every entry's slot.  The order inside an expert's segment is the entries' own order (row, k): stable.
//   moe_gather_kernel     the split rows copied into their slots (expert-contiguous segments)
//   moe_combine_kernel    x[row] += sum over k = 0 .. top_k-1 of weight_k * y[slot(row, k)], fp32, in that order, one owner per element
//   silu_split_kernel     non-gated experts: silu of FC1's fp32 rows -> the split operand of FC2
// Rows whose token is <pad> are not routed: their entries carry expert -1, take no slot and are skipped by the combine.
#include "common.h"

namespace pgmi {

namespace {

__device__ __forceinline__ float moe_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float moe_wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ double moe_wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// One wave per row, 4 rows per block; a lane holds the f32x4 groups lane + 64 i of the row (as layernorm_kernel).  w == nullptr: no
// normalisation (the rows are taken as given: pgmi_op_moe).  y16 == nullptr: no operand is written.  gate != nullptr: the router.
//
// Router arithmetic: the reference forms the logits with an fp32 GEMM, whose summation order is the BLAS's own; here every product
// o[c] * gate[e][c] is exact in double and the sum is carried in double, so the fp32 logit is the correctly rounded dot product of
// the fp32 operands up to one rounding -- as close to any fp32 summation order as an order-free result can be.  Softmax, the
// division by the sum of the chosen weights and the weights are fp32 as in the reference.  Top-k: the largest probability, ties to the
// lower expert index, k times.
template <int NV>
__global__ __launch_bounds__(256) void rmsnorm_route_kernel(const float* __restrict__ x, const float* __restrict__ w, int rows, int D,
                                                            float eps, unsigned short* __restrict__ y16,
                                                            const float* __restrict__ gate, int E, int top_k,
                                                            const int32_t* __restrict__ tokens, int pad_id,
                                                            int32_t* __restrict__ ids, float* __restrict__ wts) {
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
    if (w) {
        const float rstd = 1.0f / sqrtf(moe_wave_sum(q) / (float)D + eps);
        const f32x4* wr = reinterpret_cast<const f32x4*>(w);
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int c = lane + 64 * i;
            if (c < nv) {
                const f32x4 wv = wr[c];
#pragma unroll
                for (int k = 0; k < 4; ++k) v[i][k] = v[i][k] * rstd * wv[k];
            }
        }
    }
    if (y16) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int c = lane + 64 * i;
            if (c < nv) store_split4(v[i], y16, (size_t)row, c, lane, D);      // D % 8 == 0: a lane and its neighbour are in the row together
        }
    }
    if (!gate) return;
    if (tokens && tokens[row] == pad_id) {                     // a padding row: routed nowhere
        if (lane < top_k) { ids[(size_t)row * top_k + lane] = -1; wts[(size_t)row * top_k + lane] = 0.0f; }
        return;
    }
    float logit = -INFINITY;                                   // lane e: expert e's logit; lanes >= E stay out of every reduction
    for (int e = 0; e < E; ++e) {
        const f32x4* gr = reinterpret_cast<const f32x4*>(gate + (size_t)e * D);
        double acc = 0.0;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int c = lane + 64 * i;
            if (c < nv) {
                const f32x4 gv = gr[c];
#pragma unroll
                for (int k = 0; k < 4; ++k) acc += (double)v[i][k] * (double)gv[k];
            }
        }
        acc = moe_wave_sum_d(acc);
        if (lane == e) logit = (float)acc;
    }
    const float mx = moe_wave_max(logit);
    const float ex = lane < E ? expf(logit - mx) : 0.0f;
    float p = ex / moe_wave_sum(ex);
    if (lane >= E) p = -1.0f;
    float chosen_w = 0.0f, wsum = 0.0f;                         // lane j < top_k keeps the j-th choice
    int chosen_e = -1;
    for (int j = 0; j < top_k; ++j) {
        const float best = moe_wave_max(p);
        const unsigned long long tie = __ballot(p == best);
        const int e = __ffsll((long long)tie) - 1;              // ties: the lower expert index
        if (lane == j) { chosen_e = e; chosen_w = best; }
        wsum += best;                                           // k = 0, 1, ...: the order of sum(dim=-1) over the top-k values
        if (lane == e) p = -1.0f;
    }
    if (lane < top_k) {
        ids[(size_t)row * top_k + lane] = chosen_e;
        wts[(size_t)row * top_k + lane] = chosen_w / wsum;
    }
}

constexpr int kMoeBlock = 1024;                                 // (row, k) entries per block of the permutation kernels
constexpr int kMoeWaves = kMoeBlock / kWave;

// cnt[blk][e] = entries of block blk routed to expert e
__global__ __launch_bounds__(kMoeBlock) void moe_count_kernel(const int32_t* __restrict__ ids, int n, int E, int32_t* __restrict__ cnt) {
    __shared__ int32_t wc[kMoeWaves][kWave];
    const int j = blockIdx.x * kMoeBlock + threadIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int id = j < n ? ids[j] : -1;
    for (int e = 0; e < E; ++e) {
        const int c = __popcll(__ballot(id == e));
        if (lane == e) wc[wave][e] = c;
    }
    __syncthreads();
    if (threadIdx.x < E) {
        int s = 0;
        for (int wv = 0; wv < kMoeWaves; ++wv) s += wc[wv][threadIdx.x];
        cnt[(size_t)blockIdx.x * E + threadIdx.x] = s;
    }
}

// One block of 64 threads, thread e: base[blk][e] = entries of expert e in blocks before blk; counts[e]; seg[e] = first slot of expert e,
// seg[0] = 0 and every segment start a multiple of `tile` (seg[E] = the padded total).  counts | seg go out in one array [2 E + 1].
__global__ void moe_offsets_kernel(const int32_t* __restrict__ cnt, int nblk, int E, int tile, int32_t* __restrict__ base,
                                   int32_t* __restrict__ counts_seg) {
    __shared__ int32_t tot[kWave];
    const int e = threadIdx.x;
    if (e < E) {
        int s = 0;
        for (int b = 0; b < nblk; ++b) {
            base[(size_t)b * E + e] = s;
            s += cnt[(size_t)b * E + e];
        }
        tot[e] = s;
        counts_seg[e] = s;
    }
    __syncthreads();
    if (e == 0) {
        int o = 0;
        for (int i = 0; i < E; ++i) {
            counts_seg[E + i] = o;
            o += (tot[i] + tile - 1) / tile * tile;
        }
        counts_seg[2 * E] = o;
    }
}

// slot[j] = seg[e] + base[blk][e] + (entries of e before j inside the block), -1 for an unrouted entry
__global__ __launch_bounds__(kMoeBlock) void moe_slots_kernel(const int32_t* __restrict__ ids, int n, int E,
                                                              const int32_t* __restrict__ base, const int32_t* __restrict__ counts_seg,
                                                              int32_t* __restrict__ slot) {
    __shared__ int32_t wc[kMoeWaves][kWave];
    const int j = blockIdx.x * kMoeBlock + threadIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int id = j < n ? ids[j] : -1;
    int rank = 0;
    for (int e = 0; e < E; ++e) {
        const unsigned long long b = __ballot(id == e);
        if (lane == e) wc[wave][e] = __popcll(b);
        if (id == e) rank = __popcll(b & ((1ull << lane) - 1ull));
    }
    __syncthreads();
    if (j >= n) return;
    if (id < 0) { slot[j] = -1; return; }
    int before = 0;
    for (int wv = 0; wv < wave; ++wv) before += wc[wv][id];
    slot[j] = counts_seg[E + id] + base[(size_t)blockIdx.x * E + id] + before + rank;
}

// a16[slot[j]] = h16[j / top_k]: rows of 2 D halfs (4 D bytes, a multiple of 128), one wave per entry, 16 bytes per lane and step
__global__ __launch_bounds__(256) void moe_gather_kernel(const unsigned short* __restrict__ h16, const int32_t* __restrict__ slot, int n,
                                                         int top_k, int D, unsigned short* __restrict__ a16) {
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (j >= n) return;
    const int s = slot[j];
    if (s < 0) return;
    const u32x4* src = reinterpret_cast<const u32x4*>(h16 + (size_t)(j / top_k) * 2 * D);
    u32x4* dst = reinterpret_cast<u32x4*>(a16 + (size_t)s * 2 * D);
    const int nq = D / 4;                                       // 16-byte pieces of a row
    for (int c = lane; c < nq; c += 64) dst[c] = src[c];
}

// x[row] += sum_k wts[row][k] * y[slot[row][k]]: products and sums rounded one by one (no contraction), k = 0 first
__global__ __launch_bounds__(256) void moe_combine_kernel(const float* __restrict__ y, const int32_t* __restrict__ slot,
                                                          const float* __restrict__ wts, int rows, int top_k, int D,
                                                          float* __restrict__ x) {
    const int nv = D >> 2;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)rows * nv) return;
    const int row = (int)(i / nv), c = (int)(i % nv);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    bool any = false;
    for (int k = 0; k < top_k; ++k) {
        const int s = slot[(size_t)row * top_k + k];
        if (s < 0) continue;                                    // an unrouted entry (a <pad> row) adds nothing
        const float wk = wts[(size_t)row * top_k + k];
        const f32x4 yv = reinterpret_cast<const f32x4*>(y + (size_t)s * D)[c];
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = any ? __fadd_rn(acc[q], __fmul_rn(yv[q], wk)) : __fmul_rn(yv[q], wk);
        any = true;
    }
    if (!any) return;                                           // the row keeps x
    f32x4* xr = reinterpret_cast<f32x4*>(x + (size_t)row * D) + c;
    f32x4 xv = *xr;
#pragma unroll
    for (int q = 0; q < 4; ++q) xv[q] = __fadd_rn(xv[q], acc[q]);
    *xr = xv;
}

// g16[r] = split(silu(t[r])), rows of F columns; one thread per 8 columns (16 bytes of hi, 16 bytes of lo)
__global__ __launch_bounds__(256) void silu_split_kernel(const float* __restrict__ t, int64_t n8, int F, unsigned short* __restrict__ g16) {
    typedef _Float16 h8 __attribute__((ext_vector_type(8)));
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n8) return;
    const int f8 = F / 8;
    const int64_t row = i / f8;
    const int c = (int)(i % f8) * 8;
    const f32x4* src = reinterpret_cast<const f32x4*>(t + row * F + c);
    const f32x4 a = src[0], b = src[1];
    h8 hi, lo;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float z = k < 4 ? a[k] : b[k - 4];
        const float sv = z / (1.0f + expf(-z));
        _Float16 h, l;
        split_act(sv, h, l);
        hi[k] = h;
        lo[k] = l;
    }
    unsigned short* dst = g16 + ki_off((size_t)row, c, F);
    *reinterpret_cast<h8*>(dst) = hi;
    *reinterpret_cast<h8*>(dst + 32) = lo;
}

template <typename... Args>
void launch_route_nv(int nv, dim3 grid, hipStream_t s, Args... a) {
    if (nv <= 1) hipLaunchKernelGGL((rmsnorm_route_kernel<1>), grid, dim3(256), 0, s, a...);
    else if (nv <= 2) hipLaunchKernelGGL((rmsnorm_route_kernel<2>), grid, dim3(256), 0, s, a...);
    else if (nv <= 5) hipLaunchKernelGGL((rmsnorm_route_kernel<5>), grid, dim3(256), 0, s, a...);
    else if (nv <= 10) hipLaunchKernelGGL((rmsnorm_route_kernel<10>), grid, dim3(256), 0, s, a...);
    else hipLaunchKernelGGL((rmsnorm_route_kernel<20>), grid, dim3(256), 0, s, a...);
}

}  // namespace

int launch_rmsnorm_route(const float* x, const float* w, int rows, int D, float eps, unsigned short* y16, const MoeRoute& r,
                         hipStream_t s) {
    // a lane holds at most 20 f32x4 groups (D <= 5120), pairs of lanes write 8-column groups of the K-interleaved operand
    if (rows <= 0 || D <= 0 || D % 32 || D > 5120) { set_error("rmsnorm: D = %d must be a multiple of 32, at most 5120", D); return PGMI_EINVAL; }
    if (r.gate && (r.E < 2 || r.E > kWave || r.top_k < 1 || r.top_k > r.E || !r.ids || !r.wts)) {
        set_error("router: %d experts, top-%d: this build routes 2 .. 64 experts, top_k <= experts", r.E, r.top_k);
        return PGMI_EINVAL;
    }
    launch_route_nv((D / 4 + 63) / 64, dim3((rows + 3) / 4), s, x, w, rows, D, eps, y16, r.gate, r.E, r.top_k, r.tokens, r.pad_id, r.ids, r.wts);
    return PGMI_OK;
}

int moe_perm_blocks(int n_entries) { return (n_entries + kMoeBlock - 1) / kMoeBlock; }

void launch_moe_permute(const int32_t* ids, int n_entries, int E, int tile, int32_t* blk_cnt, int32_t* blk_base, int32_t* counts_seg,
                        int32_t* slot, hipStream_t s) {
    const int nblk = moe_perm_blocks(n_entries);
    hipLaunchKernelGGL(moe_count_kernel, dim3(nblk), dim3(kMoeBlock), 0, s, ids, n_entries, E, blk_cnt);
    hipLaunchKernelGGL(moe_offsets_kernel, dim3(1), dim3(kWave), 0, s, blk_cnt, nblk, E, tile, blk_base, counts_seg);
    hipLaunchKernelGGL(moe_slots_kernel, dim3(nblk), dim3(kMoeBlock), 0, s, ids, n_entries, E, blk_base, counts_seg, slot);
}

void launch_moe_gather(const unsigned short* h16, const int32_t* slot, int n_entries, int top_k, int D, unsigned short* a16, hipStream_t s) {
    hipLaunchKernelGGL(moe_gather_kernel, dim3((n_entries + 3) / 4), dim3(256), 0, s, h16, slot, n_entries, top_k, D, a16);
}

void launch_moe_combine(const float* y, const int32_t* slot, const float* wts, int rows, int top_k, int D, float* x, hipStream_t s) {
    const int64_t n = (int64_t)rows * (D / 4);
    hipLaunchKernelGGL(moe_combine_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, y, slot, wts, rows, top_k, D, x);
}

void launch_silu_split(const float* t, int rows, int F, unsigned short* g16, hipStream_t s) {
    const int64_t n8 = (int64_t)rows * (F / 8);
    hipLaunchKernelGGL(silu_split_kernel, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, s, t, n8, F, g16);
}

}  // namespace pgmi
