// S3F kernels (include/pgmi.h, S3F section): the surface half of proteingym/baselines/S3F's SurfGVP.  The GVP-GNN over
// the surface graph runs on s2f.hip's row kernels and launch_gemm_f32; what is here is what the surface adds.
//
//   s3f_knn_kernel        brute-force k nearest candidates of every query point in fp32: one query per thread, the candidates in LDS
//                         tiles of 256, a sorted top-k in registers.  Candidates are visited in ascending index and a candidate only
//                         displaces a strictly farther one, so ties go to the lower index.  Two instantiations: surface -> surface
//                         (k = 16, the point itself left out, the list stored in ascending index: the edges of a centre) and surface ->
//                         C-alpha (k = 3, nearest first, with the distances).
//   s3f_edge_kernel       surf_W_e on every edge in double, one edge per thread: 16 RBFs of |p_j - p_i| over 0 .. 20, tuple LayerNorm
//                         (16, 1), GVP (16, 1) -> (64, 1) with the vector gate.  The edge vector is p_source - p_centre, the opposite of
//                         the residue graph's.
//   s3f_row_kernel        one surface point of one masked copy per block: the mean of its three residues' rows of Z plus the structure
//                         term T, LayerNorm(2 D) and ReLU, written as the operand row of the MLP's second Linear.
//   s3f_message_kernel    s2f_message_kernel for the fixed-degree graph: every point has exactly 16 incoming edges, so two points fill
//                         one 32-row tile and no MFMA row is padding (the residue kernel pads every node to 32).  One block per (copy,
//                         pair of points); the rows stay in LDS from the gather to the two sums, each over its point's 16 rows in
//                         ascending edge order.  No atomics, no per-edge activation in HBM.  With an odd point count the last tile's
//                         upper half repeats the last edge and is not summed.
//   s3f_colsum_*          the column sum of surf_W_out's rows (after its ReLU) of one copy in a fixed order: 64-row partial sums, then
//                         the partials in ascending order.  Neither depends on what else is in the launch.
//                         s2f_head_kernel (s2f.hip) adds the pooled row of a row's pool group from these sums.
#include <algorithm>

#include "s2f_tile.h"

namespace pgmi {

// ---- k-NN ----------------------------------------------------------------------------------------------------------------------
// q [nq][3], c [nc][3] with nc >= K (+ 1 when SKIP_SELF: q and c are then the same array).  idx [nq][K]; dist (nullable) [nq][K] = the
// distances (square roots).  BY_INDEX: the list in ascending index instead of nearest first.
template <int K, bool SKIP_SELF, bool BY_INDEX>
__global__ __launch_bounds__(256) void s3f_knn_kernel(const float* __restrict__ q, int nq, const float* __restrict__ c, int nc,
                                                      int32_t* __restrict__ idx, float* __restrict__ dist) {
    __shared__ float cs[256 * 3];
    const int tid = threadIdx.x;
    const int qi = blockIdx.x * 256 + tid, qc = min(qi, nq - 1);
    const float qx = q[(size_t)qc * 3], qy = q[(size_t)qc * 3 + 1], qz = q[(size_t)qc * 3 + 2];
    float bd[K];
    int bi[K];
#pragma unroll
    for (int k = 0; k < K; ++k) { bd[k] = INFINITY; bi[k] = 0; }
    for (int c0 = 0; c0 < nc; c0 += 256) {                      // block-uniform
        const int n = min(256, nc - c0);
        __syncthreads();
        for (int t = tid; t < n * 3; t += 256) cs[t] = c[(size_t)c0 * 3 + t];
        __syncthreads();
        for (int j = 0; j < n; ++j) {
            const float dx = qx - cs[3 * j], dy = qy - cs[3 * j + 1], dz = qz - cs[3 * j + 2];
            const float d = dx * dx + dy * dy + dz * dz;
            if (d < bd[K - 1] && !(SKIP_SELF && c0 + j == qc)) {
                bd[K - 1] = d;
                bi[K - 1] = c0 + j;
#pragma unroll
                for (int k = K - 1; k > 0; --k) {
                    const bool sw = bd[k] < bd[k - 1];
                    const float td = sw ? bd[k - 1] : bd[k];
                    const int ti = sw ? bi[k - 1] : bi[k];
                    bd[k - 1] = sw ? bd[k] : bd[k - 1];
                    bi[k - 1] = sw ? bi[k] : bi[k - 1];
                    bd[k] = td;
                    bi[k] = ti;
                }
            }
        }
    }
    if (BY_INDEX) {
#pragma unroll
        for (int pass = 0; pass < K - 1; ++pass)
#pragma unroll
            for (int k = 0; k < K - 1 - pass; ++k) {
                const bool sw = bi[k + 1] < bi[k];
                const int ti = sw ? bi[k] : bi[k + 1];
                const float td = sw ? bd[k] : bd[k + 1];
                bi[k] = sw ? bi[k + 1] : bi[k];
                bd[k] = sw ? bd[k + 1] : bd[k];
                bi[k + 1] = ti;
                bd[k + 1] = td;
            }
    }
    if (qi < nq) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            idx[(size_t)qi * K + k] = bi[k];
            if (dist) dist[(size_t)qi * K + k] = sqrtf(bd[k]);
        }
    }
}

// ---- surf_W_e ------------------------------------------------------------------------------------------------------------------
constexpr int S3F_WE = 32 + 1 + 64 * 17 + 64 + 1 + 64 + 1;      // surf_W_e's tensors in blob order: LayerNorm, wh, ws + b, wv, wsv + b

// edge e = (src[e] -> e / 16); es [E][64], ev [E][3]
__global__ __launch_bounds__(256) void s3f_edge_kernel(const float* __restrict__ pos, const int32_t* __restrict__ src, int64_t E,
                                                       const float* __restrict__ we, float* __restrict__ es, float* __restrict__ ev) {
    __shared__ float w[S3F_WE];
    for (int t = threadIdx.x; t < S3F_WE; t += 256) w[t] = we[t];
    __syncthreads();
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const float *lnw = w, *lnb = w + 16, *wh = w + 32, *ws = w + 33, *bs = ws + 64 * 17, *wv = bs + 64, *wsv = wv + 1, *bsv = wsv + 64;
    const int64_t i = e / S3F_DEG, j = src[e];
    double vec[3], d2 = 0.0;
    for (int c = 0; c < 3; ++c) { vec[c] = (double)pos[3 * j + c] - (double)pos[3 * i + c]; d2 += vec[c] * vec[c]; }
    const double d = sqrt(d2);
    double f[17], mean = 0.0, var = 0.0;
    const float step = 20.0f / 15.0f;                           // torch.linspace(0, 20, 16) in float32, as s2f_edge_embed has it
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const float mu = k < 8 ? step * (float)k : 20.0f - step * (float)(15 - k);
        const double z = (d - (double)mu) / 1.25;
        f[k] = exp(-z * z);
        mean += f[k];
    }
    mean /= 16.0;
#pragma unroll
    for (int k = 0; k < 16; ++k) var += (f[k] - mean) * (f[k] - mean);
    const double rstd = 1.0 / sqrt(var / 16.0 + 1e-5);
#pragma unroll
    for (int k = 0; k < 16; ++k) f[k] = (f[k] - mean) * rstd * lnw[k] + lnb[k];
    const double vden = sqrt(fmax(d2, 1e-8));
    double vh[3], n2 = 0.0;
    for (int c = 0; c < 3; ++c) { vh[c] = (double)wh[0] * (vec[c] / vden); n2 += vh[c] * vh[c]; }
    f[16] = sqrt(fmax(n2, 1e-8));
    double gate = bsv[0];
    for (int n = 0; n < 64; ++n) {
        double a = bs[n];
#pragma unroll
        for (int k = 0; k < 17; ++k) a += (double)ws[n * 17 + k] * f[k];
        es[e * 64 + n] = (float)a;
        gate += (double)wsv[n] * a;
    }
    const double sg = 1.0 / (1.0 + exp(-gate));
    for (int c = 0; c < 3; ++c) ev[e * 3 + c] = (float)((double)wv[0] * vh[c] * sg);
}

// ---- surface MLP row -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float s3f_block_sum(float x, float* red) {     // the four wave sums added in wave order
    x = s2f_wave_sum(x);
    __syncthreads();                                            // red is free
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// grid = B Ns.  Z [B L][H]; T [Ns][H]; res [Ns][3]; out [B Ns][H] = relu(LayerNorm(((Z[r0] + Z[r1]) + Z[r2]) / 3 + T[p])); H floats of
// dynamic LDS hold the row between the passes.
__global__ __launch_bounds__(256) void s3f_row_kernel(const float* __restrict__ Z, const float* __restrict__ T, const int32_t* __restrict__ res,
                                                      const float* __restrict__ lnw, const float* __restrict__ lnb, int L, int Ns, int H,
                                                      float* __restrict__ out) {
    extern __shared__ float xrow[];
    __shared__ float red[4];
    const int tid = threadIdx.x;
    const int64_t r = blockIdx.x, b = r / Ns;
    const int p = (int)(r - b * Ns);
    const float* z0 = Z + (b * L + res[3 * p]) * H;
    const float* z1 = Z + (b * L + res[3 * p + 1]) * H;
    const float* z2 = Z + (b * L + res[3 * p + 2]) * H;
    const float* t = T + (size_t)p * H;
    float sum = 0.0f;
    for (int c = tid; c < H; c += 256) {
        const float x = ((z0[c] + z1[c]) + z2[c]) / 3.0f + t[c];
        xrow[c] = x;
        sum += x;
    }
    const float mean = s3f_block_sum(sum, red) / (float)H;
    float var = 0.0f;
    for (int c = tid; c < H; c += 256) {                        // a thread reads back the columns it wrote
        const float x = xrow[c] - mean;
        var += x * x;
    }
    const float rstd = 1.0f / sqrtf(s3f_block_sum(var, red) / (float)H + 1e-5f);
    for (int c = tid; c < H; c += 256) out[r * H + c] = fmaxf((xrow[c] - mean) * rstd * lnw[c] + lnb[c], 0.0f);
}

// ---- fused message kernel of the fixed-degree graph (the tile, its LDS, the gather and the GVP stages: s2f_tile.h) ------------------
static_assert(FE_M == 2 * S3F_DEG, "a tile holds the edges of two points");
// grid = B tiles, tiles = ceil(Ns / 2).  Operands as s2f_message_kernel's, with src [Ns][16] (the sources of a centre in ascending
// index) in place of the CSR.  ds [B Ns][256], dv [B Ns][16][3] = the mean message.
__global__ __launch_bounds__(256, 2) void s3f_message_kernel(const float* __restrict__ P, const float* __restrict__ VT,
                                                             const float* __restrict__ Es, const float* __restrict__ ev,
                                                             const float* __restrict__ whe, const float* __restrict__ Wnt, const S2fMsgWeights w,
                                                             const int32_t* __restrict__ src, int Ns, int tiles, float* __restrict__ ds,
                                                             float* __restrict__ dv) {
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x / tiles;
    const int p0 = 2 * (int)(blockIdx.x - b * tiles);
    const int64_t nb = b * Ns;
    fe_tile<true>(P, VT, Es, ev, whe, Wnt, w, src, nb, p0 * S3F_DEG, Ns * S3F_DEG - 1, p0, min(p0 + 1, Ns - 1));
    const int np = min(2, Ns - p0);
    for (int q = 0; q < np; ++q) {
        float sum_s = 0.0f, sum_v = 0.0f;
        for (int row = q * S3F_DEG; row < (q + 1) * S3F_DEG; ++row) {
            sum_s += fe_As[row * FE_LDA + tid];
            if (tid < SV * 3) sum_v += fe_Vh[row * FE_LDV + tid];
        }
        const int64_t node = nb + p0 + q;
        ds[node * SS + tid] = sum_s / (float)S3F_DEG;
        if (tid < SV * 3) dv[node * (SV * 3) + tid] = sum_v / (float)S3F_DEG;
    }
}

// ---- pooled row ----------------------------------------------------------------------------------------------------------------
constexpr int S3F_SUM_ROWS = 64;
// grid (nblk, B): part [B][nblk][256] = the sum of rows [64 blk, 64 blk + 64) of relu(copy b's x [Ns][256]), in ascending row order
__global__ __launch_bounds__(256) void s3f_colsum_part_kernel(const float* __restrict__ x, int Ns, int nblk, float* __restrict__ part) {
    const int64_t b = blockIdx.y;
    const int r0 = blockIdx.x * S3F_SUM_ROWS, r1 = min(r0 + S3F_SUM_ROWS, Ns);
    float a = 0.0f;
    for (int r = r0; r < r1; ++r) a += fmaxf(x[(b * Ns + r) * SS + threadIdx.x], 0.0f);
    part[(b * nblk + blockIdx.x) * SS + threadIdx.x] = a;
}
// grid B: sums [B][256] = the partials in ascending order
__global__ __launch_bounds__(256) void s3f_colsum_final_kernel(const float* __restrict__ part, int nblk, float* __restrict__ sums) {
    const int64_t b = blockIdx.x;
    float a = 0.0f;
    for (int k = 0; k < nblk; ++k) a += part[(b * nblk + k) * SS + threadIdx.x];
    sums[b * SS + threadIdx.x] = a;
}

// ---- launchers -----------------------------------------------------------------------------------------------------------------
int launch_s3f_knn(const float* q, int nq, const float* c, int nc, int k, int32_t* idx, float* dist, hipStream_t s) {
    const dim3 grid((unsigned)((nq + 255) / 256)), block(256);
    if (nq < 1 || !((k == 16 && q == c && nc >= 17 && !dist) || (k == 3 && q != c && nc >= 3))) {
        set_error("s3f: k-NN of %d points among %d with k = %d is not one this kernel runs", nq, nc, k);
        return PGMI_EINVAL;
    }
    if (k == 16) hipLaunchKernelGGL((s3f_knn_kernel<16, true, true>), grid, block, 0, s, q, nq, c, nc, idx, dist);
    else hipLaunchKernelGGL((s3f_knn_kernel<3, false, false>), grid, block, 0, s, q, nq, c, nc, idx, dist);
    return PGMI_OK;
}

void launch_s3f_edges(const float* pos, const int32_t* src, int Ns, const float* we, float* es, float* ev, hipStream_t s) {
    const int64_t E = (int64_t)Ns * S3F_DEG;
    hipLaunchKernelGGL(s3f_edge_kernel, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, s, pos, src, E, we, es, ev);
}

int launch_s3f_rows(const float* Z, const float* T, const int32_t* res, const float* lnw, const float* lnb, int L, int Ns, int H, int64_t rows,
                    float* out, hipStream_t s) {
    if (H < 64 || H > 8192 || rows < 1 || rows % Ns || rows > 0x7fffffffLL) {
        set_error("s3f: surface MLP rows=%lld Ns=%d H=%d is not a shape this kernel runs", (long long)rows, Ns, H);
        return PGMI_EINVAL;
    }
    hipLaunchKernelGGL(s3f_row_kernel, dim3((unsigned)rows), dim3(256), (size_t)H * sizeof(float), s, Z, T, res, lnw, lnb, L, Ns, H, out);
    return PGMI_OK;
}

int launch_s3f_message(const float* P, const float* VT, const float* Es, const float* ev, const float* whe, const float* Wnt,
                       const S2fMsgWeights& w, const int32_t* src, int Ns, int64_t nodes, float* ds, float* dv, hipStream_t s) {
    const int64_t tiles = ((int64_t)Ns + 1) / 2;
    if (w.ldw < FE_K || w.ldw % 4 || Ns < S3F_DEG + 1 || Ns > (1 << 20) || nodes < Ns || nodes % Ns || nodes / Ns * tiles > 0x7fffffffLL) {
        set_error("s3f: message stage ldw=%d Ns=%d nodes=%lld is not one this kernel runs", w.ldw, Ns, (long long)nodes);
        return PGMI_EINVAL;
    }
    hipLaunchKernelGGL(s3f_message_kernel, dim3((unsigned)(nodes / Ns * tiles)), dim3(256), 0, s, P, VT, Es, ev, whe, Wnt, w, src, Ns, (int)tiles,
                       ds, dv);
    return PGMI_OK;
}

int s3f_colsum_blocks(int Ns) { return (Ns + S3F_SUM_ROWS - 1) / S3F_SUM_ROWS; }

void launch_s3f_colsum(const float* x, int Ns, int copies, float* part, float* sums, hipStream_t s) {
    const int nblk = s3f_colsum_blocks(Ns);
    hipLaunchKernelGGL(s3f_colsum_part_kernel, dim3((unsigned)nblk, (unsigned)copies), dim3(256), 0, s, x, Ns, nblk, part);
    hipLaunchKernelGGL(s3f_colsum_final_kernel, dim3((unsigned)copies), dim3(256), 0, s, part, nblk, sums);
}

}  // namespace pgmi
