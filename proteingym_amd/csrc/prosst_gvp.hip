// ProSST structure-quantizer kernels (include/pgmi.h, ProSST section): the GVP-GNN of proteingym/baselines/prosst's
// AutoGraphEncoder at node (256, 32), edge (64, 2), no vector gates, activations (relu, sigmoid of the channel norm); fp32 only.
// A row is a node copy (node q of anchor i's subgraph) or an edge; every kernel works row by row and reads nothing of a row that is not
// an operand of it, so a subgraph's bits do not depend on what else is in the launch.  The dense Linears between the kernels are
// launch_gemm_f32 (api_prosst.hip).
//
//   prosst_message_kernel   the three message GVPs of a layer on a tile of 32 edge rows that lives in LDS from the gather to the store.
//                           The first GVP is linear in [s_j | e_s | s_i] and [v_j | e_v | v_i] before its norm: a row gathers the
//                           per-node products (P = s [Wj | Wi]^T, VT = [wh_j v | wh_i v]) and the edge's share (Es = We e_s + b from the
//                           structure pass, wh_e e_v on the fly), takes the 66 channel norms and adds Wn |vh|.  The two 288 -> 256
//                           GVPs run on v_mfma_f32_16x16x4_f32 with their weights read from L2.  Tiles are cut from the edge list, not
//                           from a node's edges, so every tile but the last is full whatever the in-degree; the messages [rows][352] go
//                           to memory once and prosst_aggregate_kernel sums a node copy's rows in ascending order (no atomics).
//   prosst_aggregate_kernel the mean of a node copy's messages: rows off[r] .. off[r + 1], either themselves or, for the shared layer
//                           0, the global edges they name.
//   prosst_node_ln_kernel   (s, v) + dh -> tuple LayerNorm.
//   prosst_vtab_kernel      wh v of a GVP for every row, and with outA its channel norms behind the row's scalars: the GVP's GEMM operand.
//   prosst_gvp_mid_kernel   the vector half of a feed-forward GVP after its ws GEMM: v = wv vh, the ungated vector non-linearity,
//                           relu on s; then the NEXT GVP's wh v and norms.
//   prosst_pool_kernel      relu, the mean over a subgraph's node copies, the L2 normalisation.
//   prosst_centre_norms / prosst_argmin   |c|^2 per centre; argmin_k |c_k|^2 - 2 x.c_k with the lowest index on a tie.
#include <algorithm>

#include "prosst_impl.h"

namespace pgmi {

namespace {

constexpr int QS = PQ_S, QV = PQ_V, QH0 = PQ_H0;
constexpr int QM = 32;                // edge rows of a tile: two 16-row MFMA tiles
constexpr int QK = PQ_KM;             // 288 operand columns of the second and third message GVP: [s | |vh|]
constexpr int Q_LDA = QK + 4;         // LDS row stride of the operand tile
constexpr int Q_LDV = QH0 * 3 + 1;    // LDS row stride of the vector tile
constexpr int Q_LDN = QH0 + 1;        // LDS row stride of the first GVP's channel norms
constexpr int Q_V3 = QV * 3;          // 96 floats of a node's vectors

// The LDS of a message block: 37 376 + 25 472 + 8 576 + 8 576 + 384 = 80 384 bytes, so two blocks fit the 160 KB of a CU.
static __shared__ __attribute__((aligned(16))) float q_As[QM * Q_LDA];
static __shared__ float q_Vh[QM * Q_LDV];
static __shared__ float q_scr[QM * Q_LDN];      // the gather's norms; a mid stage's next wh [32][32] (row stride 33) after them
static __shared__ float q_wl[QV * (QH0 + 1)];   // a mid stage's wv [32][h], row stride h + 1 (odd: the 32 rows hit 32 banks)
static __shared__ int32_t q_row[3 * QM];        // per tile row: its global edge, its source row, its target row

__device__ __forceinline__ float q_wave_sum(float x) {
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    return x;
}
__device__ __forceinline__ float q_norm3(float a, float b, float c) { return sqrtf(fmaxf(a * a + b * b + c * c, 1e-8f)); }

// tile rows -> q_As [QM][0 .. 256) = the first message GVP's ws output, q_Vh [QM][66][3] = its vh.  Row `row` of the tile is edge row
// min(row0 + row, rows - 1): rows past the end repeat the last one and are never stored.
__device__ __noinline__ void q_gather(const float* __restrict__ P, const float* __restrict__ VT, const float* __restrict__ Es,
                                      const float* __restrict__ ev, const float* __restrict__ whe, const float* __restrict__ Wnt,
                                      const int32_t* __restrict__ gid, const int32_t* __restrict__ src, const int32_t* __restrict__ dst,
                                      int32_t base, int64_t row0, int64_t rows) {
    const int tid = threadIdx.x;
    if (tid < QM) {
        const int64_t k = min(row0 + tid, rows - 1);
        q_row[tid] = gid ? gid[k] : (int32_t)k;
        q_row[QM + tid] = src[k] - base;
        q_row[2 * QM + tid] = dst[k] - base;
    }
    __syncthreads();
#pragma unroll 2
    for (int idx = tid; idx < QM * QH0 * 3; idx += 256) {
        const int row = idx / (QH0 * 3), t = idx - row * (QH0 * 3), h = t / 3, d = t - 3 * h;
        const size_t e = (size_t)q_row[row], j = (size_t)q_row[QM + row], i = (size_t)q_row[2 * QM + row];
        float x = fmaf(whe[2 * h + 1], ev[e * 6 + 3 + d], whe[2 * h] * ev[e * 6 + d]);
        x += VT[j * (2 * QH0 * 3) + t] + VT[i * (2 * QH0 * 3) + QH0 * 3 + t];
        q_Vh[row * Q_LDV + t] = x;
    }
    __syncthreads();
    for (int idx = tid; idx < QM * QH0; idx += 256) {
        const int row = idx / QH0, h = idx - row * QH0;
        const float* p = q_Vh + row * Q_LDV + h * 3;
        q_scr[row * Q_LDN + h] = q_norm3(p[0], p[1], p[2]);
    }
    __syncthreads();
    float wn[QH0];
#pragma unroll
    for (int h = 0; h < QH0; ++h) wn[h] = Wnt[h * QS + tid];
#pragma unroll 2
    for (int row = 0; row < QM; ++row) {
        const size_t e = (size_t)q_row[row], j = (size_t)q_row[QM + row], i = (size_t)q_row[2 * QM + row];
        const float a = (P[j * 512 + tid] + Es[e * QS + tid]) + P[i * 512 + QS + tid];
        float n = 0.0f;
#pragma unroll
        for (int h = 0; h < QH0; ++h) n = fmaf(wn[h], q_scr[row * Q_LDN + h], n);
        q_As[row * Q_LDA + tid] = a + n;
    }
    __syncthreads();
}

// The vector half of one GVP on the tile.  In: q_As[row][0 .. 256) = ws [s | |vh|] + b, q_Vh[row] = vh [h][3].  v = wv vh [32][3]; with
// act, v_c *= sigmoid(|v_c|) and s = relu(s), in place.  With nwh [32][32], the next GVP's wh: q_Vh[row] = nwh v and
// q_As[row][256 .. 288) = its channel norms, so q_As[row] is that GVP's operand row.  Without: q_Vh[row] = v.  A thread owns four
// (row, channel) pairs with their three components.
__device__ __noinline__ void q_mid(const float* __restrict__ wv, int h, bool act, const float* __restrict__ nwh) {
    const int tid = threadIdx.x;
    for (int t = tid; t < QV * h; t += 256) q_wl[t + t / h] = wv[t];
    if (nwh)
        for (int t = tid; t < QV * QV; t += 256) q_scr[t + t / QV] = nwh[t];
    __syncthreads();
    float out[4][3];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int p = tid + 256 * k, row = p >> 5, o = p & 31;
        float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
#pragma unroll 2
        for (int q = 0; q < h; ++q) {
            const float w = q_wl[o * (h + 1) + q];
            const float* x = q_Vh + row * Q_LDV + q * 3;
            a0 = fmaf(w, x[0], a0); a1 = fmaf(w, x[1], a1); a2 = fmaf(w, x[2], a2);
        }
        if (act) {
            const float g = 1.0f / (1.0f + expf(-q_norm3(a0, a1, a2)));
            a0 *= g; a1 *= g; a2 *= g;
        }
        out[k][0] = a0; out[k][1] = a1; out[k][2] = a2;
    }
    if (act) {
#pragma unroll 4
        for (int row = 0; row < QM; ++row) q_As[row * Q_LDA + tid] = fmaxf(q_As[row * Q_LDA + tid], 0.0f);
    }
    __syncthreads();                                            // every vh is read
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int p = tid + 256 * k, row = p >> 5, o = p & 31;
#pragma unroll
        for (int d = 0; d < 3; ++d) q_Vh[row * Q_LDV + o * 3 + d] = out[k][d];
    }
    __syncthreads();
    if (!nwh) return;                                           // block-uniform
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int p = tid + 256 * k, row = p >> 5, o = p & 31;
        float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
#pragma unroll 4
        for (int q = 0; q < QV; ++q) {
            const float w = q_scr[o * (QV + 1) + q];
            const float* x = q_Vh + row * Q_LDV + q * 3;
            a0 = fmaf(w, x[0], a0); a1 = fmaf(w, x[1], a1); a2 = fmaf(w, x[2], a2);
        }
        out[k][0] = a0; out[k][1] = a1; out[k][2] = a2;
    }
    __syncthreads();                                            // every v is read
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int p = tid + 256 * k, row = p >> 5, o = p & 31;
#pragma unroll
        for (int d = 0; d < 3; ++d) q_Vh[row * Q_LDV + o * 3 + d] = out[k][d];
        q_As[row * Q_LDA + QS + o] = q_norm3(out[k][0], out[k][1], out[k][2]);
    }
    __syncthreads();
}

// q_As[QM][0 .. 256) <- q_As[QM][0 .. 288) W^T + bias on v_mfma_f32_16x16x4_f32; W [256][288] in global memory (L2 resident: every
// block reads the same 0.3 MB).  Wave w owns columns [64 w, 64 w + 64).  Lane (r = lane & 15, g = lane >> 4): k step (q, e) of the MFMA
// is operand column 16 q + 4 g + e for both operands, so a lane reads its A rows and its W rows as float4.  C layout: column lane & 15,
// row 4 g + v.  The operand order and the accumulation are s2f_tile.h's fe_gemm at K = 288.
__device__ __noinline__ void q_gemm(const float* __restrict__ W, const float* __restrict__ bias) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
    f32x4 acc[2][4];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) acc[rt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* wrow = W + (size_t)(wave * 64 + r) * QK + 4 * g;
    const float* arow = q_As + r * Q_LDA + 4 * g;
    f32x4 a[2], bf[4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) bf[ct] = *reinterpret_cast<const f32x4*>(wrow + (size_t)ct * 16 * QK);
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) a[rt] = *reinterpret_cast<const f32x4*>(arow + rt * 16 * Q_LDA);
#pragma unroll 1
    for (int q = 0; q < QK / 16; ++q) {
        const int qn = min(q + 1, QK / 16 - 1);                 // the next step's operands load under this step's MFMAs
        f32x4 an[2], bn[4];
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) bn[ct] = *reinterpret_cast<const f32x4*>(wrow + (size_t)ct * 16 * QK + 16 * qn);
#pragma unroll
        for (int rt = 0; rt < 2; ++rt) an[rt] = *reinterpret_cast<const f32x4*>(arow + rt * 16 * Q_LDA + 16 * qn);
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
            for (int v = 0; v < 4; ++v) q_As[(rt * 16 + 4 * g + v) * Q_LDA + col] = acc[rt][ct][v] + bc;
    }
    __syncthreads();
}

}  // namespace

// One block per tile of QM edge rows; grid = ceil(rows / QM).  P [.][512] = (Pj | Pi) and VT [.][132][3] = (wh_j v | wh_i v) per node
// row; Es [E][256], ev [E][2][3] per global edge; whe [66][2]; Wnt [66][256].  Edge row k: global edge gid[k] (gid null: k itself), source
// node row src[k] - base, target node row dst[k] - base (base: the first node copy of the chunk).  msg [rows][352] = the row's message [s | v].
__global__ __launch_bounds__(256, 2) void prosst_message_kernel(const float* __restrict__ P, const float* __restrict__ VT,
                                                                const float* __restrict__ Es, const float* __restrict__ ev,
                                                                const float* __restrict__ whe, const float* __restrict__ Wnt,
                                                                const ProsstMsgWeights w, const int32_t* __restrict__ gid,
                                                                const int32_t* __restrict__ src, const int32_t* __restrict__ dst, int32_t base,
                                                                int64_t rows, float* __restrict__ msg) {
    const int tid = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * QM;
    q_gather(P, VT, Es, ev, whe, Wnt, gid, src, dst, base, row0, rows);
    q_mid(w.wv0, QH0, true, w.wh1);
    q_gemm(w.ws1, w.bs1);
    q_mid(w.wv1, QV, true, w.wh2);
    q_gemm(w.ws2, w.bs2);
    q_mid(w.wv2, QV, false, nullptr);
    const int n = (int)min((int64_t)QM, rows - row0);
    for (int row = 0; row < n; ++row) {
        float* o = msg + (size_t)(row0 + row) * PQ_MSG;
        o[tid] = q_As[row * Q_LDA + tid];
        if (tid < Q_V3) o[QS + tid] = q_Vh[row * Q_LDV + tid];
    }
}

// s [rows][256] = gs[nodes[r]], v [rows][96] = gv[nodes[r]]: every copy of a residue enters layer 0 with W_v's row of the residue
__global__ void prosst_gather_kernel(const float* __restrict__ gs, const float* __restrict__ gv, const int32_t* __restrict__ nodes, int64_t rows,
                                     float* __restrict__ s, float* __restrict__ v) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= rows * PQ_MSG) return;
    const int64_t r = t / PQ_MSG;
    const int c = (int)(t - r * PQ_MSG);
    const size_t n = (size_t)nodes[r];
    if (c < QS) s[r * QS + c] = gs[n * QS + c];
    else v[r * Q_V3 + c - QS] = gv[n * Q_V3 + c - QS];
}

// ds [rows][256], dv [rows][96] = the mean of message rows k in [off[r], off[r + 1]) in ascending k, zero without any: row k itself, or
// with gid the row gid[k] of msg (layer 0 shared over the global edges).  One wave per node copy.
__global__ __launch_bounds__(256) void prosst_aggregate_kernel(const float* __restrict__ msg, const int32_t* __restrict__ off,
                                                               const int32_t* __restrict__ gid, int64_t rows, float* __restrict__ ds,
                                                               float* __restrict__ dv) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int k0 = off[r], k1 = off[r + 1];
    float a[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int k = k0; k < k1; ++k) {
        const float* m = msg + (size_t)(gid ? gid[k] : k - off[0]) * PQ_MSG;
#pragma unroll
        for (int c = 0; c < 5; ++c) a[c] += m[lane + 64 * c];
        if (lane < PQ_MSG - 320) a[5] += m[lane + 320];
    }
    const float cnt = (float)max(k1 - k0, 1);
#pragma unroll
    for (int c = 0; c < 4; ++c) ds[r * QS + lane + 64 * c] = a[c] / cnt;
    dv[r * Q_V3 + lane] = a[4] / cnt;
    if (lane < Q_V3 - 64) dv[r * Q_V3 + 64 + lane] = a[5] / cnt;
}

// x = (rs, rv) + (ds, dv) (ds null: none) -> tuple LayerNorm -> os [rows][256], ov [rows][32][3]: the scalar LayerNorm (eps 1e-5) and
// v / sqrt(mean_c max(|v_c|^2, 1e-8)).  With outA: os also into outA [rows][lda], the scalar columns of a GVP's operand row.
__global__ __launch_bounds__(256) void prosst_node_ln_kernel(const float* __restrict__ rs, const float* __restrict__ rv,
                                                             const float* __restrict__ ds, const float* __restrict__ dv,
                                                             const float* __restrict__ lnw, const float* __restrict__ lnb, int lda, int64_t rows,
                                                             float* __restrict__ os, float* __restrict__ ov, float* __restrict__ outA) {
    __shared__ float vs[4][Q_V3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * 4 + wave;
    const bool live = r0 < rows;
    const int64_t r = live ? r0 : rows - 1;
    float x[4], xv[2];
#pragma unroll
    for (int k = 0; k < 4; ++k) x[k] = rs[r * QS + lane + 64 * k];
    xv[0] = rv[r * Q_V3 + lane];
    xv[1] = lane < Q_V3 - 64 ? rv[r * Q_V3 + 64 + lane] : 0.0f;
    if (ds) {
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] += ds[r * QS + lane + 64 * k];
        xv[0] += dv[r * Q_V3 + lane];
        if (lane < Q_V3 - 64) xv[1] += dv[r * Q_V3 + 64 + lane];
    }
    const float mean = q_wave_sum(x[0] + x[1] + x[2] + x[3]) * (1.0f / QS);
    float var = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) { x[k] -= mean; var += x[k] * x[k]; }
    const float rstd = 1.0f / sqrtf(q_wave_sum(var) * (1.0f / QS) + 1e-5f);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = lane + 64 * k;
        x[k] = x[k] * rstd * lnw[c] + lnb[c];
        if (live) os[r * QS + c] = x[k];
        if (outA && live) outA[r * lda + c] = x[k];
    }
    vs[wave][lane] = xv[0];
    if (lane < Q_V3 - 64) vs[wave][64 + lane] = xv[1];
    __syncthreads();
    float n2 = 0.0f;
    if (lane < QV) {
        const float* p = &vs[wave][lane * 3];
        n2 = fmaxf(p[0] * p[0] + p[1] * p[1] + p[2] * p[2], 1e-8f);
    }
    const float vden = sqrtf(q_wave_sum(n2) * (1.0f / QV));
    if (live) {
        ov[r * Q_V3 + lane] = xv[0] / vden;
        if (lane < Q_V3 - 64) ov[r * Q_V3 + 64 + lane] = xv[1] / vden;
    }
}

// outV [rows][h][3] = wh v of v [rows][32][3], wh [h][32], h <= 132.  With outA [rows][lda] (lda >= 256 + h): columns 256 .. 256 + h =
// the channel norms, the rest of the row's tail zero.  One wave per row.
__global__ __launch_bounds__(256) void prosst_vtab_kernel(const float* __restrict__ v, const float* __restrict__ wh, int h, int lda, int64_t rows,
                                                          float* __restrict__ outV, float* __restrict__ outA) {
    __shared__ float vs[4][Q_V3];
    __shared__ float vhs[4][2 * PQ_H0 * 3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * 4 + wave;
    const bool live = r0 < rows;
    const int64_t r = live ? r0 : rows - 1;
    vs[wave][lane] = v[r * Q_V3 + lane];
    if (lane < Q_V3 - 64) vs[wave][64 + lane] = v[r * Q_V3 + 64 + lane];
    __syncthreads();
    for (int t = lane; t < h * 3; t += 64) {
        const int q = t / 3, d = t - 3 * q;
        float a = 0.0f;
#pragma unroll
        for (int o = 0; o < QV; ++o) a = fmaf(wh[q * QV + o], vs[wave][o * 3 + d], a);
        vhs[wave][t] = a;
        if (live) outV[r * (h * 3) + t] = a;
    }
    __syncthreads();
    if (outA && live) {
        for (int c = lane; c < lda - QS; c += 64) {
            const float* p = &vhs[wave][min(c, h - 1) * 3];
            outA[r * lda + QS + c] = c < h ? q_norm3(p[0], p[1], p[2]) : 0.0f;
        }
    }
}

// One feed-forward GVP's vector half on `rows` rows.  spre [rows][so] = ws [s | |vh|] + b; vh [rows][h][3]; wv [vo][h]; h, vo <= 64.
// v = wv vh; act: v_c *= sigmoid(|v_c|) and s = relu(s).  With nwh [h2][vo] (h2 <= 64): outA [rows][lda] = [s | |nwh v| | 0],
// outV [rows][h2][3] = nwh v.  Without: outV [rows][vo][3] = v and outA is not written (s stays in spre).
__global__ __launch_bounds__(256) void prosst_gvp_mid_kernel(const float* __restrict__ spre, const float* __restrict__ vh,
                                                             const float* __restrict__ wv, const float* __restrict__ nwh, int so, int vo, int h,
                                                             int h2, int act, int lda, int64_t rows, float* __restrict__ outA,
                                                             float* __restrict__ outV) {
    __shared__ float vhs[4][64 * 3];
    __shared__ float vs[4][64 * 3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * 4 + wave;
    const bool live = r0 < rows;
    const int64_t r = live ? r0 : rows - 1;
    for (int t = lane; t < h * 3; t += 64) vhs[wave][t] = vh[r * (h * 3) + t];
    __syncthreads();
    if (lane < vo) {
        float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
        for (int q = 0; q < h; ++q) {
            const float w = wv[lane * h + q];
            a0 = fmaf(w, vhs[wave][q * 3], a0); a1 = fmaf(w, vhs[wave][q * 3 + 1], a1); a2 = fmaf(w, vhs[wave][q * 3 + 2], a2);
        }
        if (act) {
            const float g = 1.0f / (1.0f + expf(-q_norm3(a0, a1, a2)));
            a0 *= g; a1 *= g; a2 *= g;
        }
        vs[wave][lane * 3] = a0; vs[wave][lane * 3 + 1] = a1; vs[wave][lane * 3 + 2] = a2;
        if (!nwh && live) {
            outV[r * (vo * 3) + lane * 3] = a0; outV[r * (vo * 3) + lane * 3 + 1] = a1; outV[r * (vo * 3) + lane * 3 + 2] = a2;
        }
    }
    __syncthreads();
    if (!nwh || !live) return;                      // no barrier below
    for (int c = lane; c < so; c += 64) {
        const float x = spre[r * so + c];
        outA[r * lda + c] = act ? fmaxf(x, 0.0f) : x;
    }
    for (int c = lane; c < lda - so; c += 64) {
        float n = 0.0f;
        if (c < h2) {
            float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
            for (int o = 0; o < vo; ++o) {
                const float w = nwh[c * vo + o];
                a0 = fmaf(w, vs[wave][o * 3], a0); a1 = fmaf(w, vs[wave][o * 3 + 1], a1); a2 = fmaf(w, vs[wave][o * 3 + 2], a2);
            }
            outV[r * (h2 * 3) + c * 3] = a0; outV[r * (h2 * 3) + c * 3 + 1] = a1; outV[r * (h2 * 3) + c * 3 + 2] = a2;
            n = q_norm3(a0, a1, a2);
        }
        outA[r * lda + so + c] = n;
    }
}

// One block per subgraph b, one column per thread: pooled [b][256] = the mean over the node copies [node_off[b], node_off[b + 1]) of
// relu(pre[r]) in ascending r (W_out's scalar activation, then scatter_mean); emb [b] = pooled / max(|pooled|, 1e-12).  node_off is
// relative to the chunk: pre's row 0 is copy node_off[0].
__global__ __launch_bounds__(256) void prosst_pool_kernel(const float* __restrict__ pre, const int32_t* __restrict__ node_off,
                                                          float* __restrict__ pooled, float* __restrict__ emb) {
    __shared__ float part[4];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int r0 = node_off[b] - node_off[0], r1 = node_off[b + 1] - node_off[0];
    float a = 0.0f;
    for (int r = r0; r < r1; ++r) a += fmaxf(pre[(size_t)r * QS + tid], 0.0f);
    a /= (float)max(r1 - r0, 1);
    const float w = q_wave_sum(a * a);
    if ((tid & 63) == 0) part[tid >> 6] = w;
    __syncthreads();
    const float nrm = sqrtf(((part[0] + part[1]) + part[2]) + part[3]);
    pooled[(size_t)b * QS + tid] = a;
    emb[(size_t)b * QS + tid] = a / fmaxf(nrm, 1e-12f);
}

// cn [K] = |c_k|^2 of c [K][256]; one wave per centre
__global__ __launch_bounds__(256) void prosst_centre_norms_kernel(const float* __restrict__ c, int K, float* __restrict__ cn) {
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= K) return;
    float a = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) { const float x = c[(size_t)k * QS + lane + 64 * j]; a = fmaf(x, x, a); }
    a = q_wave_sum(a);
    if (lane == 0) cn[k] = a;
}

// tok [r] = argmin_k cn[k] - 2 G[r][k], the lowest k on a tie; G [rows][K] = x c^T.  One wave per row.
__global__ __launch_bounds__(256) void prosst_argmin_kernel(const float* __restrict__ G, const float* __restrict__ cn, int64_t rows, int K,
                                                            int32_t* __restrict__ tok) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    float best = INFINITY;
    int bk = 0x7fffffff;
    for (int k = lane; k < K; k += 64) {
        const float d = fmaf(-2.0f, G[r * K + k], cn[k]);
        if (d < best) { best = d; bk = k; }                     // ascending k inside a lane: the first minimum stays
    }
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o);
        const int ok = __shfl_xor(bk, o);
        if (ob < best || (ob == best && ok < bk)) { best = ob; bk = ok; }
    }
    if (lane == 0) tok[r] = bk == 0x7fffffff ? 0 : bk;
}

// ---- launchers -----------------------------------------------------------------------------------------------------------------
int launch_prosst_message(const float* P, const float* VT, const float* Es, const float* ev, const float* whe, const float* Wnt,
                          const ProsstMsgWeights& w, const int32_t* gid, const int32_t* src, const int32_t* dst, int32_t base, int64_t rows, float* msg,
                          hipStream_t s) {
    if (rows <= 0) return PGMI_OK;
    if (rows > 0x7fffffffLL) { set_error("prosst: %lld edge rows in one message launch", (long long)rows); return PGMI_EINVAL; }
    hipLaunchKernelGGL(prosst_message_kernel, dim3((unsigned)((rows + QM - 1) / QM)), dim3(256), 0, s, P, VT, Es, ev, whe, Wnt, w, gid, src, dst,
                       base, rows, msg);
    return PGMI_OK;
}

void launch_prosst_gather(const float* gs, const float* gv, const int32_t* nodes, int64_t rows, float* s, float* v, hipStream_t st) {
    const int64_t n = rows * PQ_MSG;
    hipLaunchKernelGGL(prosst_gather_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, gs, gv, nodes, rows, s, v);
}

void launch_prosst_aggregate(const float* msg, const int32_t* off, const int32_t* gid, int64_t rows, float* ds, float* dv, hipStream_t s) {
    hipLaunchKernelGGL(prosst_aggregate_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, msg, off, gid, rows, ds, dv);
}

void launch_prosst_node_ln(const float* rs, const float* rv, const float* ds, const float* dv, const float* lnw, const float* lnb, int lda,
                           int64_t rows, float* os, float* ov, float* outA, hipStream_t s) {
    hipLaunchKernelGGL(prosst_node_ln_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, rs, rv, ds, dv, lnw, lnb, lda, rows, os, ov, outA);
}

int launch_prosst_vtab(const float* v, const float* wh, int h, int lda, int64_t rows, float* outV, float* outA, hipStream_t s) {
    if (h < 1 || h > 2 * PQ_H0 || (outA && lda < QS + h) || rows <= 0) {
        set_error("prosst: vector table h=%d lda=%d rows=%lld is not one this kernel runs", h, lda, (long long)rows);
        return PGMI_EINVAL;
    }
    hipLaunchKernelGGL(prosst_vtab_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, v, wh, h, lda, rows, outV, outA);
    return PGMI_OK;
}

int launch_prosst_gvp_mid(const float* spre, const float* vh, const float* wv, const float* nwh, int so, int vo, int h, int h2, int act,
                          int lda, int64_t rows, float* outA, float* outV, hipStream_t s) {
    if (so < 1 || vo < 1 || vo > 64 || h < 1 || h > 64 || h2 < 0 || h2 > 64 || (nwh && (!outA || lda < so + h2)) || rows <= 0) {
        set_error("prosst: GVP shape so=%d vo=%d h=%d h2=%d lda=%d is not one this kernel runs", so, vo, h, h2, lda);
        return PGMI_EINVAL;
    }
    hipLaunchKernelGGL(prosst_gvp_mid_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, spre, vh, wv, nwh, so, vo, h, h2, act, lda, rows,
                       outA, outV);
    return PGMI_OK;
}

void launch_prosst_pool(const float* pre, const int32_t* node_off, int n_sub, float* pooled, float* emb, hipStream_t s) {
    hipLaunchKernelGGL(prosst_pool_kernel, dim3((unsigned)n_sub), dim3(256), 0, s, pre, node_off, pooled, emb);
}

void launch_prosst_centre_norms(const float* c, int K, float* cn, hipStream_t s) {
    hipLaunchKernelGGL(prosst_centre_norms_kernel, dim3((unsigned)((K + 3) / 4)), dim3(256), 0, s, c, K, cn);
}

void launch_prosst_argmin(const float* G, const float* cn, int64_t rows, int K, int32_t* tok, hipStream_t s) {
    hipLaunchKernelGGL(prosst_argmin_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, G, cn, rows, K, tok);
}

}  // namespace pgmi
