// S2F kernels (include/pgmi.h, S2F section): the GVP-GNN of proteingym/baselines/S3F over ESM2's residue rows.
// Scalar width 256, 16 vector channels in the node state; fp32 only.  Every kernel works row by row (an edge of a masked copy, or
// a node of a masked copy) and reads nothing of another copy, so a row's bits do not depend on what else is in the launch; the dense
// Linears between them are launch_gemm_f32 (api_s2f.hip), whose per-element sum order does not depend on the row count either.
//
//   s2f_message_kernel    the three message GVPs of a layer and the mean at the centre, one block per (copy, node), the node's edge
//                         rows in LDS throughout.  The first GVP is linear in [s_j | e_s | s_i] and [v_j | e_v | v_i] before the norm,
//                         so its per-node products (P = s [Wj | Wi]^T, VT = [wh_j v | wh_i v]) come from N-row launches and the
//                         edge's share (Es = We e_s + b, wh_e e_v) from the structure pass; a row gathers the three, takes the 33
//                         channel norms and adds Wn |vh|.  The two 272 -> 256 GVPs run on the fp32 MFMA with their weights read
//                         from L2; no per-edge activation goes to HBM.
//   s2f_gvp_mid_kernel    the vector half of any GVP after its ws GEMM and its gate GEMM (wsv s + b on s before the scalar activation):
//                         v = wv vh * sigmoid(gate), s = relu(s) or s; then the NEXT GVP's wh v and channel norms, written as that
//                         GVP's GEMM operand row [s | |vh| | 0 pad].
//   s2f_node_ln_kernel    (s, v) + dh -> tuple LayerNorm; dh is the mean message or the feed-forward output; then the next GVP's
//                         wh v / norms as above.
//   s2f_head_kernel       relu, S3F's pooled row when there is one, Linear(256 -> 20), the ESM logits on low-pLDDT rows, log-softmax
//                         over 20.
//   s2f_pick_logits_kernel  the 20 amino-acid columns of ESM2's log-probability rows of the L residues.
#include <algorithm>

#include "s2f_tile.h"

namespace pgmi {

// ---- fused message kernel (the tile, its LDS, the gather and the GVP stages: s2f_tile.h) ------------------------------------------
// The three message GVPs of one layer and the mean at the centre, one block per (masked copy b, node i); grid = B L.  The node's
// edges [off[i], off[i + 1]) go through in tiles of FE_M rows that live in LDS from the gather to the sum; the sum runs over the rows
// in ascending edge order, one column per thread, so nothing of another node or copy enters a row's bits and no atomics are needed.
// P [B L][512] = (Pj | Pi); VT [B L][66][3] = (wh_j v | wh_i v), null when v = 0; Es [E][256]; ev [E][3]; whe [33]; Wnt [33][256].
// ds [B L][256], dv [B L][16][3] = the mean message, zero for a node without edges.
__global__ __launch_bounds__(256, 2) void s2f_message_kernel(const float* __restrict__ P, const float* __restrict__ VT,
                                                          const float* __restrict__ Es, const float* __restrict__ ev,
                                                          const float* __restrict__ whe, const float* __restrict__ Wnt, const S2fMsgWeights w,
                                                          const int32_t* __restrict__ src, const int32_t* __restrict__ off, int L,
                                                          float* __restrict__ ds, float* __restrict__ dv) {
    const int tid = threadIdx.x;
    const int64_t node = blockIdx.x;
    const int i = (int)(node % L);
    const int64_t nb = node - i;                                // b L
    const int e0 = off[i], e1 = off[i + 1];
    float sum_s = 0.0f, sum_v = 0.0f;
#pragma unroll 1
    for (int c0 = e0; c0 < e1; c0 += FE_M) {                    // block-uniform: every barrier below is reached by all threads
        fe_tile<false>(P, VT, Es, ev, whe, Wnt, w, src, nb, c0, e1 - 1, i, i);
        const int n = min(FE_M, e1 - c0);
        for (int row = 0; row < n; ++row) {
            sum_s += fe_As[row * FE_LDA + tid];
            if (tid < SV * 3) sum_v += fe_Vh[row * FE_LDV + tid];
        }
        __syncthreads();                                        // the next tile overwrites fe_As and fe_Vh
    }
    const float cnt = (float)max(e1 - e0, 1);
    ds[node * SS + tid] = sum_s / cnt;
    if (tid < SV * 3) dv[node * (SV * 3) + tid] = sum_v / cnt;
}

// One GVP's vector half on `rows` rows.  spre [rows][so] = ws [s | |vh|] + b; vh [rows][h][3]; wv [vo][h]; gpre [rows][vo] = wsv spre +
// b, the gate before its sigmoid (a GEMM of its own on spre: api_s2f.hip).
// so in {256, 1024}, vo <= 32, h <= 33.  With nwh [h2][vo] (h2 <= 32): outA [rows][lda] = [act(s) | |nwh v| | 0], outV [rows][h2][3] =
// nwh v.  Without: outV [rows][vo][3] = v, and outA (nullable) [rows][lda] = act(s).
__global__ __launch_bounds__(256) void s2f_gvp_mid_kernel(const float* __restrict__ spre, const float* __restrict__ vh,
                                                          const float* __restrict__ wv, const float* __restrict__ gpre,
                                                          const float* __restrict__ nwh, int so, int vo, int h,
                                                          int h2, int relu, int lda, int64_t rows, float* __restrict__ outA,
                                                          float* __restrict__ outV) {
    __shared__ float vhs[4][SH0 * 3 + 1];
    __shared__ float vs[4][32 * 3];
    __shared__ float gs[4][32];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * 4 + wave;
    const bool live = r0 < rows;
    const int64_t r = live ? r0 : rows - 1;
    const int nk = so >> 6;                       // 4 or 16 columns per lane
    float s[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) s[k] = k < nk ? spre[r * so + lane + 64 * k] : 0.0f;
    for (int t = lane; t < h * 3; t += 64) vhs[wave][t] = vh[r * (h * 3) + t];
    if (lane < vo) gs[wave][lane] = 1.0f / (1.0f + expf(-gpre[r * vo + lane]));
    __syncthreads();
    for (int t = lane; t < vo * 3; t += 64) {
        const int o = t / 3, d = t - 3 * o;
        float a = 0.0f;
        for (int q = 0; q < h; ++q) a = fmaf(wv[o * h + q], vhs[wave][q * 3 + d], a);
        a *= gs[wave][o];
        vs[wave][t] = a;
        if (!nwh && live) outV[r * (vo * 3) + t] = a;
    }
    if (outA && live) {
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (k < nk) outA[r * lda + lane + 64 * k] = relu ? fmaxf(s[k], 0.0f) : s[k];
    }
    __syncthreads();
    if (nwh) {
        for (int t = lane; t < h2 * 3; t += 64) {
            const int q = t / 3, d = t - 3 * q;
            float a = 0.0f;
            for (int o = 0; o < vo; ++o) a = fmaf(nwh[q * vo + o], vs[wave][o * 3 + d], a);
            vhs[wave][t] = a;                      // vh of this GVP is dead: every lane passed the barrier above
            if (live) outV[r * (h2 * 3) + t] = a;
        }
    }
    __syncthreads();
    if (nwh && live) {
        for (int c = so + lane; c < lda; c += 64) outA[r * lda + c] = c < so + h2 ? s2f_vnorm(&vhs[wave][(c - so) * 3]) : 0.0f;
    }
}

// rows = B * L.  x = (rs, rv) + dh; rv null: zero vectors.  dh (ds [rows][256], dv [rows][16][3]) is the mean message or the
// feed-forward output; ds null: none.
// Tuple LayerNorm -> os [rows][256], ov [rows][16][3].  Then with wh [h][16] (h <= 66): outV [rows][h][3] = wh ov, and with vn != 0
// outA [rows][lda] = [os | |wh ov| | 0].
__global__ __launch_bounds__(256) void s2f_node_ln_kernel(const float* __restrict__ rs, const float* __restrict__ rv,
                                                          const float* __restrict__ ds, const float* __restrict__ dv,
                                                          const float* __restrict__ lnw,
                                                          const float* __restrict__ lnb, const float* __restrict__ wh, int h, int vn, int lda,
                                                          int64_t rows, float* __restrict__ os, float* __restrict__ ov,
                                                          float* __restrict__ outA, float* __restrict__ outV) {
    __shared__ float vs[4][SV * 3];
    __shared__ float vhs[4][66 * 3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * 4 + wave;
    const bool live = r0 < rows;
    const int64_t r = live ? r0 : rows - 1;
    float x[4], xv = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) x[k] = rs[r * SS + lane + 64 * k];
    if (rv && lane < SV * 3) xv = rv[r * (SV * 3) + lane];
    if (ds) {
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] += ds[r * SS + lane + 64 * k];
        if (lane < SV * 3) xv += dv[r * (SV * 3) + lane];
    }
    const float mean = s2f_wave_sum(x[0] + x[1] + x[2] + x[3]) * (1.0f / SS);
    float var = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) { x[k] -= mean; var += x[k] * x[k]; }
    const float rstd = 1.0f / sqrtf(s2f_wave_sum(var) * (1.0f / SS) + 1e-5f);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = lane + 64 * k;
        x[k] = x[k] * rstd * lnw[c] + lnb[c];
        if (live) os[r * SS + c] = x[k];
        if (outA && live) outA[r * lda + c] = x[k];
    }
    if (lane < SV * 3) vs[wave][lane] = xv;
    __syncthreads();
    float n2 = 0.0f;
    if (lane < SV) {
        const float* p = &vs[wave][lane * 3];
        n2 = fmaxf(p[0] * p[0] + p[1] * p[1] + p[2] * p[2], 1e-8f);
    }
    const float vden = sqrtf(s2f_wave_sum(n2) * (1.0f / SV));
    __syncthreads();
    if (lane < SV * 3) {
        xv = xv / vden;
        vs[wave][lane] = xv;
        if (live) ov[r * (SV * 3) + lane] = xv;
    }
    __syncthreads();
    if (h > 0) {
        for (int t = lane; t < h * 3; t += 64) {
            const int q = t / 3, d = t - 3 * q;
            float a = 0.0f;
#pragma unroll
            for (int o = 0; o < SV; ++o) a = fmaf(wh[q * SV + o], vs[wave][o * 3 + d], a);
            vhs[wave][t] = a;
            if (live) outV[r * (h * 3) + t] = a;
        }
    }
    __syncthreads();
    if (h > 0 && vn && live) {
        for (int c = SS + lane; c < lda; c += 64) outA[r * lda + c] = c < SS + h ? s2f_vnorm(&vhs[wave][(c - SS) * 3]) : 0.0f;
    }
}

// rows = copies * L rows of x [.][256] (W_out before its ReLU): logits = W hx + b over 20 letters, hx = relu(x); rows whose
// plddt[r % L] < thr read seq [rows][20] instead; log-softmax.  With sums [copies][256] and grp [copies][2] (S3F; both null otherwise),
// grp = the first and one past the last copy of the row's pool group: hx = relu(x) + the pooled row, the sum of the group's copy sums
// in ascending copy order over (copies * Ns).  One wave per row.
__global__ __launch_bounds__(256) void s2f_head_kernel(const float* __restrict__ x, const float* __restrict__ sums, const int32_t* __restrict__ grp,
                                                       int Ns, const float* __restrict__ W, const float* __restrict__ bias,
                                                       const float* __restrict__ seq, const float* __restrict__ plddt, float thr, int L,
                                                       int64_t rows, float* __restrict__ lp) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    float hx[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) hx[k] = fmaxf(x[r * SS + lane + 64 * k], 0.0f);
    if (sums) {
        const int s = (int)(r / L), g0 = grp[2 * s], g1 = grp[2 * s + 1];
        const float cnt = (float)(g1 - g0) * (float)Ns;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float a = 0.0f;
            for (int t = g0; t < g1; ++t) a += sums[(size_t)t * SS + lane + 64 * k];
            hx[k] = hx[k] + a / cnt;
        }
    }
    float logit = -INFINITY;
    for (int c = 0; c < 20; ++c) {
        float p = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; ++k) p = fmaf(hx[k], W[c * SS + lane + 64 * k], p);
        p = s2f_wave_sum(p);
        if (lane == c) logit = p + bias[c];
    }
    if (plddt[r % L] < thr && lane < 20) logit = seq[r * 20 + lane];
    float mx = logit;
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    const float ex = s2f_wave_sum(lane < 20 ? expf(logit - mx) : 0.0f);
    if (lane < 20) lp[r * 20 + lane] = logit - mx - logf(ex);
}

// out [B L][20] = lp [(b T + 1 + i)][cols[c]] of ESM2's [B T][V] rows
__global__ void s2f_pick_logits_kernel(const float* __restrict__ lp, const int32_t* __restrict__ cols, int L, int T, int V, int64_t n,
                                       float* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const int c = (int)(t % 20);
    const int64_t r = t / 20, b = r / L;
    const int i = (int)(r % L);
    out[t] = lp[(b * T + 1 + i) * V + cols[c]];
}

// ---- launchers -----------------------------------------------------------------------------------------------------------------
int launch_s2f_message(const float* P, const float* VT, const float* Es, const float* ev, const float* whe, const float* Wnt,
                       const S2fMsgWeights& w, const int32_t* src, const int32_t* off, int L, int64_t nodes, float* ds, float* dv, hipStream_t s) {
    if (w.ldw < FE_K || w.ldw % 4 || L < 1 || nodes % L || nodes > 0x7fffffffLL) {
        set_error("s2f: message stage ldw=%d L=%d nodes=%lld is not one this kernel runs", w.ldw, L, (long long)nodes);
        return PGMI_EINVAL;
    }
    if (nodes <= 0) return PGMI_OK;
    hipLaunchKernelGGL(s2f_message_kernel, dim3((unsigned)nodes), dim3(256), 0, s, P, VT, Es, ev, whe, Wnt, w, src, off, L, ds, dv);
    return PGMI_OK;
}

int launch_s2f_gvp_mid(const float* spre, const float* vh, const float* wv, const float* gpre, const float* nwh, int so,
                       int vo, int h, int h2, int relu, int lda, int64_t rows, float* outA, float* outV, hipStream_t s) {
    if ((so != 256 && so != 1024) || vo < 1 || vo > 32 || h < 1 || h > SH0 || h2 < 0 || h2 > 32 || (nwh && (!outA || lda < so + h2)) ||
        (outA && lda < so)) {
        set_error("s2f: GVP shape so=%d vo=%d h=%d h2=%d lda=%d is not one this kernel runs", so, vo, h, h2, lda);
        return PGMI_EINVAL;
    }
    if (rows <= 0) return PGMI_OK;
    hipLaunchKernelGGL(s2f_gvp_mid_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, spre, vh, wv, gpre, nwh, so, vo, h, h2, relu,
                       lda, rows, outA, outV);
    return PGMI_OK;
}

int launch_s2f_node_ln(const float* rs, const float* rv, const float* ds, const float* dv, const float* lnw, const float* lnb, const float* wh, int h, int vn, int lda, int64_t rows, float* os, float* ov,
                       float* outA, float* outV, hipStream_t s) {
    if (h < 0 || h > 66 || (h > 0 && vn && (!outA || lda < SS + h)) || (outA && lda < SS) || rows <= 0) {
        set_error("s2f: node stage h=%d lda=%d rows=%lld is not one this kernel runs", h, lda, (long long)rows);
        return PGMI_EINVAL;
    }
    hipLaunchKernelGGL(s2f_node_ln_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, rs, rv, ds, dv, lnw, lnb, wh, h,
                       vn, lda, rows, os, ov, outA, outV);
    return PGMI_OK;
}

void launch_s2f_head(const float* x, const float* sums, const int32_t* grp, int Ns, const float* W, const float* bias, const float* seq,
                     const float* plddt, float thr, int L, int64_t rows, float* lp, hipStream_t s) {
    hipLaunchKernelGGL(s2f_head_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, x, sums, grp, Ns, W, bias, seq, plddt, thr, L, rows, lp);
}

void launch_s2f_pick_logits(const float* lp, const int32_t* cols, int L, int T, int V, int64_t rows, float* out, hipStream_t s) {
    const int64_t n = rows * 20;
    hipLaunchKernelGGL(s2f_pick_logits_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, lp, cols, L, T, V, n, out);
}

}  // namespace pgmi
