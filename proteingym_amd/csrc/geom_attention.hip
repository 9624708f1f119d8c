// ESM3's geometric attention (proteingym/baselines/evoscale/esm/layers/geom_attention.py GeometricReasoningOriginalImpl.forward),
// fp32 throughout, no MFMA: a head is three floats wide.
//
// Per token the projection row holds, in the reference's column order, q_rot | k_rot | v (H x 3 each) and then q_dist | k_dist
// (H x 3 each).  With the token's frame (R, t): q_rot, k_rot and v are rotated by R, q_dist and k_dist are rotated and translated
// (R p + t), and for head h
//     score(i, j) = (q_rot_i . k_rot_j) / sqrt(3) * w_rot[h]  -  |q_dist_i - k_dist_j| / sqrt(3) * w_dist[h]
// (a norm, not a squared norm; w_* = softplus of the per-head scale parameters, taken by the caller).  The softmax runs over the
// keys, the weighted sum of v is rotated back by R_i^T, and the rows of frameless queries are zero.
//
// Masked keys.  The reference adds finfo.min to the score of a frameless key rather than -inf.  For a framed query that is the
// same as leaving the key out: the query itself is a framed key of its own row, so the row maximum is a finite score of ordinary
// size, and exp(finfo.min - max) is exactly 0 in fp32.  A frameless query whose keys are all frameless would get the reference's
// uniform softmax over finfo.min scores -- but its row is zeroed (mask_and_zero_frameless) whatever it attended to.  So frameless
// keys are skipped and frameless queries write zeros; the uniform softmax is never formed.
//
// Launch shape.  A block of 256 threads serves QT queries x 256 / QT heads of one batch row: thread (q, hl) owns query
// i = blockIdx.x * QT + q of head blockIdx.y * (256 / QT) + hl.  Keys go through LDS in tiles of QT: thread (q, hl) stages key
// k0 + q of its own head -- k_rot, k_dist and v already moved to the global frame, nine floats -- and then every thread walks the
// tile.  All lanes of a wave read the same key (and, for QT >= 64, the same head), so the LDS reads are broadcasts; for QT = 16 a
// wave holds four heads, whose tiles are padded apart by 8 floats so that the four addresses fall on different banks.  Scores are
// taken eight keys at a time: one running-maximum update and one rescale per eight exps.
// Frames are shared by every batch row (frame_stride = 0: the masked rows of one window) or given per row (frame_stride = S: the
// structure tokenizer's neighbourhoods).
#include "common.h"

namespace pgmi {

namespace {

constexpr int kGeoThreads = 256;
constexpr int kGeoChunk = 8;

template <int QT>
__global__ __launch_bounds__(kGeoThreads) void geom_attention_kernel(const float* __restrict__ proj, int pitch,
                                                                      const float* __restrict__ rot, const float* __restrict__ trans,
                                                                      const int32_t* __restrict__ fmask, int frame_stride,
                                                                      const float* __restrict__ w_rot, const float* __restrict__ w_dist,
                                                                      int S, int H, float* __restrict__ out, int opitch) {
    constexpr int HB = kGeoThreads / QT;
    constexpr int HSTRIDE = QT * 9 + 8;
    __shared__ float sk[HB * HSTRIDE];
    __shared__ int32_t sm[QT];

    const int q = threadIdx.x % QT, hl = threadIdx.x / QT;
    const int b = blockIdx.z;
    const int i = blockIdx.x * QT + q;
    const int h = blockIdx.y * HB + hl;
    const bool head_ok = h < H;
    const bool q_ok = head_ok && i < S;
    const size_t row0 = (size_t)b * S;                       // first projection / output row of this batch row
    const size_t f0 = (size_t)b * frame_stride;              // first frame of this batch row
    const float inv_sqrt3 = 0.57735026918962576f;

    // the query, in the global frame
    float R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    float qr[3] = {0, 0, 0}, qd[3] = {0, 0, 0};
    bool framed = false;
    float wr = 0.f, wd = 0.f;
    if (q_ok) {
        const float* fr = rot + (f0 + i) * 9;
        const float* ft = trans + (f0 + i) * 3;
#pragma unroll
        for (int c = 0; c < 9; ++c) R[c] = fr[c];
        framed = fmask[f0 + i] != 0;
        const float* p = proj + (row0 + i) * (size_t)pitch;
        const float a0 = p[3 * h], a1 = p[3 * h + 1], a2 = p[3 * h + 2];
        const float* pd = p + 9 * H + 3 * h;
        const float d0 = pd[0], d1 = pd[1], d2 = pd[2];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            qr[r] = R[3 * r] * a0 + R[3 * r + 1] * a1 + R[3 * r + 2] * a2;
            qd[r] = R[3 * r] * d0 + R[3 * r + 1] * d1 + R[3 * r + 2] * d2 + ft[r];
        }
        wr = w_rot[h] * inv_sqrt3;
        wd = w_dist[h] * inv_sqrt3;
#pragma unroll
        for (int r = 0; r < 3; ++r) qr[r] *= wr;             // (q . k) / sqrt(3) * w_rot
    }

    float mx = -INFINITY, den = 0.f, acc[3] = {0.f, 0.f, 0.f};
    const float* kt = sk + hl * HSTRIDE;
    for (int k0 = 0; k0 < S; k0 += QT) {
        __syncthreads();                                     // the previous tile has been read
        const int j = k0 + q;
        if (hl == 0) sm[q] = (j < S && fmask[f0 + j] != 0) ? 1 : 0;
        if (head_ok && j < S) {
            const float* fr = rot + (f0 + j) * 9;
            const float* ft = trans + (f0 + j) * 3;
            const float* p = proj + (row0 + j) * (size_t)pitch;
            const float* pk = p + 3 * H + 3 * h;
            const float* pv = p + 6 * H + 3 * h;
            const float* pd = p + 12 * H + 3 * h;
            const float k_0 = pk[0], k_1 = pk[1], k_2 = pk[2];
            const float v_0 = pv[0], v_1 = pv[1], v_2 = pv[2];
            const float d_0 = pd[0], d_1 = pd[1], d_2 = pd[2];
            float* dst = sk + hl * HSTRIDE + q * 9;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const float r0 = fr[3 * r], r1 = fr[3 * r + 1], r2 = fr[3 * r + 2];
                dst[r] = r0 * k_0 + r1 * k_1 + r2 * k_2;
                dst[3 + r] = r0 * d_0 + r1 * d_1 + r2 * d_2 + ft[r];
                dst[6 + r] = r0 * v_0 + r1 * v_1 + r2 * v_2;
            }
        }
        __syncthreads();
        const int n = min(QT, S - k0);
        for (int c0 = 0; c0 < n; c0 += kGeoChunk) {
            float sc[kGeoChunk];
            float cmax = -INFINITY;
#pragma unroll
            for (int c = 0; c < kGeoChunk; ++c) {
                const int jj = c0 + c;
                sc[c] = -INFINITY;
                if (jj < n && sm[jj]) {                      // the same key in every lane: a uniform branch
                    const float* kk = kt + jj * 9;
                    const float dot = qr[0] * kk[0] + qr[1] * kk[1] + qr[2] * kk[2];
                    const float e0 = qd[0] - kk[3], e1 = qd[1] - kk[4], e2 = qd[2] - kk[5];
                    sc[c] = dot - sqrtf(e0 * e0 + e1 * e1 + e2 * e2) * wd;
                    cmax = fmaxf(cmax, sc[c]);
                }
            }
            if (cmax == -INFINITY) continue;                 // no framed key in this chunk
            const float nm = fmaxf(mx, cmax);
            const float corr = expf(mx - nm);                // mx = -inf on the first chunk: exp(-inf) = 0
            den *= corr; acc[0] *= corr; acc[1] *= corr; acc[2] *= corr;
            mx = nm;
#pragma unroll
            for (int c = 0; c < kGeoChunk; ++c) {
                const int jj = c0 + c;
                if (jj < n && sm[jj]) {
                    const float* kk = kt + jj * 9;
                    const float pw = expf(sc[c] - nm);
                    den += pw;
                    acc[0] += pw * kk[6]; acc[1] += pw * kk[7]; acc[2] += pw * kk[8];
                }
            }
        }
    }
    if (!q_ok) return;
    float* o = out + (row0 + i) * (size_t)opitch + 3 * h;
    if (!framed || den == 0.f) { o[0] = 0.f; o[1] = 0.f; o[2] = 0.f; return; }
    const float inv = 1.0f / den;
    const float g0 = acc[0] * inv, g1 = acc[1] * inv, g2 = acc[2] * inv;
    // back to the query's frame: R^T
    o[0] = R[0] * g0 + R[3] * g1 + R[6] * g2;
    o[1] = R[1] * g0 + R[4] * g1 + R[7] * g2;
    o[2] = R[2] * g0 + R[5] * g1 + R[8] * g2;
}

template <int QT>
void launch_qt(const GeomAttLaunch& g) {
    const dim3 grid((g.S + QT - 1) / QT, (g.H + kGeoThreads / QT - 1) / (kGeoThreads / QT), g.B);
    geom_attention_kernel<QT><<<grid, kGeoThreads, 0, g.stream>>>(g.proj, g.pitch, g.rot, g.trans, g.mask, g.per_row_frames ? g.S : 0,
                                                                   g.w_rot, g.w_dist, g.S, g.H, g.out, g.opitch);
}

}  // namespace

int geom_key_tile(int S) { return S <= 16 ? 16 : S <= 64 ? 64 : 256; }

int launch_geom_attention(const GeomAttLaunch& g) {
    if (!g.proj || !g.rot || !g.trans || !g.mask || !g.w_rot || !g.w_dist || !g.out || g.B <= 0 || g.S <= 0 || g.H <= 0 ||
        g.pitch < 15 * g.H || g.opitch < 3 * g.H || g.B > 65535) {
        set_error("geom_attention: unsupported shape B=%d S=%d H=%d pitch=%d opitch=%d (B <= 65535)", g.B, g.S, g.H, g.pitch, g.opitch);
        return PGMI_EINVAL;
    }
    if (g.opitch > 3 * g.H)                                  // the out-projection's K padding: zeros
        PGMI_HIP(hipMemsetAsync(g.out, 0, (size_t)g.B * g.S * g.opitch * sizeof(float), g.stream));
    switch (geom_key_tile(g.S)) {
        case 16: launch_qt<16>(g); break;
        case 64: launch_qt<64>(g); break;
        default: launch_qt<256>(g);
    }
    PGMI_HIP(hipGetLastError());
    return PGMI_OK;
}

}  // namespace pgmi
