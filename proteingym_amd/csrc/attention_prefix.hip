// Segment-causal attention over a shared prefix on the 16-bit matrix pipe, split-fp16 (f16x3) operands: PoET's two attention tiers
// (proteingym/baselines/PoET/poet/models/modules/transformer.py TieredTransformerEncoderLayer.forward_packed; the cached-memory form
// poet/models/poet.py _apply_causal_prefix_attention).
//
// A launch holds B segments of packed query rows (segment b = rows seg_off[b] .. seg_off[b + 1] - 1).  A query at position t of its
// segment sees, through ONE online softmax, first the P keys of a prefix shared by every segment (no mask) and then the keys 0 .. t of
// its own segment.  The four uses: prompt tier 1 (B = prompt sequences, P = 0), prompt tier 2 (B = 1, the whole prompt, P = 0; its K / V
// planes ARE the layer's prefix cache), variant tier 1 (B = variants, P = 0), variant tier 2 (B = variants, P = prompt length, prefix
// planes = the cache).
//
// Arithmetic: that of attention_f16.hip word for word -- S^T = K Q^T per (32 keys x 32 queries) tile with v_mfma_f32_32x32x16_f16, every
// product as x_hi y_hi + 2^-11 (x_hi y_lo + x_lo y_hi) in separate accumulators, base-2 online softmax with the deferred per-row
// rescale, P split by split_p, O^T = V^T P^T.  One wave = one query tile = 32 consecutive positions 32 j .. 32 j + 31 of ONE segment.
//
// Operand layout (written by prefix_prep_kernel below; the prefix cache keeps exactly this, so scoring never re-packs it):
//   q16  [plane][packed row][H * 64]     q rotated, times log2(e) (and head_dim^-1/2 from the weights)
//   k16  [plane][H][pitch][64]           k rotated; row = PADDED row: every segment starts at a multiple of 32 (tile e of the launch's
//                                        (segment, tile) list owns padded rows 32 e .. 32 e + 31), pad rows = 0
//   vt16 [plane][H][64][pitch]           V transposed, padded rows as columns, the keys of each 32-key tile with bits 2 and 3 of the key
//                                        index swapped (the order the S^T accumulator holds them), pad keys = 0
// Key tiles keep their ABSOLUTE alignment -- prefix tile kt = prefix keys 32 kt .. +31, own tile kt = own keys 32 kt .. +31 -- and a
// query tile always holds the same 32 positions of its segment, so a row goes through the same tiles in the same order whatever else
// is in the launch: the same bits.  All addressing is 64-bit pointer arithmetic (a plane of a 24 576-token prompt at 16 heads is 50 MB,
// but nothing here assumes it stays below 2^31 bytes).
//
// Sharing: a workgroup is 4 waves = 4 query tiles, usually of different segments (variants).  The prefix phase is block-wide: each
// prefix tile (K hi | K lo | V^T hi | V^T lo, 16 KiB) is fetched ONCE per workgroup into a double-buffered LDS stage (global ->
// registers -> LDS, the next tile's loads in flight under the current tile's MFMAs, one barrier per tile) and consumed by all four
// waves; the workgroups of one head run on one XCD (block i -> XCD i % 8 -> heads h = 8 s + i % 8), so the head's prefix planes are
// fetched into that XCD's L2 once.  The own-segment phase is per wave, fragments straight from global memory (L2): a variant's own
// keys are ~2 % of a 24 k prefix; the prompt's tier 2 (once per prompt and layer) runs entirely in this phase.
// LDS budget: 2 stages x 16 KiB = 32 KiB per workgroup, 4 waves: up to 4 workgroups per CU fit the 160 KiB, registers (one wave per
// SIMD per workgroup at ~200 VGPRs) allow 2.
//
// Cross-attention (ESM-IF1's encoder_attn, api_esmif1.hip) is the OWN = false instantiation: the prefix phase alone, the planes of the
// encoded backbone as the prefix (P = S memory keys, the last S % 32 pad keys masked to P = 0 exactly by the same `lim` test), no
// own-segment planes.  Its budget is the prefix phase's: the same 32 KiB of LDS and the same registers less the own-phase fragments.
// The q planes come from cross_q_prep_kernel (no k / v of the decoder rows exist).  The OWN = true code is what it was.
#include "attention_f16_common.h"

namespace pgmi {

constexpr int PFX_WPB = 4;
constexpr int PFX_KCH = AKT * 8, PFX_VCH = 64 * 4;          // 16-byte chunks per K plane / V^T plane of a tile
constexpr int PFX_STG = 2 * PFX_KCH + 2 * PFX_VCH;          // chunks per LDS stage (16 KiB)

// stored position j (0 .. 31) of a V^T tile -> key of the tile: bits 2 and 3 swapped
__device__ __forceinline__ int vt_key(int j) { return (j & ~12) | ((j & 4) << 1) | ((j & 8) >> 1); }

// fp32 q | k | v rows [R][3 H 64] -> the operand planes.  Grid (tiles, H), 256 threads: tile e = 32 positions of segment ent_seg[e].
__global__ __launch_bounds__(256) void prefix_prep_kernel(
    const float* __restrict__ qkv, const int32_t* __restrict__ pos, const float* __restrict__ cos_t, const float* __restrict__ sin_t,
    const int32_t* __restrict__ seg_off, const int32_t* __restrict__ ent_seg, const int32_t* __restrict__ ent_tile, int H,
    unsigned short* __restrict__ q16, size_t q_plane, unsigned short* __restrict__ k16, unsigned short* __restrict__ vt16, size_t pitch) {
    __shared__ unsigned short sv[2][32][64 + 8];               // the tile's V rows, both planes (row pitch 72 halfs: the transposed read spreads over the banks)
    const int e = blockIdx.x, h = blockIdx.y, tid = threadIdx.x;
    const int b = ent_seg[e], jt = ent_tile[e];
    const int s0 = seg_off[b], len = seg_off[b + 1] - s0;
    const int t = tid >> 3, c = tid & 7;                       // position inside the tile, 8-dim chunk
    const int tp = jt * 32 + t;                                // position inside the segment
    const bool valid = tp < len;
    const size_t Da = (size_t)H * 64, kv_plane = (size_t)H * pitch * 64;
    const size_t row = (size_t)s0 + tp, prow = (size_t)e * 32 + t;
    const float* src = qkv + row * 3 * Da + (size_t)h * 64 + 8 * c;
    float cs[8], sn[8];
    if (valid && pos) {
        const size_t p = (size_t)pos[row] * 64 + 8 * c;
#pragma unroll
        for (int i = 0; i < 8; ++i) { cs[i] = cos_t[p + i]; sn[i] = sin_t[p + i]; }
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) { cs[i] = 1.0f; sn[i] = 0.0f; }
    }
#pragma unroll
    for (int which = 0; which < 3; ++which) {
        float x[8];
        if (valid) {
            const f32x4 a0 = *reinterpret_cast<const f32x4*>(src + which * Da), a1 = *reinterpret_cast<const f32x4*>(src + which * Da + 4);
#pragma unroll
            for (int i = 0; i < 4; ++i) { x[i] = a0[i]; x[4 + i] = a1[i]; }
            if (which < 2) {                                   // slots (i, i + 32) rotate together: y = x cos -/+ partner sin
                const float* ps = src + which * Da + ((c < 4) ? 32 : -32);
                const f32x4 p0 = *reinterpret_cast<const f32x4*>(ps), p1 = *reinterpret_cast<const f32x4*>(ps + 4);
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const float pv = i < 4 ? p0[i] : p1[i - 4];
                    x[i] = (c < 4) ? x[i] * cs[i] + (-pv) * sn[i] : x[i] * cs[i] + pv * sn[i];
                }
            }
            if (which == 0) {
#pragma unroll
                for (int i = 0; i < 8; ++i) x[i] *= kQLog2e;
            }
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) x[i] = 0.0f;
        }
        _Float16 hh[8], ll[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) split_act(x[i], hh[i], ll[i]);
        const u32x4 vh = {pack_h2(hh[0], hh[1]), pack_h2(hh[2], hh[3]), pack_h2(hh[4], hh[5]), pack_h2(hh[6], hh[7])};
        const u32x4 vl = {pack_h2(ll[0], ll[1]), pack_h2(ll[2], ll[3]), pack_h2(ll[4], ll[5]), pack_h2(ll[6], ll[7])};
        if (which == 0) {
            if (valid) {
                unsigned short* dst = q16 + row * Da + (size_t)h * 64 + 8 * c;
                *reinterpret_cast<u32x4*>(dst) = vh;
                *reinterpret_cast<u32x4*>(dst + q_plane) = vl;
            }
        } else if (which == 1) {                               // pad rows of the tile are written too (zeros)
            unsigned short* dst = k16 + ((size_t)h * pitch + prow) * 64 + 8 * c;
            *reinterpret_cast<u32x4*>(dst) = vh;
            *reinterpret_cast<u32x4*>(dst + kv_plane) = vl;
        } else {
            *reinterpret_cast<u32x4*>(&sv[0][t][8 * c]) = vh;
            *reinterpret_cast<u32x4*>(&sv[1][t][8 * c]) = vl;
        }
    }
    __syncthreads();
    const int d = tid >> 2, ch = tid & 3;                      // V^T: dim d, stored positions 8 ch .. 8 ch + 7
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        unsigned short w[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) w[i] = sv[p][vt_key(8 * ch + i)][d];
        const u32x4 v = {(unsigned)w[0] | ((unsigned)w[1] << 16), (unsigned)w[2] | ((unsigned)w[3] << 16),
                         (unsigned)w[4] | ((unsigned)w[5] << 16), (unsigned)w[6] | ((unsigned)w[7] << 16)};
        *reinterpret_cast<u32x4*>(vt16 + p * kv_plane + ((size_t)h * 64 + d) * pitch + (size_t)e * 32 + 8 * ch) = v;
    }
}

struct PrefixAttArgs {
    const unsigned short* q16; size_t q_plane;
    const unsigned short* k16; const unsigned short* vt16; size_t pitch;          // own segments
    const unsigned short* pk16; const unsigned short* pvt16; size_t ppitch;       // shared prefix
    int P;
    const int32_t* seg_off; const int32_t* ent_seg; const int32_t* ent_tile;
    int n_ent, n_grp, H;
    float* ctx; unsigned short* ctx16;
};

template <int OUT, bool OWN = true>
__global__ __launch_bounds__(PFX_WPB * 64) void prefix_attention_kernel(const PrefixAttArgs a) {
    __shared__ __attribute__((aligned(16))) u32x4 lds[2 * PFX_STG];
    // XCD-local order: workgroup i runs on XCD i % 8; head 8 s + i % 8 keeps all its workgroups (and its prefix planes) on one XCD
    const int k = (int)blockIdx.x >> 3;
    const int hslot = k / a.n_grp, grp = k - hslot * a.n_grp;
    const int h = hslot * 8 + ((int)blockIdx.x & 7);
    if (h >= a.H) return;                                       // block-uniform: the last head group is padded
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, kh = lane >> 5;
    const int e = grp * PFX_WPB + wave;
    const bool active = e < a.n_ent;
    const int ec = active ? e : a.n_ent - 1;
    const int b = a.ent_seg[ec], jt = a.ent_tile[ec];
    const int s0 = a.seg_off[b], len = a.seg_off[b + 1] - s0;
    const int q0 = jt * 32;                                     // the wave's first query position inside its segment
    const size_t prow0 = (size_t)(ec - jt) * 32;                // padded row of the segment's key 0
    const size_t Da = (size_t)a.H * 64;
    const size_t kv_plane = (size_t)a.H * a.pitch * 64, pkv_plane = (size_t)a.H * a.ppitch * 64;

    u32x4 qh[4], ql[4];                                         // lane (r, kh): Q[q0 + r][16 s + 8 kh .. + 7], both planes
    {
        const unsigned short* qp = a.q16 + ((size_t)s0 + min(q0 + r, len - 1)) * Da + (size_t)h * 64 + kh * 8;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            qh[s] = *reinterpret_cast<const u32x4*>(qp + s * 16);
            ql[s] = *reinterpret_cast<const u32x4*>(qp + a.q_plane + s * 16);
        }
    }
    f32x16 om[2], oc[2];
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int v = 0; v < 16; ++v) { om[dt][v] = 0.f; oc[dt][v] = 0.f; }
    float m_run = -INFINITY, l_run = 0.f;
    constexpr float kInvLo = 1.0f / kLoScale;
    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

    // One key tile through the online softmax (attention_f16.hip's tile body).  Keys key0 + i of the tile with key0 + i >= lim are masked
    // when need_mask (wave-uniform); every tile that gets here holds at least one visible key per row.
    auto update = [&](const u32x4 (&kfh)[4], const u32x4 (&kfl)[4], const u32x4 (&vfh)[2][2], const u32x4 (&vfl)[2][2], int key0,
                      bool need_mask, int lim) {
        f32x16 sm, sc;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            sc = mfma_h(kfh[s], ql[s], s == 0 ? zero16 : sc);
            sc = mfma_h(kfl[s], qh[s], sc);
            sm = mfma_h(kfh[s], qh[s], s == 0 ? zero16 : sm);
        }
        float st[16];
#pragma unroll
        for (int v = 0; v < 16; ++v) st[v] = fmaf(sc[v], kInvLo, sm[v]);
        if (need_mask) {
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int key = key0 + (v & 3) + 8 * (v >> 2) + 4 * kh;
                if (key >= lim) st[v] = -INFINITY;
            }
        }
        float mloc = st[0];
#pragma unroll
        for (int v = 1; v < 16; ++v) mloc = fmaxf(mloc, st[v]);
        {
            const unsigned int mu = __builtin_bit_cast(unsigned int, mloc);
            const auto sw = __builtin_amdgcn_permlane32_swap(mu, mu, false, false);
            const unsigned int x0 = sw[0], x1 = sw[1];
            mloc = fmaxf(__builtin_bit_cast(float, x0), __builtin_bit_cast(float, x1));
        }
        const float m_new = fmaxf(m_run, mloc);
        // deferred rescale: the branch is wave-wide, the new reference PER ROW (a row that moved by less keeps alpha == 1 and its
        // reference), so a row's bits depend on its own scores only
        if (!__all(m_new <= m_run + kAttDefer)) {
            const bool moved = m_new > m_run + kAttDefer;
            const float alpha = moved ? __builtin_amdgcn_exp2f(m_run - m_new) : 1.0f;
            l_run *= alpha;
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                for (int v = 0; v < 16; ++v) { om[dt][v] *= alpha; oc[dt][v] *= alpha; }
            if (moved) m_run = m_new;
        }
        const float mb = m_run - 10.0f;
#pragma unroll
        for (int v = 0; v < 16; ++v) st[v] = __builtin_amdgcn_exp2f(st[v] - mb);       // P * 2^10
        l_run += ((st[0] + st[1]) + (st[2] + st[3])) + ((st[4] + st[5]) + (st[6] + st[7])) +
                 (((st[8] + st[9]) + (st[10] + st[11])) + ((st[12] + st[13]) + (st[14] + st[15])));
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            u32x4 ph, pl;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const u32x2 p = split_p(st[8 * m + 2 * i], st[8 * m + 2 * i + 1]);
                ph[i] = p[0];
                pl[i] = p[1];
            }
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) {
                oc[dt] = mfma_h(vfh[dt][m], pl, oc[dt]);
                oc[dt] = mfma_h(vfl[dt][m], ph, oc[dt]);
                om[dt] = mfma_h(vfh[dt][m], ph, om[dt]);
            }
        }
    };

    // ---- the shared prefix: block-wide, tiles staged through LDS ----
    const int npt = (a.P + AKT - 1) / AKT;
    if (npt > 0) {
        u32x4 stg[4];
        // thread tid moves chunk tid of each of the four plane tiles: K (key tid / 8, chunk tid % 8, swizzled), V^T (dim tid / 4, chunk tid % 4)
        const int kkey = tid >> 3, kc = (tid & 7) ^ k_swizzle<64>(kkey);
        const int vd = tid >> 2, vc = (tid & 3) ^ ((vd >> 2) & 3);
        const unsigned short* ksrc = a.pk16 + ((size_t)h * a.ppitch + kkey) * 64 + kc * 8;
        const unsigned short* vsrc = a.pvt16 + ((size_t)h * 64 + vd) * a.ppitch + vc * 8;
        auto fetch = [&](int kt) {
            stg[0] = *reinterpret_cast<const u32x4*>(ksrc + (size_t)kt * AKT * 64);
            stg[1] = *reinterpret_cast<const u32x4*>(ksrc + pkv_plane + (size_t)kt * AKT * 64);
            stg[2] = *reinterpret_cast<const u32x4*>(vsrc + (size_t)kt * AKT);
            stg[3] = *reinterpret_cast<const u32x4*>(vsrc + pkv_plane + (size_t)kt * AKT);
        };
        auto stash = [&](int buf) {
            u32x4* dst = lds + buf * PFX_STG + tid;
            dst[0] = stg[0]; dst[PFX_KCH] = stg[1]; dst[2 * PFX_KCH] = stg[2]; dst[2 * PFX_KCH + PFX_VCH] = stg[3];
        };
        fetch(0);
        stash(0);
        __syncthreads();
        for (int kt = 0; kt < npt; ++kt) {
            const bool more = kt + 1 < npt;
            if (more) fetch(kt + 1);                            // the next tile's loads fly during this tile's MFMAs
            if (active) {
                const u32x4* Kb = lds + (kt & 1) * PFX_STG;
                const u32x4* Vb = Kb + 2 * PFX_KCH;
                u32x4 kfh[4], kfl[4], vfh[2][2], vfl[2][2];
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const int ci = r * 8 + ((2 * s + kh) ^ k_swizzle<64>(r));
                    kfh[s] = Kb[ci];
                    kfl[s] = Kb[PFX_KCH + ci];
                }
#pragma unroll
                for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                    for (int m = 0; m < 2; ++m) {
                        const int ci = v_chunk(dt * 32 + r, m, kh);
                        vfh[dt][m] = Vb[ci];
                        vfl[dt][m] = Vb[PFX_VCH + ci];
                    }
                update(kfh, kfl, vfh, vfl, kt * AKT, kt * AKT + AKT > a.P, a.P);
            }
            if (more) stash((kt + 1) & 1);                      // the other stage: last read before the previous barrier
            __syncthreads();
        }
    }
    if (!active) return;                                        // no barrier below

    // ---- the wave's own segment: causal, tiles 0 .. jt, fragments straight from global memory ----
    if constexpr (OWN) {
        const unsigned short* kb = a.k16 + ((size_t)h * a.pitch + prow0 + r) * 64 + kh * 8;
        const unsigned short* vb = a.vt16 + ((size_t)h * 64 + r) * a.pitch + prow0 + kh * 8;
        for (int kt = 0; kt <= jt; ++kt) {
            u32x4 kfh[4], kfl[4], vfh[2][2], vfl[2][2];
            const unsigned short* kp = kb + (size_t)kt * AKT * 64;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                kfh[s] = *reinterpret_cast<const u32x4*>(kp + s * 16);
                kfl[s] = *reinterpret_cast<const u32x4*>(kp + kv_plane + s * 16);
            }
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                for (int m = 0; m < 2; ++m) {
                    const unsigned short* vp = vb + (size_t)dt * 32 * a.pitch + (size_t)kt * AKT + 16 * m;
                    vfh[dt][m] = *reinterpret_cast<const u32x4*>(vp);
                    vfl[dt][m] = *reinterpret_cast<const u32x4*>(vp + kv_plane);
                }
            update(kfh, kfl, vfh, vfl, kt * AKT, kt == jt, q0 + r + 1);       // the diagonal tile: keys beyond the query are masked
        }
    }

    const float l_tot = l_run + __shfl_xor(l_run, 32);
    const float inv = 1.0f / l_tot;
    const bool row_ok = q0 + r < len;
    const size_t orow = (size_t)s0 + min(q0 + r, len - 1);
    if (OUT == ATT_OUT_SPLIT) store_ctx_split<2>(om, oc, inv, kInvLo, row_ok, a.ctx16 + orow * (2 * Da) + (size_t)h * 128, kh);
    else if (row_ok) store_ctx_f32<2>(om, oc, inv, kInvLo, a.ctx + orow * Da + (size_t)h * 64 + 4 * kh);
}

static int prefix_check(const PrefixAttLaunch& p) {
    if (p.H <= 0 || p.n_seg <= 0 || p.n_ent <= 0 || p.P < 0 || !p.seg_off || !p.ent_seg || !p.ent_tile || !p.q16 || !p.k16 || !p.vt16 ||
        (p.P > 0 && (!p.pk16 || !p.pvt16))) {
        set_error("prefix attention: bad arguments H=%d segments=%d tiles=%d P=%d", p.H, p.n_seg, p.n_ent, p.P);
        return PGMI_EINVAL;
    }
    if (p.pitch % 32 || (size_t)p.n_ent * 32 > p.pitch || (p.P > 0 && (p.ppitch % 32 || (size_t)(p.P + 31) / 32 * 32 > p.ppitch))) {
        set_error("prefix attention: %d query tiles / %d prefix keys do not fit the operand pitches %zu / %zu", p.n_ent, p.P, p.pitch, p.ppitch);
        return PGMI_EINVAL;
    }
    return PGMI_OK;
}

int launch_prefix_prep(const PrefixAttLaunch& p) {
    int rc = prefix_check(p);
    if (rc) return rc;
    if (!p.qkv || (p.pos && (!p.cos_t || !p.sin_t))) { set_error("prefix attention prep: bad arguments"); return PGMI_EINVAL; }
    hipLaunchKernelGGL(prefix_prep_kernel, dim3(p.n_ent, p.H), dim3(256), 0, p.stream, p.qkv, p.pos, p.cos_t, p.sin_t, p.seg_off, p.ent_seg,
                       p.ent_tile, p.H, p.q16, p.q_plane, p.k16, p.vt16, p.pitch);
    PGMI_HIP(hipGetLastError());
    return PGMI_OK;
}

int launch_prefix_attention(const PrefixAttLaunch& p) {
    int rc = prefix_check(p);
    if (rc) return rc;
    if ((p.out == ATT_OUT_F32 && !p.ctx) || (p.out == ATT_OUT_SPLIT && !p.ctx16) || (p.out != ATT_OUT_F32 && p.out != ATT_OUT_SPLIT)) {
        set_error("prefix attention: fp32 or split-plane context rows only");
        return PGMI_EINVAL;
    }
    PrefixAttArgs a;
    a.q16 = p.q16; a.q_plane = p.q_plane;
    a.k16 = p.k16; a.vt16 = p.vt16; a.pitch = p.pitch;
    a.pk16 = p.pk16; a.pvt16 = p.pvt16; a.ppitch = p.ppitch; a.P = p.P;
    a.seg_off = p.seg_off; a.ent_seg = p.ent_seg; a.ent_tile = p.ent_tile;
    a.n_ent = p.n_ent; a.n_grp = (p.n_ent + PFX_WPB - 1) / PFX_WPB; a.H = p.H;
    a.ctx = p.ctx; a.ctx16 = p.ctx16;
    const long long blocks = 8ll * ((p.H + 7) / 8) * a.n_grp;
    if (blocks > 0x7fffffffll) { set_error("prefix attention: launch of %lld workgroups", blocks); return PGMI_EINVAL; }
    if (p.out == ATT_OUT_SPLIT) hipLaunchKernelGGL(prefix_attention_kernel<ATT_OUT_SPLIT>, dim3((unsigned)blocks), dim3(PFX_WPB * 64), 0, p.stream, a);
    else hipLaunchKernelGGL(prefix_attention_kernel<ATT_OUT_F32>, dim3((unsigned)blocks), dim3(PFX_WPB * 64), 0, p.stream, a);
    PGMI_HIP(hipGetLastError());
    return PGMI_OK;
}

// fp32 q rows [rows][H 64] -> the two q16 planes, times log2(e): what prefix_prep_kernel does to its q block without rotary.
// One thread per 8-column chunk.
__global__ __launch_bounds__(256) void cross_q_prep_kernel(const float* __restrict__ q, size_t n_chunks, unsigned short* __restrict__ q16,
                                                           size_t q_plane) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_chunks) return;
    const f32x4 a0 = *reinterpret_cast<const f32x4*>(q + i * 8), a1 = *reinterpret_cast<const f32x4*>(q + i * 8 + 4);
    _Float16 hh[8], ll[8];
#pragma unroll
    for (int k = 0; k < 4; ++k) { split_act(a0[k] * kQLog2e, hh[k], ll[k]); split_act(a1[k] * kQLog2e, hh[4 + k], ll[4 + k]); }
    const u32x4 vh = {pack_h2(hh[0], hh[1]), pack_h2(hh[2], hh[3]), pack_h2(hh[4], hh[5]), pack_h2(hh[6], hh[7])};
    const u32x4 vl = {pack_h2(ll[0], ll[1]), pack_h2(ll[2], ll[3]), pack_h2(ll[4], ll[5]), pack_h2(ll[6], ll[7])};
    *reinterpret_cast<u32x4*>(q16 + i * 8) = vh;
    *reinterpret_cast<u32x4*>(q16 + q_plane + i * 8) = vl;
}

int launch_cross_q_prep(const float* q, size_t rows, int H, unsigned short* q16, size_t q_plane, hipStream_t s) {
    const size_t n_chunks = rows * (size_t)H * 8, blocks = (n_chunks + 255) / 256;
    if (!q || !q16 || rows == 0 || H <= 0 || q_plane < rows * (size_t)H * 64 || blocks > 0x7fffffffull) {
        set_error("cross attention prep: bad arguments rows=%zu H=%d", rows, H);
        return PGMI_EINVAL;
    }
    hipLaunchKernelGGL(cross_q_prep_kernel, dim3((unsigned)blocks), dim3(256), 0, s, q, n_chunks, q16, q_plane);
    PGMI_HIP(hipGetLastError());
    return PGMI_OK;
}

int launch_cross_attention(const PrefixAttLaunch& p) {
    if (p.H <= 0 || p.n_seg <= 0 || p.n_ent <= 0 || p.P <= 0 || !p.seg_off || !p.ent_seg || !p.ent_tile || !p.q16 || !p.pk16 || !p.pvt16) {
        set_error("cross attention: bad arguments H=%d segments=%d tiles=%d S=%d", p.H, p.n_seg, p.n_ent, p.P);
        return PGMI_EINVAL;
    }
    if (p.ppitch % 32 || (size_t)(p.P + 31) / 32 * 32 > p.ppitch) {
        set_error("cross attention: %d memory keys do not fit the operand pitch %zu", p.P, p.ppitch);
        return PGMI_EINVAL;
    }
    if ((p.out == ATT_OUT_F32 && !p.ctx) || (p.out == ATT_OUT_SPLIT && !p.ctx16) || (p.out != ATT_OUT_F32 && p.out != ATT_OUT_SPLIT)) {
        set_error("cross attention: fp32 or split-plane context rows only");
        return PGMI_EINVAL;
    }
    PrefixAttArgs a;
    a.q16 = p.q16; a.q_plane = p.q_plane;
    a.k16 = nullptr; a.vt16 = nullptr; a.pitch = 0;
    a.pk16 = p.pk16; a.pvt16 = p.pvt16; a.ppitch = p.ppitch; a.P = p.P;
    a.seg_off = p.seg_off; a.ent_seg = p.ent_seg; a.ent_tile = p.ent_tile;
    a.n_ent = p.n_ent; a.n_grp = (p.n_ent + PFX_WPB - 1) / PFX_WPB; a.H = p.H;
    a.ctx = p.ctx; a.ctx16 = p.ctx16;
    const long long blocks = 8ll * ((p.H + 7) / 8) * a.n_grp;
    if (blocks > 0x7fffffffll) { set_error("cross attention: launch of %lld workgroups", blocks); return PGMI_EINVAL; }
    if (p.out == ATT_OUT_SPLIT) hipLaunchKernelGGL((prefix_attention_kernel<ATT_OUT_SPLIT, false>), dim3((unsigned)blocks), dim3(PFX_WPB * 64), 0, p.stream, a);
    else hipLaunchKernelGGL((prefix_attention_kernel<ATT_OUT_F32, false>), dim3((unsigned)blocks), dim3(PFX_WPB * 64), 0, p.stream, a);
    PGMI_HIP(hipGetLastError());
    return PGMI_OK;
}

}  // namespace pgmi
