// Fused multi-head self-attention on the 16-bit matrix pipe with split-fp16 (f16x3) operands.
//
// Math: q k^T, fp32 softmax, P v (reference: /root/reference/proteingym/baselines/esm/esm/multihead_attention.py:357-387;
// Tranception: tranception/model_pytorch.py:155-183).  One wave = 32 queries of one head, S^T = K Q^T so the query lives in the
// lane, P is consumed straight from the accumulator registers.  Every product is evaluated as
//     x y  ~=  x_hi y_hi + 2^-11 (x_hi y_lo + x_lo y_hi),   x_hi = fp16(x), x_lo = fp16((x - x_hi) 2^11)
// with v_mfma_f32_32x32x16_f16: 24 MFMAs per (32q x 32k) tile.  The 2^-11 terms are kept in their own accumulators and folded in
// fp32 (S = main + corr/2048 before the softmax, O likewise at the end), so no fp16 subnormal is ever produced.
// Operands arrive already split (from the fused QKV projection's epilogue, gemm16x_kernel.h OUT 2, or from the prep passes below):
//   qk16 [plane][M][2D]      q | k, row-major (hi plane, lo 2^11 plane); q carries head_dim^-1/2 log2(e)
//   vt16 [plane][B*H*64][Tp] V transposed per (sequence, head), keys of each 32-key tile stored with bits 2 and 3 of the key index
//                            swapped (the order the S^T accumulator holds them), pad keys = 0
#include <stdlib.h>
#include <string.h>
#include <algorithm>

#include "attention_f16_common.h"

namespace pgmi {

// DO < DH (head_dim 256): a workgroup computes the scores over all DH dims but the context of only the DO dims d0 .. d0 + DO - 1 of its
// head (d0 = slice * DO, DH / DO slices per head, one more level of the launch's (sequence, head) list): the O accumulators of a
// 32 x 256 tile (256 registers per lane) would not fit beside the Q fragments; S is recomputed once per slice.
template <int WPB, int OUT, int NSTG, int DH = 64, bool RAG = false, int DO = DH>
__global__ __launch_bounds__(WPB * 64) void attention_f16x3_v2_kernel(
    const unsigned short* __restrict__ qk16, size_t qk_plane, const unsigned short* __restrict__ vt16,
    size_t vt_plane, const int32_t* __restrict__ kv_len, const float* __restrict__ slopes, int T, int H,
    int Tp, float* __restrict__ ctx, unsigned short* __restrict__ ctx16, RagMap rag, int dense_nblk, int nseq) {
    constexpr float defer_thr = kAttDefer;
    // slopes != nullptr selects the Tranception flavour (tranception/model_pytorch.py:155-183): causal
    // mask (key <= query) and the grouped-ALiBi bias slope[h] * key added to the scaled scores.
    constexpr int NT = WPB * 64;
    // A tile is 16 wave-instructions of 64 chunks (K hi, K lo, V^T hi, V^T lo: 1024 x 16 B) at DH 64, 32 at DH 128, 48 at DH 256 / DO 128.
    // Every wave issues the same number NDMA of them (counted vmcnt needs a per-wave constant).
    constexpr int KCPR = DH / 8;                        // 16-byte chunks per key row of a K plane
    constexpr int KCH = AKT * KCPR, VCH = DO * 4;       // chunks per K plane / V^T plane (the slice's DO rows) of a tile
    constexpr int NSL = DH / DO;                        // context slices per head
    static_assert(NSL == 1 || (OUT == ATT_OUT_SPLIT && !RAG), "sliced context: split-plane output of dense launches only");
    constexpr int STG_CH = 2 * KCH + 2 * VCH;           // chunks per stage (16 KB at DH 64, 32 KB at DH 128)
    constexpr int NWI = STG_CH / 64;                    // wave-instructions per tile
    static_assert(NWI % WPB == 0, "the wave-instructions of a stage divide evenly over the waves");
    constexpr int NDMA = NWI / WPB;
    constexpr int NS = DH / 16, ND = DO / 32;
    extern __shared__ __attribute__((aligned(16))) u32x4 lds[];   // [NSTG][STG_CH]

    // Dense launches with dense_nblk > 0 are one-dimensional in the XCD-local order (xcd_local_pair), else a (query block, head, sequence) grid
    int b, h, qblk_dense, hs;                   // hs: (head, slice) index, h * NSL + slice
    if (RAG) {
        b = rag.ent_seq[blockIdx.x];
        hs = blockIdx.y;
        qblk_dense = 0;
    } else if (dense_nblk > 0) {
        const int pair = xcd_local_pair(dense_nblk, qblk_dense);
        if (pair >= nseq * H * NSL) return;
        b = pair / (H * NSL);
        hs = pair - b * (H * NSL);
    } else {
        b = blockIdx.z;
        hs = blockIdx.y;
        qblk_dense = blockIdx.x;
    }
    h = hs / NSL;
    const int d0 = (hs - h * NSL) * DO;         // first context dim of this workgroup's slice
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);     // provably wave-uniform: scalar branches, SGPR DMA bases
    const int r = lane & 31, kh = lane >> 5;
    const int D = H * DH;
    const int Tk = (!RAG && kv_len) ? kv_len[b] : T;
    // RAG: p0 = first token the sequence owns, a0 = its tile; row0 / rrow0 = operand row of ITS token a0 / of its root's token 0; kt0 = first
    // own key tile; orow0 + t = context (output) row of token t >= p0
    const int p0 = RAG ? rag.seq_p[b] : 0, a0 = p0 & ~(AKT - 1), kt0 = a0 / AKT;
    const int qblk = RAG ? rag.ent_j[blockIdx.x] : qblk_dense;
    const int row0 = RAG ? rag.seq_q[b] : b * T, rrow0 = RAG ? rag.seq_q[rag.seq_root[b]] : 0;
    const int orow0 = RAG ? rag.seq_off[b] - p0 : b * T;
    const int Tpo = RAG ? (T - a0 + 31) / 32 * 32 : Tp;            // row pitch of the sequence's own V^T block
    const int q0 = a0 + (qblk * WPB + wave) * 32;                  // absolute position of the wave's first query
    const bool active = q0 < T;
    // (Two workgroups share a CU, one wave of each per SIMD.  Measured and not kept, profiles/r3: a static priority for the wave in
    // the odd hardware slot, -3 %; the lane <-> lane + 32 max exchange through LDS instead of v_permlane32_swap, -1.3 %; 8-byte
    // epilogue stores, -8 %; Q fragments straight from global memory, -2 %.)

    // Q fragments: lane (r,kh) holds Q[q0+r][16s + 8kh .. +7] of both planes.  Loaded straight from the planes each of the 2 NS
    // 16-byte loads of a wave touches 32 different rows (one per lane pair): 8 x 32 row segments for an 8 KB tile.  With
    // kQviaLds the wave's Q tile is instead moved like a K tile -- 8 lanes per 128-byte row, DMA into LDS in the K tile's swizzled
    // image (ring stages 1 and 2 are still free) -- and the fragments are read from there: a quarter of the row segments on the
    // texture-address path, which this kernel keeps busy (9 % of wave-cycles with its FIFO full).
    constexpr bool q_lds = NSTG >= 3;
    u32x4 qh[NS], ql[NS];
    if (!q_lds) {
        const int qrow = min(q0 + r, T - 1);
        const unsigned short* qp = qk16 + ((size_t)row0 + (qrow - a0)) * (2 * D) + h * DH + kh * 8;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            qh[s] = *reinterpret_cast<const u32x4*>(qp + s * 16);
            ql[s] = *reinterpret_cast<const u32x4*>(qp + qk_plane + s * 16);
        }
    }

    // DMA map: LDS slot f (0 .. STG_CH-1 within a stage) <- global chunk
    //   f in [0, 2 KCH):        K plane p = f / KCH, key = (f % KCH) / KCPR, slot chunk c' = f % KCPR, source chunk c = c' ^ swz(key)
    //                           swz(key) = (key >> 1) & 7 for 128-byte rows (DH 64), key & 15 for 256-byte rows (DH 128)
    //   f in [2 KCH, STG_CH):   V^T plane p, row d = (g >> 2) % DH, c' = g & 3, source chunk c = c' ^ ((d >> 2) & 3)
    // Every wave-instruction (64 slots) lies inside ONE plane of one tensor, so the tensor, the plane and the (sequence, head,
    // tile) part of the address are wave-uniform: they go into the buffer descriptor and the SGPR offset, the lane keeps one
    // 32-bit byte offset per instruction -- no per-tile address arithmetic.
    // The descriptors are based at THIS block's sequence / (sequence, head) in the hi plane, so the 32-bit offsets only span one plane
    // stride plus one sequence (the launcher checks plane * 2 + extent < 4 GiB): operand arrays themselves may be larger than 4 GiB
    // (an MSA Transformer workspace of 1024 x 1024 tokens).  b and h are block-uniform: the bases stay in SGPRs.
    const size_t seq_halfs = (size_t)T * (2 * D), vt_halfs = (size_t)DH * Tp;
    const unsigned long long qk_bytes = std::min<unsigned long long>(0xFFFFFFFFull, (unsigned long long)qk_plane * 2ull + seq_halfs * 2ull);
    const unsigned long long vt_bytes = std::min<unsigned long long>(0xFFFFFFFFull, (unsigned long long)vt_plane * 2ull + vt_halfs * 2ull);
    const __amdgpu_buffer_rsrc_t rsQK = operand_rsrc(qk16 + (size_t)row0 * (2 * D), qk_bytes);
    const __amdgpu_buffer_rsrc_t rsVT = operand_rsrc(vt16 + (RAG ? (size_t)rag.seq_vt[b] + (size_t)h * DH * Tpo : ((size_t)b * H + h) * vt_halfs), vt_bytes);
    // RAG: the root's planes for the key tiles before kt0 (the root owns all of its T tokens: V^T row pitch Tp)
    const __amdgpu_buffer_rsrc_t rsQKr = operand_rsrc(qk16 + (size_t)rrow0 * (2 * D), qk_bytes);
    const __amdgpu_buffer_rsrc_t rsVTr = operand_rsrc(vt16 + (RAG ? (size_t)rag.seq_vt[rag.seq_root[b]] + (size_t)h * DH * Tp : (size_t)0), vt_bytes);
    // causal: keys beyond the block's last query tile are never needed (uniform bound for the block)
    const bool causal = slopes != nullptr;
    const int last_q = min(T, a0 + (qblk * WPB + WPB) * 32);
    const int nkt = causal ? (min(Tk, last_q) + AKT - 1) / AKT : (Tk + AKT - 1) / AKT;
    // voff_last: the same offsets for the LAST key tile with its K rows clamped to the sequence's last row (finite, masked by Tk) --
    // the only tile that can reach past row T-1, i.e. into the next sequence or past the end of the operand
    int voff[NDMA], voff_last[NDMA], voff_root[NDMA], sbase[NDMA], sstep[NDMA], slot0[NDMA];
    bool is_k[NDMA];
#pragma unroll
    for (int i = 0; i < NDMA; ++i) {
        int wi = wave + WPB * i;                          // wave-instruction index 0 .. NWI-1
        // Never taken (wave < WPB and WPB divides NWI), but hipcc cannot see that `wave` is below WPB: without this line it compiles a
        // different kernel (145 to 997 fewer instructions, every instantiation).  That is a kernel change, to be made and timed as one.
        if (wi >= NWI) wi -= NWI;
        slot0[i] = wi * 64;
        is_k[i] = wi < 2 * KCH / 64;
        if (is_k[i]) {
            const int p = wi / (KCH / 64), key = ((wi % (KCH / 64)) * 64 + lane) / KCPR;
            const int c = (lane % KCPR) ^ k_swizzle<DH>(key);
            voff[i] = voff_root[i] = key * (2 * D) * 2 + c * 16;
            voff_last[i] = min(key, T - 1 - (nkt - 1) * AKT) * (2 * D) * 2 + c * 16;
            sbase[i] = (int)((unsigned int)p * (unsigned int)qk_plane * 2u + (unsigned int)(D + h * DH) * 2u);
            sstep[i] = AKT * (2 * D) * 2;
        } else {
            const int wv = wi - 2 * KCH / 64, p = wv / (VCH / 64), g = (wv % (VCH / 64)) * 64 + lane;
            const int d = g >> 2, c = (g & 3) ^ ((d >> 2) & 3);
            voff[i] = voff_last[i] = (d0 + d) * Tpo * 2 + c * 16;
            voff_root[i] = (d0 + d) * Tp * 2 + c * 16;
            sbase[i] = (int)((unsigned int)p * (unsigned int)vt_plane * 2u);
            sstep[i] = (AKT / 8) * 16;
        }
    }
    auto issue_tile = [&](int kt, int buf) {
        u32x4* base = lds + buf * STG_CH;
        const bool from_root = RAG && kt < kt0;               // wave-uniform: a scalar select of the descriptor
#pragma unroll
        for (int i = 0; i < NDMA; ++i) {
            const int vo = from_root ? voff_root[i] : ((kt == nkt - 1) ? voff_last[i] : voff[i]);
            const int so = sbase[i] + (from_root ? kt : kt - kt0) * sstep[i];
            // (soffset goes through a named local: with the array expression written in the call hipcc 7.2 silently drops the kernel's host stub)
            if (is_k[i]) __builtin_amdgcn_raw_ptr_buffer_load_lds(from_root ? rsQKr : rsQK, (__attribute__((address_space(3))) void*)(base + slot0[i]), 16, vo, so, 0, 0);
            else __builtin_amdgcn_raw_ptr_buffer_load_lds(from_root ? rsVTr : rsVT, (__attribute__((address_space(3))) void*)(base + slot0[i]), 16, vo, so, 0, 0);
        }
    };

    // NSTG-deep LDS ring, K/V tiles prefetched NSTG-1 ahead with counted vmcnt (the DMAs stay in
    // flight across the barrier; a __syncthreads() would drain them)
    constexpr float kLog2e = 1.4426950408889634f;
    const float slope2 = causal ? slopes[h] * kLog2e : 0.0f;      // the q planes carry log2(e) (kQLog2e), the ALiBi term must too
    if (q_lds) {
        issue_tile(0, 0);
        u32x4* qbase = lds + STG_CH + wave * (2 * KCH);             // this wave's half of stages 1 .. 2: [2 planes][32 rows][KCPR chunks]
        if (active) {
            constexpr int NQ = 2 * KCH / 64;                        // wave-instructions of 1 KiB
#pragma unroll
            for (int i = 0; i < NQ; ++i) {
                const int f = i * 64 + lane, pq = f / KCH, row = (f % KCH) / KCPR;
                const int c = (f % KCPR) ^ k_swizzle<DH>(row);
                const int vo = (int)(((unsigned int)(min(q0 + row, T - 1) - a0) * (unsigned int)(2 * D) + (unsigned int)(h * DH)) * 2u + (unsigned int)c * 16u);
                const int so = (int)((unsigned int)pq * (unsigned int)qk_plane * 2u);
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsQK, (__attribute__((address_space(3))) void*)(qbase + i * 64), 16, vo, so, 0, 0);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");            // this wave's share of tile 0 and its own Q tile have landed
        if (active) {
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const int ci = r * KCPR + ((2 * s + kh) ^ k_swizzle<DH>(r));
                qh[s] = qbase[ci];
                ql[s] = qbase[KCH + ci];
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                               // every wave holds its Q in registers: stages 1 and 2 are free again
        asm volatile("" ::: "memory");
#pragma unroll
        for (int t = 1; t < NSTG - 1; ++t)
            if (t < nkt) issue_tile(t, t);
    } else {
#pragma unroll
        for (int t = 0; t < NSTG - 1; ++t)
            if (t < nkt) issue_tile(t, t);
    }

    f32x16 om[ND], oc[ND];
#pragma unroll
    for (int dt = 0; dt < ND; ++dt)
#pragma unroll
        for (int v = 0; v < 16; ++v) { om[dt][v] = 0.f; oc[dt][v] = 0.f; }
    // base-2 online softmax with P scaled by 2^10 (keeps every P hi in fp16's normal range; the
    // factor cancels in O / l because l accumulates the same scaled P)
    float m_run = -INFINITY, l_run = 0.f;
    constexpr float kInvLo = 1.0f / kLoScale;

    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    auto wanted = [&](int kt) -> bool { return active && !(causal && kt * AKT > q0 + 31); };   // causal: tiles above the diagonal are skipped
    // S^T = K Q^T of one key tile: main and 2^-11 correction accumulators
    auto scores = [&](int buf, f32x16& sm, f32x16& sc) {
        const u32x4* Kb = lds + buf * STG_CH;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int ci = r * KCPR + ((2 * s + kh) ^ k_swizzle<DH>(r));
            const u32x4 kfh = Kb[ci], kfl = Kb[KCH + ci];
            sc = mfma_h(kfh, ql[s], s == 0 ? zero16 : sc);       // s == 0: the accumulator operand is the inline constant 0
            sc = mfma_h(kfl, qh[s], sc);
            sm = mfma_h(kfh, qh[s], s == 0 ? zero16 : sm);
        }
    };
    // tile t of this wave's DMA share has landed once at most `younger` tiles issued after it remain in flight
    auto wait_tile = [&](int younger) {
        if (younger >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NDMA) : "memory");
        else if (younger == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NDMA) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    };
    int cur = 0;
    for (int kt = 0; kt < nkt; ++kt) {
        wait_tile(min(NSTG - 2, nkt - 1 - kt));
        __builtin_amdgcn_s_barrier();          // tile kt visible to all waves; slot of tile kt-1 is free
        asm volatile("" ::: "memory");
        if (kt + NSTG - 1 < nkt) issue_tile(kt + NSTG - 1, (cur == 0) ? NSTG - 1 : cur - 1);
        if (wanted(kt)) {
            const u32x4* Vb = lds + cur * STG_CH + 2 * KCH;
            f32x16 sm, sc;
            scores(cur, sm, sc);
            float st[16];
            if (causal) {
                // ALiBi: slope * key index (model_pytorch.py:167-168), key = 32 kt + 4 kh + c_v with c_v a compile-time constant per
                // accumulator register; the causal mask (:161-165) only on tiles that reach beyond the wave's first query -- every
                // tile below the diagonal band is fully visible and skips the 16 compares and selects
                const float kb = (float)(kt * AKT + 4 * kh);                // key index as a float: small integers, every sum below is exact
#pragma unroll
                for (int v = 0; v < 16; ++v)
                    st[v] = fmaf(slope2, kb + (float)((v & 3) + 8 * (v >> 2)), fmaf(sc[v], kInvLo, sm[v]));
                if (kt * AKT + AKT - 1 > q0) {
#pragma unroll
                    for (int v = 0; v < 16; ++v) {
                        const int key = kt * AKT + (v & 3) + 8 * (v >> 2) + 4 * kh;
                        if (key > q0 + r) st[v] = -INFINITY;
                    }
                }
            } else {
#pragma unroll
                for (int v = 0; v < 16; ++v) st[v] = fmaf(sc[v], kInvLo, sm[v]);
            }
            if (kt * AKT + AKT > Tk) {
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    const int key = kt * AKT + (v & 3) + 8 * (v >> 2) + 4 * kh;
                    if (key >= Tk) st[v] = -INFINITY;
                }
            }
            float mloc = st[0];
#pragma unroll
            for (int v = 1; v < 16; ++v) mloc = fmaxf(mloc, st[v]);
            {                                             // v_permlane32_swap: both halves of the query's row without an LDS round trip
                const unsigned int mu = __builtin_bit_cast(unsigned int, mloc);
                const auto sw = __builtin_amdgcn_permlane32_swap(mu, mu, false, false);
                const unsigned int s0 = sw[0], s1 = sw[1];
                mloc = fmaxf(__builtin_bit_cast(float, s0), __builtin_bit_cast(float, s1));
            }
            const float m_new = fmaxf(m_run, mloc);
            // Deferred rescale: the running reference m_run may lag the true row maximum by up to defer_thr (base-2 units).  P is
            // then up to 2^(10 + defer_thr) instead of 2^10 -- still exact to 22 bits in its hi | lo split and, for defer_thr <= 5,
            // inside fp16's range -- and O and l carry the same factor, which cancels in O / l.  The O-wide rescale (36 packed
            // multiplies on 64 accumulator registers + their wait for the previous P V MFMAs) then runs on the first key tiles
            // only instead of on nearly every tile.  defer_thr = 0: rescale whenever any lane's maximum moved (exact running max).
            // The branch is wave-wide (some row moved by more than defer_thr), the new reference is PER ROW: a row that moved by less keeps
            // alpha == 1 and its reference, so its bits depend on its own scores only -- not on which rows share its wave.
            if (!__all(m_new <= m_run + defer_thr)) {
                const bool moved = m_new > m_run + defer_thr;
                const float alpha = moved ? __builtin_amdgcn_exp2f(m_run - m_new) : 1.0f;
                l_run *= alpha;
#pragma unroll
                for (int dt = 0; dt < ND; ++dt)
#pragma unroll
                    for (int v = 0; v < 16; ++v) { om[dt][v] *= alpha; oc[dt][v] *= alpha; }
                if (moved) m_run = m_new;
            }
            const float mb = m_run - 10.0f;
            typedef float f32x2 __attribute__((ext_vector_type(2)));
#pragma unroll
            for (int v = 0; v < 16; v += 2) {                    // packed fp32 subtract (v_pk_add_f32): same values, half the issue slots
                const f32x2 dlt = f32x2{st[v], st[v + 1]} - f32x2{mb, mb};
                st[v] = __builtin_amdgcn_exp2f(dlt[0]);          // P * 2^10 in [0, 1024 * 2^defer_thr]
                st[v + 1] = __builtin_amdgcn_exp2f(dlt[1]);
            }
            // row sum as a tree (four independent chains of depth 2 + 2): a 16-long serial add chain is 16 dependent-issue latencies
            l_run += ((st[0] + st[1]) + (st[2] + st[3])) + ((st[4] + st[5]) + (st[6] + st[7])) +
                     (((st[8] + st[9]) + (st[10] + st[11])) + ((st[12] + st[13]) + (st[14] + st[15])));
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                u32x4 ph, pl;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const u32x2 p = split_p(st[8 * m + 2 * e], st[8 * m + 2 * e + 1]);
                    ph[e] = p[0];
                    pl[e] = p[1];
                }
#pragma unroll
                for (int dt = 0; dt < ND; ++dt) {
                    const int ci = v_chunk(dt * 32 + r, m, kh);
                    const u32x4 vfh = Vb[ci], vfl = Vb[VCH + ci];
                    oc[dt] = mfma_h(vfh, pl, oc[dt]);
                    oc[dt] = mfma_h(vfl, ph, oc[dt]);
                    om[dt] = mfma_h(vfh, ph, om[dt]);
                }
            }
        }
        cur = (cur == NSTG - 1) ? 0 : cur + 1;
    }

    if (active) {
        const float l_tot = l_run + __shfl_xor(l_run, 32);
        const float inv = 1.0f / l_tot;
        const bool row_ok = q0 + r < T && q0 + r >= p0;                 // rows beyond T, or before the sequence's own first token, are not written
        const size_t orow = (size_t)(orow0 + max(min(q0 + r, T - 1), p0));
        if (OUT == ATT_OUT_BF16) store_ctx_bf16<ND>(om, oc, inv, kInvLo, row_ok, ctx16 + orow * (size_t)D + (size_t)h * DH, kh);
        else if (OUT == ATT_OUT_SPLIT) store_ctx_split<ND>(om, oc, inv, kInvLo, row_ok, ctx16 + orow * (size_t)(2 * D) + (size_t)((h * DH + d0) / 32) * 64, kh);
        else if (row_ok) store_ctx_f32<ND>(om, oc, inv, kInvLo, ctx + (size_t)(orow0 + q0 + r) * D + (size_t)h * DH + 4 * kh);
    }
}

// Measured and NOT kept (round 5, profiles/r5/att_ab_2_persistent_kernel_with_prefetch.log; the code is in git history, commit "experiment:
// persistent attention kernel"): the PERSISTENT form of the dense head_dim-64 kernel -- a workgroup walks a contiguous run of (sequence, head,
// query block) items, the next item's first K / V^T tile and Q tile in flight (DMA) under the current item's epilogue arithmetic, its stores
// issued after the next Q tile is read; bits equal to this kernel's -- is 9 % slower at T = 288, 13 % at T = 1024, 5 % at T = 152: the per-item
// state (descriptors, bounds) becomes mutable and leaves the SGPRs (54 spilled), 225 VGPRs instead of 188, one more barrier per item, and what the
// prefetch hides is small beside that.  The XCD-local block ORDER alone (the query blocks of one (sequence, head) on one XCD, K / V^T fetched
// into its L2 once) is +2.5 % at T = 1024 and -2 % at T = 288 (att_ab_1_xcd_local_order.log): fetch traffic is not what bounds this kernel.

// Every instantiation of the v2 family, written once: the dense, the head_dim 128 / 256 and the ragged launches all pick theirs here.
// lds: NSTG stages of K (2 planes x 32 keys x DH / 8) + V^T (2 x DO x 4) chunks of 16 B.
using Att16v2Kernel = decltype(&attention_f16x3_v2_kernel<4, ATT_OUT_F32, 3, 64, false, 64>);
struct Att16v2Inst { int wpb, out, head_dim; bool rag; Att16v2Kernel fn; size_t lds_bytes; };
template <int WPB, int OUT, int NSTG, int DH, bool RAG = false, int DO = DH>
static constexpr Att16v2Inst att16v2_inst() {
    return {WPB, OUT, DH, RAG, attention_f16x3_v2_kernel<WPB, OUT, NSTG, DH, RAG, DO>, (size_t)NSTG * (8 * DH + 8 * DO) * 16};
}
static const Att16v2Inst kAtt16v2[] = {
    att16v2_inst<1, ATT_OUT_F32, 3, 64>(),   att16v2_inst<2, ATT_OUT_F32, 3, 64>(),   att16v2_inst<4, ATT_OUT_F32, 3, 64>(),
    att16v2_inst<1, ATT_OUT_SPLIT, 3, 64>(), att16v2_inst<2, ATT_OUT_SPLIT, 3, 64>(), att16v2_inst<4, ATT_OUT_SPLIT, 3, 64>(),
    att16v2_inst<1, ATT_OUT_BF16, 3, 64>(),  att16v2_inst<2, ATT_OUT_BF16, 3, 64>(),  att16v2_inst<4, ATT_OUT_BF16, 3, 64>(),
    att16v2_inst<1, ATT_OUT_SPLIT, 3, 64, true>(), att16v2_inst<2, ATT_OUT_SPLIT, 3, 64, true>(), att16v2_inst<4, ATT_OUT_SPLIT, 3, 64, true>(),
    att16v2_inst<4, ATT_OUT_F32, 3, 128>(),  att16v2_inst<4, ATT_OUT_SPLIT, 3, 128>(), att16v2_inst<4, ATT_OUT_BF16, 3, 128>(),
    att16v2_inst<4, ATT_OUT_SPLIT, 2, 256, false, 128>(),
};

// The one function between a caller's descriptor and a v2 kernel.  rag != nullptr: the ragged form (grid = entries x H), else dense (dense_grid).
static int launch_att16v2(const AttLaunch& a, int wpb, dim3 grid, const RagMap* rag, int dense_nblk) {
    for (const Att16v2Inst& k : kAtt16v2) {
        if (k.wpb != wpb || k.out != a.out || k.head_dim != a.head_dim || k.rag != (rag != nullptr)) continue;
        if (k.lds_bytes > 65536) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k.fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)k.lds_bytes);
            if (e != hipSuccess) { set_error("hipFuncSetAttribute: %s", hipGetErrorString(e)); return PGMI_EHIP; }
        }
        hipLaunchKernelGGL(k.fn, grid, dim3(wpb * 64), k.lds_bytes, a.stream, a.qk16, a.qk_plane, a.vt16, a.vt_plane, a.kv_len, a.slopes,
                           a.T, a.H, (a.T + 31) / 32 * 32, a.ctx, a.ctx16, rag ? *rag : RagMap{}, dense_nblk, a.B);
        PGMI_HIP(hipGetLastError());
        return PGMI_OK;
    }
    set_error("attention_f16x3_v2: no kernel for %d waves, output %d, head_dim %d%s", wpb, (int)a.out, a.head_dim, rag ? ", ragged" : "");
    return PGMI_EINVAL;
}

// Launch option (pgmi_set_option "att_xcd_local", default 1): 1 = the one-dimensional XCD-local order of the dense launches, 0 = the
// (query block, head, sequence) grid of rounds 1-4 (kept for the interleaved A/B of scripts/att_bench.py: block order does not touch a
// row's arithmetic, same bits).
static int g_att_xcd_local = -1;     // -1: by shape -- XCD-local from two query blocks per sequence on.  (Round 5, v2 kernel: +2.5 % at T = 1024, -2 % at
                                     // T = 288, so it was used from eight blocks on; with the pipelined kernel, round 6: +5 % at T = 152, +3.5 % at 230 / 256, 0 at 288,
                                     // +1.6 / +0.7 / +3 % at 322 / 352 / 382, +3 % at 502, +2 % at 739, +6 % at 902; causal: -1 ... +3 %: profiles/r6/att_ab_6_*)
int att_set_option(const char* name, long long value) {
    if (!strcmp(name, "att_xcd_local")) { g_att_xcd_local = (int)value; return PGMI_OK; }
    if (!strcmp(name, "att_v3")) { att_v3_set_option((int)value); return PGMI_OK; }
    return PGMI_EINVAL;
}
// grid of a dense launch of nblk query blocks x H heads x B sequences, and the dense_nblk argument that goes with it
static dim3 dense_grid(int nblk, int H, int B, int* dense_nblk) {
    if (g_att_xcd_local == 0 || (g_att_xcd_local < 0 && nblk < 2)) { *dense_nblk = 0; return dim3(nblk, H, B); }
    *dense_nblk = nblk;
    const long long pairs = (long long)H * B, groups = (pairs + 7) / 8;
    return dim3((unsigned)(groups * 8 * nblk), 1, 1);
}

// Query tiles (waves) per workgroup for sequences of T tokens, head_dim 64: the tiles are spread evenly over ceil(n / 4) blocks
int att16_waves_per_block(int T) {
    const int n32 = (T + 31) / 32, nblk = (n32 + 3) / 4;
    const int wpb = (n32 + nblk - 1) / nblk;
    return wpb == 3 ? 4 : wpb;                    // measured: a 4th (idle) wave that only helps loading beats 3-wave blocks
}

// The K / V^T DMA addresses both planes of ONE sequence / (sequence, head) through a buffer descriptor based there, with 32-bit
// byte offsets: the lo plane sits one plane stride further, so plane stride + one sequence must stay below 4 GiB (the arrays
// themselves may be larger).  Every supported model fits with room (ESM2-15B at 98 304 rows: 2.0e9 bytes per q|k plane; an MSA
// Transformer workspace of 1024 x 1024 tokens: 3.2e9); anything beyond is refused here instead of wrapping.
static int check_operand_range(const char* who, const AttLaunch& a) {
    const unsigned long long Tp = (unsigned long long)(a.T + 31) / 32 * 32;
    const unsigned long long seq_bytes = (unsigned long long)a.T * 2ull * (unsigned long long)a.H * (unsigned long long)a.head_dim * 2ull;
    const unsigned long long vt_bytes = (unsigned long long)a.head_dim * Tp * 2ull;
    if ((unsigned long long)a.qk_plane * 2ull + seq_bytes >= (1ull << 32) || (unsigned long long)a.vt_plane * 2ull + vt_bytes >= (1ull << 32)) {
        set_error("%s: operand planes of %zu / %zu halfs exceed the 32-bit offset range of the K / V^T DMA "
                  "(plane stride + one sequence must stay below 4 GiB: create the model with a smaller max_rows)", who, a.qk_plane, a.vt_plane);
        return PGMI_EINVAL;
    }
    return PGMI_OK;
}

// (prep pass over a.qkv ->) split planes -> attention.  Tp = T rounded up to 32.
int launch_attention_f16x3_v2(const AttLaunch& a) {
    const int B = a.B, T = a.T, H = a.H, head_dim = a.head_dim;
    if (B <= 0 || T <= 0 || H <= 0 || a.out < ATT_OUT_F32 || a.out > ATT_OUT_BF16 || (head_dim != 64 && head_dim != 128 && head_dim != 256)) {
        set_error("attention_f16x3_v2: bad arguments B=%d T=%d H=%d out=%d head_dim=%d", B, T, H, (int)a.out, head_dim);
        return PGMI_EINVAL;
    }
    const int n32 = (T + 31) / 32, Tp = n32 * 32;
    int rc = check_operand_range("attention_f16x3_v2", a);
    if (rc) return rc;
    int dn = 0;
    if (head_dim == 256) {
        // ProGen2-xlarge: H heads of 256 = 4 H slot groups of 64; causal only, fused-QKV operands, split-plane context out.  Sizing (160 KiB
        // LDS per CU; VGPRs and AGPRs share one file of 512 per lane at one wave per SIMD): Q fragments of 256 dims are 2 x 16 x 4 = 128
        // registers per lane, and the O accumulators (main + 2^-11 correction) of all 256 dims would be 256 more -- so each workgroup
        // keeps the context of one 128-dim slice (DO = 128: 128 O registers; two slices per head, S computed by both).  A stage holds K
        // (2 planes x 32 keys x 512 B) and the slice's V^T (2 x 128 x 64 B) = 48 KiB; the ring is 2 stages (96 KiB) with Q straight from
        // the planes: the Q-via-LDS staging of the 3-stage ring would need 4 waves x 32 KiB inside stages 1 .. 2.
        if (a.qkv || a.conv || !a.slopes || a.out != ATT_OUT_SPLIT) { set_error("attention_f16x3_v2: head_dim 256 is the causal, fused-QKV, split-plane-output flavour only"); return PGMI_EINVAL; }
        const dim3 grid = dense_grid((n32 + 3) / 4, 2 * H, B, &dn);       // (sequence, head, slice) pairs
        return launch_att16v2(a, 4, grid, nullptr, dn);
    }
    if (head_dim == 128) {
        // ESM2-15B class: H heads of 128 = 2 H slot groups of 64 in the operand planes; only the fused-QKV operand path
        // (no prep pass), no depth-wise convolution; 3-stage ring (3 x 32 KB).  slopes != nullptr: the causal flavour (ProGen2, head
        // dims 80 / 96 / 128 zero-padded into the 128-lane layout; its all-zero slopes make the ALiBi term exactly 0)
        if (a.qkv || a.conv) { set_error("attention_f16x3_v2: head_dim 128 needs operands from the fused QKV projection"); return PGMI_EINVAL; }
        const dim3 grid = dense_grid((n32 + 3) / 4, H, B, &dn);
        return launch_att16v2(a, 4, grid, nullptr, dn);
    }
    if (a.qkv && a.conv && a.rotary) { set_error("attention_f16x3_v2: depth-wise convolution and rotary together are not a model this library knows"); return PGMI_EINVAL; }
    if (a.qkv && a.conv && H % 4) { set_error("attention_f16x3_v2: the depth-wise convolution has four head groups, H = %d is not a multiple of 4", H); return PGMI_EINVAL; }
    if (a.qkv && a.conv)   // Tranception: LDS-staged depth-wise conv + split
        launch_qkv_prep_conv(dim3(n32, H, B), a.stream, a.qkv, a.conv, T, H, Tp, a.qk16, a.qk_plane, a.vt16, a.vt_plane, nullptr);
    else if (a.qkv)        // operands not prepared by the fused QKV epilogue: run the prep pass
        launch_qkv_prep(dim3(n32, H, B), a.stream, a.qkv, a.cos_t, a.sin_t, a.rotary, T, H, Tp, a.qk16, a.qk_plane, a.vt16, a.vt_plane);
    const int wpb = att16_waves_per_block(T);
    const dim3 grid = dense_grid((n32 + wpb - 1) / wpb, H, B, &dn);
    return att_v3_serves(a) ? launch_att16v3(a, wpb, grid, dn) : launch_att16v2(a, wpb, grid, nullptr, dn);
}

// Tranception prefix-shared scoring (RagMap): depth-wise conv prep over a list of n_tiles (sequence, 32-token tile) entries, then causal
// grouped-ALiBi attention over a list of n_blocks (sequence, block of att16_waves_per_block(T) query tiles) entries; split-plane context rows out (packed rows).
int launch_attention_tr_ragged(const AttLaunch& a, const AttRagged& rg) {
    const int T = a.T, H = a.H;
    if (T <= 0 || H <= 0 || !a.qkv || !a.conv || !a.slopes || a.head_dim != 64 || a.out != ATT_OUT_SPLIT || rg.n_tiles <= 0 || rg.n_blocks <= 0) {
        set_error("attention_tr_ragged: bad arguments T=%d H=%d tiles=%d blocks=%d", T, H, rg.n_tiles, rg.n_blocks);
        return PGMI_EINVAL;
    }
    const int rc = check_operand_range("attention_tr_ragged", a);
    if (rc) return rc;
    const RagMap tiles{rg.seq_off, rg.seq_p, rg.seq_q, rg.seq_root, rg.seq_vt, rg.tile_seq, rg.tile_j};
    launch_qkv_prep_conv(dim3(rg.n_tiles, H, 1), a.stream, a.qkv, a.conv, T, H, (T + 31) / 32 * 32, a.qk16, a.qk_plane, a.vt16, a.vt_plane, &tiles);
    // the same instantiation (waves per block) as the dense launch of T tokens: a row is computed by the same code
    const RagMap rag{rg.seq_off, rg.seq_p, rg.seq_q, rg.seq_root, rg.seq_vt, rg.blk_seq, rg.blk_j};
    return launch_att16v2(a, att16_waves_per_block(T), dim3(rg.n_blocks, H, 1), &rag, 0);
}

}  // namespace pgmi
