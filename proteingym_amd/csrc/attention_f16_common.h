// Shared by attention_f16.hip (the v2 kernel family and the launchers), attention_f16_v3.hip (the software-pipelined dense kernel) and
// attention_f16_prep.hip (the prep passes): the device code both kernels run word for word, and what the launchers need of each other.
#pragma once
#include "common.h"

namespace pgmi {

typedef _Float16 h2 __attribute__((ext_vector_type(2)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

constexpr int AKT = 32;                       // keys per tile
constexpr float kAttDefer = 4.0f;             // lag allowed before O is rescaled (base-2 units; see the rescale in the kernel): +3.5 % (T = 288) / +4.5 % (T = 1024) over 0

__device__ __forceinline__ unsigned int pack_h2(_Float16 a, _Float16 b) {
    const h2 t = {a, b};
    return __builtin_bit_cast(unsigned int, t);
}
__device__ __forceinline__ f32x16 mfma_h(u32x4 a, u32x4 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(h8, a), __builtin_bit_cast(h8, b), c, 0, 0, 0);
}


// DH = 64: one head = 64 lanes of the operand planes (head dims below 64 arrive zero-padded).  DH = 128 (ESM2-15B): a head is two
// adjacent 64-lane slot groups of the planes; S sums 8 k16 steps instead of 4, O has 4 d tiles instead of 2.
// Measured and NOT kept (round 4, scripts/att_bench.py, profiles/r4/README.md): one workgroup of 8 / 9 waves per (sequence, head)
// (K / V^T read once instead of once per query block; every query tile of T = 288 in one block) -4 % / -36 %; the score MFMAs of key
// tile kt + 1 issued inside the softmax of tile kt (own accumulators, 4-stage ring, 235 VGPRs) -3 ... -5 % at every shape.  Two
// waves share a SIMD's matrix pipe AND its VALU issue: work moved between them, or between a wave's own phases, does not net.
// RAG (Tranception prefix-shared scoring, api_tranception.hip run_tranception_shared): the launch holds SUFFIXES of sequences of T tokens.  Sequence
// b owns the packed rows [seq_off[b], seq_off[b] + T - seq_p[b]) of the residual stream / context = its tokens seq_p[b] .. T-1, and in
// the attention operand planes the rows [seq_q[b], seq_q[b] + T - a) and the V^T block seq_vt[b] (row pitch roundup(T - a, 32)) for the
// tokens from a = seq_p[b] rounded down to a multiple of 32 (the prep pass fills the head of that tile from the root's inputs).  The keys
// before a are those of its ROOT sequence seq_root[b], which is in the same launch with seq_p = 0 (the model is causal: a sequence that
// equals its root up to token seq_p - 1 has the root's K and V there, bit for bit).  Key tiles keep their ABSOLUTE alignment -- tile
// kt = keys 32 kt .. 32 kt + 31 -- and every query tile holds the same 32 queries as in a full forward, so each row goes through the
// same tiles in the same order: the same bits.  Context rows of the tokens before seq_p are not written.
// blockIdx.x indexes a list of (sequence, query block) entries.
struct RagMap {
    const int32_t* seq_off;
    const int32_t* seq_p;
    const int32_t* seq_q;
    const int32_t* seq_root;
    const uint32_t* seq_vt;        // halfs, per plane
    const int32_t* ent_seq;        // per entry of the launch's list (query blocks here, 32-token tiles in the prep pass)
    const int32_t* ent_j;
};

// Context rows as ONE bf16 plane, row-major [rows][H * DH] (ATT_OUT_BF16: the bf16 throughput mode's out-projection operand).  The split-plane
// epilogue's lane exchange with two dwords per (lane, column group): lane (r, kh) holds columns 8 g + 4 kh .. + 3 of its row; one
// v_permlane32_swap per dword gives every lane 8 consecutive columns = one 16-byte store.  All 64 lanes take part in the swaps.
template <int ND>
__device__ __forceinline__ void store_ctx_bf16(const f32x16 (&om)[ND], const f32x16 (&oc)[ND], float inv, float inv_lo, bool row_ok,
                                               unsigned short* row_head, int kh) {
    auto rne = [](float f) -> unsigned int {
        unsigned int u = __builtin_bit_cast(unsigned int, f);
        u += 0x7fffu + ((u >> 16) & 1u);
        return u >> 16;
    };
#pragma unroll
    for (int dt = 0; dt < ND; ++dt)
#pragma unroll
        for (int gp = 0; gp < 2; ++gp) {
            unsigned int w[2][2];
#pragma unroll
            for (int gi = 0; gi < 2; ++gi) {
                const int g = 2 * gp + gi;
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = fmaf(oc[dt][4 * g + e], inv_lo, om[dt][4 * g + e]) * inv;
                w[gi][0] = rne(v[0]) | (rne(v[1]) << 16);
                w[gi][1] = rne(v[2]) | (rne(v[3]) << 16);
            }
            unsigned int first[2], second[2];
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const auto sw = __builtin_amdgcn_permlane32_swap(w[0][k], w[1][k], false, false);
                first[k] = sw[0];
                second[k] = sw[1];
            }
            if (row_ok) *reinterpret_cast<u32x4*>(row_head + dt * 32 + 8 * (2 * gp + kh)) = u32x4{first[0], first[1], second[0], second[1]};
        }
}

// Context rows as split fp16 planes (ATT_OUT_SPLIT: the f16x3 out-projection's K-interleaved operand, common.h ki_off), 16-byte
// stores: lane (r, kh) holds columns 8g + 4kh .. + 3 of its query row for g = 0 .. 3; one v_permlane32_swap per dword hands lane (r, 0)
// its partner's half of an even g and lane (r, 1) its partner's half of the following odd g, so every lane owns 8 consecutive columns =
// one dwordx4 per plane: 8 store instructions per lane instead of 16 of half the width (a row-per-lane store touches 32-64 lines per
// instruction: the epilogue is bound by store issue, not by bytes).  All 64 lanes take part in the swaps; rows that are not the
// wave's to write (row_ok false) only skip the stores.  rowp: the row's first half of the 32-column group the tile dt = 0 starts at.
template <int ND>
__device__ __forceinline__ void store_ctx_split(const f32x16 (&om)[ND], const f32x16 (&oc)[ND], float inv, float inv_lo, bool row_ok,
                                                unsigned short* rowp, int kh) {
#pragma unroll
    for (int dt = 0; dt < ND; ++dt)
#pragma unroll
        for (int gp = 0; gp < 2; ++gp) {
            unsigned int w[2][4];                        // [g parity][hi0 hi1 lo0 lo1]
#pragma unroll
            for (int gi = 0; gi < 2; ++gi) {
                const int g = 2 * gp + gi;
                _Float16 hh[4], ll[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) split_act(fmaf(oc[dt][4 * g + e], inv_lo, om[dt][4 * g + e]) * inv, hh[e], ll[e]);
                w[gi][0] = pack_h2(hh[0], hh[1]); w[gi][1] = pack_h2(hh[2], hh[3]);
                w[gi][2] = pack_h2(ll[0], ll[1]); w[gi][3] = pack_h2(ll[2], ll[3]);
            }
            unsigned int first[4], second[4];            // columns c .. c + 3 and c + 4 .. c + 7 of this lane's 8-column run
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const auto sw = __builtin_amdgcn_permlane32_swap(w[0][k], w[1][k], false, false);
                first[k] = sw[0];                        // kh 0: own g even          kh 1: partner's (kh 0) g odd
                second[k] = sw[1];                       // kh 0: partner's g even    kh 1: own g odd
            }
            if (row_ok) {
                unsigned short* dst = rowp + dt * 64 + 8 * (2 * gp + kh);
                *reinterpret_cast<u32x4*>(dst) = u32x4{first[0], first[1], second[0], second[1]};
                *reinterpret_cast<u32x4*>(dst + 32) = u32x4{first[2], first[3], second[2], second[3]};
            }
        }
}

// Context rows as fp32 (ATT_OUT_F32): lane (r, kh) stores its four columns of every 8-column group.  dst: column 4 kh of the head in the row.
template <int ND>
__device__ __forceinline__ void store_ctx_f32(const f32x16 (&om)[ND], const f32x16 (&oc)[ND], float inv, float inv_lo, float* dst) {
#pragma unroll
    for (int dt = 0; dt < ND; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            float val[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) val[e] = fmaf(oc[dt][4 * g + e], inv_lo, om[dt][4 * g + e]) * inv;
            *reinterpret_cast<f32x4*>(dst + dt * 32 + 8 * g) = f32x4{val[0], val[1], val[2], val[3]};
        }
}

// Dense launches in the XCD-local order (dense_nblk > 0) are ONE-dimensional (workgroup i runs on XCD i % 8): the dense_nblk query
// blocks of one (sequence, head) are the workgroups i, i + 8, i + 16 ... of a group of 8 dense_nblk consecutive ones -- the same
// XCD, dispatched together -- so that the K and V^T tiles every one of them streams reach that XCD's L2 once instead of once per
// query block (the (nblk, H, B) grid, dense_nblk == 0, puts them on different XCDs: 2.45 x the algorithmic bytes fetched at
// T = 288, profiles/r4).  Returns the workgroup's (sequence, head[, slice]) pair -- the last group is padded: a pair beyond the
// launch's has nothing to do -- and its query block.
__device__ __forceinline__ int xcd_local_pair(int dense_nblk, int& qblk) {
    const int within = (int)blockIdx.x % (8 * dense_nblk);
    qblk = within >> 3;
    return ((int)blockIdx.x / (8 * dense_nblk)) * 8 + (within & 7);
}

// Buffer descriptor of an operand tensor based at `base` (a sequence's rows / a (sequence, head)'s V^T block in the hi plane), `bytes` long
__device__ __forceinline__ __amdgpu_buffer_rsrc_t operand_rsrc(const unsigned short* base, unsigned long long bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned short*>(base), 0, (int)(unsigned int)bytes, 0x00020000);
}

// A K or Q tile image in LDS has rows of DH / 8 chunks of 16 bytes; chunk c of a row sits at c ^ k_swizzle(row): the row's bits that
// spread the 32 rows a fragment read touches over the banks (128-byte rows, DH 64: two rows share a bank group; 256-byte rows: none do)
template <int DH>
__device__ __forceinline__ int k_swizzle(int row) { return DH == 64 ? ((row >> 1) & 7) : (row & 15); }
// Chunk of a V^T tile image (rows of 4 chunks = 32 keys per dim, swizzled by (d >> 2) & 3) that holds keys 16 m + 8 kh .. + 7 of dim d
__device__ __forceinline__ int v_chunk(int d, int m, int kh) { return d * 4 + ((2 * m + kh) ^ ((d >> 2) & 3)); }

// P (two probabilities x 2^10, in [0, 1024 * 2^kAttDefer]) as split fp16 pairs {hi, lo}: hi by truncation (pkrtz), lo = (p - hi) 2^11 as one
// mixed-precision fma on the fp16 hi (v_fma_mix_f32): p 2^11 (one packed multiply for the pair) and the fma are both exact
__device__ __forceinline__ u32x2 split_p(float p0, float p1) {
    typedef __fp16 fp16x2 __attribute__((ext_vector_type(2)));
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    const fp16x2 hi2 = __builtin_amdgcn_cvt_pkrtz(p0, p1);
    const f32x2 ps = f32x2{p0, p1} * f32x2{kLoScale, kLoScale};
    const float l0 = fmaf((float)hi2[0], -kLoScale, ps[0]), l1 = fmaf((float)hi2[1], -kLoScale, ps[1]);
    const fp16x2 lo2 = __builtin_amdgcn_cvt_pkrtz(l0, l1);
    return u32x2{__builtin_bit_cast(unsigned int, hi2), __builtin_bit_cast(unsigned int, lo2)};
}

// ---- launchers ----------------------------------------------------------------------------------------------------------------------
// attention_f16_prep.hip: operands for launches that do not come from the fused QKV projection
void launch_qkv_prep(dim3 grid, hipStream_t s, const float* qkv, const float* cos_t, const float* sin_t, int rotary, int T, int H, int Tp,
                     unsigned short* qk16, size_t qk_plane, unsigned short* vt16, size_t vt_plane);
void launch_qkv_prep_conv(dim3 grid, hipStream_t s, const float* qkv, const float* conv, int T, int H, int Tp, unsigned short* qk16, size_t qk_plane,
                          unsigned short* vt16, size_t vt_plane, const RagMap* rag);          // rag == nullptr: dense (grid = tiles x H x B)
// attention_f16_v3.hip: the software-pipelined dense kernel.  grid / dense_nblk: attention_f16.hip dense_grid
bool att_v3_serves(const AttLaunch& a);
void att_v3_set_option(int value);
int launch_att16v3(const AttLaunch& a, int wpb, dim3 grid, int dense_nblk);

}  // namespace pgmi
