// Shared declarations for libpgmi (gfx950 / MI355X only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include "../../include/pgmi.h"

namespace pgmi {

void set_error(const char* fmt, ...);

#define PGMI_HIP(expr)                                                                   \
    do {                                                                                 \
        hipError_t _e = (expr);                                                          \
        if (_e != hipSuccess) {                                                          \
            pgmi::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e),       \
                            __FILE__, __LINE__);                                         \
            return PGMI_EHIP;                                                            \
        }                                                                                \
    } while (0)

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kWave = 64;
constexpr int kHeadDim = 64;

enum Epilogue { EPI_NONE = 0, EPI_GELU = 1, EPI_SQRELU = 2, EPI_GELU_TANH = 3,   // erf-GELU (ESM), squared ReLU (Tranception), tanh-GELU (ProGen2)
                EPI_SWIGLU = 4,     // ESM C's FC1: W rows in blocks of 64 = 32 gate | 32 up rows; out column 32 b + i = silu(gate) * up, N / 2 wide
                EPI_RELU = 5 };     // ESM-IF1's decoder FC1 (f16x3 only)

// f16x3 activation split: x ~= hi + lo * 2^-11 with hi = fp16(x) and lo = fp16((x - hi) * 2^11).
// The scaled lo keeps its 11 bits for every |x| >= 2^-14 (an unscaled lo would be an fp16
// subnormal whenever |x| < 0.125); |x| below fp16's normal range goes entirely into lo, so no
// subnormal ever reaches the MFMA inputs.  The GEMM multiplies lo by (w_hi * 2^-11), which is
// exact because weights are pre-scaled to ~2^13.
constexpr float kLoScale = 2048.0f;
// The split q planes consumed by attention_f16x3_v2_kernel are pre-multiplied by log2(e): its online softmax works in base 2
// (v_exp_f32 is 2^x) and the scores come out of the MFMAs already in base-2 units -- 16 multiplies per 32 x 32 tile saved.
constexpr float kQLog2e = 1.4426950408889634f;

// K-interleaved layout of an f16x3 GEMM operand [rows][K] (K % 32 == 0): every group of 32 consecutive k is stored as the
// 32 hi halfs (64 B) followed by the 32 lo halfs (64 B), so a row's share of a 32-deep K tile is ONE 128-byte line.
// Returns the half index of the hi value of (row, k); its lo value sits 32 halfs further.  Row pitch: 2 K halfs.
__host__ __device__ __forceinline__ size_t ki_off(size_t row, int k, int K) {
    return row * (size_t)(2 * K) + (size_t)(k >> 5) * 64 + (size_t)(k & 31);
}
#if defined(__HIPCC__)
__device__ __forceinline__ void split_act(float x, _Float16& hi, _Float16& lo) {
    hi = (fabsf(x) < 6.103515625e-05f) ? (_Float16)0.0f : (_Float16)x;
    lo = (_Float16)((x - (float)hi) * kLoScale);
}
// split_act for four values at a time, the same (hi, lo) pairs in fewer VALU issue slots: the flush of |x| < 2^-14 is a select on x in front of
// two PACKED RNE conversions, and lo = fma(hi, -2^11, 2^11 x) is one mixed-precision fma on the fp16 hi (attention_f16_common.h split_p does
// the same for P).  2^11 x is exact (a power of two; beyond 2^117 it overflows, where hi is already infinite), x - hi is exact in fp32 (hi is x
// rounded to 11 bits, or 0), so the fma's single rounding has nothing to round: lo32 = (x - hi) 2^11, the value split_act converts.  A NaN or
// an infinity in x gives a non-finite hi AND lo, as there.  Every fused operation is written out; nothing here is left to -ffp-contract.
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void split_act4(f32x4 x, f16x4& hi, f16x4& lo) {
    f32x4 xz, lo32;
#pragma unroll
    for (int e = 0; e < 4; ++e) xz[e] = (fabsf(x[e]) < 6.103515625e-05f) ? 0.0f : x[e];
    hi = __builtin_convertvector(xz, f16x4);
    const f32x4 xs = x * f32x4{kLoScale, kLoScale, kLoScale, kLoScale};
#pragma unroll
    for (int e = 0; e < 4; ++e) lo32[e] = __builtin_fmaf((float)hi[e], -kLoScale, xs[e]);
    lo = __builtin_convertvector(lo32, f16x4);
}
// The same for a value that is a product a b (squared ReLU: t t).  Behind split_act the compiler had fused that product into the subtraction
// of hi in every instantiation (-ffp-contract): lo = (fma(a, b, -hi)) 2^11 sees the UNROUNDED product, hi the rounded one.  Written out here
// so that the planes keep those bits and no instantiation can decide otherwise.  (SwiGLU's silu(gate) up is fused differently again -- this
// form does not give its bits -- and keeps the scalar split_act.)
__device__ __forceinline__ void split_act4_prod(f32x4 a, f32x4 b, f16x4& hi, f16x4& lo) {
    const f32x4 x = a * b;
    f32x4 xz, lo32;
#pragma unroll
    for (int e = 0; e < 4; ++e) xz[e] = (fabsf(x[e]) < 6.103515625e-05f) ? 0.0f : x[e];
    hi = __builtin_convertvector(xz, f16x4);
#pragma unroll
    for (int e = 0; e < 4; ++e) lo32[e] = __builtin_fmaf(a[e], b[e], -(float)hi[e]);
    lo = __builtin_convertvector(lo32 * f32x4{kLoScale, kLoScale, kLoScale, kLoScale}, f16x4);
}
// The columns 4 c .. 4 c + 3 of `row` (D columns, D % 8 == 0) into the K-interleaved split operand, for kernels whose lane `lane` of a wave
// holds the f32x4 group c = lane + 64 i: lanes (2m, 2m+1) hold one group of 8 columns; the even lane stores the 16 bytes of hi values, the
// odd lane the 16 bytes of lo values (one exchange of 8 bytes with the neighbour), so 8 lanes write one 128-byte line with one store each.
// Both lanes of a pair must call it together.
__device__ __forceinline__ void store_split4(f32x4 o, unsigned short* y16, size_t row, int c, int lane, int D) {
    typedef _Float16 h4 __attribute__((ext_vector_type(4)));
    typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    h4 hi, lo;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        _Float16 a, b;
        split_act(o[k], a, b);
        hi[k] = a;
        lo[k] = b;
    }
    const u32x2 H = __builtin_bit_cast(u32x2, hi), L = __builtin_bit_cast(u32x2, lo);
    const bool odd = lane & 1;
    const unsigned int s0 = odd ? H[0] : L[0], s1 = odd ? H[1] : L[1];
    const unsigned int r0 = __shfl_xor(s0, 1), r1 = __shfl_xor(s1, 1);
    const u32x4 out = odd ? u32x4{r0, r1, L[0], L[1]} : u32x4{H[0], H[1], r0, r1};
    *reinterpret_cast<u32x4*>(y16 + ki_off(row, 4 * (c & ~1), D) + (odd ? 32 : 0)) = out;
}
#endif

// ---- elementwise.hip ---------------------------------------------------------------------
// tokens_out[b,t] = (t == mask_pos[b]) ? <mask> : wt[start[b] + t]
void launch_make_masked_windows(const int32_t* wt, const int32_t* win_start, const int32_t* mask_rel,
                                int B, int T, int32_t* tokens_out, hipStream_t s);
// tokens[b, mask_pos[b]] = <mask> (in place)
void launch_apply_mask(int32_t* tokens, const int32_t* mask_pos, int B, int T, hipStream_t s);
// per sequence: scale[b] (token-dropout rescale), pos_idx[b,t] (learned-position index), kv_len[b]; mask_id = the model's <mask> id
void launch_seq_stats(const int32_t* tokens, int B, int T, int token_dropout, float* scale,
                      int32_t* pos_idx, int32_t* kv_len, hipStream_t s, int mask_id = PGMI_TOK_MASK);
void launch_zero_pad_rows(const int32_t* tokens, int rows, int D, float* x, hipStream_t s);
void launch_embed(const int32_t* tokens, const float* scale, const int32_t* pos_idx,
                  const float* embed_tokens, const float* embed_positions, int token_dropout,
                  int rows, int T, int D, float* x, hipStream_t s, int mask_id = PGMI_TOK_MASK);
void launch_layernorm(const float* x, const float* w, const float* b, int rows, int D, float eps,
                      float* y, hipStream_t s);
// y[i,:] = x[row_idx[i],:]
void launch_gather_rows(const float* x, const int32_t* row_idx, int n, int D, float* y, hipStream_t s);
// idx[i] = first + i * stride, i < n
void launch_strided_index(int first, int stride, int n, int32_t* idx, hipStream_t s);
// out[r,:] = log_softmax(h[r,:] @ E^T + bias); E [V,D]
void launch_vocab_logsoftmax(const float* h, const float* E, const float* bias, int rows, int D,
                             int V, float* out, int32_t* nonfinite, hipStream_t s);
void launch_layernorm16(const float* x, const float* w, const float* b, int rows, int D, float eps,
                        unsigned short* y16, int mode, hipStream_t s);
// Weight-only RMSNorm (ProGen3): y16[r] = split(x[r] * rsqrt(mean(x[r]^2) + eps) * w), the K-interleaved f16x3 operand that
// launch_layernorm16 mode 1 writes; D % 32 == 0, D <= 5120
int launch_rmsnorm16(const float* x, const float* w, int rows, int D, float eps, unsigned short* y16, hipStream_t s);
void launch_scatter_rows(const float* src, const int32_t* dst_row, int n, int V, float* table,
                         hipStream_t s);
void launch_row_index(const int32_t* mask_rel, int B, int T, int32_t* out, hipStream_t s);
void launch_fill_f32(float* p, int64_t n, float v, hipStream_t s);
// Tranception: per-sequence sum over t < len-1 of log p(tok[t+1] | tok[<=t]) from lp [B*T,V]
// (scoring_utils.py:118-128), with the retrieval fusion (model_pytorch.py:806-830) on rows
// [a0, a0+n) when prior != nullptr: value = (1-alpha)*lp + alpha*prior[row0 +/- i]; eve != nullptr (TranceptEVE,
// trancepteve/model_pytorch.py:1113-1133; same rows as prior): value = (1-beta)*value + beta*eve[row], except that an eve entry of
// -inf leaves the value alone when eve_fallback != 0.
void launch_seq_loglik(const float* lp, const int32_t* tokens, const int32_t* lens, int B, int T, int V,
                       const float* prior, const int32_t* a0, const int32_t* row0, const int32_t* n,
                       const int32_t* flip, float alpha, const float* eve, float beta, int eve_fallback, float* out, hipStream_t s);
void launch_seq_loglik_ragged(const float* lp, const int32_t* tokens, const int32_t* seq_off, const int32_t* seq_p,
                              const int32_t* seq_root, int B, int T, int V, const float* prior, const int32_t* a0,
                              const int32_t* row0, const int32_t* n, const int32_t* flip, float alpha, const float* eve, float beta,
                              int eve_fallback, float* out, hipStream_t s);
// ProGen2: out[b] = sum over t < n_kept[b] of lp[b*T + t, col[b*T + t]] (lp [B*T,V], one wave per sequence, fixed lane order)
void launch_pg2_seq_loglik(const float* lp, const int32_t* col, const int32_t* n_kept, int B, int T, int V, float* out, hipStream_t s);
// causal decoder (api_gpt.hip): x[row] = E[tokens[row]] + P[row % T]
void launch_embed_learned(const int32_t* tokens, const float* E, const float* P, int rows, int T, int D, float* x, hipStream_t s);
// ESM-IF1's decoder (api_esmif1.hip): x[row] = scale * E[tokens[row]] + P[pos[row]] (P: the sinusoidal table built at creation)
void launch_embed_scaled_pos(const int32_t* tokens, const int32_t* pos, const float* E, const float* P, float scale, int rows, int D,
                             float* x, hipStream_t s);
// log-softmax over V > 64 columns of fp32 logits [rows][ldl] (ldl % 4 == 0, pad columns excluded by index): out[r] = log p(tgt[r])
// when tgt != nullptr, else the full rows out [rows][V]
void launch_wide_logsoftmax(const float* logits, int ldl, int rows, int V, const int32_t* tgt, float* out, int32_t* nonfinite,
                            hipStream_t s);
// out[b] = sum of terms[off[b] .. off[b+1]) in double, left to right
void launch_seq_sum(const float* terms, const int32_t* off, int B, double* out, hipStream_t s);
void launch_score_mutants(const float* table, int V, const int32_t* sub_pos, const int32_t* sub_wt,
                          const int32_t* sub_mt, const int64_t* mut_off, int64_t n_mut,
                          double* scores, hipStream_t s);
// H = 64-lane slot groups per token; rot_halves = table rows per token (2 for head_dim 128: the slot group's parity picks the row)
void launch_rotary(float* qkv, const float* cos_t, const float* sin_t, int rows, int T, int H,
                   hipStream_t s, int rot_halves = 1);
// pseudo-perplexity (compute_fitness.py:258-279): rows enumerated on the device from a resident sequence library
void launch_make_pppl_rows(const uint8_t* tok8, const int64_t* seq_off, const int32_t* sid, const int64_t* rp, int J,
                           int64_t g0, int bc, int T, int32_t* tokens, int32_t* row_idx, int32_t* target, hipStream_t s);
void launch_pppl_pick(const float* lp, const int32_t* target, int bc, int V, float* terms, hipStream_t s);
void launch_pppl_sum(const float* terms, const int64_t* rp, const int32_t* sid, int J, int64_t first, double* out, hipStream_t s);
// SaProt (api_saprot.hip): token rows [bc][T] of the position sets [s0, s0 + bc) (CSR set_off / set_pos, positions ascending inside a
// set) with the masked ids, and keep[e - set_off[s0]] = the flat row of entry e
void launch_saprot_rows(const int32_t* wt, const int32_t* set_off, const int32_t* set_pos, int s0, int bc, int T, int first, int groups,
                        int width, int32_t* tokens, int32_t* keep, hipStream_t s);
// MULAN (api_mulan.hip): per row (b, t) of the position sets [s0, s0 + bc) the adapter's input y[row][D] = bias + sum_k a_k W[:, k]
// (W [D][7], fp32, k ascending), the row's seven values a chosen on the fly: 4 for t = 0, t = T - 1 and plddt[t] <= 70, -4 where t is
// in the set (this wins), else angles[t][7].  wt != nullptr: also tokens[row] = wt[t] or mask_id in the set, and
// keep[e - set_off[s0]] = the flat row of entry e (launch_saprot_rows' outputs); nullptr: the tokens are the caller's
void launch_mulan_rows(const int32_t* wt, const int32_t* set_off, const int32_t* set_pos, int s0, int bc, int T, int mask_id,
                       const float* angles, const float* plddt, const float* W, const float* bias, int D, int32_t* tokens, int32_t* keep,
                       float* y, hipStream_t s);
// MULAN: x[row] = (E[tokens[row]] + st[row]), zero for <mask> under token dropout, * 0.88 / scale[b] (launch_embed's order); pad rows 0
void launch_mulan_embed(const int32_t* tokens, const float* scale, const float* E, const float* st, int token_dropout, int rows, int T,
                        int D, float* x, hipStream_t s, int mask_id);
// per row of h [rows][D] against E [V][D] (V <= 512), in double: full [rows][V] = log-softmax (nullable); group [rows][groups] =
// lse(logits[first + g width .. + width)) - lse(row) (nullable)
int launch_group_logsoftmax(const float* h, const float* E, const float* bias, int rows, int D, int V, int first, int groups, int width,
                            float* full, float* group, int32_t* nonfinite, hipStream_t s);
// what launch_group_logsoftmax refuses (PGMI_EINVAL and its message), for a caller that must know before it allocates
int group_logsoftmax_check(int D, int V, int first, int groups, int width);

// ---- moe.hip (ProGen3's routed expert block; the kernels are described there) -------------------------------------------------
// The router of launch_rmsnorm_route: gate fp32 [E][D] (nullptr: no routing), 2 <= E <= 64, 1 <= top_k <= E; tokens / pad_id (nullable):
// rows whose token is pad_id are routed nowhere (expert -1, weight 0); ids / wts [rows][top_k]: the chosen experts, best first, and their
// weights divided by their sum.
struct MoeRoute {
    const float* gate = nullptr;
    int E = 0, top_k = 0;
    const int32_t* tokens = nullptr;
    int pad_id = 0;
    int32_t* ids = nullptr;
    float* wts = nullptr;
};
// launch_rmsnorm16 with the router on the normalised row while it is in registers.  w == nullptr: the rows are taken as they are;
// y16 == nullptr: no operand is written.
int launch_rmsnorm_route(const float* x, const float* w, int rows, int D, float eps, unsigned short* y16, const MoeRoute& r, hipStream_t s);
// The token -> expert permutation of n_entries = rows * top_k entries (ids, -1 = unrouted): counts_seg [2 E + 1] = per-expert counts,
// then the first slot of every expert's segment (multiples of `tile`) and the padded total; slot [n_entries] (-1 = unrouted), in the
// entries' own order inside a segment.  blk_cnt / blk_base: scratch of moe_perm_blocks(n_entries) * E each.
int moe_perm_blocks(int n_entries);
void launch_moe_permute(const int32_t* ids, int n_entries, int E, int tile, int32_t* blk_cnt, int32_t* blk_base, int32_t* counts_seg,
                        int32_t* slot, hipStream_t s);
// a16[slot[j]] = h16[j / top_k]: split rows of D columns
void launch_moe_gather(const unsigned short* h16, const int32_t* slot, int n_entries, int top_k, int D, unsigned short* a16, hipStream_t s);
// x[row] += sum over k = 0 .. top_k-1 of wts[row][k] * y[slot[row][k]] (fp32 rows of D columns); unrouted rows keep x
void launch_moe_combine(const float* y, const int32_t* slot, const float* wts, int rows, int top_k, int D, float* x, hipStream_t s);
// g16 = split(silu(t)): fp32 rows of F columns (F % 32 == 0) -> the K-interleaved operand
void launch_silu_split(const float* t, int rows, int F, unsigned short* g16, hipStream_t s);

// ---- eve.hip (EVE / DeepSequence; the kernels are described there) ------------------------------------------------------------
// Noise tensor ids of the Philox counter (include/pgmi.h pgmi_eve_noise names the tensors): z eps; dropout keeps 0 .. n_dec; hidden
// weight / bias eps per layer; W_out, b_out, conv, sparsity, temperature eps.
enum EveTensor { PGMI_EVE_T_Z = 0, PGMI_EVE_T_KEEP = 1, PGMI_EVE_T_W = 16, PGMI_EVE_T_B = 32, PGMI_EVE_T_WOUT = 48, PGMI_EVE_T_BOUT = 49,
                 PGMI_EVE_T_CONV = 50, PGMI_EVE_T_SPARSITY = 51, PGMI_EVE_T_TEMP = 52 };
void launch_eve_gather(const uint8_t* res, const float* W0t, const float* b, int rows, int L, int ld, int act, float* out, hipStream_t s);
void launch_eve_act(float* x, int rows, int n, int ld, int act, uint32_t keep24, float scale, uint64_t seed, uint32_t sample, int tensor,
                    int64_t row_base, const uint8_t* inj, int64_t inj_row0, hipStream_t s);
void launch_eve_latent(const float* mulv, int ldz, int64_t mulv_row0, int rows, int z, int ld, uint32_t keep24, float scale, uint64_t seed,
                       uint32_t sample, int64_t row_base, const float* inj_eps, const uint8_t* inj_keep, int64_t inj_row0, float* h,
                       hipStream_t s);
void launch_eve_sample(const float* mean, const float* sd, int64_t n, int K, int Kp, uint64_t seed, uint32_t sample, int tensor,
                       const float* inj, float* out, hipStream_t s);
void launch_eve_sample_final(const float* w_mean, const float* w_sd, const float* c_mean, const float* c_sd, const float* s_mean,
                             const float* s_sd, int L, int H, int Hp, int C, int Ht, bool conv, uint64_t seed, uint32_t sample,
                             const float* inj_w, const float* inj_c, const float* inj_s, float* out, hipStream_t s);
void launch_eve_elbo(const float* logits, const uint8_t* res, const float* mulv, int ldz, int z, const float* temp, int rows, int L,
                     int64_t loc0, float* elbo, float* bce, float* kld, double* acc, int first, hipStream_t s);
void launch_eve_fill_normal(uint64_t seed, uint32_t sample, int tensor, uint64_t e0, int64_t n, float* out, hipStream_t s);
void launch_eve_fill_keep(uint64_t seed, uint32_t sample, int tensor, uint64_t e0, int64_t n, uint32_t keep24, uint8_t* out, hipStream_t s);
// the log-prior of one row (pgmi_eve_log_prior): up to EVE_PRIOR_S samples per launch; p[s] = sample s's injected tensor (nullptr: generator)
constexpr int EVE_PRIOR_S = 4;
struct EvePriorPtrs { const float* p[EVE_PRIOR_S] = {nullptr, nullptr, nullptr, nullptr}; };
void launch_eve_prior_latent(const float* mulv, int z, int ld, uint64_t seed, uint32_t sample, const EvePriorPtrs& inj, int S, float* h,
                             hipStream_t s);
void launch_eve_prior_hidden(const float* w_mean, const float* w_sd, const float* b_mean, const float* b_sd, int N, int K, uint64_t seed,
                             uint32_t sample, int tw, int tb, const EvePriorPtrs& inj_w, const EvePriorPtrs& inj_b, int S, const float* x,
                             int ldx, int act, float* y, int ldy, hipStream_t s);
int eve_prior_blocks(int L, int H);                      // blocks of the final kernel = rows of its partial sums per sample
int eve_prior_kmax(int H);                               // logits a block can touch = row pitch of the partial sums
int eve_prior_max_samples(int C, bool conv);
void launch_eve_prior_final(const float* w_mean, const float* w_sd, const float* c_mean, const float* c_sd, const float* s_mean,
                            const float* s_sd, int L, int H, int C, int Ht, bool conv, uint64_t seed, uint32_t sample,
                            const EvePriorPtrs& inj_w, const EvePriorPtrs& inj_c, const EvePriorPtrs& inj_s, int S, const float* h, int ldh,
                            float* partial, hipStream_t s);
void launch_eve_prior_finish(const float* partial, int S, const float* b_mean, const float* b_sd, const float* t_mean, const float* t_sd,
                             uint64_t seed, uint32_t sample, const EvePriorPtrs& inj_b, const EvePriorPtrs& inj_t, int L, int H, int sample0,
                             double* acc, hipStream_t s);
int eve_set_option(const char* name, long long value);   // api_eve.hip: "eve_max_rows", "eve_fixed_sample", "eve_prior_batch"

// ---- mpnn.hip (ProteinMPNN; the kernels are described there) -------------------------------------------------------------------
void launch_mpnn_graph(const float* X, const float* mask, int L, int K, int32_t* E_idx, float* D_nb, hipStream_t s);
void launch_mpnn_edge_feat(const float* X, const int32_t* ridx, const int32_t* chain, const int32_t* E_idx, const float* D_nb,
                           const float* Wpos, const float* bpos, const float* Wt, const float* ln_w, const float* ln_b, int L, int K, float* E,
                           hipStream_t s);
void launch_mpnn_concat(const float* hV, const float* hE, const int32_t* E_idx, int L, int K, float* out, hipStream_t s);
void launch_mpnn_edge_sum(const float* msg, const float* mask, const int32_t* E_idx, int L, int K, float* out, hipStream_t s);
// out[r] = LayerNorm(a[r % a_rows] + (b[r] + kb bias) / div) * rowmask[r % L]; b, bias, rowmask nullable; 128 columns
void launch_mpnn_add_ln(const float* a, int64_t a_rows, const float* b, const float* bias, float kb, float div, const float* ln_w,
                        const float* ln_b, const float* rowmask, int L, int64_t rows, float* out, hipStream_t s);
// out [B][L][128] = sum over a node's K edges of GELU(W2 GELU(pre) + b2); AP = [A | P] rows of 256, ap_bstride 0 when shared by the batch
int launch_mpnn_dec_edge(const float* Ep, const float* T, const float* Penc, const float* AP, int64_t ap_bstride, const float* W2,
                         const float* b2, const int32_t* E_idx, const float* mask, const uint8_t* S, const int32_t* rank, int B, int L, int K,
                         float* out, hipStream_t s);
void launch_mpnn_head(const float* h, const float* W, const float* bias, const uint8_t* S, int64_t rows, float* lp, float* nll,
                      hipStream_t s);
void launch_mpnn_score(const float* nll, const float* mask, int B, int L, double* out, hipStream_t s);
int mpnn_set_option(const char* name, long long value);   // api_mpnn.hip: "mpnn_max_rows"

// S2F (s2f.hip; operands and shapes at the kernels)
constexpr int S2F_S = 256, S2F_V = 16, S2F_H0 = 33;    // node scalar width, node vector channels, hidden vector channels of the first message GVP (2 * 16 + 1)
struct S2fMsgWeights {    // device pointers of a layer's message GVPs: the first one's vector half, then the second and the third
    const float *wv0, *wsv0, *bsv0;
    const float *wh1, *ws1, *bs1, *wv1, *wsv1, *bsv1;
    const float *wh2, *ws2, *bs2, *wv2, *wsv2, *bsv2;
    int ldw;              // row stride of ws1 / ws2
};
int launch_s2f_message(const float* P, const float* VT, const float* Es, const float* ev, const float* whe, const float* Wnt,
                       const S2fMsgWeights& w, const int32_t* src, const int32_t* off, int L, int64_t nodes, float* ds, float* dv, hipStream_t s);
int launch_s2f_gvp_mid(const float* spre, const float* vh, const float* wv, const float* gpre, const float* nwh, int so,
                       int vo, int h, int h2, int relu, int lda, int64_t rows, float* outA, float* outV, hipStream_t s);
int launch_s2f_node_ln(const float* rs, const float* rv, const float* ds, const float* dv, const float* lnw, const float* lnb, const float* wh, int h, int vn, int lda, int64_t rows, float* os, float* ov,
                       float* outA, float* outV, hipStream_t s);
void launch_s2f_head(const float* x, const float* sums, const int32_t* grp, int Ns, const float* W, const float* bias, const float* seq,
                     const float* plddt, float thr, int L, int64_t rows, float* lp, hipStream_t s);
void launch_s2f_pick_logits(const float* lp, const int32_t* cols, int L, int T, int V, int64_t rows, float* out, hipStream_t s);
int s2f_set_option(const char* name, long long value);    // api_s2f.hip: "s2f_max_rows"
int prosst_set_option(const char* name, long long value); // api_prosst.hip: "prosst_max_rows", "prosst_share_layer0"

// S3F (s3f.hip; operands and shapes at the kernels)
constexpr int S3F_DEG = 16;                            // incoming edges of every surface point
int launch_s3f_knn(const float* q, int nq, const float* c, int nc, int k, int32_t* idx, float* dist, hipStream_t s);
void launch_s3f_edges(const float* pos, const int32_t* src, int Ns, const float* we, float* es, float* ev, hipStream_t s);
int launch_s3f_rows(const float* Z, const float* T, const int32_t* res, const float* lnw, const float* lnb, int L, int Ns, int H, int64_t rows,
                    float* out, hipStream_t s);
int launch_s3f_message(const float* P, const float* VT, const float* Es, const float* ev, const float* whe, const float* Wnt,
                       const S2fMsgWeights& w, const int32_t* src, int Ns, int64_t nodes, float* ds, float* dv, hipStream_t s);
int s3f_colsum_blocks(int Ns);
void launch_s3f_colsum(const float* x, int Ns, int copies, float* part, float* sums, hipStream_t s);

// ProtSSN's EGNN (egnn.hip; operands and shapes at the kernels).  split: the operand is written as K-interleaved split planes, else fp32 rows
void launch_egnn_edge_rows(const float* P, const float* S, const int32_t* centre, const int32_t* nb, int edges, int Hp, bool split, void* out,
                           hipStream_t s);
void launch_egnn_aggregate(const float* x, const float* msg, const int32_t* off, const int32_t* eid, int L, int D, int hp, bool split, void* out,
                           hipStream_t s);
void launch_egnn_silu_rows(const float* t, int rows, int F, float* out, hipStream_t s);
void launch_egnn_head(const float* x, const float* W, const float* bias, int rows, int D, float* lp, hipStream_t s);

// ---- vespag.hip (VespaG: the packed-row scatter and the head's row kernel; the kernels are described there) ---------------------
// out[dst_row[i], :] = src[i, :], i < n (D % 4 == 0); *nonfinite |= 1 when a value is NaN / inf (nullable)
void launch_packed_scatter(const float* src, const int32_t* dst_row, int n, int D, float* out, int32_t* nonfinite, hipStream_t s);
// y [rows][20] = LeakyReLU(h [rows][H], slope) W2^T + b2 with exact 0.0 at column wt_col[row] (-1: none); W2 [20][H], H <= 768
void launch_vespag_head(const float* h, const float* W2, const float* b2, const int32_t* wt_col, int rows, int H, float slope, float* y,
                        hipStream_t s);

// ---- mlstm.hip (UniRep's mLSTM step around the two GEMMs; the kernels are described there) -------------------------------------
// m = Tmx[tok[row * tok_stride]] * g1 [rows][Hp] -> the second product's operand: split rows m16, or fp32 m32 (exactly one)
void launch_mlstm_m(const float* g1, const float* Tmx, const int32_t* tok, int tok_stride, int rows, int Hp, unsigned short* m16,
                    float* m32, hipStream_t s);
struct MlstmGate {
    const float* z = nullptr;           // [rows][4 Hp]: m wh, gate g in columns g Hp ..
    const float* Tx = nullptr;          // [26][4 Hp]: x wx + b per token
    const int32_t* tok = nullptr;       // token of row r at tok[r * tok_stride]
    int tok_stride = 0;
    float* c = nullptr;                 // [rows][Hp] fp32, updated in place
    unsigned short* h16 = nullptr;      // the next step's operand: split rows, or
    float* h32 = nullptr;               // fp32 rows (exactly one)
    float* hwin = nullptr;              // nullable: fp32 h rows for the head
    float* z_out = nullptr;             // nullable: the pre-activations z + Tx [rows][4 Hp]
    int rows = 0, Hp = 0;
};
void launch_mlstm_gate(const MlstmGate& a, hipStream_t s);
// c / h of row r = entry join[r] of the target's table; terms[r][t < join[r]] from the target's log-probability rows (tlp nullable)
void launch_mlstm_init(const float* ctab, const uint32_t* htab, const float* tlp, const int32_t* tgt, const int32_t* join, int rows,
                       int Hp, int Lc, float* c, uint32_t* h, float* terms, hipStream_t s);
// the Dense(25) head + log-softmax over the window's steps t0 .. t0 + nw - 1 (slot t % W of hwin), rows with join <= t
void launch_mlstm_head(const float* hwin, size_t slot_stride, int W, const float* Wd, const float* bd, const int32_t* tgt,
                       const int32_t* join, int Lc, int t0, int nw, int rows, int Hp, float* terms, float* lp, hipStream_t s);
void launch_mlstm_score(const float* terms, const int32_t* tgt, int rows, int Lc, double* out, hipStream_t s);
int unirep_set_option(const char* name, long long value);   // api_unirep.hip: "unirep_max_rows"

// ---- conv_f16.hip (CARP's ByteNet block; the kernels are described there) ------------------------------------------------------
// out32 [M][C] = bias + sum over tap j of W[:, j, :] A[m + (j - taps/2) dilation] over the taps that stay inside row m's segment
// (seg_off [n_seg + 1] on the device, seg_off[n_seg] = M).  A16: the K-interleaved split rows [M][C]; W16: the weight permuted to
// [C out][taps][C in] = [C][taps C] and split as every f16x3 weight (launch_split16 mode 0), out_scale its W16::out_scale.
int launch_dilated_conv16(const unsigned short* A16, const unsigned short* W16, float out_scale, const float* bias, const int32_t* seg_off,
                          int n_seg, int64_t M, int C, int taps, int dilation, float* out32, hipStream_t s);
// the same in fp32 through an im2col buffer col [M][taps C] and launch_gemm_f32; W fp32 [C][taps C]
int launch_dilated_conv32(const float* x, const float* W, const float* bias, const int32_t* seg_off, int n_seg, int64_t M, int C, int taps,
                          int dilation, float* col, float* out32, hipStream_t s);
// y = gelu_erf(LayerNorm(x)) per row of D columns (D % 32 == 0, D <= 5120): the K-interleaved split operand, or fp32 rows
int launch_ln_gelu16(const float* x, const float* w, const float* b, int rows, int D, float eps, unsigned short* y16, hipStream_t s);
int launch_ln_gelu32(const float* x, const float* w, const float* b, int rows, int D, float eps, float* y, hipStream_t s);

// ---- gemm_f32.hip ------------------------------------------------------------------------
// C[M,N] = epi(A[M,K] W[N,K]^T + bias[N]) (+ residual[M,N]); K % 32 == 0.
// ---- msa_transformer.hip ------------------------------------------------------------------
void launch_msa_window_tokens(const int32_t* full, int R, int Tfull, int start, int Tw, int mask_col, int32_t* out, hipStream_t s);
void launch_add_row_embedding(float* x, const float* pe, int R, int C, int D, hipStream_t s);
void launch_permute_rows(const float* src, float* dst, int A, int B, int D, hipStream_t s);
// tied row attention operands for the 16-bit pipe (msa_transformer.hip)
void launch_tied_prep_qk(const float* qkv, int64_t M, int D, unsigned short* q16, unsigned short* k16, hipStream_t s);
void launch_pack_vt16(const float* qkv, int R, int C, int Kp, int H, unsigned short* Vt, hipStream_t s);
int launch_tied_softmax16(const float* part, int H, int S, int C, int Kp, float scale, unsigned short* P, hipStream_t s);
float tied_w_scale();
// The tied row attention of one alignment, from the fp32 q | k | v rows of its projection to the split-plane context rows: operand
// prep, split-K scores GEMM, softmax, update GEMM (launch_gemm16_ex).  One launch, fields assigned by name.
struct TiedRowLaunch {
    const float* qkv = nullptr;         // fp32 [R*C][3*H*64], token order (r, c), q pre-scaled by head_dim^-1/2
    int R = 0, C = 0, H = 0;
    int S = 0;                          // K splits of the scores GEMM: divides R, 1 .. 16 (tied_row_splits: the product's choice)
    unsigned short* qctx16 = nullptr;   // 2 planes x R*C*H*64 halfs, K-interleaved rows: the q operand, then overwritten by the context rows
    unsigned short* k16 = nullptr;      // the same size: the k operand
    float* part = nullptr;              // H * S * C * tied_row_kp(C): split-K partial scores
    float* p = nullptr;                 // H * C * tied_row_kp(C): the probabilities as split planes (4 bytes per element like fp32)
    float* vt = nullptr;                // H * R * 64 * tied_row_kp(C): V^T as split planes
    hipStream_t stream = nullptr;
};
int tied_row_kp(int C);                              // the update GEMM's K: columns j, zero-padded to a multiple of 64
int tied_row_splits(int R, int C, int H);            // S: divides R, ~2 rounds of score tiles at most
int tied_row_check(int R, int C, int H, int S);      // PGMI_EINVAL with a message for what launch_tied_row_attention refuses
int launch_tied_row_attention(const TiedRowLaunch& t);

int launch_gemm_f32(const float* A, const float* W, const float* bias, const float* residual,
                    float* C, int M, int N, int K, int epilogue, hipStream_t s);

// ---- gemm_f16.hip ------------------------------------------------------------------------
void gemm_options_from_env();                      // PGMI_GEMM_HALF_TAIL / PGMI_GEMM_MAX_ROWS (test hooks): at model creation, never per launch
int gemm_set_option(const char* name, long long value);
// The 16-bit GEMM: C = epi(A W^T * out_scale + bias) (+ residual) on the persistent kernel (gemm16x_kernel.h).  f16x3 (bf = false):
// A / W are fp16 hi | lo halfs in K-interleaved rows (ki_off), K % 32 == 0; bf16 (bf = true): one row-major plane each, K % 64 == 0,
// out_scale 1.  One launch, fields assigned by name; what a caller does not need keeps its default.
struct GemmLaunch {
    const unsigned short* A = nullptr;  // activations [M][K]
    const unsigned short* W = nullptr;  // weight [N][K] (model.h W16::p)
    float out_scale = 1.0f;             // W16::out_scale
    const float* bias = nullptr;        // [N]
    const float* residual = nullptr;    // fp32 [M][N]; may be out32 (in place)
    // exactly one output: fp32 rows [M][N], or the next GEMM's 16-bit operand (f16x3: K-interleaved split rows, N % 32 == 0 -- with
    // EPI_SWIGLU N / 2 columns wide, N % 64 == 0, no residual; bf16: one plane [M][N])
    float* out32 = nullptr;
    unsigned short* out16 = nullptr;
    int M = 0, N = 0, K = 0;
    int epilogue = EPI_NONE;
    bool bf = false;
    int variant = 0;                    // PGMI_GEMM_VARIANT (tuning, bit-neutral): gemm_f16.hip gemm_group_m
    hipStream_t stream = nullptr;
    // The fused QKV projection (vt16 != nullptr): N = 3 D, D % 64 == 0, M % T == 0; out16 takes the q | k rows [M][2 D] as two planes
    // qk_plane halfs apart and vt16 the transposed, key-permuted V planes -- the attention kernels' operands (AttLaunch) instead of an
    // fp32 [M][3 D] tensor; rotary applied to q, k if set.  H = 64-lane slot groups per token (heads, or 2 x heads for head_dim 128);
    // rot_halves = rotary table rows per token (1, or 2 for head_dim 128: the slot group's parity selects the frequencies).
    struct Qkv {
        unsigned short* vt16 = nullptr;
        size_t vt_plane = 0, qk_plane = 0;
        const float* cos_t = nullptr;
        const float* sin_t = nullptr;
        int rotary = 0, T = 0, H = 0, rot_halves = 1;
    } qkv;
};
int launch_gemm16(const GemmLaunch& g);
struct XMap;                                       // gemm16x_kernel.h: batched / strided operand and output maps
int launch_gemm16_ex(const unsigned short* A, const unsigned short* W, float* Cf, unsigned short* Ch, int M, int N, int K,
                     float out_scale, XMap xm, int nbatch, hipStream_t s);
// x [n/K rows][K] fp32 -> mode 0: f16x3 weight (hi/lo of x*scale), 1: bf16 plane, 2: f16x3 activation split; the
// f16x3 forms are written K-interleaved (ki_off)
void launch_split16(const float* x, int64_t n, float scale, int mode, int K, unsigned short* out, hipStream_t s);

// ESM C (api_esmc.hip): fp32 q | k | v rows [B*T][3D] of the bias-free QKV projection -> the split-fp16 attention operands (qk16 /
// vt16, the layout of qkv_prep_kernel).  q and k get a weight-only LayerNorm over the full width D (q_w / k_w, eps), the rotate-half
// rotary of 64-dim heads (cos_t / sin_t [t][64]) and q the log2(e) factor.  D = 64 H <= 2048.
int launch_qkln_prep(const float* qkv, const float* q_w, const float* k_w, float eps, const float* cos_t, const float* sin_t, int B,
                     int T, int H, unsigned short* qk16, size_t qk_plane, unsigned short* vt16, size_t vt_plane, hipStream_t s);

// ---- geom_attention.hip ------------------------------------------------------------------
// ESM3's geometric attention (the file's header has the formula), fp32 in and out.  proj [B*S][pitch]: per token q_rot | k_rot | v |
// q_dist | k_dist, H x 3 each (pitch >= 15 H).  Frames rot [n][S][9] (row-major 3x3), trans [n][S][3], mask [n][S] (non-zero = framed)
// with n = 1 shared by the B rows, or n = B (per_row_frames).  w_rot / w_dist [H]: softplus of the per-head scales.  out [B*S][opitch]:
// column 3 h + c; the columns 3 H .. opitch are written as zeros (the K padding of the out-projection that follows).
struct GeomAttLaunch {
    const float* proj = nullptr;
    int pitch = 0;
    const float *rot = nullptr, *trans = nullptr;
    const int32_t* mask = nullptr;
    bool per_row_frames = false;
    const float *w_rot = nullptr, *w_dist = nullptr;
    int B = 0, S = 0, H = 0;
    float* out = nullptr;
    int opitch = 0;
    hipStream_t stream = nullptr;
};
int launch_geom_attention(const GeomAttLaunch& g);
int geom_key_tile(int S);                              // keys per LDS tile (= queries per block) the launch picks for S: 16, 64 or 256
// ESM3's input embedding: x[r] = seq_embed[tokens[r]] + struct_embed[stok[r % T]] + cst[plddt[r % T]]  (cst [2][D])
void launch_esm3_embed(const int32_t* tokens, const int32_t* stok, const int32_t* plddt, const float* seq_embed, const float* struct_embed,
                       const float* cst, int rows, int T, int D, float* x, hipStream_t s);

// ---- attention_f32.hip -------------------------------------------------------------------
// qkv [B*T, 3*H*head_dim] (q pre-scaled by head_dim^-1/2); kv_len[b] (nullable) = valid keys.  Output: ctx fp32 [B*T, H*head_dim].
int launch_attention_f32(const float* qkv, const int32_t* kv_len, int B, int T, int H, float* ctx, hipStream_t s,
                         int head_dim = 64);   // 128: heads of two adjacent slot groups

// ---- attention_f16.hip -------------------------------------------------------------------
// What an attention launch writes its context rows as: the value is also the kernels' OUT template argument.
enum AttOut {
    ATT_OUT_F32 = 0,      // fp32 rows [rows][H * head_dim] in ctx
    ATT_OUT_SPLIT = 1,    // split fp16 hi | lo, K-interleaved rows (ki_off) in ctx16: the f16x3 out-projection's operand
    ATT_OUT_BF16 = 2      // one bf16 plane, row-major, in ctx16: the bf16 mode's out-projection operand
};
// Split-fp16 (f16x3) attention on the 16-bit MFMA pipe: operands as attention-ready fp16 planes (from the fused QKV projection, or
// from a prep pass over qkv != nullptr: rotary / Tranception depth-wise conv fused), tiles moved with direct-to-LDS loads.  One launch,
// fields assigned by name; what a caller does not need keeps its default.
struct AttLaunch {
    // operand planes (scratch when qkv != nullptr): qk16 2 planes of q | k rows, stride qk_plane >= B*T*2*H*head_dim halfs; vt16 2 planes of
    // V^T per (sequence, head), stride vt_plane >= B*H*head_dim*roundup(T,32) halfs
    unsigned short* qk16 = nullptr;
    size_t qk_plane = 0;
    unsigned short* vt16 = nullptr;
    size_t vt_plane = 0;
    int B = 1, T = 0, H = 0;
    int head_dim = 64;                  // 128: H heads of two 64-lane slot groups (ESM2-15B), 256: of four (ProGen2-xlarge); fused-QKV operands only
    const int32_t* kv_len = nullptr;    // [B] valid keys per sequence; nullptr: T
    const float* slopes = nullptr;      // [H] != nullptr: the causal flavour, slopes[h] * key added to the scores (grouped ALiBi; all zero: causal only)
    AttOut out = ATT_OUT_F32;
    float* ctx = nullptr;               // ATT_OUT_F32
    unsigned short* ctx16 = nullptr;    // ATT_OUT_SPLIT / ATT_OUT_BF16
    hipStream_t stream = nullptr;
    // optional prep pass: fp32 q | k | v rows [B*T][3*H*64] -> the operand planes, through the depth-wise convolution (conv != nullptr,
    // Tranception) or else the rotary tables (rotary != 0)
    const float* qkv = nullptr;
    const float* conv = nullptr;
    const float* cos_t = nullptr;
    const float* sin_t = nullptr;
    int rotary = 0;
};
int launch_attention_f16x3_v2(const AttLaunch& a);

// Tranception prefix-shared scoring: device arrays that describe a launch over SUFFIXES of sequences (attention_f16.hip RagMap).
struct AttRagged {
    const int32_t* seq_off;        // [sequences] first packed row of the sequence (its token seq_p): residual stream, q | k | v inputs, context
    const int32_t* seq_p;          // [sequences] first token the sequence owns (0 for a root); a = seq_p rounded down to a multiple of 32
    const int32_t* seq_q;          // [sequences] row of the q | k operand planes of the sequence's token a
    const int32_t* seq_root;       // [sequences] the sequence whose rows stand for the tokens before seq_p
    const uint32_t* seq_vt;        // [sequences] offset (halfs, per plane) of the sequence's V^T block [H][64][roundup(T - a, 32)]
    const int32_t* tile_seq;       // [n_tiles] 32-token tiles from token a on: sequence, tile index
    const int32_t* tile_j;
    const int32_t* blk_seq;        // [n_blocks] blocks of att16_waves_per_block(T) query tiles: sequence, block index inside the suffix
    const int32_t* blk_j;
    int n_tiles, n_blocks;
};
// ---- attention_prefix.hip (PoET) ------------------------------------------------------------
// Segment-causal attention over a shared prefix: n_seg segments of packed rows, each causal within itself, all seeing the P prefix keys
// unmasked.  The launch's query tiles are a device list of n_ent (segment, 32-position tile) entries in (segment, tile) order; entry e
// owns the padded rows 32 e .. 32 e + 31 of the own-segment K / V^T planes.  One descriptor serves the prep pass (fp32 q | k | v rows ->
// planes) and the attention; fields assigned by name.
struct PrefixAttLaunch {
    const float* qkv = nullptr;         // prep: fp32 [rows][3 H 64], q pre-scaled by head_dim^-1/2
    const int32_t* pos = nullptr;       // prep: [rows] rotary position of every packed row (nullptr: no rotary)
    const float* cos_t = nullptr;       // prep: rotary tables [positions][64] (model.h upload_rotary, one slot group)
    const float* sin_t = nullptr;
    const int32_t* seg_off = nullptr;   // [n_seg + 1] first packed row of every segment
    const int32_t* ent_seg = nullptr;   // [n_ent]
    const int32_t* ent_tile = nullptr;  // [n_ent]
    int n_seg = 0, n_ent = 0, H = 0;
    unsigned short* q16 = nullptr;      // [2][rows][H 64], planes q_plane halfs apart
    size_t q_plane = 0;
    unsigned short* k16 = nullptr;      // own segments: [2][H][pitch][64] and [2][H][64][pitch], planes H * pitch * 64 halfs apart
    unsigned short* vt16 = nullptr;
    size_t pitch = 0;                   // padded rows the planes are allocated for (multiple of 32, >= 32 n_ent)
    const unsigned short* pk16 = nullptr;   // the prefix, same layout with pitch ppitch; read when P > 0
    const unsigned short* pvt16 = nullptr;
    size_t ppitch = 0;
    int P = 0;
    AttOut out = ATT_OUT_SPLIT;         // ATT_OUT_F32 (ctx) or ATT_OUT_SPLIT (ctx16), packed rows of H 64 columns
    float* ctx = nullptr;
    unsigned short* ctx16 = nullptr;
    hipStream_t stream = nullptr;
};
int launch_prefix_prep(const PrefixAttLaunch& p);
int launch_prefix_attention(const PrefixAttLaunch& p);
// Cross-attention (ESM-IF1's encoder_attn): the prefix phase alone.  Every query row of every segment sees the P keys of the pk16 / pvt16
// planes, unmasked, and nothing else; k16 / vt16 / pitch / qkv / pos are not read.  launch_cross_q_prep: fp32 q rows [rows][H 64]
// (pre-scaled by head_dim^-1/2) -> the q16 planes (times log2 e); launch_cross_attention: q16 -> ctx / ctx16.
int launch_cross_q_prep(const float* q, size_t rows, int H, unsigned short* q16, size_t q_plane, hipStream_t s);
int launch_cross_attention(const PrefixAttLaunch& p);

int att16_waves_per_block(int T);
int att_set_option(const char* name, long long value);      // "att_xcd_local": block order of the dense attention launches (A/B only)
// a: qkv, conv, slopes, T, H, the operand planes, ctx16 (ATT_OUT_SPLIT, packed rows) and the stream; B and kv_len are not read
int launch_attention_tr_ragged(const AttLaunch& a, const AttRagged& rg);

}  // namespace pgmi
