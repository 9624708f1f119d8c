// UniRep's multiplicative LSTM (proteingym/baselines/unirep/unirep.py mLSTMCell1900.call, :118-132) around the two products of a step.
// A step of the active rows is, on the handle's stream and in this order (api_unirep.hip ur_step):
//   g1 = h_prev wmh                 the shared GEMM (f16x3: launch_gemm16 on the split h rows; fp32: launch_gemm_f32)
//   m  = Tmx[token] * g1            mlstm_m_kernel: unirep.py:123 with the input-side product folded into a 26-row table; written as
//                                   the second product's operand (split rows, or fp32)
//   z' = m wh                       the shared GEMM, N = 4 Hp: the columns of gate g (i, f, o, u: unirep.py:125) are g Hp .. g Hp + Hp
//   z = z' + Tx[token]; gates; c, h mlstm_gate_kernel: unirep.py:124-131 (Tx = x wx + b per token); c fp32 in place, h as the next
//                                   step's operand and as an fp32 row of the head's window
// Every kernel here is element-local or row-local with a fixed order of its sums, and the GEMMs' sums do not depend on the row count,
// so a row's bits do not depend on the rows around it: that is what makes a start from the target's stored state exact.
// Hp = H rounded up to 32; the padded units have zero weights and zero table entries: z = 0, c = 0.5 * 0 + 0.5 * tanh(0) = 0,
// h = 0.5 * tanh(0) = 0, exactly.
// sigmoid is 1 / (1 + expf(-x)) with the library's expf and a true division, tanh the library's tanhf: no fast-math forms.
#include "common.h"

namespace pgmi {

constexpr int MLSTM_OUT = 25;        // Dense(vocab - 1), unirep.py:396

__device__ __forceinline__ float mlstm_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }

// One thread per 4 columns.  Hp % 8 == 0, so a row has an even number of groups and the lanes (2m, 2m + 1) hold the two groups of one
// 8-column block of one row, both inside the grid or both outside it: what store_split4 needs.
__global__ void __launch_bounds__(256) mlstm_m_kernel(const float* __restrict__ g1, const float* __restrict__ Tmx,
                                                      const int32_t* __restrict__ tok, int tok_stride, int rows, int Hp,
                                                      unsigned short* __restrict__ m16, float* __restrict__ m32) {
    const int G = Hp >> 2;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)rows * G) return;
    const int row = (int)(i / G), c = (int)(i % G);
    const int tk = tok[(size_t)row * tok_stride];
    const f32x4 o = ld4(g1 + (size_t)row * Hp + 4 * c) * ld4(Tmx + (size_t)tk * Hp + 4 * c);
    if (m32) st4(m32 + (size_t)row * Hp + 4 * c, o);
    else store_split4(o, m16, (size_t)row, c, threadIdx.x & 63, Hp);
}

void launch_mlstm_m(const float* g1, const float* Tmx, const int32_t* tok, int tok_stride, int rows, int Hp, unsigned short* m16,
                    float* m32, hipStream_t s) {
    const int64_t n = (int64_t)rows * (Hp >> 2);
    hipLaunchKernelGGL(mlstm_m_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, g1, Tmx, tok, tok_stride, rows, Hp, m16, m32);
}

__global__ void __launch_bounds__(256) mlstm_gate_kernel(MlstmGate a) {
    const int Hp = a.Hp, G = Hp >> 2;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)a.rows * G) return;
    const int row = (int)(i / G), c = (int)(i % G);
    const int tk = a.tok[(size_t)row * a.tok_stride];
    const float* zr = a.z + (size_t)row * 4 * Hp + 4 * c;
    const float* tx = a.Tx + (size_t)tk * 4 * Hp + 4 * c;
    const f32x4 zi = ld4(zr) + ld4(tx), zf = ld4(zr + Hp) + ld4(tx + Hp), zo = ld4(zr + 2 * Hp) + ld4(tx + 2 * Hp),
                zu = ld4(zr + 3 * Hp) + ld4(tx + 3 * Hp);
    if (a.z_out) {
        float* q = a.z_out + (size_t)row * 4 * Hp + 4 * c;
        st4(q, zi); st4(q + Hp, zf); st4(q + 2 * Hp, zo); st4(q + 3 * Hp, zu);
    }
    const size_t e = (size_t)row * Hp + 4 * c;
    const f32x4 cp = ld4(a.c + e);
    f32x4 cn, h;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float ig = mlstm_sigmoid(zi[k]), fg = mlstm_sigmoid(zf[k]), og = mlstm_sigmoid(zo[k]), u = tanhf(zu[k]);
        cn[k] = fg * cp[k] + ig * u;
        h[k] = og * tanhf(cn[k]);
    }
    st4(a.c + e, cn);
    if (a.hwin) st4(a.hwin + e, h);
    if (a.h32) st4(a.h32 + e, h);
    else store_split4(h, a.h16, (size_t)row, c, threadIdx.x & 63, Hp);
}

void launch_mlstm_gate(const MlstmGate& a, hipStream_t s) {
    const int64_t n = (int64_t)a.rows * (a.Hp >> 2);
    hipLaunchKernelGGL(mlstm_gate_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
}

// Row r of a chunk starts from entry join[r] of the target's table: c fp32, h as 4 bytes per unit in either operand form (a split row is
// 2 Hp halfs, an fp32 row Hp floats).  Entry 0 is the zero state.
__global__ void __launch_bounds__(256) mlstm_init_kernel(const float* __restrict__ ctab, const uint32_t* __restrict__ htab,
                                                         const int32_t* __restrict__ join, int rows, int Hp, float* __restrict__ c,
                                                         uint32_t* __restrict__ h) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)rows * Hp) return;
    const int row = (int)(i / Hp), k = (int)(i % Hp);
    const size_t src = (size_t)join[row] * Hp + k;
    c[i] = ctab[src];
    h[i] = htab[src];
}

// terms[r][t] for t < join[r]: the target's log-probability row t at the row's own target token (unirep.py:355: class = target - 1)
__global__ void __launch_bounds__(256) mlstm_prefix_terms_kernel(const float* __restrict__ tlp, const int32_t* __restrict__ tgt,
                                                                 const int32_t* __restrict__ join, int rows, int Lc,
                                                                 float* __restrict__ terms) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)rows * Lc) return;
    const int row = (int)(i / Lc), t = (int)(i % Lc);
    if (t >= join[row]) return;
    const int y = tgt[i];
    terms[i] = y > 0 ? tlp[(size_t)t * MLSTM_OUT + (y - 1)] : 0.0f;
}

void launch_mlstm_init(const float* ctab, const uint32_t* htab, const float* tlp, const int32_t* tgt, const int32_t* join, int rows,
                       int Hp, int Lc, float* c, uint32_t* h, float* terms, hipStream_t s) {
    const int64_t n = (int64_t)rows * Hp, nt = (int64_t)rows * Lc;
    hipLaunchKernelGGL(mlstm_init_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, ctab, htab, join, rows, Hp, c, h);
    if (tlp)
        hipLaunchKernelGGL(mlstm_prefix_terms_kernel, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, s, tlp, tgt, join, rows, Lc, terms);
}

// The head over a window of steps t0 .. t0 + nw - 1 (unirep.py:396-408): one wave per (step, row).  logits = h Wd + bd in fp32 (each
// lane a fixed stride of the columns, then a butterfly over the wave: one order for every row), log-softmax over the 25 classes,
// terms[row][t] = log p(target - 1); lp (nullable) receives the whole row.  Rows that have not joined at step t are skipped.
__global__ void __launch_bounds__(256) mlstm_head_kernel(const float* __restrict__ hwin, size_t slot_stride, int W,
                                                         const float* __restrict__ Wd, const float* __restrict__ bd,
                                                         const int32_t* __restrict__ tgt, const int32_t* __restrict__ join, int Lc, int t0,
                                                         int nw, int rows, int Hp, float* __restrict__ terms, float* __restrict__ lp) {
    const int lane = threadIdx.x & 63;
    const int64_t id = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (id >= (int64_t)nw * rows) return;
    const int w = (int)(id / rows), row = (int)(id % rows), t = t0 + w;
    if (join[row] > t) return;
    const float* h = hwin + (size_t)(t % W) * slot_stride + (size_t)row * Hp;
    float acc[MLSTM_OUT];
#pragma unroll
    for (int v = 0; v < MLSTM_OUT; ++v) acc[v] = 0.0f;
    for (int k = 4 * lane; k < Hp; k += 256) {
        const f32x4 hv = ld4(h + k);
#pragma unroll
        for (int v = 0; v < MLSTM_OUT; ++v) {
            const f32x4 wv = ld4(Wd + (size_t)v * Hp + k);
            acc[v] += hv[0] * wv[0] + hv[1] * wv[1] + hv[2] * wv[2] + hv[3] * wv[3];
        }
    }
    float mx = -INFINITY;
#pragma unroll
    for (int v = 0; v < MLSTM_OUT; ++v) {
        float a = acc[v];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) a += __shfl_xor(a, o);
        acc[v] = a + bd[v];
        mx = fmaxf(mx, acc[v]);
    }
    float se = 0.0f;
#pragma unroll
    for (int v = 0; v < MLSTM_OUT; ++v) se += expf(acc[v] - mx);
    const float lse = mx + logf(se);
    const size_t e = (size_t)row * Lc + t;
    const int y = tgt[e];
    float term = 0.0f;
#pragma unroll
    for (int v = 0; v < MLSTM_OUT; ++v) {
        const float l = acc[v] - lse;
        if (v == y - 1) term = l;
        if (lp && lane == v) lp[e * MLSTM_OUT + v] = l;
    }
    if (lane == 0) terms[e] = term;
}

void launch_mlstm_head(const float* hwin, size_t slot_stride, int W, const float* Wd, const float* bd, const int32_t* tgt,
                       const int32_t* join, int Lc, int t0, int nw, int rows, int Hp, float* terms, float* lp, hipStream_t s) {
    const int64_t n = (int64_t)nw * rows;
    hipLaunchKernelGGL(mlstm_head_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, hwin, slot_stride, W, Wd, bd, tgt, join, Lc, t0,
                       nw, rows, Hp, terms, lp);
}

// tfa.seq2seq.sequence_loss with average_across_timesteps (unirep.py:403-408): per row sum(xent * mask) / (sum(mask) + 1e-12), mask =
// sign(target); the fp32 terms are added in double, left to right.
__global__ void __launch_bounds__(256) mlstm_score_kernel(const float* __restrict__ terms, const int32_t* __restrict__ tgt, int rows, int Lc,
                                                          double* __restrict__ out) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= rows) return;
    double s = 0.0, n = 0.0;
    for (int t = 0; t < Lc; ++t) {
        const size_t e = (size_t)row * Lc + t;
        if (tgt[e] > 0) { s -= (double)terms[e]; n += 1.0; }
    }
    out[row] = s / (n + 1e-12);
}

void launch_mlstm_score(const float* terms, const int32_t* tgt, int rows, int Lc, double* out, hipStream_t s) {
    hipLaunchKernelGGL(mlstm_score_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, terms, tgt, rows, Lc, out);
}

}  // namespace pgmi
