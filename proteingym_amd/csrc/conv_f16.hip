// CARP's ByteNet block kernels (api_carp.hip): the dilated 1-D convolution over packed sequences as an implicit GEMM on the f16x3
// path, its fp32 fallback (im2col + launch_gemm_f32) and the row kernel LayerNorm -> erf-GELU -> operand.
//
// The convolution.  out[m][n] = bias[n] + sum over tap j, channel c of W[n][j][c] * A[m + (j - taps/2) dilation][c], where a tap
// whose source row lies outside the segment (sequence) of row m contributes nothing: the zero padding of conv1d at both ends of every
// sequence, and no tap ever reads a neighbour's rows.  As a GEMM this is M x N = C with K = taps C, whose A operand is never
// materialised: K tile kt = tap j, channels 32 kc .. 32 kc + 31 is the 128-byte line kc of source row m + (j - taps/2) dilation of
// the K-interleaved split operand [M][C] (common.h ki_off) -- the same rows, read in place, once per tap.
//   * Tile 128 (M) x BN (N; 128, or 64 for C = 64) x 32 (K), 4 waves as 2 x 2, wave tile 64 x BN / 2 in 16 x 16 accumulators of
//     v_mfma_f32_16x16x32_f16.  Fragment and accumulator layout, the XOR-swizzled LDS image of a K tile and the three split products
//     (w_lo a_hi, (w_hi 2^-11) a_lo, w_hi a_hi) are those of gemm16x_kernel.h.
//   * Both operands are staged global -> registers -> LDS, the next K tile's loads in flight under the current tile's MFMAs.  A row
//     outside its segment is a select to zero on the loaded registers (the address is clamped to row 0, so the load itself is always
//     in range): nothing depends on what a dropped direct-to-LDS lane leaves in its slot.
//   * The sum order of an output element is fixed -- taps ascending, K ascending inside a tap, the three products in the order above --
//     and an out-of-segment tap adds exact zeros, so a row's bits depend on its own segment only: not on M, on the other segments, on
//     the tile it lands in or on the launch.
#include "common.h"
#include "gemm16x_kernel.h"          // mfma16x16, u32x4; no GEMM kernel is instantiated here

namespace pgmi {

constexpr int CV_BM = 128, CV_NT = 256;

// The segment of packed row m: the last s with seg_off[s] <= m (empty segments are skipped).  seg_off [n_seg + 1], ascending.
__device__ __forceinline__ void conv_segment(const int32_t* __restrict__ seg_off, int n_seg, int m, int& lo, int& hi) {
    int a = 0, b = n_seg - 1;
    while (a < b) {
        const int mid = (a + b + 1) >> 1;
        if (seg_off[mid] <= m) a = mid; else b = mid - 1;
    }
    lo = seg_off[a];
    hi = seg_off[a + 1];
}

template <int BN>
__global__ __launch_bounds__(CV_NT) void dilated_conv16_kernel(const unsigned short* __restrict__ A, const unsigned short* __restrict__ W,
                                                               const float* __restrict__ bias, const int32_t* __restrict__ seg_off,
                                                               int n_seg, int M, int C, int taps, int dilation, float out_scale,
                                                               int tiles_n, float* __restrict__ out) {
    constexpr int TM = 4, TN = BN / 32;          // M16 / N16 tiles per wave
    constexpr int LA = CV_BM * 8 / CV_NT;        // 16-byte chunks a thread stages per K tile: A (4) and W (BN / 32)
    constexpr int LW = BN * 8 / CV_NT;
    __shared__ __attribute__((aligned(16))) u32x4 sA[CV_BM * 8];
    __shared__ __attribute__((aligned(16))) u32x4 sW[BN * 8];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int r = lane & 15, kq = lane >> 4;
    const int m0 = (int)(blockIdx.x / tiles_n) * CV_BM, n0 = (int)(blockIdx.x % tiles_n) * BN;
    const int row_lo = tid >> 3, c8 = tid & 7;   // slot tid + 256 i = (row row_lo + 32 i, chunk c8): 8 lanes move one row's line
    const int nkc = C >> 5, nk = taps * nkc, K = taps * C;

    int lo[LA], hi[LA];
#pragma unroll
    for (int i = 0; i < LA; ++i) {
        const int m = m0 + row_lo + 32 * i;
        lo[i] = hi[i] = 0;                       // a row beyond M: no tap is ever inside
        if (m < M) conv_segment(seg_off, n_seg, m, lo[i], hi[i]);
        hi[i] = min(hi[i], M);
        lo[i] = max(lo[i], 0);
    }
    const unsigned short* wrow[LW];
#pragma unroll
    for (int i = 0; i < LW; ++i) wrow[i] = W + (size_t)min(n0 + row_lo + 32 * i, C - 1) * (size_t)(2 * K) + c8 * 8;

    u32x4 ra[LA], rw[LW];
    auto load_tile = [&](int kt) {
        const int tap = kt / nkc, kc = kt - tap * nkc;
        const int shift = (tap - (taps >> 1)) * dilation;
#pragma unroll
        for (int i = 0; i < LA; ++i) {
            const int src = m0 + row_lo + 32 * i + shift;
            const bool in = src >= lo[i] && src < hi[i];
            const u32x4 v = *reinterpret_cast<const u32x4*>(A + (size_t)(in ? src : 0) * (size_t)(2 * C) + kc * 64 + c8 * 8);
            ra[i] = in ? v : u32x4{0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (int i = 0; i < LW; ++i) rw[i] = *reinterpret_cast<const u32x4*>(wrow[i] + (size_t)kt * 64);
    };
    auto store_tile = [&]() {
#pragma unroll
        for (int i = 0; i < LA; ++i) {
            const int row = row_lo + 32 * i;
            sA[row * 8 + (c8 ^ ((row >> 1) & 7))] = ra[i];
        }
#pragma unroll
        for (int i = 0; i < LW; ++i) {
            const int row = row_lo + 32 * i;
            sW[row * 8 + (c8 ^ ((row >> 1) & 7))] = rw[i];
        }
    };

    f32x4 acc[TN][TM];
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int i = 0; i < TM; ++i) acc[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int fsw = (r >> 1) & 7;
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    const h2 sc = {(_Float16)(1.0f / kLoScale), (_Float16)(1.0f / kLoScale)};

    load_tile(0);
    for (int kt = 0; kt < nk; ++kt) {
        __syncthreads();                         // the previous tile's fragments have been read
        store_tile();
        __syncthreads();
        if (kt + 1 < nk) load_tile(kt + 1);
        u32x4 af[2][TM], wf[2][TN], whs[TN];
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int c = (p * 4 + kq) ^ fsw;    // chunk kq of the hi half (p = 0) / the lo half (p = 1) of the row's line
#pragma unroll
            for (int i = 0; i < TM; ++i) af[p][i] = sA[((wm * TM + i) * 16 + r) * 8 + c];
#pragma unroll
            for (int j = 0; j < TN; ++j) wf[p][j] = sW[((wn * TN + j) * 16 + r) * 8 + c];
        }
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {        // w_hi 2^-11: exact, the weights are pre-scaled to ~2^13
                const unsigned int u = wf[0][j][e];
                const h2 t = __builtin_bit_cast(h2, u) * sc;
                whs[j][e] = __builtin_bit_cast(unsigned int, t);
            }
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int i = 0; i < TM; ++i) acc[j][i] = mfma16x16<false>(wf[1][j], af[0][i], acc[j][i]);      // w_lo a_hi
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int i = 0; i < TM; ++i) acc[j][i] = mfma16x16<false>(whs[j], af[1][i], acc[j][i]);        // (w_hi 2^-11)(a_lo 2^11)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int i = 0; i < TM; ++i) acc[j][i] = mfma16x16<false>(wf[0][j], af[0][i], acc[j][i]);      // w_hi a_hi
    }

    // accumulator of M16 tile i, N16 tile j: lane holds row 16 i + r, columns 16 j + 4 kq + e
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = n0 + (wn * TN + j) * 16 + 4 * kq;
        if (n >= C) continue;                    // C % 32 == 0: the four columns are inside together
        const f32x4 bv = *reinterpret_cast<const f32x4*>(bias + n);
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int m = m0 + (wm * TM + i) * 16 + r;
            if (m >= M) continue;
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = __builtin_fmaf(acc[j][i][e], out_scale, bv[e]);
            *reinterpret_cast<f32x4*>(out + (size_t)m * C + n) = o;
        }
    }
}

static int conv_check(const void* a, const void* w, const void* bias, const void* seg_off, int n_seg, int64_t M, int C, int taps,
                      int dilation, const void* out) {
    if (!a || !w || !bias || !seg_off || !out) { set_error("dilated conv: null argument"); return PGMI_EINVAL; }
    if (n_seg < 1 || M < 1 || M > (1LL << 30)) { set_error("dilated conv: %lld rows in %d segments", (long long)M, n_seg); return PGMI_EINVAL; }
    if (C < 32 || C % 32 || C > 8192) { set_error("dilated conv: C = %d must be a multiple of 32 in 32 .. 8192", C); return PGMI_EINVAL; }
    if (taps < 1 || taps > 15 || !(taps & 1)) { set_error("dilated conv: %d taps (odd, 1 .. 15)", taps); return PGMI_EINVAL; }
    if (dilation < 1 || dilation > (1 << 20)) { set_error("dilated conv: dilation %d", dilation); return PGMI_EINVAL; }
    return PGMI_OK;
}

int launch_dilated_conv16(const unsigned short* A16, const unsigned short* W16, float out_scale, const float* bias, const int32_t* seg_off,
                          int n_seg, int64_t M, int C, int taps, int dilation, float* out32, hipStream_t s) {
    int rc = conv_check(A16, W16, bias, seg_off, n_seg, M, C, taps, dilation, out32);
    if (rc) return rc;
    const int64_t tiles_m = (M + CV_BM - 1) / CV_BM;
    if (C <= 64) {
        const int tiles_n = (C + 63) / 64;
        hipLaunchKernelGGL((dilated_conv16_kernel<64>), dim3((unsigned)(tiles_m * tiles_n)), dim3(CV_NT), 0, s, A16, W16, bias, seg_off,
                           n_seg, (int)M, C, taps, dilation, out_scale, tiles_n, out32);
    } else {
        const int tiles_n = (C + 127) / 128;
        hipLaunchKernelGGL((dilated_conv16_kernel<128>), dim3((unsigned)(tiles_m * tiles_n)), dim3(CV_NT), 0, s, A16, W16, bias, seg_off,
                           n_seg, (int)M, C, taps, dilation, out_scale, tiles_n, out32);
    }
    PGMI_HIP(hipGetLastError());
    return PGMI_OK;
}

// ---- fp32 fallback: col[m][j C + c] = x[m + (j - taps/2) dilation][c] inside the segment, else 0; then launch_gemm_f32 ----
__global__ __launch_bounds__(256) void conv_im2col_kernel(const float* __restrict__ x, const int32_t* __restrict__ seg_off, int n_seg, int M,
                                                          int C, int taps, int dilation, float* __restrict__ col) {
    const int m = blockIdx.x;
    int lo, hi;
    conv_segment(seg_off, n_seg, m, lo, hi);
    hi = min(hi, M);
    lo = max(lo, 0);
    const int nv = C >> 2;
    for (int j = 0; j < taps; ++j) {
        const int src = m + (j - (taps >> 1)) * dilation;
        const bool in = src >= lo && src < hi;
        const f32x4* sr = reinterpret_cast<const f32x4*>(x + (size_t)(in ? src : 0) * C);
        f32x4* dr = reinterpret_cast<f32x4*>(col + ((size_t)m * taps + j) * C);
        for (int c = threadIdx.x; c < nv; c += 256) dr[c] = in ? sr[c] : f32x4{0.f, 0.f, 0.f, 0.f};
    }
}

int launch_dilated_conv32(const float* x, const float* W, const float* bias, const int32_t* seg_off, int n_seg, int64_t M, int C, int taps,
                          int dilation, float* col, float* out32, hipStream_t s) {
    int rc = conv_check(x, W, bias, seg_off, n_seg, M, C, taps, dilation, out32);
    if (rc) return rc;
    if (!col || M * (int64_t)taps * C >= (1LL << 31)) { set_error("dilated conv (fp32): im2col buffer of %lld x %d elements", (long long)M, taps * C); return PGMI_EINVAL; }
    hipLaunchKernelGGL(conv_im2col_kernel, dim3((unsigned)M), dim3(256), 0, s, x, seg_off, n_seg, (int)M, C, taps, dilation, col);
    return launch_gemm_f32(col, W, bias, nullptr, out32, (int)M, C, taps * C, EPI_NONE, s);
}

// ---- LayerNorm -> erf-GELU -> the next product's operand; one wave per row, the row in registers (launch_layernorm16's shape) ----
// The GELU is the exact form 0.5 x (1 + erff(x / sqrt 2)), not the GEMM epilogue's fitted one: three of these sit in every block, in
// front of every product, and the row kernel is bound by memory, not by VALU issue.
__device__ __forceinline__ float conv_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

template <int NV, bool SPLIT>
__global__ __launch_bounds__(256) void ln_gelu_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
                                                      int rows, int D, float eps, float* __restrict__ y32, unsigned short* __restrict__ y16) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const int nv = D >> 2;
    const f32x4* xr = reinterpret_cast<const f32x4*>(x + (size_t)row * D);
    f32x4 v[NV];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = lane + 64 * i;
        v[i] = (c < nv) ? xr[c] : f32x4{0.f, 0.f, 0.f, 0.f};
        s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
    }
    const float mean = conv_wave_sum(s) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = lane + 64 * i;
        if (c < nv) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float d = v[i][k] - mean;
                q += d * d;
            }
        }
    }
    const float rstd = 1.0f / sqrtf(conv_wave_sum(q) / (float)D + eps);
    const f32x4* wr = reinterpret_cast<const f32x4*>(w);
    const f32x4* br = reinterpret_cast<const f32x4*>(b);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = lane + 64 * i;
        if (c < nv) {                            // D % 8 == 0: both lanes of a pair are inside together (store_split4)
            const f32x4 wv = wr[c], bv = br[c];
            f32x4 o;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float t = (v[i][k] - mean) * rstd * wv[k] + bv[k];
                o[k] = 0.5f * t * (1.0f + erff(t * 0.70710678118654752440f));
            }
            if constexpr (SPLIT) store_split4(o, y16, (size_t)row, c, lane, D);
            else reinterpret_cast<f32x4*>(y32 + (size_t)row * D)[c] = o;
        }
    }
}

template <bool SPLIT>
static void ln_gelu_dispatch(const float* x, const float* w, const float* b, int rows, int D, float eps, float* y32, unsigned short* y16,
                             hipStream_t s) {
    const dim3 grid((rows + 3) / 4), block(256);
    const int nv = (D / 4 + 63) / 64;
    if (nv <= 1) hipLaunchKernelGGL((ln_gelu_kernel<1, SPLIT>), grid, block, 0, s, x, w, b, rows, D, eps, y32, y16);
    else if (nv <= 2) hipLaunchKernelGGL((ln_gelu_kernel<2, SPLIT>), grid, block, 0, s, x, w, b, rows, D, eps, y32, y16);
    else if (nv <= 5) hipLaunchKernelGGL((ln_gelu_kernel<5, SPLIT>), grid, block, 0, s, x, w, b, rows, D, eps, y32, y16);
    else hipLaunchKernelGGL((ln_gelu_kernel<20, SPLIT>), grid, block, 0, s, x, w, b, rows, D, eps, y32, y16);
}

static int ln_gelu_check(const void* x, const void* w, const void* b, int rows, int D, const void* y) {
    if (!x || !w || !b || !y || rows < 1) { set_error("ln_gelu: bad argument"); return PGMI_EINVAL; }
    if (D < 32 || D % 32 || D > 5120) { set_error("ln_gelu: D = %d must be a multiple of 32 in 32 .. 5120", D); return PGMI_EINVAL; }
    return PGMI_OK;
}

int launch_ln_gelu16(const float* x, const float* w, const float* b, int rows, int D, float eps, unsigned short* y16, hipStream_t s) {
    int rc = ln_gelu_check(x, w, b, rows, D, y16);
    if (rc) return rc;
    ln_gelu_dispatch<true>(x, w, b, rows, D, eps, nullptr, y16, s);
    return PGMI_OK;
}

int launch_ln_gelu32(const float* x, const float* w, const float* b, int rows, int D, float eps, float* y, hipStream_t s) {
    int rc = ln_gelu_check(x, w, b, rows, D, y);
    if (rc) return rc;
    ln_gelu_dispatch<false>(x, w, b, rows, D, eps, y, nullptr, s);
    return PGMI_OK;
}

}  // namespace pgmi
