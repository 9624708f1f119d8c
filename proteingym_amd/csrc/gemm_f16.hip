// GEMMs on the 16-bit matrix cores: C = epi(A W^T * 2^-s + bias) (+ residual).
//
// Replaces nn.Linear on the ESM hot path (modules.py:134-140, multihead_attention.py:258-261, 394) in the f16x3
// (default, parity-gated) and bf16 (throughput, not parity-gated) modes.
//
// f16x3: every fp32 operand x is carried as two fp16 planes, hi = fp16(x) and a low part (weights:
// lo = fp16(x - hi); activations: lo = fp16((x - hi) 2^11), common.h split_act); the kernel accumulates
//     a_hi w_hi + a_hi w_lo + (a_lo 2^11)(w_hi 2^-11)
// in the fp32 MFMA accumulator (the dropped a_lo w_lo term is 2^-22 relative).  fp16 x fp16 products are exact in
// fp32, so the result has ~22 mantissa bits -- measured fp32-class on the full 33- and 36-layer models --
// at 3 MFMAs of the 2.5 PFLOP/s pipe per product block instead of 1 MFMA of the 157 TFLOP/s fp32 pipe.  Weights are
// pre-scaled by a per-tensor power of two 2^s (exact) so that their lo plane stays in fp16's normal range; 2^-s is
// applied in the epilogue.  Activations arrive already split (the producing LayerNorm / GELU / attention epilogue
// writes both planes: the same 4 bytes per element as fp32).
//
// Operand layout in HBM ("K-interleaved planes", common.h ki_off): a row of K elements is stored as K/32 groups of
// 128 bytes = 32 hi halfs followed by the 32 lo halfs of the same k.  One row's share of a 32-deep K tile is then ONE
// full 128-byte line: 8 consecutive lanes fetch it with one dwordx4 each.  With two separate planes the same data was
// two 64-byte half lines, every line was requested twice (the other half one K tile later, long evicted from the 32 KB
// L1) and the texture-address unit handled twice the lines: measured with the phase-timing instantiation,
// 288 -> 325 TFLOP/s on the FC2 shape from the access pattern alone.
//
// bf16: one row-major bf16 plane per operand, no scaling, one MFMA per product block, on the same kernel (gemm16x_kernel.h BF).
//
// Launch path: a caller fills a GemmLaunch (common.h) and calls launch_gemm16 -- argument checks, launch_gemm16x (row chunks under
// the 32-bit offset range), launch_gemm16x_one (the TilePlan), launch_x (the instantiation table kGemmInst; set-attribute, launch,
// error).  launch_gemm16_ex (the batched / strided form, XMap) makes its own TilePlan and ends in launch_x too.
//
// Roofline: MFMA-bound; peak 2.5 PFLOP/s of 16-bit MFMA = 833 TFLOP/s of fp32-equivalent algorithmic FLOPs in f16x3.
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <mutex>

#include "common.h"
#include "gemm16x_kernel.h"            // typedefs, gelu_erf16, QkvOut, TilePlan, gemm16x_kernel (the persistent ping-pong kernel)

namespace pgmi {

// Per-device launch state (a process may drive several devices through distinct model handles: nothing here is shared
// between devices).  Indexed by the current HIP device of the calling thread; written under a mutex because two handles on two
// devices may launch from two host threads.
constexpr int kMaxDevices = 64;
static int g_num_cus[kMaxDevices];
static std::mutex g_xdev_mu;

static int x_num_cus() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) dev = 0;
    std::lock_guard<std::mutex> lk(g_xdev_mu);
    int& n = g_num_cus[dev];
    if (!n) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, dev) == hipSuccess) n = prop.multiProcessorCount;
        if (n <= 0) n = 256;
        n -= n % 8;                                              // the XCD-aware item order wants a multiple of 8
        if (n <= 0) n = 8;
    }
    return n;
}

// Row panels per group of the grouped tile order.  An XCD's 32 concurrent tiles then cover ~g row panels x 32/g column panels: per K
// step g A slices + 32/g W slices miss its L2.  W (the layer's weights, 6.5 - 26 MB) is shared by every tile of the launch and
// stays in the Infinity Cache; A (the activations, 0.4 - 1.7 GB) streams from HBM: fewer A slices per step win although the slice
// count is the same -- measured (scripts/gemm_ab.py, BLAT shape) g = 8 -> 4: QKV 400 -> 414, out 374 -> 383, FC2 419 -> 429 TFLOP/s,
// FC1 unchanged; g = 2 within noise of 4, 16 / 32 / 64 worse.  Tile order does not touch a row's arithmetic: same bits.
// FC1 (N = 5120: 20 column panels) runs at the same speed with 4 and with 8 but fetches less with 8 (3.26 vs 3.47 GB per launch: with
// 20 column panels a group of 4 rows is 80 tiles = 2.5 rounds of an XCD, and the partial rounds straddle two groups): wide outputs keep 8.
constexpr int kGroupM = 4, kGroupMWide = 8, kWideTilesN = 16;
// Test hooks (bit-neutral: both only change how a launch is cut into items / row chunks).  Read from the environment when a model is
// created and at the op-level entries (gemm_options_from_env), changed on a live model through pgmi_set_option -- never per launch.
//   PGMI_GEMM_HALF_TAIL / "gemm_half_tail": 0 = no half-height tail items;  PGMI_GEMM_MAX_ROWS / "gemm_max_rows": force row chunks
// An option set through pgmi_set_option stays in force: creating another model or calling an op-level entry re-reads the environment
// only for the options nobody has set explicitly (value -1 hands an option back to the environment / its default).  Process-wide and
// not synchronised: they are test hooks, changed between launches by the thread that launches.
struct GemmOptions { int half_tail = 1; long long max_rows = 0; bool half_tail_set = false, max_rows_set = false; };
static GemmOptions g_opt;
void gemm_options_from_env() {
    const char* h = getenv("PGMI_GEMM_HALF_TAIL");
    const char* r = getenv("PGMI_GEMM_MAX_ROWS");
    if (!g_opt.half_tail_set) g_opt.half_tail = h ? atoi(h) : 1;
    if (!g_opt.max_rows_set) g_opt.max_rows = r ? atoll(r) : 0;
}
int gemm_set_option(const char* name, long long value) {
    if (!strcmp(name, "gemm_half_tail")) {
        g_opt.half_tail_set = value >= 0;
        if (value >= 0) g_opt.half_tail = (int)value; else gemm_options_from_env();
        return PGMI_OK;
    }
    if (!strcmp(name, "gemm_max_rows")) {
        g_opt.max_rows_set = value >= 0;
        if (value >= 0) g_opt.max_rows = value; else gemm_options_from_env();
        return PGMI_OK;
    }
    return PGMI_EINVAL;
}

// PGMI_GEMM_VARIANT (tuning; GemmLaunch::variant) -> the row panels per group of the grouped tile order; 0 = by shape.  Everything below
// 1000 is the product's configuration; 1000 + t takes the low four bits of t (the interleaved A/B of scripts/gemm_ab.py).  Tile order
// does not touch a row's arithmetic: same bits at every value.  No value is refused: 2000, which once selected the first bf16 kernel,
// decodes like any other value of 1000 or above (1000 & 15 = 8 row panels).
static int gemm_group_m(int variant) { return variant >= 1000 ? (variant - 1000) & 15 : 0; }

// Every gemm16x_kernel instantiation of the library, keyed by (epilogue, output kind = the kernel's OUT, XM, BF).
enum { X_OUT_F32 = 0, X_OUT_16 = 1, X_OUT_QKV = 2 };
using GemmKernel = decltype(&gemm16x_kernel<EPI_NONE, X_OUT_F32>);
struct GemmInst { int epi, out; bool xm, bf; GemmKernel fn; };
template <int EPI, int OUT, bool XM = false, bool BF = false>
static GemmInst inst() { return {EPI, OUT, XM, BF, gemm16x_kernel<EPI, OUT, XM, BF>}; }
static const GemmInst kGemmInst[] = {
    inst<EPI_NONE, X_OUT_F32>(),                   inst<EPI_NONE, X_OUT_16>(),                   inst<EPI_NONE, X_OUT_QKV>(),
    inst<EPI_GELU, X_OUT_F32>(),                   inst<EPI_GELU, X_OUT_16>(),
    inst<EPI_SQRELU, X_OUT_F32>(),                 inst<EPI_SQRELU, X_OUT_16>(),
    inst<EPI_GELU_TANH, X_OUT_F32>(),              inst<EPI_GELU_TANH, X_OUT_16>(),
    inst<EPI_SWIGLU, X_OUT_16>(),                                                                // f16x3, split-plane output only
    inst<EPI_RELU, X_OUT_F32>(),                   inst<EPI_RELU, X_OUT_16>(),                   // f16x3 only (ESM-IF1's decoder)
    inst<EPI_NONE, X_OUT_F32, false, true>(),      inst<EPI_NONE, X_OUT_16, false, true>(),      inst<EPI_NONE, X_OUT_QKV, false, true>(),
    inst<EPI_GELU, X_OUT_F32, false, true>(),      inst<EPI_GELU, X_OUT_16, false, true>(),
    inst<EPI_SQRELU, X_OUT_F32, false, true>(),    inst<EPI_SQRELU, X_OUT_16, false, true>(),
    inst<EPI_GELU_TANH, X_OUT_F32, false, true>(), inst<EPI_GELU_TANH, X_OUT_16, false, true>(),
    inst<EPI_NONE, X_OUT_F32, true>(),             inst<EPI_NONE, X_OUT_16, true>(),             // launch_gemm16_ex
};

// One launch of one instantiation on min(G, n_items) workgroups: table lookup, set-attribute (per launch), launch, error.  c_plane is
// the fused QKV's q | k plane stride and 0 for every other output kind.
static int launch_x(const GemmLaunch& g, int out, bool xm, size_t c_plane, int G, int n_items, const TilePlan& tp, const QkvOut& qo,
                    const XMap& xmap) {
    const GemmInst* k = nullptr;
    for (const GemmInst& i : kGemmInst)
        if (i.epi == g.epilogue && i.out == out && i.xm == xm && i.bf == g.bf) { k = &i; break; }
    if (!k) {
        set_error("gemm16: no kernel for epilogue %d, output kind %d, xmap %d, bf16 %d", g.epilogue, out, (int)xm, (int)g.bf);
        return PGMI_EINVAL;
    }
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k->fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)X_LDS_BYTES);
    if (e != hipSuccess) { set_error("hipFuncSetAttribute: %s", hipGetErrorString(e)); return PGMI_EHIP; }
    hipLaunchKernelGGL(k->fn, dim3(std::min(G, n_items)), dim3(XNT), X_LDS_BYTES, g.stream, g.A, g.W, g.bias, g.residual, g.out32, g.out16,
                       c_plane, g.M, g.N, g.K, g.out_scale, tp, qo, xmap);
    PGMI_HIP(hipGetLastError());
    return PGMI_OK;
}

static int launch_gemm16x_one(const GemmLaunch& g, int group_m) {
    const int M = g.M, N = g.N, K = g.K;
    const bool qkv = g.qkv.vt16 != nullptr;
    const unsigned long long eb = g.bf ? 2ull : 4ull;                // operand bytes per k element (gemm16x_kernel.h: BF)
    TilePlan tp{};
    tp.group_m = group_m > 0 ? group_m : ((N + XBN - 1) / XBN >= kWideTilesN ? kGroupMWide : kGroupM);
    tp.tiles_m = (M + XBM - 1) / XBM;
    tp.tiles_n = (N + XBN - 1) / XBN;
    const int T = tp.tiles_m * tp.tiles_n, G = x_num_cus();
    tp.n_main = T;
    if ((unsigned long long)std::max(M, N) * (unsigned long long)K * eb >= (1ull << 32) ||
        (g.out32 && (unsigned long long)M * (unsigned long long)N * 4ull >= (1ull << 31))) {      // launch_gemm16x chunks M below this
        set_error("gemm16x: operand of %d x %d split elements (or %d x %d outputs) exceeds the 32-bit offset range", std::max(M, N), K, M, N);
        return PGMI_EINVAL;
    }
    const int rem = T % G;
    // Half-height tail (every output kind but the fused QKV): the last, partial round of tiles leaves G - rem CUs idle for a whole
    // tile time (N = 1280 at the BLAT shape: 6.29 rounds cost 7).  Its tiles are cut into their upper and lower 128 rows -- two
    // items on two CUs, each over the full K range in the same order, so every output element is computed exactly as in a
    // full tile (bit-identical: a row's bits must not depend on how many rows travel with it, tests/test_gpu_cli.py) -- when
    // all the halves still fit one round.
    if (g_opt.half_tail && !qkv && rem > 0 && 2 * rem <= G) {
        tp.n_main = T - rem; tp.half = 1; tp.n_tail = 2 * rem;
    }
    QkvOut qo{};
    if (qkv) qo = QkvOut{g.qkv.vt16, g.qkv.vt_plane, g.qkv.cos_t, g.qkv.sin_t, g.qkv.T, g.qkv.H, (g.qkv.T + 31) / 32 * 32, g.qkv.rotary, g.qkv.rot_halves};
    return launch_x(g, qkv ? X_OUT_QKV : g.out16 ? X_OUT_16 : X_OUT_F32, false, qkv ? g.qkv.qk_plane : 0, G, tp.n_main + tp.n_tail, tp, qo, XMap{});
}

// Batched / strided form (XMap, gemm16x_kernel.h): the MSA Transformer's tied row attention.  M, N, K are ONE batch's; nbatch batches
// share the launch (xm.tiles_per_batch is filled in here).  fp32 output (Cf; always through the LDS-transpose epilogue) or split
// planes (Ch; dense or scattered by xm.o_*).  M just above a multiple of 128: 128-row tiles throughout (TilePlan.half = 2).
int launch_gemm16_ex(const unsigned short* A, const unsigned short* W, float* Cf, unsigned short* Ch, int M, int N, int K,
                     float out_scale, XMap xm, int nbatch, hipStream_t s) {
    if (M <= 0 || N <= 0 || K <= 0 || (K % 64) != 0 || (N % 4) != 0 || (!Cf && !Ch) || (Cf && Ch) || nbatch < 1 ||
        (Ch && (N % 64) != 0) || (xm.a_run_bytes && (K / 32) % (1 << xm.k_run_log2) != 0)) {
        set_error("gemm16_ex: unsupported shape/args M=%d N=%d K=%d batches=%d", M, N, K, nbatch);
        return PGMI_EINVAL;
    }
    TilePlan tp{};
    tp.group_m = kGroupM;
    const int rows_last = M % XBM;                                // rows in the last 256-row panel
    const bool all_half = rows_last > 0 && rows_last <= XBM / 2;  // ... at most half of it: 128-row tiles waste less
    tp.tiles_m = all_half ? (M + XBM / 2 - 1) / (XBM / 2) : (M + XBM - 1) / XBM;
    tp.tiles_n = (N + XBN - 1) / XBN;
    const int per = tp.tiles_m * tp.tiles_n, T = per * nbatch, G = x_num_cus();
    xm.tiles_per_batch = per;
    if (xm.batch_inner < 1) xm.batch_inner = 1;
    if (all_half) { tp.half = 2; tp.n_main = 0; tp.n_tail = T; } else { tp.n_main = T; }
    GemmLaunch g;
    g.A = A; g.W = W; g.out_scale = out_scale;
    g.out32 = Cf; g.out16 = Ch;
    g.M = M; g.N = N; g.K = K;
    g.stream = s;
    return launch_x(g, Ch ? X_OUT_16 : X_OUT_F32, true, 0, G, T, tp, QkvOut{}, xm);
}

// The kernel addresses its operands with 32-bit byte offsets from a buffer descriptor (no 64-bit address arithmetic in the
// memory phases): one launch covers at most 2^32 bytes of A, i.e. rows * K * 4 < 4 GiB.  Larger activations (ESM2-15B FC2:
// K = 20480 allows 52 428 rows; an MSA Transformer alignment of 400 x 1024 tokens at K = 3072) are cut into row chunks --
// rows are independent and every row is computed exactly as in one launch (bit-identical), the chunks run back to back on the
// stream.  Fused QKV output: chunks are whole sequences (the V^T scatter is per (sequence, head)).
static int launch_gemm16x(const GemmLaunch& g) {
    const int M = g.M, N = g.N, K = g.K, group_m = gemm_group_m(g.variant);
    const bool qkv = g.qkv.vt16 != nullptr;
    const unsigned long long lim = (1ull << 32) - 1;
    const unsigned long long eb = g.bf ? 2ull : 4ull;
    if ((unsigned long long)N * (unsigned long long)K * eb > lim) {
        set_error("gemm16x: weight of %d x %d split elements exceeds the 32-bit offset range", N, K);
        return PGMI_EINVAL;
    }
    const long long test_rows = g_opt.max_rows;                          // tests: force chunking at small shapes
    long long max_rows = (long long)(lim / ((unsigned long long)K * eb));
    if (g.out32) max_rows = std::min(max_rows, (long long)(((1ull << 31) - 1) / ((unsigned long long)N * 4ull)));   // the fp32 epilogue's buffer offsets
    if (test_rows > 0) max_rows = std::min(max_rows, test_rows);
    if (M <= max_rows) return launch_gemm16x_one(g, group_m);
    long long per = qkv ? (max_rows / g.qkv.T) * g.qkv.T : (max_rows / XBM) * XBM;
    if (per <= 0) per = qkv ? 0 : max_rows;
    if (per <= 0) { set_error("gemm16x: one sequence of %d tokens x K = %d exceeds the 32-bit offset range", g.qkv.T, K); return PGMI_EINVAL; }
    // halfs per output row: the q | k rows of the fused QKV; SwiGLU: N / 2 output columns
    const size_t n_out16 = qkv ? (size_t)(2 * (N / 3)) : (size_t)(g.bf ? 1 : 2) * (g.epilogue == EPI_SWIGLU ? (size_t)N / 2 : (size_t)N);
    for (long long m0 = 0; m0 < M; m0 += per) {
        GemmLaunch c = g;
        c.M = (int)std::min<long long>(per, M - m0);
        c.A = g.A + (size_t)m0 * (size_t)K * (g.bf ? 1 : 2);                           // K-interleaved rows: 2 K halfs each (bf16: K)
        if (g.residual) c.residual = g.residual + (size_t)m0 * N;
        if (g.out32) c.out32 = g.out32 + (size_t)m0 * N;
        if (g.out16) c.out16 = g.out16 + (size_t)m0 * n_out16;
        if (qkv) c.qkv.vt16 = g.qkv.vt16 + (size_t)(m0 / g.qkv.T) * (size_t)g.qkv.H * kHeadDim * (size_t)((g.qkv.T + 31) / 32 * 32);   // rows m0.. are sequences m0 / T ..
        const int rc = launch_gemm16x_one(c, group_m);
        if (rc) return rc;
    }
    return PGMI_OK;
}

int launch_gemm16(const GemmLaunch& g) {
    const int M = g.M, N = g.N, K = g.K;
    // K: whole 32-deep K tiles for the f16x3 form (one 128-byte line per row and tile; an odd tile count is fine: ESM2-35M has
    // K = 480 = 15 tiles), 64 for the bf16 form's K tile
    const int k_step = g.bf ? 64 : 32;
    if (g.qkv.vt16) {                                      // the fused QKV projection: N = 3 D
        const int D = N / 3, T = g.qkv.T;
        if (M <= 0 || K <= 0 || D <= 0 || N != 3 * D || (K % k_step) || (D % 64) || T <= 0 || M % T || g.qkv.rot_halves < 1 || !g.out16 || g.out32 ||
            g.residual || g.epilogue != EPI_NONE) {
            set_error("gemm16_qkv: unsupported shape M=%d D=%d K=%d T=%d", M, D, K, T);
            return PGMI_EINVAL;
        }
        return launch_gemm16x(g);
    }
    if (M <= 0 || N <= 0 || K <= 0 || (K % k_step) != 0 || (N % 4) != 0 || (!g.out32 && !g.out16) || (g.out32 && g.out16)) {
        set_error("gemm16: unsupported shape/args M=%d N=%d K=%d (K %% %d == 0, N %% 4 == 0 required)", M, N, K, k_step);
        return PGMI_EINVAL;
    }
    if (g.epilogue == EPI_SWIGLU && (g.bf || !g.out16 || g.residual || (N % 64) != 0)) {
        set_error("gemm16: the SwiGLU epilogue is f16x3 with split-plane output, no residual and N %% 64 == 0 (N = %d)", N);
        return PGMI_EINVAL;
    }
    if (!g.bf && g.out16 && (N % 32) != 0) {
        set_error("gemm16: split output needs N %% 32 == 0 (K-interleaved operand of the next GEMM), got %d", N);
        return PGMI_EINVAL;
    }
    if (g.bf && g.out_scale != 1.0f) { set_error("gemm16: bf16 weights are not pre-scaled"); return PGMI_EINVAL; }
    return launch_gemm16x(g);
}

// ---- fp32 -> 16-bit operands (weights at load time; activations in the op-level tests and the MSA tied-attention path) ----
// mode 0: f16x3 weight: hi = fp16(x*scale), lo = fp16(x*scale - hi), K-interleaved rows of length K
// mode 1: bf16 (single plane, RNE)
// mode 2: f16x3 activation split (lo scaled by 2^11, see split_act), K-interleaved rows of length K
__global__ void split16_kernel(const float* __restrict__ x, int64_t n, float scale, int mode, int K,
                               unsigned short* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float v = x[i] * scale;
    if (mode == 1) {
        out[i] = f32_to_bf16_rne(v);
        return;
    }
    _Float16 hi, lo;
    if (mode == 2) {
        split_act(v, hi, lo);
    } else {
        hi = (_Float16)v;
        lo = (_Float16)(v - (float)hi);
    }
    const size_t o = ki_off((size_t)(i / K), (int)(i % K), K);
    out[o] = __builtin_bit_cast(unsigned short, hi);
    out[o + 32] = __builtin_bit_cast(unsigned short, lo);
}
void launch_split16(const float* x, int64_t n, float scale, int mode, int K, unsigned short* out, hipStream_t s) {
    hipLaunchKernelGGL(split16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, n, scale, mode, K, out);
}

}  // namespace pgmi
