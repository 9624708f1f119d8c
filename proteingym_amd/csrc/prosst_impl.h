// The ProSST structure quantizer (include/pgmi.h, ProSST section): the handle behind pgmi_prosst (api_prosst.hip) and the
// launchers of prosst_gvp.hip.  One subgraph per residue, each through a six-layer GVP-GNN at node (256, 32) / edge (64, 2) without
// vector gates; fp32 throughout.  A "row" is a node copy: node q of the subgraph of anchor i.
#pragma once

#include "model.h"

namespace pgmi {

constexpr int PQ_S = 256, PQ_V = 32, PQ_ES = 64, PQ_EV = 2;     // node (s, v) and edge (s, v) widths
constexpr int PQ_H0 = 2 * PQ_V + PQ_EV;                         // 66 hidden vector channels of the first message GVP
constexpr int PQ_NS_IN = 20, PQ_NV_IN = 3, PQ_ES_IN = 32;       // input features: node (20, 3), edge (32, 1)
constexpr int PQ_KM = PQ_S + PQ_V;                              // 288 operand columns [s | norms] of the second / third message GVP and W_out
constexpr int PQ_FS = 4 * PQ_S, PQ_FV = 2 * PQ_V;               // feed-forward hidden (1024, 64)
constexpr int PQ_K0 = PQ_S + PQ_FV, PQ_K1 = PQ_FS + PQ_FV;      // 320 and 1088 operand columns of the feed-forward GVPs
constexpr int PQ_MSG = PQ_S + 3 * PQ_V;                         // 352 floats of a message [s | v]
constexpr int PQ_MAX_L = 8192, PQ_MAX_LAYERS = 8, PQ_MAX_K = 8192, PQ_DEPTH = 50;
constexpr long long PQ_ROWS_LIMIT = 1 << 20;
constexpr int PQ_OP_ROWS = 1 << 20;                             // pgmi_op_prosst_assign: rows per call, and
constexpr long long PQ_OP_PRODUCTS = 1LL << 28;                 // n K products per call (a 1 GiB table)

// device pointers of a layer's message GVPs after the gather: the first one's wv, then the second and the third (ws row stride 288)
struct ProsstMsgWeights {
    const float *wv0;
    const float *wh1, *ws1, *bs1, *wv1;
    const float *wh2, *ws2, *bs2, *wv2;
};
struct ProsstGvp {        // wh [h][vi], ws [so][si + h], bs [so], wv [vo][h] (null without vector outputs)
    float *wh = nullptr, *ws = nullptr, *bs = nullptr, *wv = nullptr;
};
struct ProsstLayer {
    // first message GVP, split by input block: Wji [512][256] = Wj rows then Wi rows; We [256][64] + b0; Wnt [66][256]; whji [132][32] =
    // the v_j then the v_i columns of wh; whe [66][2]
    float *Wji = nullptr, *We = nullptr, *b0 = nullptr, *Wnt = nullptr, *whji = nullptr, *whe = nullptr;
    ProsstGvp m0, m1, m2, f0, f1;
    float *n0w = nullptr, *n0b = nullptr, *n1w = nullptr, *n1b = nullptr;
    DevBuf<float> Es;     // per structure: We e_s + b0 [E][256]
};

// prosst_gvp.hip (operands and shapes at the kernels)
int launch_prosst_message(const float* P, const float* VT, const float* Es, const float* ev, const float* whe, const float* Wnt,
                          const ProsstMsgWeights& w, const int32_t* gid, const int32_t* src, const int32_t* dst, int32_t base, int64_t rows, float* msg,
                          hipStream_t s);
void launch_prosst_gather(const float* gs, const float* gv, const int32_t* nodes, int64_t rows, float* s, float* v, hipStream_t st);
void launch_prosst_aggregate(const float* msg, const int32_t* off, const int32_t* gid, int64_t rows, float* ds, float* dv, hipStream_t s);
void launch_prosst_node_ln(const float* rs, const float* rv, const float* ds, const float* dv, const float* lnw, const float* lnb, int lda,
                           int64_t rows, float* os, float* ov, float* outA, hipStream_t s);
int launch_prosst_vtab(const float* v, const float* wh, int h, int lda, int64_t rows, float* outV, float* outA, hipStream_t s);
int launch_prosst_gvp_mid(const float* spre, const float* vh, const float* wv, const float* nwh, int so, int vo, int h, int h2, int act,
                          int lda, int64_t rows, float* outA, float* outV, hipStream_t s);
void launch_prosst_pool(const float* pre, const int32_t* node_off, int n_sub, float* pooled, float* emb, hipStream_t s);
void launch_prosst_centre_norms(const float* c, int K, float* cn, hipStream_t s);
void launch_prosst_argmin(const float* G, const float* cn, int64_t rows, int K, int32_t* tok, hipStream_t s);

}  // namespace pgmi

struct pgmi_prosst {
    pgmi_model pm;                       // device, stream, allocation pool and profiling state (pgmi_prosst_profile_model)
    pgmi_prosst_config cfg;
    std::vector<float> wv_host, we_host; // W_v's and W_e's tensors in blob order: the structure pass runs them on the host
    std::vector<pgmi::ProsstLayer> layers;
    float *onw = nullptr, *onb = nullptr;
    pgmi::ProsstGvp wout;
    // structure: global edges (a -> b) in row-major order, the subgraphs' node CSR, and per node copy its incoming subgraph edges
    int L = 0, E = 0;
    int64_t N = 0, ES = 0;               // node copies and subgraph edges over all subgraphs
    std::vector<int32_t> h_a, h_b, h_goff, h_node_off, h_nodes, h_in_off, h_in_gid, h_in_src;
    std::vector<float> h_es, h_ev;       // W_e's output [E][64], [E][2][3]
    pgmi::DevBuf<int32_t> ea, eb, nodes, node_off, in_off, in_gid, in_src, in_dst;
    pgmi::DevBuf<float> gs, gv, es, ev, P0, VT0, msg0;      // gs / gv: W_v's output [L][256], [L][32][3]; msg0: layer 0's messages [E][352]
    bool have_msg0 = false, have_emb = false;
    // workspace of a chunk
    pgmi::DevBuf<float> s, v, s1, v1, P, VT, msg, ds, dv, A, A2, pre, vhA, vhB, pooled, emb, cent, cn, G;
    pgmi::DevBuf<int32_t> tok;
};
