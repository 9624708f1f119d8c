// The GVP-GNN handle behind pgmi_s2f (api_s2f.hip) and what api_s3f.hip runs of it: S3F's residue half is this handle unchanged, and
// its surface half is a second one (`fixed_degree` = 16) whose blob has no residue_embdding and no 20-way Linear, whose graph is the
// surface k-NN graph and whose input rows come from the surface MLP instead of s2f_embed.
#pragma once

#include "model.h"

namespace pgmi {

constexpr int S2F_ES = 64, S2F_RBF = 16, S2F_MAX_L = 8192, S2F_MAX_LAYERS = 8;   // S2F_S, S2F_V, S2F_H0 and S3F_DEG: common.h
constexpr int S2F_KP = 288;                            // 256 + 16 (or 32) norm columns, rounded up to the GEMM's K tile
constexpr int S2F_FS = 4 * S2F_S, S2F_FV = 2 * S2F_V;  // feed-forward hidden dims (1024, 32)
constexpr int S2F_FK = S2F_FS + S2F_FV;                // 1056, a multiple of 32
constexpr long long S2F_ROWS_LIMIT = 1 << 20;

// one GVP on the device: ws zero-padded along K to Kp columns ([s | norms | 0])
struct S2fGvp {
    float *wh = nullptr, *ws = nullptr, *bs = nullptr, *wv = nullptr, *wsv = nullptr, *bsv = nullptr;
    int si = 0, vi = 0, h = 0, so = 0, vo = 0, Kp = 0;
};
struct S2fLayer {
    // first message GVP, split by input block: Wji [512][256] = Wj rows then Wi rows; We [256][64] + b; Wnt [33][256]; whji [66][16];
    // whe [33]; and its vector half in m0 (ws unused there)
    float *Wji = nullptr, *We = nullptr, *b0 = nullptr, *Wnt = nullptr, *whji = nullptr, *whe = nullptr;
    S2fGvp m0, m1, m2, f0, f1;
    float *n0w, *n0b, *n1w, *n1b;
    DevBuf<float> Es;         // per structure: We e_s + b [E][256]
};
struct S2fSetHost { std::vector<int32_t> toks, ridx; };   // host scratch of s2f_fill_esm: a chunk's tokens and residue row indices

}  // namespace pgmi

struct pgmi_s2f {
    pgmi_model pm;                       // device, stream, allocation pool and profiling state (pgmi_s2f_profile_model)
    pgmi_model* esm = nullptr;           // borrowed; its stream is pm.stream when set
    bool own_stream = false;             // pm.stream was created for this handle
    int fixed_degree = 0;                // 0: the residue graph (CSR `off`).  16: a surface half, every node has exactly 16 edges
    pgmi_s2f_config cfg;
    int D = 0;
    float *Wre = nullptr, *vnw = nullptr, *vnb = nullptr, *Wv = nullptr, *bv = nullptr;
    std::vector<float> we_host;          // W_e's tensors in blob order: the structure pass runs it on the host
    std::vector<pgmi::S2fLayer> layers;
    float *onw = nullptr, *onb = nullptr;
    pgmi::S2fGvp wout;
    float *Wlin = nullptr, *blin = nullptr;
    // structure
    int L = 0, E = 0;
    std::vector<int32_t> h_src, h_dst, h_off;
    std::vector<float> h_es, h_ev;
    pgmi::DevBuf<int32_t> src, off;
    pgmi::DevBuf<float> es, ev, plddt;
    // workspace of a chunk
    pgmi::DevBuf<float> feat, h0, s, v, s1, v1, P, VT, pre, gate, A, vhA, vhB, mV, seq, lp;
    pgmi::DevBuf<int32_t> ridx, toks, cols;
};

namespace pgmi {

int s2f_check(const pgmi_s2f_config* c);
int64_t s2f_count(const pgmi_s2f_config* c, bool surface);     // surface: without residue_embdding and linear
// a handle on `device`; esm (nullable) lends its stream, else stream_of (nullable) does, else the handle creates one
int s2f_new(const pgmi_s2f_config* cfg, const float* w, int64_t n_weights, pgmi_model* esm, pgmi_s2f* stream_of, int device, int fixed_degree,
            pgmi_s2f** out);
int s2f_structure(pgmi_s2f* m, const float* pos, const float* plddt, int L);
int s2f_edge_tables(pgmi_s2f* m, size_t E);                     // every layer's Es [E][256] from m->es; both structure passes end in it
long long s2f_row_cap();                                        // pgmi_set_option("s2f_max_rows"), or the default
int s2f_workspace(pgmi_s2f* m, int per);
// bc masked copies, in three steps: m->feat [bc L][D] -> m->s (s2f_embed); the layers and W_out, m->s / m->v -> m->pre [bc L][256], the
// node state after the last layer left in m->s / m->v (s2f_layers); m->pre and m->seq -> m->lp (s2f_head; sums, grp, Ns: S3F's pooled
// row, else null, null, 0)
int s2f_embed(pgmi_s2f* m, int bc);
int s2f_layers(pgmi_s2f* m, int bc);
int s2f_head(pgmi_s2f* m, const float* pre, const float* seq, const float* sums, const int32_t* grp, int Ns, int64_t rows, float* lp);
// What S2F's and S3F's entries share around the GNN (api_s2f.hip, at the definitions): the fill of a gvp_forward chunk; the checks of
// set_logprobs' arguments, with the model's name in the messages; its buffers; the ESM2 fill of a chunk of masked copies; the scatter
// of a chunk's tables into `out` and `full`.
int s2f_fill_rows(pgmi_s2f* m, const float* node_feat, const float* seq_logits, int s0, int bc);
int s2f_check_sets(const pgmi_s2f* m, const char* name, const int32_t* wt_tokens, int T, const int32_t* aa_cols, const int32_t* set_off,
                   const int32_t* set_pos, int n_sets, const float* out);
int s2f_set_buffers(pgmi_s2f* m, int per, int T, const int32_t* aa_cols, S2fSetHost* h);
int s2f_fill_esm(pgmi_s2f* m, const int32_t* wt_tokens, int T, const int32_t* set_off, const int32_t* set_pos, int s0, int bc, S2fSetHost* h);
void s2f_scatter(const float* lp, int L, const int32_t* set_off, const int32_t* set_pos, int s0, int bc, float* out, float* full);

}  // namespace pgmi
