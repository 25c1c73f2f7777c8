// swx_model.h -- private to the host-side drivers of libswx.so (swx_runtime / swx_decoder / swx_decjob / swx_score / swx_testhooks):
// the model handle with its arena and workspace layouts, the decode-state layout, and the few host functions that cross those files
#pragma once
#include <map>
#include <memory>
#include <string>
#include <vector>
#include "swx_common.h"
#include "swx_kernels.h"
#include "swx_decode.h"

enum SlotKind { SK_MAT = 0, SK_VEC = 1, SK_CONV = 2 };

struct Slot {
    size_t off = 0;        // byte offset in the arena
    int kind = SK_VEC;
    int64_t rows = 0, cols = 0;   // source shape (MAT: [rows][cols]; CONV: out_c=rows, in_c=cols)
    int64_t dst_ld = 0;    // MAT: destination leading dimension; CONV: padded in-channels
    bool loaded = false;
};

struct LayerW {
    size_t ln1_g, ln1_b, wqkv, bqkv, wo, bo;
    size_t lnx_g, lnx_b, wcq, bcq, wckv, bckv, wco, bco;   // decoder only
    size_t ln2_g, ln2_b, w1, b1, w2, b2;
    // decoder, f16: LayerNorm-folded copies for the third-generation decode step (swx_decstep.hip): W.gamma, c1, c2
    size_t wqkv_f, qkv_c1, qkv_c2, wcq_f, cq_c1, cq_c2, w1_f, w1_c1, w1_c2;     // folded + packed in MFMA fragment order
    size_t wo_p, wco_p, w2_p;                                                   // packed copies of the other three
};

inline size_t align_up(size_t v, size_t a = 256) { return (v + a - 1) / a * a; }

constexpr int FIN_CAP = 32;
constexpr int MAX_GROUP = 16;
constexpr int MAX_SUPPRESS = 4096;
constexpr int SMALL_I32 = 8192;

// The bookkeeping of one decode job (the device side of DecodeBufs, swx_decode.h) as byte offsets from a base pointer: the one
// list both owners lay out -- the workspace (ws_layout, swx_runtime.hip) and the scripted-logits hook (script_layout, swx_decjob.hip).
struct DecodeStateOff {
    size_t tokens0, tokens1, anc0, anc1, pos0, begin, sum_lp, sum_lp_next, row_done, win_done, win_done_prev, n_done;
    size_t fin_tokens, fin_score, fin_len, fin_count, cand_lp, cand_tok;
};

// take(bytes) hands out the next region of the owner's buffer.  W_max windows, M_max rows, TS = n_ctx + 1.  n_begin = int32 entries
// behind `begin`: 3 * W_max in the workspace (ragged decode job: [W] initial lengths | [2W] prefill rows of the final LayerNorms),
// W in the script, which has no prefill.
template <typename Take>
void swx_decode_state_layout(Take take, size_t W_max, size_t M_max, size_t TS, size_t n_ctx, size_t n_begin, DecodeStateOff &o)
{
    o.tokens0 = take(M_max * TS * 4);
    o.tokens1 = take(M_max * TS * 4);
    o.anc0 = take(M_max * n_ctx * 4);
    o.anc1 = take(M_max * n_ctx * 4);
    o.pos0 = take(M_max * 4);
    o.begin = take(n_begin * 4);
    o.sum_lp = take(M_max * 4);
    o.sum_lp_next = take(M_max * 4);
    o.row_done = take(M_max * 4);
    o.win_done = take(W_max * 4);
    o.win_done_prev = take(W_max * 4);
    o.n_done = take(256);
    o.fin_tokens = take(W_max * FIN_CAP * TS * 4);
    o.fin_score = take(W_max * FIN_CAP * 4);
    o.fin_len = take(W_max * FIN_CAP * 4);
    o.fin_count = take(W_max * 4);
    o.cand_lp = take(M_max * (MAX_GROUP + 1) * 4);
    o.cand_tok = take(M_max * (MAX_GROUP + 1) * 4);
}

struct swx_model {
    swx_dims dims;
    int dtype;
    size_t esz;                     // bytes per compute element
    int Cp;                         // conv1 input channels padded to a multiple of 32
    std::map<std::string, Slot> slots;
    std::vector<LayerW> enc, dec;
    size_t o_conv1_w, o_conv1_b, o_conv2_w, o_conv2_b, o_enc_pos, o_lnpost_g, o_lnpost_b;
    size_t o_tok_emb, o_dec_pos, o_ln_g, o_ln_b;
    size_t o_hann, o_twiddle, o_filters, o_heads, o_zeros;
    size_t arena_bytes = 0;
    unsigned char *arena = nullptr;
    bool has_fold = false;          // the layout holds the folded copies (f16, d % 128 == 0)
    // ... and swx_weights_finalize has filled them.  The state belongs to the ARENA, not to the handle: views made by
    // swx_share_weights hold the same flag, so a tensor reloaded through the owner (flag cleared until the next finalize)
    // takes every view off the folded copies as well
    std::shared_ptr<bool> fold_state = std::make_shared<bool>(false);
    bool is_folded() const { return has_fold && *fold_state; }
    // alignment heads
    std::vector<std::vector<int>> heads_by_layer;   // per decoder layer
    std::vector<int> head_slot0;                    // first capture slot of each layer
    int n_align = 0;
    std::vector<int32_t> heads_flat;      // heads of all layers, layer-major (device copy: ws + L.heads)
    // workspace
    unsigned char *ws = nullptr;
    size_t ws_bytes = 0;
    int max_windows = 0, max_rows = 0, ws_n_align = 0;
    struct WsLayout {
        size_t melT, h1, x, h, qkv, att, u, gmax, small_i32, zeros_i32, ticket;
        DecodeStateOff dec;        // dec.begin: [W] initial lengths | [2W] prefill rows (swx_decode, ragged job)
        size_t logits, hid2;
        size_t kcache, vcache, sk, sv, cap, mean, sd, suppress, slabs, heads, win_uid;
        size_t total;
        int64_t rows_big, logits_rows;
        size_t slab_bytes;
    } L;

    template <typename P> P *A(size_t off) const { return (P *)(arena + off); }
    template <typename P> P *Wp(size_t off) const { return (P *)(ws + off); }

    // captured two-step decode graphs (swx_decode): keyed on everything a kernel argument of the step depends on
    struct StepGraph { std::vector<uint64_t> key; hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr; uint64_t used = 0; };
    std::vector<StepGraph> graphs;
    uint64_t graph_clock = 0;
    std::vector<int32_t> ragged_hv;       // host side of a ragged decode job's per-window arrays: lives on the handle so that the
                                          // upload needs no host wait (swx_decode returns only when its stream has drained)
    hipStream_t cap_stream = nullptr;   // capture happens here (the caller's stream may be the null stream, which cannot capture)
    bool graphs_off = false;            // set when capture / replay failed in three swx_decode calls of this handle: eager from then on
    int graph_failures = 0;
    int64_t n_captures = 0, n_replays = 0, n_eager_units = 0;      // swx_graph_stats
    void drop_graphs() {
        for (auto &g : graphs) { if (g.exec) (void)hipGraphExecDestroy(g.exec); if (g.graph) (void)hipGraphDestroy(g.graph); }
        graphs.clear();
    }
    ~swx_model() { drop_graphs(); if (cap_stream) (void)hipStreamDestroy(cap_stream); }
};

inline hipStream_t S(void *s) { return (hipStream_t)s; }

#define SWX_TRY(expr) do { int _r = (expr); if (_r < 0) return _r; } while (0)

inline int64_t xkv_plain_elems(const swx_dims &D)      // K [1500][d] | V^T [d][KP]
{
    return (int64_t)D.n_audio_ctx * D.n_text_state + (int64_t)D.n_text_state * SWX_VT_KP;
}
inline int64_t xkv_packed_elems(const swx_dims &D)     // f16 only: K and V^T again, in MFMA fragment order per head (swx_xattn.hip)
{
    return (int64_t)D.n_text_head * swx_xkv_packed_elems_per_head(D.n_audio_ctx);
}
inline int64_t xkv_chunk_elems(const swx_model *m)
{
    return xkv_plain_elems(m->dims) + (m->dtype == SWX_F16 ? xkv_packed_elems(m->dims) : 0);
}

struct FwdCfg {
    int W;                 // windows
    int rpw;               // logical rows per window in this pass
    int row_mul;           // logical row id = grid row * row_mul
    int n_new;             // new tokens per row
    const int32_t *tokens; int64_t ld_tok;
    int xkv_W;             // windows in the cross-K/V buffer `xkv` was cut from (its layer stride); 0 = W.  A pass over windows
                           // [w0, w0 + W) of a larger job points xkv at window w0's chunk of layer 0
    const int32_t *pos0;   // device, indexed by logical row id
    unsigned char *kcache, *vcache;
    size_t layer_stride;   // bytes between layers in the cache (0 = single-layer scratch)
    int cache_rows;        // rows per layer in the cache
    int k_chunked;         // f16: the K cache rows are [H][8][n_ctx][8] (KLayout, swx_kernels.h: the decode caches) instead of row-major
    int32_t *anc;
    const unsigned char *xkv;
    bool capture; int cap_row0, cap_rows, cap_ld_n;
    int step_pos;          // decode step: position of the new token when the host knows it (profiler's byte count), else 0
    int pos_bound;         // decode step: upper bound of every row's position (initial tokens + sample budget), 0 = unknown
    unsigned char *qcap;   // non-null: the cross-attention queries of every layer are copied here, [L][rows][d] (swx_score_q)
    bool xattn_by_blocks;  // strict f32: the cross-attention kernel must not depend on n_new (AttnArgs::f32_no_split)
};

// swx_decoder.hip
GemmArgs swx_gemm_args(const void *A, int64_t lda, const void *W, int64_t ldw, const float *bias, void *C, int64_t ldc,
                       int M, int N, int K, int epi);
int swx_gemm_residual(swx_model *m, const void *A, int64_t lda, size_t w_off, size_t b_off, void *X, int64_t ldx, int M, int N,
                      int K, hipStream_t s);
int swx_decoder_forward(swx_model *m, const FwdCfg &f, hipStream_t s);
int swx_logits_gemm(swx_model *m, const void *hid, int64_t ld, int rows, float *out, hipStream_t s);
int swx_final_ln(swx_model *m, const void *src, int rows, hipStream_t s);
