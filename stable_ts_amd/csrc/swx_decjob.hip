// swx_decjob.hip -- one decode job on the host side: the binding of its device bookkeeping (DecodeBufs), the step graph, the loop
// of swx_decode, and swx_test_decode_script, which runs the same binding and the same exits on the caller's logits
#include <algorithm>
#include <cmath>
#include <cstring>
#include <cstdio>
#include "swx_model.h"

namespace {

// The captured two-step graph of a decode job, from the handle's cache or captured now.  `record` enqueues the two units on the
// stream it is given.  The key lists everything a kernel argument of the step depends on: the decode configuration, the
// buffers (workspace / arena / cross-K/V / timestamp mask), the switches, the K cache layout the job latched.  Buffer CONTENTS are read at run time.
template <typename F>
swx_model::StepGraph *step_graph(swx_model *m, const DecodeBufs &b, const void *d_xkv, int cur, int k_chunked, F record)
{
    const swx_decode_cfg &c = b.cfg;
    uint32_t tbits, pbits;
    memcpy(&tbits, &c.temperature, 4); memcpy(&pbits, &c.patience, 4);
    std::vector<uint64_t> key = {
        (uint64_t)c.n_windows, (uint64_t)c.n_group, (uint64_t)c.beam, tbits, pbits, (uint64_t)c.sample_len, (uint64_t)c.sample_begin,
        (uint64_t)c.sot_index, (uint64_t)c.suppress_blank, (uint64_t)c.apply_timestamp_rules, (uint64_t)(int64_t)c.max_initial_timestamp_index,
        (uint64_t)c.eot, (uint64_t)c.sot, (uint64_t)(int64_t)c.no_timestamps, (uint64_t)c.timestamp_begin, (uint64_t)(int64_t)c.no_speech,
        (uint64_t)(int64_t)c.blank_token, (uint64_t)c.n_suppress, (uint64_t)c.min_tokens, (uint64_t)c.seed,
        (uint64_t)(uintptr_t)b.ts_mask, (uint64_t)(uintptr_t)b.win_uid, (uint64_t)(uintptr_t)d_xkv, (uint64_t)(uintptr_t)m->arena,
        (uint64_t)(uintptr_t)m->ws, (uint64_t)m->ws_bytes, (uint64_t)swx_flags(), (uint64_t)cur, (uint64_t)m->is_folded(),
        (uint64_t)(uintptr_t)c.noise, (uint64_t)(uintptr_t)b.begin, (uint64_t)k_chunked};
    ++m->graph_clock;
    for (auto &g : m->graphs) if (g.key == key) { g.used = m->graph_clock; return &g; }
    if (!m->cap_stream && hipStreamCreateWithFlags(&m->cap_stream, hipStreamNonBlocking) != hipSuccess) { m->cap_stream = nullptr; return nullptr; }
    swx_model::StepGraph ng;
    if (hipStreamBeginCapture(m->cap_stream, hipStreamCaptureModeThreadLocal) != hipSuccess) return nullptr;
    const int rc = record(m->cap_stream);
    hipError_t er = hipStreamEndCapture(m->cap_stream, &ng.graph);
    if (rc < 0 || er != hipSuccess || !ng.graph) { if (ng.graph) (void)hipGraphDestroy(ng.graph); return nullptr; }
    if (hipGraphInstantiate(&ng.exec, ng.graph, nullptr, nullptr, 0) != hipSuccess) { (void)hipGraphDestroy(ng.graph); return nullptr; }
    ng.key = std::move(key); ng.used = m->graph_clock;
    ++m->n_captures;
    constexpr size_t MAX_GRAPHS = 8;
    if (m->graphs.size() >= MAX_GRAPHS) {       // least recently used entry makes room
        size_t lru = 0;
        for (size_t i = 1; i < m->graphs.size(); ++i) if (m->graphs[i].used < m->graphs[lru].used) lru = i;
        (void)hipGraphExecDestroy(m->graphs[lru].exec); (void)hipGraphDestroy(m->graphs[lru].graph);
        m->graphs[lru] = std::move(ng);
        return &m->graphs[lru];
    }
    m->graphs.push_back(std::move(ng));
    return &m->graphs.back();
}

// row idx[j] of src -> row j of dst, row_bytes (a multiple of 16) each; grid (n)
__global__ __launch_bounds__(64) void gather_prefill_rows_kernel(const unsigned char *__restrict__ src, const int32_t *__restrict__ idx,
                                                                 unsigned char *__restrict__ dst, int row_bytes)
{
    const int j = blockIdx.x;
    const uint4 *sp = (const uint4 *)(src + (size_t)idx[j] * row_bytes);
    uint4 *dp = (uint4 *)(dst + (size_t)j * row_bytes);
    for (int i = threadIdx.x; i < row_bytes / 16; i += 64) dp[i] = sp[i];
}

// The exit conditions of the decode loop, looked at after the selection of token i (swx_decode and swx_test_decode_script: one
// function so that the two loops cannot drift apart).  Returns 1 when the loop ends, 0 when it goes on, < 0 on a HIP error.
//  * tokens.shape[-1] > n_ctx (decode.py:60).  n_min = the shortest window's initial tokens: in a ragged job a longer window met
//    this earlier and was frozen on the device (decode_step_finish_kernel); the job ends when the shortest window meets it
//  * every window done: one host sync every DECODE_POLL steps, pointless while EOT is still suppressed by min_tokens
//  * the budget sample_len used up
constexpr int DECODE_POLL = 8;
int decode_loop_stop(int i, int n_min, int n_ctx, int min_tokens, int sample_len, int W, const int32_t *d_n_done, hipStream_t s)
{
    const int steps = i + 1;
    if (n_min + i + 1 > n_ctx) return 1;
    if ((steps % DECODE_POLL == 0 && steps >= min_tokens) || steps == sample_len) {
        int32_t h_done = 0;
        hipError_t er = hipMemcpyAsync(&h_done, d_n_done, 4, hipMemcpyDeviceToHost, s);
        if (er != hipSuccess) return -100 - (int)er;
        er = hipStreamSynchronize(s);
        if (er != hipSuccess) return -100 - (int)er;
        if (h_done >= W) return 1;
    }
    return steps >= sample_len ? 1 : 0;
}

// the beam search's candidate budget per window: round(n_group * patience), patience <= 0 = 1
int beam_max_cand(const swx_decode_cfg &cfg)
{
    const float pat = cfg.patience > 0.f ? cfg.patience : 1.0f;
    return (int)lrintf((float)cfg.n_group * pat);   // Python round(): half-to-even, as lrintf in the default mode
}

// every token id the filters write at must be a vocabulary id (upstream raises IndexError; here: size out of range)
bool token_ids_ok(const swx_decode_cfg &cfg, int V)
{
    for (int t : {cfg.eot, cfg.sot, cfg.timestamp_begin}) if (t < 0 || t >= V) return false;
    for (int t : {cfg.no_timestamps, cfg.no_speech, cfg.blank_token}) if (t < -1 || t >= V) return false;
    return true;
}

// The one binding of a decode job (swx_decode and swx_test_decode_script: one function, so that the job the scripted test
// exercises is the job the product runs).  Checks what holds for any job -- the group size (-1), then the suppress count, the six
// token ids and the beam's candidate budget (-2) -- and fills `b`: the configuration the kernels see (host pointers nulled, noise
// only where the sampling decoder draws, sample_begin = n_init, the longest window's initial tokens), the shape, and every pointer
// of the bookkeeping laid out by swx_decode_state_layout at `base`.  Left to the caller, whose sources differ: cfg.sot_index,
// begin, suppress, ts_mask, win_uid.  A check whose place among the CALLER's own checks decides the code an input with two faults
// returns is also made there, ahead of this call (see both call sites).
int bind_decode_job(const swx_decode_cfg &cfg, int V, int n_ctx, int n_init, unsigned char *base, const DecodeStateOff &o, float *logits,
                    DecodeBufs &b)
{
    const int W = cfg.n_windows, G = cfg.n_group;
    if (G <= 0 || G > MAX_GROUP) return -1;
    if (cfg.n_suppress > MAX_SUPPRESS || cfg.n_suppress < 0) return -2;
    if (!token_ids_ok(cfg, V)) return -2;
    b = DecodeBufs{};
    b.cfg = cfg;
    b.cfg.sample_begin = n_init;
    b.cfg.sample_begins = nullptr; b.cfg.sot_indices = nullptr;      // host pointers: the kernels read b.begin
    b.cfg.window_uid = nullptr;          // a host pointer: the kernels read the device copy (b.win_uid) only
    if (cfg.beam || cfg.temperature == 0.f) b.cfg.noise = nullptr;      // only the sampling decoder draws
    b.W = W; b.G = G; b.M = W * G; b.V = V; b.TS = n_ctx + 1; b.n_ctx = n_ctx; b.n_init = n_init;
    b.max_cand = cfg.beam ? beam_max_cand(cfg) : 0;
    if (cfg.beam && (b.max_cand <= 0 || b.max_cand > FIN_CAP)) return -2;
    b.fin_cap = FIN_CAP;
    auto P = [&](size_t off) { return (void *)(base + off); };
    b.tokens[0] = (int32_t *)P(o.tokens0); b.tokens[1] = (int32_t *)P(o.tokens1);
    const bool use_anc = G > 1;
    b.anc[0] = use_anc ? (int32_t *)P(o.anc0) : nullptr;
    b.anc[1] = use_anc ? (int32_t *)P(o.anc1) : nullptr;
    b.pos0 = (int32_t *)P(o.pos0);
    b.sum_lp = (float *)P(o.sum_lp); b.sum_lp_next = (float *)P(o.sum_lp_next);
    b.row_done = (int32_t *)P(o.row_done);
    b.win_done = (int32_t *)P(o.win_done); b.win_done_prev = (int32_t *)P(o.win_done_prev);
    b.n_done = (int32_t *)P(o.n_done);
    b.step_dev = b.n_done + 1;
    b.fin_tokens = (int32_t *)P(o.fin_tokens); b.fin_score = (float *)P(o.fin_score);
    b.fin_len = (int32_t *)P(o.fin_len); b.fin_count = (int32_t *)P(o.fin_count);
    b.cand_lp = (float *)P(o.cand_lp); b.cand_tok = (int32_t *)P(o.cand_tok);
    b.logits = logits;
    return 0;
}
}  // namespace

extern "C" {

// ----------------------------------------------------------------------------------------------------- decode
int swx_decode_gout(const swx_decode_cfg *cfg)
{
    if (!cfg) return 0;
    if (!cfg->beam) return cfg->n_group;
    const int mc = beam_max_cand(*cfg);
    return mc > cfg->n_group ? mc : cfg->n_group;
}

int swx_decode(swx_model *m, const swx_decode_cfg *cfg, const int32_t *d_init_tokens, const int32_t *d_suppress,
               const uint8_t *d_ts_mask, const void *d_xkv, int32_t *d_tokens_out, int32_t *d_lens_out,
               float *d_sumlp_out, float *d_nospeech, void *stream)
{
    if (!m || !m->arena || !m->ws) return -9;
    if (!cfg || !d_init_tokens || !d_xkv) return -1;
    const swx_dims &D = m->dims;
    const int W = cfg->n_windows, G = cfg->n_group, M = W * G;
    if (W <= 0 || G <= 0 || G > MAX_GROUP) return -1;
    if (W > m->max_windows || M > m->max_rows) return -8;
    if (cfg->n_suppress > MAX_SUPPRESS || cfg->n_suppress < 0) return -2;
    // Initial tokens per window (swx.h: sample_begins / sot_indices).  Arrays whose entries all agree ARE the job with one common
    // length: n_init / sot_index take the common value and every line below is the uniform job's.  Otherwise the job is ragged:
    // nb[w] / si[w] per window, n_init = the longest (row stride of d_init_tokens, bound of the positions), n_min = the shortest.
    int n_init = cfg->sample_begin, sot_index = cfg->sot_index;
    std::vector<int32_t> nb, si;
    if (cfg->sample_begins || cfg->sot_indices) {
        nb.resize(W); si.resize(W);
        for (int w = 0; w < W; ++w) {
            nb[w] = cfg->sample_begins ? cfg->sample_begins[w] : cfg->sample_begin;
            si[w] = cfg->sot_indices ? cfg->sot_indices[w] : cfg->sot_index;
            if (nb[w] <= 0 || nb[w] > D.n_text_ctx || si[w] < 0 || si[w] >= nb[w]) return -1;
        }
        n_init = *std::max_element(nb.begin(), nb.end());
        sot_index = si[0];
    }
    const int n_min = nb.empty() ? n_init : *std::min_element(nb.begin(), nb.end());
    const bool ragged = !nb.empty() && (n_min != n_init || *std::min_element(si.begin(), si.end()) != *std::max_element(si.begin(), si.end()));
    if (n_init <= 0 || n_init > D.n_text_ctx || sot_index < 0 || sot_index >= n_init) return -1;
    hipStream_t s = S(stream);
    const int d = D.n_text_state;
    const size_t e = m->esz;

    // The binding shared with swx_test_decode_script, on the workspace's copy of the layout.  This caller's own: the handle checks
    // above (-9 / -8); the group size and the suppress count looked at BEFORE the binding, because here the workspace bound (-8) and
    // the initial-token checks (-1) fall between them and the rest; sot_index; the suppress list copied into the workspace; the
    // window_uid upload; the ragged run table (m->ragged_hv), whose prefill rows ride behind `begin`.
    DecodeBufs b;
    SWX_TRY(bind_decode_job(*cfg, D.n_vocab, D.n_text_ctx, n_init, m->ws, m->L.dec, m->Wp<float>(m->L.logits), b));
    b.cfg.sot_index = sot_index;
    const bool use_anc = G > 1;
    b.ts_mask = d_ts_mask;
    int32_t *sup = m->Wp<int32_t>(m->L.suppress);
    if (cfg->n_suppress > 0) {
        hipError_t er = hipMemcpyAsync(sup, d_suppress, (size_t)cfg->n_suppress * 4, hipMemcpyDeviceToDevice, s);
        if (er != hipSuccess) return -100 - (int)er;
    }
    b.suppress = sup;
    b.win_uid = nullptr;
    if (cfg->window_uid) {
        int32_t *d_uid = m->Wp<int32_t>(m->L.win_uid);
        hipError_t eu = hipMemcpyAsync(d_uid, cfg->window_uid, (size_t)W * 4, hipMemcpyHostToDevice, s);
        if (eu == hipSuccess) eu = hipStreamSynchronize(s);        // the caller's array may be freed when this call returns
        if (eu != hipSuccess) return -100 - (int)eu;
        b.win_uid = d_uid;
    }
    // ragged job: the prefill is made over RUNS of neighbouring windows of one KIND, padded to the run's longest window.  The kind
    // is what the pass's kernel choice depends on, so that a window is computed by the kernels it gets alone: one initial token
    // (decoder_forward takes the single-token pass), 2-16 (the cross-attention's <= 16-query kernel, which splits the KEYS over
    // its waves: another summation order than the query-block kernel), more than 16.  Every other kernel of the pass computes a
    // row the same way whatever the launch (tests/test_gpu_batch_invariance.py).  One more choice does follow the PADDED length:
    // swx_self_attention takes self_attn_cached below 8 new tokens, self_attn_cached_mq_f16<4> for 8-31, <8> from 32 on -- a window
    // of 5 tokens next to one of 12 runs another self-attention kernel than alone.  Those three are bit-identical by construction
    // (one arithmetic order, swx_selfattn.hip) and that is RELIED upon here; tests/test_gpu_ragged_decode.py has neighbours on both
    // sides of 8 and of 32.  Rows past a window's own length are computed
    // and never read: causal attention keeps them out of the real rows, and their K/V slots are overwritten by the window's
    // first sampled tokens before a step attends to them.
    auto kind = [](int n) { return n == 1 ? 0 : n <= 16 ? 1 : 2; };
    struct Run { int w0, w1, n_new; };
    std::vector<Run> runs;
    int32_t *d_pre_rows = nullptr;
    if (ragged) {
        std::vector<int32_t> &hv = m->ragged_hv;         // [W] lengths | [2W] rows of a run's residual stream for the final LayerNorms
        hv.assign(3 * (size_t)W, 0);
        for (int w0 = 0; w0 < W; ) {
            int w1 = w0 + 1, n_new = nb[w0];
            while (w1 < W && kind(nb[w1]) == kind(nb[w0])) { n_new = std::max(n_new, (int)nb[w1]); ++w1; }
            runs.push_back({w0, w1, n_new});
            for (int w = w0; w < w1; ++w) {
                hv[w] = nb[w];
                hv[W + 2 * w] = (w - w0) * n_new + si[w];
                hv[W + 2 * w + 1] = (w - w0) * n_new + nb[w] - 1;
            }
            w0 = w1;
        }
        int32_t *d_begin = m->Wp<int32_t>(m->L.dec.begin);
        hipError_t eb = hipMemcpyAsync(d_begin, hv.data(), hv.size() * 4, hipMemcpyHostToDevice, s);
        if (eb != hipSuccess) return -100 - (int)eb;
        b.begin = d_begin;
        d_pre_rows = d_begin + W;
    }
    hipError_t er = hipMemsetAsync(b.win_done_prev, 0, (size_t)W * 4, s);
    if (er != hipSuccess) return -100 - (int)er;

    SWX_TRY(swx_decode_init(b, d_init_tokens, s));

    const size_t layer_stride = (size_t)m->max_rows * D.n_text_ctx * d * e;
    // K cache layout of this job (KLayout, swx_kernels.h), latched HERE: the prefill writes the cache, every step reads and extends it
    // and the captured step graph bakes the strides into its kernel arguments, so a switch flipped mid-job must not reach any of them
    const int k_chunked = m->dtype == SWX_F16 && (swx_flags() & SWX_FLAG_KCACHE_CHUNKED) ? 1 : 0;
    if (swx_flags() & SWX_FLAG_TICKET) {
        // the in-launch slab reduction relies on arrival counters that every launch leaves at zero; a launch that was aborted (fault,
        // reset) would leave them non-zero and every later job would silently pick the wrong last arriver: 16 KB, once per job
        hipError_t e_ = hipMemsetAsync(m->ws + m->L.ticket, 0, (size_t)SWX_DEC_TICKETS * 4, s);
        if (e_ != hipSuccess) return -100 - (int)e_;
    }
    // ---- prefill: one row per window (row w*G), n_init tokens
    FwdCfg f{};
    f.W = W; f.rpw = 1; f.row_mul = G; f.n_new = n_init;
    f.tokens = b.tokens[0]; f.ld_tok = (int64_t)G * b.TS;
    f.pos0 = m->Wp<int32_t>(m->L.zeros_i32);      // all zeros (any stride)
    f.kcache = m->ws + m->L.kcache; f.vcache = m->ws + m->L.vcache; f.layer_stride = layer_stride; f.cache_rows = m->max_rows;
    f.k_chunked = k_chunked;
    f.anc = nullptr; f.xkv = (const unsigned char *)d_xkv; f.capture = false;
    unsigned char *x = m->ws + m->L.x, *hid2 = m->ws + m->L.hid2;
    // the prefill logits live at the tail of the logits region so that replication to rows [0, M) never overlaps
    float *lg2 = b.logits + (size_t)(m->L.logits_rows - 2 * W) * D.n_vocab;
    if (!ragged) {
        SWX_TRY(swx_decoder_forward(m, f, s));
        // final LN of the rows at sot_index and at the last initial position of every window -> [W][2][d]
        SWX_TRY(swx_layernorm(m->dtype, x + (size_t)sot_index * d * e, (int64_t)n_init * d, m->A<float>(m->o_ln_g),
                              m->A<float>(m->o_ln_b), hid2, 2 * d, W, d, s));
        SWX_TRY(swx_layernorm(m->dtype, x + (size_t)(n_init - 1) * d * e, (int64_t)n_init * d, m->A<float>(m->o_ln_g),
                              m->A<float>(m->o_ln_b), hid2 + (size_t)d * e, 2 * d, W, d, s));
    } else {
        // every run overwrites the residual stream: its two rows per window are parked (raw copies) where the prefill logits
        // will land, and the final LN runs once over all 2W of them
        unsigned char *park = (unsigned char *)(((uintptr_t)lg2 + 255) & ~(uintptr_t)255);      // (2W d-wide rows in 2W n_vocab-wide ones)
        const size_t win_xkv = (size_t)xkv_chunk_elems(m) * e, win_cache = (size_t)G * D.n_text_ctx * d * e;
        for (const Run &r : runs) {
            FwdCfg fr = f;
            fr.W = r.w1 - r.w0; fr.n_new = r.n_new; fr.xkv_W = W;
            fr.tokens = f.tokens + (size_t)r.w0 * f.ld_tok;
            fr.kcache = f.kcache + r.w0 * win_cache; fr.vcache = f.vcache + r.w0 * win_cache;
            fr.xkv = f.xkv + r.w0 * win_xkv;
            SWX_TRY(swx_decoder_forward(m, fr, s));
            hipLaunchKernelGGL(gather_prefill_rows_kernel, dim3(2 * fr.W), dim3(64), 0, s, x, d_pre_rows + 2 * r.w0,
                               park + (size_t)2 * r.w0 * d * e, (int)(d * e));
            SWX_CHECK_LAUNCH();
        }
        SWX_TRY(swx_layernorm(m->dtype, park, d, m->A<float>(m->o_ln_g), m->A<float>(m->o_ln_b), hid2, d, 2 * W, d, s));
    }
    SWX_TRY(swx_logits_gemm(m, hid2, d, 2 * W, lg2, s));
    SWX_TRY(swx_decode_after_prefill(b, lg2, d_nospeech, s));

    int cur = 0, steps = 0;
    // One unit of the loop = [forward pass of the rows' newest tokens -> final LayerNorm -> logits] + [selection of token i].
    // Token 0 is selected from the prefill logits; after every selection the loop's exit conditions are looked at:
    // context full (decode.py:60), every window done (one host sync every DECODE_POLL steps), budget used up: decode_loop_stop.
    auto unit = [&](int cur_in, hipStream_t st, bool capturing = false) -> int {
        FwdCfg g{};
        g.W = W; g.rpw = G; g.row_mul = 1; g.n_new = 1;
        g.tokens = b.tokens[cur_in]; g.ld_tok = b.TS; g.pos0 = b.pos0;
        g.kcache = f.kcache; g.vcache = f.vcache; g.layer_stride = layer_stride; g.cache_rows = m->max_rows;
        g.k_chunked = k_chunked;
        g.anc = use_anc ? b.anc[cur_in] : nullptr; g.xkv = (const unsigned char *)d_xkv; g.capture = false;
        // profiler's byte count only (steps = tokens sampled so far).  Never a captured kernel argument: a replayed graph would
        // carry the position of the step it was captured at (the profiler is off under replay, and 0 = "unknown" there)
        g.step_pos = capturing ? 0 : n_init + steps;
        // a property of the job, not of the step: safe to bake into the graph.  Ragged job: the LONGEST window's bound, so a short
        // window that alone takes self_attn_step_f16<false> (bound <= 128) takes the <true> / deep variant here: the step kernel of
        // a row then depends on the job.  The variants differ only in code for positions >= 128 that such a row never reaches and
        // are bit-identical below (swx_selfattn.hip); that identity is RELIED upon (tests/test_gpu_ragged_decode.py: 1 next to 228)
        g.pos_bound = n_init + cfg->sample_len;
        const int fr = swx_decoder_forward(m, g, st);
        if (fr < 0) return fr;
        unsigned char *hh = m->ws + m->L.h;
        if (fr == 0)   // the step leaves the raw residual stream in x
            SWX_TRY(swx_final_ln(m, x, M, st));
        SWX_TRY(swx_logits_gemm(m, hh, d, M, b.logits, st));
        return swx_decode_select(b, cur_in, st);
    };
    // returns 1 when the loop ends after the selection of token i
    auto after_select = [&](int i) -> int {
        steps = i + 1;
        return decode_loop_stop(i, n_min, D.n_text_ctx, cfg->min_tokens, cfg->sample_len, W, b.n_done, s);
    };
    SWX_TRY(swx_decode_select(b, cur, s));
    if (cfg->beam) cur ^= 1;
    int stop = after_select(0);
    if (stop < 0) return stop;
    // Units 2k, 2k+1 (k >= 1) are replayed from ONE captured graph: a step is ~290 kernel launches, which the host cannot issue
    // as fast as the device retires them below ~50 rows (sequential transcribe(): 5 rows).  Everything that differs between two
    // steps is device state (token buffers, positions, ancestor tables, the step counter); the token-buffer parity returns
    // to its start after two steps.  The poll above only falls after odd units, the context check is made for both units up front.
    const bool graph_ok = !swx_prof_on() && !(swx_flags() & SWX_FLAG_NO_GRAPH) && !m->graphs_off;
    swx_model::StepGraph *sg = nullptr;
    bool graph_failed_now = false;
    for (int i = 1; !stop; ) {
        const bool pair = graph_ok && !m->graphs_off && !graph_failed_now && i >= 2 && (i & 1) == 0 && i + 1 < cfg->sample_len && n_min + i + 1 <= D.n_text_ctx;
        if (pair) {
            if (!sg) sg = step_graph(m, b, d_xkv, cur, k_chunked, [&](hipStream_t cs) -> int {
                SWX_TRY(unit(cur, cs, true));
                return unit(cfg->beam ? cur ^ 1 : cur, cs, true);
            });
            if (sg && hipGraphLaunch(sg->exec, s) == hipSuccess) {
                ++m->n_replays;
                stop = after_select(i + 1);
                if (stop < 0) return stop;
                i += 2;
                continue;
            }
            (void)hipGetLastError();
            // capture or replay failed: this call goes on eagerly; the next swx_decode tries again, and only the third failure
            // switches replay off for the handle (swx_graph_stats reports it)
            graph_failed_now = true;
            if (++m->graph_failures >= 3) m->graphs_off = true;
            if (m->graph_failures == 1)
                fprintf(stderr, "libswx: decode-step graph capture / replay failed; launching the steps eagerly (results are identical)\n");
        }
        SWX_TRY(unit(cur, s));
        ++m->n_eager_units;
        if (cfg->beam) cur ^= 1;
        stop = after_select(i);
        if (stop < 0) return stop;
        ++i;
    }
    const int G_out = swx_decode_gout(cfg);
    SWX_TRY(swx_decode_finalize(b, cur, steps, d_tokens_out, d_lens_out, d_sumlp_out, G_out, s));
    er = hipStreamSynchronize(s);
    if (er != hipSuccess) return -100 - (int)er;
    return steps;
}

}  // extern "C"

// ---- swx_test_decode_script: the selection path of swx_decode on the caller's logits (no model, no forward pass)
namespace {
struct ScriptLayout { DecodeStateOff dec; size_t logits, win_uid, total; };
ScriptLayout script_layout(int W, int G, int V, int n_ctx)
{
    const size_t M = (size_t)W * G;
    ScriptLayout L{};
    size_t cur = 0;
    auto take = [&](size_t bytes) { size_t o = cur; cur = align_up(cur + bytes); return o; };
    swx_decode_state_layout(take, W, M, (size_t)n_ctx + 1, n_ctx, W, L.dec);
    L.logits = take(M * (size_t)V * 4);
    L.win_uid = take((size_t)W * 4);
    L.total = cur;
    return L;
}
bool script_shape_ok(const swx_decode_cfg *cfg, int V, int n_ctx)
{
    return cfg && cfg->n_windows > 0 && cfg->n_group > 0 && cfg->n_group <= MAX_GROUP && V > 0 && n_ctx > 0 && cfg->sample_len > 0;
}
}  // namespace

extern "C" {

size_t swx_test_decode_script_ws_bytes(const swx_decode_cfg *cfg, int n_vocab, int n_ctx)
{
    if (!script_shape_ok(cfg, n_vocab, n_ctx)) return 0;
    return script_layout(cfg->n_windows, cfg->n_group, n_vocab, n_ctx).total;
}

int swx_test_decode_script(const swx_decode_cfg *cfg, int n_vocab, int n_ctx, const int32_t *d_init_tokens, const int32_t *d_suppress,
                           const uint8_t *d_ts_mask, const float *d_prefill_logits, const float *d_script, int n_script,
                           int32_t *d_tokens_out, int32_t *d_lens_out, float *d_sumlp_out, float *d_nospeech, int32_t *d_anc_out,
                           int32_t *d_pos0_out, void *d_ws, size_t ws_bytes, void *stream)
{
    if (!script_shape_ok(cfg, n_vocab, n_ctx)) return -1;
    if (!d_init_tokens || !d_prefill_logits || !d_tokens_out || !d_lens_out || !d_sumlp_out || !d_ws) return -1;
    if (n_script < 0 || (n_script > 0 && !d_script)) return -1;
    const int W = cfg->n_windows, G = cfg->n_group, M = W * G, V = n_vocab;
    if (cfg->n_suppress < 0 || cfg->n_suppress > MAX_SUPPRESS || (cfg->n_suppress > 0 && !d_suppress)) return -2;
    if (!token_ids_ok(*cfg, V)) return -2;
    const ScriptLayout L = script_layout(W, G, V, n_ctx);
    if (ws_bytes < L.total || ((uintptr_t)d_ws & 255)) return -8;
    // initial tokens per window, as swx_decode reads them (sot_index plays no part: the prefill logits are the caller's)
    int n_init = cfg->sample_begin, n_min = cfg->sample_begin;
    if (cfg->sample_begins) {
        n_init = *std::max_element(cfg->sample_begins, cfg->sample_begins + W);
        n_min = *std::min_element(cfg->sample_begins, cfg->sample_begins + W);
    }
    if (n_min <= 0 || n_init > n_ctx) return -1;
    const bool ragged = n_min != n_init;
    hipStream_t s = S(stream);
    unsigned char *ws = (unsigned char *)d_ws;

    // The binding shared with swx_decode, on this hook's own layout of the caller's buffer.  This caller's own: the null-pointer
    // checks and the buffer's size / alignment (-8) above; the suppress count and the token ids looked at BEFORE the binding, because
    // here they come ahead of the buffer check (-8) and the initial-token check (-1); the suppress list is the caller's pointer, not
    // a copy; window_uid is uploaded into the layout's own W-int slot, as swx_decode uploads it into the workspace's; `begin` holds the
    // W lengths alone and is uploaded synchronously.
    DecodeBufs b;
    const int brc = bind_decode_job(*cfg, V, n_ctx, n_init, ws, L.dec, (float *)(ws + L.logits), b);
    if (brc < 0) return brc;
    const bool use_anc = G > 1;
    b.suppress = d_suppress; b.ts_mask = d_ts_mask; b.win_uid = nullptr;
    hipError_t er;
    if (ragged) {
        int32_t *d_begin = (int32_t *)(ws + L.dec.begin);
        er = hipMemcpyAsync(d_begin, cfg->sample_begins, (size_t)W * 4, hipMemcpyHostToDevice, s);
        if (er == hipSuccess) er = hipStreamSynchronize(s);          // the caller's array may be freed when this call returns
        if (er != hipSuccess) return -100 - (int)er;
        b.begin = d_begin;
    }
    if (cfg->window_uid) {
        int32_t *d_uid = (int32_t *)(ws + L.win_uid);
        er = hipMemcpyAsync(d_uid, cfg->window_uid, (size_t)W * 4, hipMemcpyHostToDevice, s);
        if (er == hipSuccess) er = hipStreamSynchronize(s);          // the caller's array may be freed when this call returns
        if (er != hipSuccess) return -100 - (int)er;
        b.win_uid = d_uid;
    }
    er = hipMemsetAsync(b.win_done_prev, 0, (size_t)W * 4, s);
    if (er != hipSuccess) return -100 - (int)er;

    // from here on work is queued on the caller's buffers: an error return waits for it too ("blocks until the loop has finished")
    auto fail = [&](int code) { (void)hipStreamSynchronize(s); return code; };
    int rc = swx_decode_init(b, d_init_tokens, s);
    if (rc >= 0) rc = swx_decode_after_prefill(b, d_prefill_logits, d_nospeech, s);
    if (rc < 0) return fail(rc);
    // token 0 is selected from the prefill logits, token i >= 1 from slice i - 1 of the script: eager launches, one step at a time
    int cur = 0, steps = 0;
    for (int i = 0; ; ++i) {
        if (i > 0) {
            if (i - 1 >= n_script) return fail(-2);                // the script is shorter than the loop
            er = hipMemcpyAsync(b.logits, d_script + (size_t)(i - 1) * M * V, (size_t)M * V * 4, hipMemcpyDeviceToDevice, s);
            if (er != hipSuccess) return fail(-100 - (int)er);
        }
        rc = swx_decode_select(b, cur, s);
        if (rc < 0) return fail(rc);
        if (cfg->beam) cur ^= 1;
        steps = i + 1;
        const int stop = decode_loop_stop(i, n_min, n_ctx, cfg->min_tokens, cfg->sample_len, W, b.n_done, s);
        if (stop < 0) return fail(stop);
        if (stop) break;
    }
    rc = swx_decode_finalize(b, cur, steps, d_tokens_out, d_lens_out, d_sumlp_out, swx_decode_gout(cfg), s);
    if (rc < 0) return fail(rc);
    if (use_anc && d_anc_out) {
        er = hipMemcpyAsync(d_anc_out, b.anc[cur], (size_t)M * n_ctx * 4, hipMemcpyDeviceToDevice, s);
        if (er != hipSuccess) return fail(-100 - (int)er);
    }
    if (d_pos0_out) {
        er = hipMemcpyAsync(d_pos0_out, b.pos0, (size_t)M * 4, hipMemcpyDeviceToDevice, s);
        if (er != hipSuccess) return fail(-100 - (int)er);
    }
    er = hipStreamSynchronize(s);
    if (er != hipSuccess) return -100 - (int)er;
    return steps;
}

}  // extern "C"
