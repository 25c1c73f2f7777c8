// swx_decoder.hip -- the decoder forward pass on the host side: the fused "dec" layer loop, the generic per-op layer loop, the
// vocabulary projection and the final LayerNorm (callers: swx_decjob.hip, swx_score.hip)
#include "swx_model.h"

GemmArgs swx_gemm_args(const void *A, int64_t lda, const void *W, int64_t ldw, const float *bias, void *C, int64_t ldc,
                       int M, int N, int K, int epi)
{
    GemmArgs g{};
    g.A = A; g.lda = lda; g.W = W; g.ldw = ldw; g.bias = bias; g.C = C; g.ldc = ldc; g.M = M; g.N = N; g.K = K; g.epi = epi;
    g.R = nullptr; g.ldr = 0; g.Rf = nullptr; g.res_mod = 1;
    return g;
}

// x += Linear(a) ; used for the attention / MLP output projections
int swx_gemm_residual(swx_model *m, const void *A, int64_t lda, size_t w_off, size_t b_off, void *X, int64_t ldx, int M, int N,
                      int K, hipStream_t s)
{
    GemmArgs g = swx_gemm_args(A, lda, m->arena + w_off, K, m->A<float>(b_off), X, ldx, M, N, K, EPI_BIAS | EPI_RES);
    g.R = X; g.ldr = ldx;
    return swx_gemm(m->dtype, g, 0, s);
}

// ------------------------------------------------------------------------------------------------ decoder forward
// The fused "dec" decoder layers in fp16, for both arms of decoder_forward: un-split "dec" GEMMs (swx_decstep.hip) that finish
// their own outputs (bias / GELU / residual / K,V scatter, LayerNorm folded; no LayerNorm launch, no f32 slabs except for the
// K = 4d projection).  8 launches per layer: QKV+scatter, self-attention, out-proj+residual, cross-q, cross-attention,
// out-proj+residual, MLP-in+GELU, MLP-out [+ its slab reduction].  (The split-K generation of rounds 1-2 -- 12 launches per
// layer -- was deleted in round 3; the generic per-op path below is the bit-identity-free reference: SWX_FLAG_NO_FAST_STEP.)
//   step (n_new == 1, one token per row): the latency-optimised self-attention kernel over the cache, and the cross-q projection
//     inside the cross-attention launch (7 launches) unless switched off.
//   multi-token (teacher-forced pass over a SMALL number of rows: align(), one window of ~110 tokens; refine / locate probes; the
//     prefill of a decode, W windows x the initial tokens, cache rows w * G): at <= 160 rows the tiled MFMA GEMM launches one or two
//     row blocks and the 16-column skinny kernel 27 us per projection, while a dec launch finishes its outputs in ~7 us; from 161
//     rows on the launcher takes the tall dec GEMM (DecGemmArgs::tall).  Self-attention (causal over the new tokens),
//     cross-attention and the alignment-head capture are the general kernels.
// Leaves the RAW residual stream in `x` (returns 0: the caller applies the final LayerNorm).
static int decoder_dec(swx_model *m, const FwdCfg &f, hipStream_t s)
{
    const swx_dims &D = m->dims;
    const int d = D.n_text_state, H = D.n_text_head;
    const size_t e = m->esz;
    const bool step = f.n_new == 1;           // decoder_forward's step arm (row_mul 1, no capture, <= 16 rows per window)
    const int R = f.W * f.rpw, rows = R * f.n_new, nq = f.rpw * f.n_new;
    f16 *x = m->Wp<f16>(m->L.x), *q = m->Wp<f16>(m->L.qkv), *att = m->Wp<f16>(m->L.att), *u = m->Wp<f16>(m->L.u);
    SWX_TRY(swx_embed(m->dtype, f.tokens, f.ld_tok, nullptr, f.pos0, R, f.n_new, m->arena + m->o_tok_emb,
                      m->A<float>(m->o_dec_pos), d, x, s));
    const int64_t chunk = xkv_chunk_elems(m);
    // Prefetch chain (DecPrefetch, swx_kernels.h): each projection touches the weights of the NEXT projection.  What the
    // counters say it warms is the 256 MB Infinity Cache, not an L2 (profiles/r03_pmc_final.csv: the consumer's FETCH_SIZE does
    // not drop -- the L2s drop their clean lines at a kernel boundary -- but it is 0.8-1.2 us faster, r03_eager_pf_*_kernels.csv),
    // so a prefetch also survives the attention kernel in between (<= 57 MB / 154 MB through a 256 MB cache).  A prefetch issued
    // BY the self-attention kernel was tried and dropped: +0.36 us on it.
    // (from 32 rows on: with one 16-row tile per panel -- sequential transcribe(), 5 rows -- a launch has 20-80 workgroups, too
    // few lanes to cover a projection, and waits for its own prefetch at its end: measured 58.0 -> 56.7x there, 460.8 -> 450.4 ms
    // per pass at 100 rows, profiles/r03_dec_prefetch_ab.txt)
    const int flags = swx_flags();
    const bool pf_on = !(flags & SWX_FLAG_NO_PREFETCH) && rows >= 32;
    auto pf_of = [&](size_t w_off, int N, int K, int epi) {
        return pf_on ? swx_dec_prefetch_of(m->A<f16>(w_off), rows, N, K, epi) : DecPrefetch{};
    };
    // one projection over all rows: out = epi(A W^T) with W packed [N][K]; DEC_RES accumulates into `out` (X), else `out` is C
    auto proj = [&](const f16 *A, int64_t lda, size_t w_off, int N, int K, int epi, size_t c1_off, size_t c2_off, f16 *out, DecPrefetch pf) {
        DecGemmArgs g{};
        g.M = rows; g.tall = step ? 0 : 1; g.A = A; g.lda = lda; g.W = m->A<f16>(w_off); g.ldw = K; g.N = N; g.K = K; g.epi = epi;
        if (epi & DEC_LN) g.c1 = m->A<float>(c1_off);
        g.c2 = m->A<float>(c2_off);
        if (epi & DEC_RES) { g.X = out; g.ldx = N; } else { g.C = out; g.ldc = (epi & DEC_QKV) ? N / 3 : N; }
        g.pf = pf;
        return g;
    };
    for (int l = 0; l < D.n_text_layer; ++l) {
        const LayerW &w = m->dec[l];
        f16 *kc = (f16 *)(f.kcache + (size_t)l * f.layer_stride), *vc = (f16 *)(f.vcache + (size_t)l * f.layer_stride);
        // q | k | v = LN1(x) Wqkv^T + b : q -> the q buffer, k / v -> the cache at each row's position
        DecGemmArgs g = proj(x, d, w.wqkv_f, 3 * d, d, DEC_LN | DEC_QKV, w.qkv_c1, w.qkv_c2, q,
                             pf_of(w.wo_p, d, d, DEC_RES));          // used after the self-attention (<= 57 MB through the cache)
        g.kcache = kc; g.vcache = vc; g.pos0 = f.pos0; g.n_ctx = D.n_text_ctx; g.d = d; g.rps = f.n_new; g.row_mul = f.row_mul;
        g.kl = swx_klayout(f.k_chunked, D.n_text_ctx, d);
        SWX_TRY(swx_gemm_dec(g, s));
        SelfAttnArgs sa{};
        sa.qkv = q; sa.ldqkv = d; sa.kcache = kc; sa.vcache = vc; sa.anc = f.anc; sa.pos0 = f.pos0; sa.o = att; sa.ldo = d;
        sa.R = R; sa.n_new = f.n_new; sa.H = H; sa.n_ctx = D.n_text_ctx; sa.d = d; sa.skip_append = 1; sa.kl = g.kl;
        if (step) { sa.step_cached = 1; sa.step_pos = f.step_pos; sa.pos_bound = f.pos_bound; }
        else sa.pos0_all_zero = f.pos0 == m->Wp<int32_t>(m->L.zeros_i32) ? 1 : 0;
        SWX_TRY(swx_self_attention(m->dtype, sa, f.row_mul, s));
        // x += att Wo^T + bo
        SWX_TRY(swx_gemm_dec(proj(att, d, w.wo_p, d, d, DEC_RES, 0, w.bo, x, pf_of(w.wcq_f, d, d, DEC_LN)), s));
        // cross-attention query = LNx(x) Wcq^T + b: on the step arm inside the cross-attention launch (AttnArgs::fq_*) unless switched off
        const bool fuse_xq = step && !(flags & (SWX_FLAG_NO_FUSED_XQ | SWX_FLAG_NO_PACKED_XKV)) && f.rpw <= 16 && d % 128 == 0 &&
                             (d == 384 || d == 512 || d == 640 || d == 768 || d == 1024 || d == 1280);
        if (!fuse_xq)
            SWX_TRY(swx_gemm_dec(proj(x, d, w.wcq_f, d, d, DEC_LN, w.cq_c1, w.cq_c2, q,
                                      pf_of(w.wco_p, d, d, DEC_RES)), s));    // used after the cross-attention (154 MB through the cache)
        if (f.qcap && !step) {
            hipError_t qe = hipMemcpyAsync(f.qcap + (size_t)l * rows * d * e, q, (size_t)rows * d * e, hipMemcpyDeviceToDevice, s);
            if (qe != hipSuccess) return -100 - (int)qe;
        }
        const unsigned char *kl = f.xkv + (size_t)l * (f.xkv_W ? f.xkv_W : f.W) * chunk * e;
        AttnArgs ca{};
        ca.q = q; ca.ldq = d; ca.k = kl; ca.v = kl + (size_t)D.n_audio_ctx * d * e; ca.ldkv = d;
        ca.k_bs = chunk; ca.v_bs = chunk; ca.vt_kp = SWX_VT_KP; ca.o = att; ca.ldo = d;
        ca.B = f.W; ca.H = H; ca.nq = nq; ca.nk = D.n_audio_ctx; ca.q_rows_per_batch = nq;
        ca.kv_packed = kl + (size_t)xkv_plain_elems(D) * e;          // fragment-ordered copy of this layer's K / V^T (also lets a
                                                                     // small multi-token pass run as 16-row groups on the decode kernel)
        if (fuse_xq) {
            ca.fq_x = x; ca.fq_ldx = d; ca.fq_rows = rows; ca.fq_w = m->A<f16>(w.wcq_f); ca.fq_c1 = m->A<float>(w.cq_c1);
            ca.fq_c2 = m->A<float>(w.cq_c2); ca.fq_k = d;
            if (pf_on) { ca.fq_pf = m->A<f16>(w.wco_p); ca.fq_pf_lines = (int)(((int64_t)d * d * 2) >> 7); }
        }
        SWX_TRY(swx_attention(m->dtype, ca, 0, s));
        if (f.capture && !m->heads_by_layer[l].empty()) {           // never on the step arm: decoder_forward sends a capture elsewhere
            SWX_TRY(swx_qk_capture(m->dtype, q, d, nq, f.cap_row0, f.cap_rows, kl, d, chunk, D.n_audio_ctx,
                                   m->Wp<int32_t>(m->L.heads) + m->head_slot0[l], (int)m->heads_by_layer[l].size(),
                                   m->head_slot0[l], m->n_align, f.W, m->Wp<float>(m->L.cap), f.cap_ld_n, D.n_audio_ctx, s));
        }
        SWX_TRY(swx_gemm_dec(proj(att, d, w.wco_p, d, d, DEC_RES, 0, w.bco, x, pf_of(w.w1_f, 4 * d, d, DEC_LN | DEC_GELU)), s));
        // MLP
        SWX_TRY(swx_gemm_dec(proj(x, d, w.w1_f, 4 * d, d, DEC_LN | DEC_GELU, w.w1_c1, w.w1_c2, u,
                                  pf_of(w.w2_p, d, 4 * d, DEC_RES | DEC_SLAB)), s));
        g = proj(u, 4 * d, w.w2_p, d, 4 * d, DEC_RES | DEC_SLAB, 0, w.b2, x,
                 l + 1 < D.n_text_layer ? pf_of(m->dec[l + 1].wqkv_f, 3 * d, d, DEC_LN | DEC_QKV) : DecPrefetch{});
        g.slabs = m->Wp<float>(m->L.slabs); g.ticket = m->Wp<int>(m->L.ticket);
        SWX_TRY(swx_gemm_dec(g, s));
    }
    return 0;
}

int swx_decoder_forward(swx_model *m, const FwdCfg &f, hipStream_t s)
{
    const int flags = swx_flags();
    const bool dec_ok = m->dtype == SWX_F16 && m->is_folded() && !(flags & SWX_FLAG_NO_FAST_STEP);
    // Multi-token passes (scoring pass, prefill, refine / locate probes) take the dec GEMMs + the 16-row-group cross-attention at
    // EVERY size since round 4: which kernels compute a row must not depend on how many windows share the launch or on the longest
    // window of the batch -- window k of a 20-window batch is bit-identical to the same window alone
    // (tests/test_gpu_batch_invariance.py).  SWX_FLAG_SCORE_TILED restores round 3's dispatch (tiled GEMMs + flash attention
    // above 160 rows: ~1.5x faster per pass at 20 windows, different rounding points) for A/B runs.
    const int64_t rows_all = (int64_t)f.W * f.rpw * f.n_new;
    if (dec_ok && f.n_new > 1 && (rows_all <= 160 || !(flags & SWX_FLAG_SCORE_TILED)) && rows_all <= m->L.rows_big &&
        swx_dec_slab_floats((int)rows_all, m->dims.n_text_state, 4 * m->dims.n_text_state) * 4 <= m->L.slab_bytes)
        return decoder_dec(m, f, s);
    if (dec_ok && f.n_new == 1 && f.row_mul == 1 && !f.capture && f.rpw <= 16 && m->dims.n_audio_ctx >= 128 &&
        (size_t)f.W * f.rpw <= (size_t)m->L.rows_big)
        return decoder_dec(m, f, s);
    const swx_dims &D = m->dims;
    const int d = D.n_text_state, H = D.n_text_head;
    const size_t e = m->esz;
    const int R = f.W * f.rpw;
    const int rows = R * f.n_new;
    if (rows > m->L.rows_big) return -8;
    unsigned char *x = m->ws + m->L.x, *h = m->ws + m->L.h, *qkv = m->ws + m->L.qkv, *att = m->ws + m->L.att, *u = m->ws + m->L.u;
    SWX_TRY(swx_embed(m->dtype, f.tokens, f.ld_tok, nullptr, f.pos0, R, f.n_new, m->arena + m->o_tok_emb,
                      m->A<float>(m->o_dec_pos), d, x, s));
    // embed indexes rows by grid row; with row_mul > 1 the caller passes pre-strided token / position views
    for (int l = 0; l < D.n_text_layer; ++l) {
        const LayerW &w = m->dec[l];
        SWX_TRY(swx_layernorm(m->dtype, x, d, m->A<float>(w.ln1_g), m->A<float>(w.ln1_b), h, d, rows, d, s));
        SWX_TRY(swx_gemm(m->dtype, swx_gemm_args(h, d, m->arena + w.wqkv, d, m->A<float>(w.bqkv), qkv, 3 * d, rows, 3 * d, d, EPI_BIAS), 0, s));
        SelfAttnArgs sa{};
        sa.qkv = qkv; sa.ldqkv = 3 * d;
        sa.kcache = f.kcache + (size_t)l * f.layer_stride;
        sa.vcache = f.vcache + (size_t)l * f.layer_stride;
        sa.anc = f.anc; sa.pos0 = f.pos0; sa.o = att; sa.ldo = d;
        sa.R = R; sa.n_new = f.n_new; sa.H = H; sa.n_ctx = D.n_text_ctx; sa.d = d;
        sa.kl = swx_klayout(f.k_chunked, D.n_text_ctx, d);
        sa.pos0_all_zero = f.pos0 == m->Wp<int32_t>(m->L.zeros_i32) ? 1 : 0;
        SWX_TRY(swx_self_attention(m->dtype, sa, f.row_mul, s));
        SWX_TRY(swx_gemm_residual(m, att, d, w.wo, w.bo, x, d, rows, d, d, s));
        // cross attention
        SWX_TRY(swx_layernorm(m->dtype, x, d, m->A<float>(w.lnx_g), m->A<float>(w.lnx_b), h, d, rows, d, s));
        SWX_TRY(swx_gemm(m->dtype, swx_gemm_args(h, d, m->arena + w.wcq, d, m->A<float>(w.bcq), qkv, d, rows, d, d, EPI_BIAS), 0, s));
        if (f.qcap) {
            hipError_t qe = hipMemcpyAsync(f.qcap + (size_t)l * rows * d * e, qkv, (size_t)rows * d * e, hipMemcpyDeviceToDevice, s);
            if (qe != hipSuccess) return -100 - (int)qe;
        }
        // cross K/V of this layer: per window [K: 1500 x d row-major | V^T: d x SWX_VT_KP, keys contiguous]
        const int64_t chunk = xkv_chunk_elems(m);
        const unsigned char *kl = f.xkv + (size_t)l * (f.xkv_W ? f.xkv_W : f.W) * chunk * e;
        AttnArgs ca{};
        ca.q = qkv; ca.ldq = d; ca.k = kl; ca.v = kl + (size_t)D.n_audio_ctx * d * e; ca.ldkv = d;
        ca.k_bs = chunk; ca.v_bs = chunk; ca.vt_kp = SWX_VT_KP; ca.o = att; ca.ldo = d;
        ca.B = f.W; ca.H = H; ca.nq = f.rpw * f.n_new; ca.nk = D.n_audio_ctx; ca.q_rows_per_batch = f.rpw * f.n_new;
        ca.f32_no_split = f.xattn_by_blocks ? 1 : 0;
        SWX_TRY(swx_attention(m->dtype, ca, 0, s));
        if (f.capture && !m->heads_by_layer[l].empty()) {
            SWX_TRY(swx_qk_capture(m->dtype, qkv, d, f.rpw * f.n_new, f.cap_row0, f.cap_rows, kl, d, chunk, D.n_audio_ctx,
                                   m->Wp<int32_t>(m->L.heads) + m->head_slot0[l], (int)m->heads_by_layer[l].size(),
                                   m->head_slot0[l], m->n_align, f.W, m->Wp<float>(m->L.cap), f.cap_ld_n, D.n_audio_ctx, s));
        }
        SWX_TRY(swx_gemm_residual(m, att, d, w.wco, w.bco, x, d, rows, d, d, s));
        // MLP
        SWX_TRY(swx_layernorm(m->dtype, x, d, m->A<float>(w.ln2_g), m->A<float>(w.ln2_b), h, d, rows, d, s));
        SWX_TRY(swx_gemm(m->dtype, swx_gemm_args(h, d, m->arena + w.w1, d, m->A<float>(w.b1), u, 4 * d, rows, 4 * d, d, EPI_BIAS | EPI_GELU), 0, s));
        SWX_TRY(swx_gemm_residual(m, u, 4 * d, w.w2, w.b2, x, d, rows, d, 4 * d, s));
    }
    return 0;
}

int swx_logits_gemm(swx_model *m, const void *hid, int64_t ld, int rows, float *out, hipStream_t s)
{
    const swx_dims &D = m->dims;
    return swx_gemm(m->dtype, swx_gemm_args(hid, ld, m->arena + m->o_tok_emb, D.n_text_state, nullptr, out, D.n_vocab, rows,
                                            D.n_vocab, D.n_text_state, EPI_OUT_F32), 0, s);
}

// the decoder's final LayerNorm: `rows` contiguous rows of the raw residual stream at `src` -> the h buffer
int swx_final_ln(swx_model *m, const void *src, int rows, hipStream_t s)
{
    const int d = m->dims.n_text_state;
    return swx_layernorm(m->dtype, src, d, m->A<float>(m->o_ln_g), m->A<float>(m->o_ln_b), m->ws + m->L.h, d, rows, d, s);
}
