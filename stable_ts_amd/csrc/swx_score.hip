// swx_score.hip -- the teacher-forced passes on the host side and the kernels that reduce their logits on the device: token
// probabilities / ranks, the next-token reduction, language identification; the scoring ABI and the head-selection ABI
#include <vector>
#include "swx_model.h"

namespace {

// one block per row: out[row] = softmax(logits[row][:n_used])[target].  RANK (swx_forward_token_ranks): also rank[row] =
// #{v < n_used : x_v < x_t or (x_v == x_t and v < t)}, the position of the target in an ascending sort on (logit, index),
// counted next to the maximum pass (integer sums: their order is free).  The probability is ONE code path for both
// instantiations -- the same per-thread elements, butterfly and LDS combine -- so swx_score's token probabilities and
// swx_forward_token_ranks' agree bit for bit on the same logits.  A target outside [0, n_used): probability 0, rank -1.
template <bool RANK>
__global__ __launch_bounds__(256) void token_prob_kernel(const float *__restrict__ logits, int V, int n_used,
                                                         const int32_t *__restrict__ target_tok, float *__restrict__ out,
                                                         int32_t *__restrict__ rank)
{
    __shared__ float sh[4];
    __shared__ int shc[4];
    const int row = blockIdx.x, tid = threadIdx.x;
    const float *lg = logits + (size_t)row * V;
    int t = 0, below = 0;
    bool ok = false;
    float xt = 0.f;
    if constexpr (RANK) {
        t = target_tok[row];
        ok = t >= 0 && t < n_used;
        xt = ok ? lg[t] : 0.f;
    }
    float mx = -__builtin_inff();
    for (int i = tid; i < n_used; i += 256) {
        const float v = lg[i];
        mx = fmaxf(mx, v);
        if constexpr (RANK) below += (v < xt || (v == xt && i < t)) ? 1 : 0;
    }
    mx = wave_max(mx);
    if constexpr (RANK) {
        const int lane = tid & 63;
        below += lane_xor<32>(below, lane); below += lane_xor<16>(below, lane); below += lane_xor<8>(below, lane);
        below += lane_xor<4>(below, lane); below += lane_xor<2>(below, lane); below += lane_xor<1>(below, lane);
        if (lane == 0) shc[tid >> 6] = below;
    }
    if ((tid & 63) == 0) sh[tid >> 6] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
    if constexpr (RANK) below = shc[0] + shc[1] + shc[2] + shc[3];
    __syncthreads();
    float sum = 0.f;
    for (int i = tid; i < n_used; i += 256) sum += expf(lg[i] - mx);
    sum = wave_sum(sum);
    if ((tid & 63) == 0) sh[tid >> 6] = sum;
    __syncthreads();
    sum = sh[0] + sh[1] + sh[2] + sh[3];
    if (tid == 0) {
        if constexpr (!RANK) t = target_tok[row];
        const bool in = t >= 0 && t < n_used;
        out[row] = in ? expf(lg[t] - mx) / sum : 0.f;
        if constexpr (RANK) rank[row] = in ? below : -1;
    }
}

// The greedy step of locate reduced on the device (swx_forward_next_token): one block per window.  x = logits[row][0 .. eot] with
// the suppressed ids at -inf (a bit mask over the ids in LDS, set once per block before the passes; the passes only read it).
// Pass 1 keeps, per thread, the two largest entries of x[0 .. eot] in the total order on (logit, index) -- token_prob_kernel's order, a
// tie goes to the higher index -- next to the maximum of x[0 .. eot - 1]; both go through the wave butterfly (lane_xor) and a
// four-slot LDS combine.  Pass 2 is token_prob_kernel's: the same per-thread elements of expf(x - max), the same butterfly, the
// same combine, p = expf(x_t - max) / sum -- so on the same row the probabilities are the bits swx_score's are.  An id outside
// [0, eot) (target -1, a top id equal to eot) has probability 0.  Nothing past column eot is read.  Dynamic LDS: (eot + 32) / 32 words.
struct Top2 { float v1, v2; int i1, i2; };
__device__ __forceinline__ bool top_gt(float av, int ai, float bv, int bi) { return av > bv || (av == bv && ai > bi); }
__device__ __forceinline__ Top2 top2_merge(const Top2 &a, const Top2 &b)
{
    Top2 r;
    if (top_gt(a.v1, a.i1, b.v1, b.i1)) {
        r.v1 = a.v1; r.i1 = a.i1;
        const bool k = top_gt(a.v2, a.i2, b.v1, b.i1);
        r.v2 = k ? a.v2 : b.v1; r.i2 = k ? a.i2 : b.i1;
    } else {
        r.v1 = b.v1; r.i1 = b.i1;
        const bool k = top_gt(a.v1, a.i1, b.v2, b.i2);
        r.v2 = k ? a.v1 : b.v2; r.i2 = k ? a.i1 : b.i2;
    }
    return r;
}
template <int O> __device__ __forceinline__ Top2 top2_step(const Top2 &x, int lane)
{
    Top2 y;
    y.v1 = lane_xor<O>(x.v1, lane); y.i1 = lane_xor<O>(x.i1, lane); y.v2 = lane_xor<O>(x.v2, lane); y.i2 = lane_xor<O>(x.i2, lane);
    return top2_merge(x, y);
}

__global__ __launch_bounds__(256) void next_token_kernel(const float *__restrict__ logits, int64_t ld, int eot,
                                                         const int32_t *__restrict__ suppress, int n_suppress,
                                                         const int32_t *__restrict__ target_tok, int32_t *__restrict__ top,
                                                         float *__restrict__ prob)
{
    extern __shared__ unsigned nt_mask[];
    __shared__ float sh[4];
    __shared__ Top2 sht[4];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const float *lg = logits + (size_t)row * ld;
    const int n_words = (eot + 32) >> 5;                    // bits 0 .. eot
    for (int i = tid; i < n_words; i += 256) nt_mask[i] = 0u;
    __syncthreads();
    for (int i = tid; i < n_suppress; i += 256) {
        const int v = suppress[i];
        if (v >= 0 && v < eot) atomicOr(&nt_mask[v >> 5], 1u << (v & 31));
    }
    __syncthreads();
    const float ninf = -__builtin_inff();
    auto x_at = [&](int i) { return ((nt_mask[i >> 5] >> (i & 31)) & 1u) ? ninf : lg[i]; };
    Top2 t{ninf, ninf, -1, -2};
    float mx = ninf;
    for (int i = tid; i <= eot; i += 256) {
        const float v = x_at(i);
        if (i < eot) mx = fmaxf(mx, v);
        if (top_gt(v, i, t.v1, t.i1)) { t.v2 = t.v1; t.i2 = t.i1; t.v1 = v; t.i1 = i; }
        else if (top_gt(v, i, t.v2, t.i2)) { t.v2 = v; t.i2 = i; }
    }
    mx = wave_max(mx);
    t = top2_step<32>(t, lane); t = top2_step<16>(t, lane); t = top2_step<8>(t, lane);
    t = top2_step<4>(t, lane); t = top2_step<2>(t, lane); t = top2_step<1>(t, lane);
    if (lane == 0) { sh[tid >> 6] = mx; sht[tid >> 6] = t; }
    __syncthreads();
    mx = fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
    t = top2_merge(top2_merge(sht[0], sht[1]), top2_merge(sht[2], sht[3]));
    __syncthreads();
    float sum = 0.f;
    for (int i = tid; i < eot; i += 256) sum += expf(x_at(i) - mx);
    sum = wave_sum(sum);
    if (lane == 0) sh[tid >> 6] = sum;
    __syncthreads();
    sum = sh[0] + sh[1] + sh[2] + sh[3];
    if (tid == 0) {
        const int ids[3] = {target_tok[row], t.i1, t.i2};
        top[2 * row] = t.i1; top[2 * row + 1] = t.i2;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int id = ids[k];
            prob[3 * row + k] = (id >= 0 && id < eot) ? expf(x_at(id) - mx) / sum : 0.f;
        }
    }
}

// rows[k] of src (row stride = n16 16-byte units) -> row k of dst: the last token row of up to 64 windows, offsets by value
struct RowList { int32_t row[64]; };
__global__ __launch_bounds__(256) void gather_row_list_kernel(const uint4 *__restrict__ src, uint4 *__restrict__ dst, int n16, RowList rows)
{
    const uint4 *s = src + (size_t)rows.row[blockIdx.x] * n16;
    uint4 *d = dst + (size_t)blockIdx.x * n16;
    for (int i = threadIdx.x; i < n16; i += 256) d[i] = s[i];
}

// tokens [W][1] -> [W][2], the token repeated (swx_forward_next_token at max_n == 1)
__global__ void repeat_token_kernel(const int32_t *__restrict__ in, int32_t *__restrict__ out, int W)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < 2 * W) out[idx] = in[idx >> 1];
}

__global__ void score_targets_kernel(const int32_t *__restrict__ tokens, int max_n, int n_sot, int rows_per_w,
                                     int32_t *__restrict__ targets, int total)
{
    // row (w, i) of the probability pass predicts tokens[w][n_sot + 1 + i]
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int w = idx / rows_per_w, i = idx % rows_per_w;
    const int p = n_sot + 1 + i;
    targets[idx] = (p < max_n) ? tokens[(size_t)w * max_n + p] : -1;
}

__global__ void fill_i32_kernel(int32_t *__restrict__ out, int32_t v, int n)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < n) out[idx] = v;
}

// Language identification (swx_detect_language): one workgroup per window.  hidden [W][d] = the final-LayerNorm'd state of the
// <|sot|> row; wave k takes language tokens k, k + 4, ... and forms dot(hidden[w], E[tok_j]) over d: the embedding row in 16-byte
// loads (VEC elements per lane), f32 products and sums in both dtypes, lane-sequential over the row and then the wave butterfly.
// The softmax over the n_lang logits and the arg-max (ties -> the lowest index, as torch.argmax) stay in LDS.  Nothing here
// depends on W, so a window's numbers are those of the same window alone.  A token id outside [0, V) is never dereferenced:
// its logit is -inf (probability 0).  Dynamic LDS: (d + n_lang) floats.
template <typename T>
__global__ __launch_bounds__(256) void lang_id_kernel(const T *__restrict__ hidden, const T *__restrict__ E, int d, int V,
                                                      const int32_t *__restrict__ lang_tokens, int n_lang,
                                                      float *__restrict__ probs, int32_t *__restrict__ best)
{
    constexpr int VEC = 16 / (int)sizeof(T);
    extern __shared__ float lang_sh[];
    __shared__ float red[4];
    __shared__ int best_j;
    float *hs = lang_sh, *lg = lang_sh + d;
    const int w = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const T *h = hidden + (size_t)w * d;
    for (int i = tid; i < d; i += 256) hs[i] = to_f32<T>(h[i]);
    if (tid == 0) best_j = n_lang;
    __syncthreads();
    for (int j = wave; j < n_lang; j += 4) {
        const int tok = lang_tokens[j];
        float acc = 0.f;
        const bool ok = tok >= 0 && tok < V;
        if (ok) {
            const T *e = E + (size_t)tok * d;
            for (int i = lane * VEC; i < d; i += 64 * VEC) {
                if constexpr (VEC == 8) {
                    const f16x8 v = *(const f16x8 *)(e + i);
#pragma unroll
                    for (int k = 0; k < 8; ++k) acc += hs[i + k] * (float)v[k];
                } else {
                    const f32x4 v = *(const f32x4 *)(e + i);
#pragma unroll
                    for (int k = 0; k < 4; ++k) acc += hs[i + k] * v[k];
                }
            }
        }
        acc = wave_sum(acc);
        if (lane == 0) lg[j] = ok ? acc : -__builtin_inff();
    }
    __syncthreads();
    float mx = -__builtin_inff();
    for (int j = tid; j < n_lang; j += 256) mx = fmaxf(mx, lg[j]);
    mx = wave_max(mx);
    if (lane == 0) red[wave] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    float sum = 0.f;
    for (int j = tid; j < n_lang; j += 256) {
        const float x = lg[j];
        if (x == mx) atomicMin(&best_j, j);
        const float p = expf(x - mx);
        lg[j] = p;
        sum += p;
    }
    sum = wave_sum(sum);
    if (lane == 0) red[wave] = sum;
    __syncthreads();
    sum = (red[0] + red[1]) + (red[2] + red[3]);
    for (int j = tid; j < n_lang; j += 256) probs[(size_t)w * n_lang + j] = lg[j] / sum;
    if (tid == 0) best[w] = best_j < n_lang ? lang_tokens[best_j] : -1;
}

}  // namespace

extern "C" {

// ------------------------------------------------------------------------------------------------------ score
// capture: raw qk of the alignment heads for token rows cap_row0 .. cap_row0 + cap_rows - 1 -> L.cap [W][n_align][cap_ld][1500]
static int score_forward(swx_model *m, const int32_t *d_tokens, const int32_t *h_n_tok, int W, int max_n, int cap_row0,
                         int cap_rows, int cap_ld, const void *d_xkv, bool capture, hipStream_t s, void *qcap = nullptr, int xkv_W = 0)
{
    const swx_dims &D = m->dims;
    if (W > m->max_windows) return -8;
    if (max_n <= 0 || max_n > D.n_text_ctx) return -2;
    for (int w = 0; w < W; ++w) if (h_n_tok[w] > max_n || h_n_tok[w] <= 0) return -1;
    FwdCfg f{};
    f.W = W; f.rpw = 1; f.row_mul = 1; f.n_new = max_n;
    f.tokens = d_tokens; f.ld_tok = max_n;
    f.pos0 = m->Wp<int32_t>(m->L.zeros_i32);
    f.kcache = m->ws + m->L.sk; f.vcache = m->ws + m->L.sv; f.layer_stride = 0; f.cache_rows = m->max_windows;
    f.anc = nullptr; f.xkv = (const unsigned char *)d_xkv;
    f.capture = capture;
    f.qcap = (unsigned char *)qcap;
    f.xkv_W = xkv_W;
    // A teacher-forced pass over several tokens: max_n is the longest window's count, and a window of <= 16 tokens must get the
    // numbers it gets next to a longer one (transcribe_many / transcribe_spans: windows of different recordings share the scoring
    // pass).  A single-token pass (max_n == 1) is one query per window in any batch and keeps the key-split kernel.
    f.xattn_by_blocks = max_n > 1;
    f.cap_row0 = cap_row0; f.cap_rows = cap_rows; f.cap_ld_n = cap_ld;
    if (capture && (cap_rows <= 0 || cap_row0 < 0 || cap_row0 + cap_rows > max_n || cap_ld < cap_rows)) return -1;
    return swx_decoder_forward(m, f, s);
}

// token probabilities of a scoring pass: rows n_sot .. n_sot+T-1 of the final-LN'd hidden states -> logits[:, :eot] ->
// softmax -> gather at the next token (timing.py:62-64); d_token_probs f32 [W][max_n]
static int score_token_probs(swx_model *m, const int32_t *d_tokens, int W, int max_n, int n_sot, int eot, float *d_token_probs,
                             hipStream_t s)
{
    const swx_dims &D = m->dims;
    const int d = D.n_text_state;
    const size_t e = m->esz;
    unsigned char *x = m->ws + m->L.x, *hh = m->ws + m->L.h;
    const int rows = W * max_n;
    SWX_TRY(swx_final_ln(m, x, rows, s));
    const int rpw = max_n - n_sot - 2;     // probability rows per window (T_max)
    if (rpw > 0) {
        float *lg = m->Wp<float>(m->L.logits);
        int32_t *targets = (int32_t *)(m->ws + m->L.att);     // att is free after the forward pass
        const int total = W * rpw;
        hipLaunchKernelGGL(score_targets_kernel, dim3(cdiv(total, 256)), dim3(256), 0, s, d_tokens, max_n, n_sot, rpw, targets, total);
        const int chunk = (int)m->L.logits_rows;
        for (int w = 0; w < W; ++w) {
            for (int r0 = 0; r0 < rpw; r0 += chunk) {
                const int nr = (rpw - r0) < chunk ? (rpw - r0) : chunk;
                const unsigned char *hid = hh + ((size_t)w * max_n + n_sot + r0) * d * e;
                SWX_TRY(swx_logits_gemm(m, hid, d, nr, lg, s));
                hipLaunchKernelGGL(token_prob_kernel<false>, dim3(nr), dim3(256), 0, s, lg, D.n_vocab, eot, targets + (size_t)w * rpw + r0,
                                   d_token_probs + (size_t)w * max_n + r0, (int32_t *)nullptr);
            }
        }
        SWX_CHECK_LAUNCH();
    }
    return 0;
}

int swx_score(swx_model *m, const int32_t *d_tokens, const int32_t *h_n_tok, int W, int max_n, int n_sot, int eot,
              const int32_t *h_n_frames, float qk_scale, int medfilt_width, const void *d_xkv, float *d_token_probs,
              float *d_neg_matrix, void *stream)
{
    if (!m || !m->arena || !m->ws) return -9;
    if (W <= 0) return 0;
    if (m->n_align != m->ws_n_align || m->n_align <= 0) return -8;
    if (2 * W + 16 > SMALL_I32) return -8;
    const swx_dims &D = m->dims;
    hipStream_t s = S(stream);
    SWX_TRY(score_forward(m, d_tokens, h_n_tok, W, max_n, n_sot, max_n - n_sot - 1, max_n, d_xkv, true, s));

    // per-window row / frame counts on the device
    std::vector<int32_t> hv(2 * W);
    for (int w = 0; w < W; ++w) {
        const int T = h_n_tok[w] - n_sot - 2;
        if (T < 0) return -1;
        hv[w] = T + 1;
        int F = h_n_frames[w];
        if (F < 1) F = 1;
        if (F > D.n_audio_ctx) F = D.n_audio_ctx;
        hv[W + w] = F;
    }
    int32_t *d_small = m->Wp<int32_t>(m->L.small_i32);
    hipError_t er = hipMemcpyAsync(d_small, hv.data(), hv.size() * 4, hipMemcpyHostToDevice, s);
    if (er != hipSuccess) return -100 - (int)er;
    er = hipStreamSynchronize(s);     // hv goes out of scope; pageable copies are staged synchronously anyway
    if (er != hipSuccess) return -100 - (int)er;

    SWX_TRY(score_token_probs(m, d_tokens, W, max_n, n_sot, eot, d_token_probs, s));
    // alignment matrix
    // scratch for the row statistics: the [W][H][1500] f32 region (>= W*H*max_n float2, max_n <= 448); the raw scores stay intact
    SWX_TRY(swx_align_weights_launch(m->Wp<float>(m->L.cap), m->Wp<float>(m->L.mean), m->Wp<float>(m->L.mean), m->Wp<float>(m->L.sd),
                                     W, m->n_align, max_n, D.n_audio_ctx, d_small, d_small + W, qk_scale, medfilt_width,
                                     d_neg_matrix, max_n, D.n_audio_ctx, s));
    return 0;
}

int swx_score_qk(swx_model *m, const int32_t *d_tokens, const int32_t *h_n_tok, int W, int max_n, int n_sot, int eot,
                 int row0, int n_rows, const void *d_xkv, float *d_token_probs, float *d_qk, void *stream)
{
    if (!m || !m->arena || !m->ws) return -9;
    if (W <= 0) return 0;
    if (m->n_align != m->ws_n_align || m->n_align <= 0) return -8;
    if (!d_qk) return -1;
    for (int w = 0; w < W; ++w) if (h_n_tok[w] - n_sot - 2 < 0) return -1;
    hipStream_t s = S(stream);
    // the capture buffer is written densely ([W][n_align][n_rows][1500]) so that one copy hands it over
    SWX_TRY(score_forward(m, d_tokens, h_n_tok, W, max_n, row0, n_rows, n_rows, d_xkv, true, s));
    if (d_token_probs) SWX_TRY(score_token_probs(m, d_tokens, W, max_n, n_sot, eot, d_token_probs, s));
    const size_t bytes = (size_t)W * m->n_align * n_rows * m->dims.n_audio_ctx * sizeof(float);
    hipError_t er = hipMemcpyAsync(d_qk, m->Wp<float>(m->L.cap), bytes, hipMemcpyDeviceToDevice, s);
    return er == hipSuccess ? 0 : -100 - (int)er;
}

int swx_forward_logits(swx_model *m, const int32_t *d_tokens, const int32_t *h_n_tok, int W, int max_n, const void *d_xkv,
                       float *d_logits, void *stream)
{
    if (!m || !m->arena || !m->ws) return -9;
    if (W <= 0) return 0;
    const swx_dims &D = m->dims;
    hipStream_t s = S(stream);
    const int d = D.n_text_state;
    SWX_TRY(score_forward(m, d_tokens, h_n_tok, W, max_n, 0, 0, max_n, d_xkv, false, s));
    unsigned char *x = m->ws + m->L.x, *hh = m->ws + m->L.h;
    const int rows = W * max_n;
    SWX_TRY(swx_final_ln(m, x, rows, s));
    return swx_logits_gemm(m, hh, d, rows, d_logits, s);
}

// The teacher-forced pass of swx_forward_logits reduced on the device to the two numbers per row refine's bisection reads.  The
// vocabulary projection runs window by window in 64-row chunks through the workspace's logits region and token_prob_kernel<true> finishes each
// chunk, so no [W][max_n][n_vocab] tensor exists anywhere.  Row j of window w predicts d_tokens[w][j + 1]: the target list of a
// chunk is the token row itself, shifted by one.  Only rows j < n_tok[w] - 1 are computed and written.
int swx_forward_token_ranks(swx_model *m, const int32_t *d_tokens, const int32_t *h_n_tok, int W, int max_n, int n_vocab_used,
                            const void *d_xkv, float *d_prob, int32_t *d_rank, void *stream)
{
    if (!m || !m->arena || !m->ws) return -9;
    if (W <= 0) return 0;
    if (!d_tokens || !h_n_tok || !d_prob || !d_rank) return -1;
    const swx_dims &D = m->dims;
    if (n_vocab_used <= 0 || n_vocab_used > D.n_vocab) return -1;
    hipStream_t s = S(stream);
    const int d = D.n_text_state;
    const size_t e = m->esz;
    SWX_TRY(score_forward(m, d_tokens, h_n_tok, W, max_n, 0, 0, max_n, d_xkv, false, s));
    unsigned char *x = m->ws + m->L.x, *hh = m->ws + m->L.h;
    SWX_TRY(swx_final_ln(m, x, W * max_n, s));
    float *lg = m->Wp<float>(m->L.logits);
    // a fixed chunk (the logits region always holds 64 rows): the projection's launch shapes then depend on the window's own
    // token count alone, never on the workspace that happens to be bound or on the batch around the window
    const int chunk = 64;
    for (int w = 0; w < W; ++w) {
        const int rows = h_n_tok[w] - 1;
        for (int r0 = 0; r0 < rows; r0 += chunk) {
            const int nr = (rows - r0) < chunk ? (rows - r0) : chunk;
            const size_t at = (size_t)w * max_n + r0;
            SWX_TRY(swx_logits_gemm(m, hh + at * d * e, d, nr, lg, s));
            hipLaunchKernelGGL(token_prob_kernel<true>, dim3(nr), dim3(256), 0, s, lg, D.n_vocab, n_vocab_used, d_tokens + at + 1,
                               d_prob + at, d_rank + at);
            SWX_CHECK_LAUNCH();
        }
    }
    return 0;
}

static int next_token_reduce(const float *lg, int64_t ld, int W, int eot, const int32_t *d_suppress, int n_suppress,
                             const int32_t *d_target, int32_t *d_top, float *d_prob, hipStream_t s)
{
    const size_t lds = (size_t)((eot + 32) >> 5) * sizeof(unsigned);
    if (lds > 48 * 1024) return -2;
    hipLaunchKernelGGL(next_token_kernel, dim3(W), dim3(256), lds, s, lg, ld, eot, d_suppress, n_suppress, d_target, d_top, d_prob);
    SWX_CHECK_LAUNCH();
    return 0;
}

// The teacher-forced pass of swx_forward_logits reduced on the device to what locate's greedy step reads: the two best ids of the
// last row and three probabilities per window.  The last token row of every window is gathered out of the residual stream (row
// offsets travel by value, 64 per launch: no upload, no host wait), so the final LayerNorm and the vocabulary projection see W
// rows.  The projection runs in chunks of 64 rows, as in swx_forward_token_ranks: for M <= 64 the vocabulary projection is one
// kernel on a grid that depends on N alone in both dtypes (f16: one 128-row tile; f32: one 64-row tile), and a row's dot products
// do not depend on the other rows of its tile -- a window's logits are the same bits in any batch.  One launch of
// next_token_kernel finishes all W rows (the logits region holds max_rows + 2 max_windows >= W rows).
int swx_forward_next_token(swx_model *m, const int32_t *d_tokens, const int32_t *h_n_tok, int W, int max_n, int eot,
                           const int32_t *d_suppress, int n_suppress, const int32_t *d_target, const void *d_xkv, int32_t *d_top,
                           float *d_prob, void *stream)
{
    if (!m || !m->arena || !m->ws) return -9;
    if (!d_tokens || !h_n_tok || !d_target || !d_xkv || !d_top || !d_prob || n_suppress < 0 || (n_suppress > 0 && !d_suppress)) return -1;
    const swx_dims &D = m->dims;
    if (eot <= 0 || eot >= D.n_vocab) return -1;
    if (W <= 0) return 0;
    const int d = D.n_text_state;
    const size_t e = m->esz;
    if (W > m->max_windows || W > m->L.logits_rows || 2 * W > SMALL_I32) return -8;
    if (((size_t)d * e) % 16 != 0) return -2;
    if (max_n <= 0) return -2;
    for (int w = 0; w < W; ++w) if (h_n_tok[w] <= 0 || h_n_tok[w] > max_n) return -1;
    hipStream_t s = S(stream);
    int n = max_n;
    if (max_n == 1) {
        int32_t *two = m->Wp<int32_t>(m->L.small_i32);
        hipLaunchKernelGGL(repeat_token_kernel, dim3(cdiv(2 * W, 256)), dim3(256), 0, s, d_tokens, two, W);
        SWX_CHECK_LAUNCH();
        d_tokens = two;
        n = 2;
    }
    SWX_TRY(score_forward(m, d_tokens, h_n_tok, W, n, 0, 0, n, d_xkv, false, s));
    unsigned char *x = m->ws + m->L.x, *hh = m->ws + m->L.h, *last = m->ws + m->L.att;     // att is free after the forward pass
    const int n16 = (int)((size_t)d * e / 16);
    for (int w0 = 0; w0 < W; w0 += 64) {
        const int nw = (W - w0) < 64 ? (W - w0) : 64;
        RowList rows{};
        for (int k = 0; k < nw; ++k) rows.row[k] = (w0 + k) * n + h_n_tok[w0 + k] - 1;
        hipLaunchKernelGGL(gather_row_list_kernel, dim3(nw), dim3(256), 0, s, (const uint4 *)x, (uint4 *)(last + (size_t)w0 * d * e), n16, rows);
        SWX_CHECK_LAUNCH();
    }
    SWX_TRY(swx_final_ln(m, last, W, s));
    float *lg = m->Wp<float>(m->L.logits);
    const int chunk = 64;
    for (int r0 = 0; r0 < W; r0 += chunk) {
        const int nr = (W - r0) < chunk ? (W - r0) : chunk;
        SWX_TRY(swx_logits_gemm(m, hh + (size_t)r0 * d * e, d, nr, lg + (size_t)r0 * D.n_vocab, s));
    }
    return next_token_reduce(lg, D.n_vocab, W, eot, d_suppress, n_suppress, d_target, d_top, d_prob, s);
}

// beside next_token_reduce, which is private to this file: the reduction alone, on the caller's logits
int swx_test_next_token_reduce(const float *d_logits, int64_t ld, int W, int eot, const int32_t *d_suppress, int n_suppress,
                               const int32_t *d_target, int32_t *d_top, float *d_prob, void *stream)
{
    if (!d_logits || !d_target || !d_top || !d_prob || n_suppress < 0 || (n_suppress > 0 && !d_suppress)) return -1;
    if (eot <= 0 || ld <= eot || W < 0) return -1;
    if (W == 0) return 0;
    return next_token_reduce(d_logits, ld, W, eot, d_suppress, n_suppress, d_target, d_top, d_prob, S(stream));
}

// Language identification on features that are already resident: the teacher-forced pass of the single token `sot` (the pass
// swx_forward_logits makes with max_n = 1, through the final LayerNorm) and lang_id_kernel over the n_lang language rows of the
// embedding -- 0.2 % of the vocabulary projection, and W * (n_lang + 1) numbers out instead of [W][n_vocab] f32.  Enqueues only:
// no allocation, no synchronisation; the launch shapes depend on (W, n_lang, d).  The token ids live on the device, so the
// host cannot refuse one that is outside the vocabulary without waiting for the stream: the kernel never dereferences such
// an id (probability 0), and the Python owner checks the list before it uploads it (Engine.detect_language).
int swx_detect_language(swx_model *m, const void *d_xkv, int W, int sot, const int32_t *d_lang_tokens, int n_lang,
                        float *d_probs, int32_t *d_best, void *stream)
{
    if (!m || !m->arena || !m->ws) return -9;
    if (!d_xkv || !d_lang_tokens || !d_probs || !d_best) return -1;
    const swx_dims &D = m->dims;
    const int d = D.n_text_state;
    if (n_lang <= 0 || n_lang > D.n_vocab || sot < 0 || sot >= D.n_vocab || W < 0) return -1;
    if (W == 0) return 0;
    if (W > m->max_windows || W > SMALL_I32) return -8;
    const size_t lds = ((size_t)d + (size_t)n_lang) * sizeof(float);
    if (d % 8 != 0 || lds > 48 * 1024) return -2;
    hipStream_t s = S(stream);
    int32_t *d_tok = m->Wp<int32_t>(m->L.small_i32);
    hipLaunchKernelGGL(fill_i32_kernel, dim3(cdiv(W, 256)), dim3(256), 0, s, d_tok, (int32_t)sot, W);
    SWX_CHECK_LAUNCH();
    const std::vector<int32_t> ones((size_t)W, 1);
    SWX_TRY(score_forward(m, d_tok, ones.data(), W, 1, 0, 0, 1, d_xkv, false, s));
    unsigned char *x = m->ws + m->L.x, *hh = m->ws + m->L.h;
    SWX_TRY(swx_final_ln(m, x, W, s));
    if (m->dtype == SWX_F16)
        hipLaunchKernelGGL(lang_id_kernel<f16>, dim3(W), dim3(256), lds, s, (const f16 *)hh, (const f16 *)(m->arena + m->o_tok_emb), d,
                           D.n_vocab, d_lang_tokens, n_lang, d_probs, d_best);
    else
        hipLaunchKernelGGL(lang_id_kernel<float>, dim3(W), dim3(256), lds, s, (const float *)hh, (const float *)(m->arena + m->o_tok_emb), d,
                           D.n_vocab, d_lang_tokens, n_lang, d_probs, d_best);
    SWX_CHECK_LAUNCH();
    return 0;
}

// ------------------------------------------------------------------------------- head-selection variants (f4)
// The teacher-forced pass of ONE window that keeps the cross-attention queries of every layer instead of any head's scores:
// d_q [n_text_layer][max_n][d] in the compute dtype (swx_qcap_bytes).  timing.py:41-67 with the hooks of :50-56 replaced by
// "keep q": a head's score row is q . K^T of the window's cross-K, which swx_cross_kv left in d_xkv.
size_t swx_qcap_bytes(const swx_model *m, int max_n)
{
    if (!m || max_n <= 0) return 0;
    return (size_t)m->dims.n_text_layer * max_n * m->dims.n_text_state * m->esz;
}

int swx_score_q(swx_model *m, const int32_t *d_tokens, const int32_t *h_n_tok, int max_n, int n_sot, int eot, const void *d_xkv,
                float *d_token_probs, void *d_q, void *stream)
{
    if (!m || !m->arena || !m->ws) return -9;
    if (!d_q || !d_tokens || !h_n_tok) return -1;
    if (h_n_tok[0] - n_sot - 2 < 0) return -1;
    hipStream_t s = S(stream);
    SWX_TRY(score_forward(m, d_tokens, h_n_tok, 1, max_n, 0, 0, max_n, d_xkv, false, s, d_q));
    if (d_token_probs) SWX_TRY(score_token_probs(m, d_tokens, 1, max_n, n_sot, eot, d_token_probs, s));
    return 0;
}

// scratch of the head-selection calls, as byte offsets (every region 256-byte aligned; include/swx.h lists the shapes).  One
// function lays out both forms and the launchers below carve their pointers from what it returns, so swx_test_heads_layout
// reports the layout the code uses.  W >= 1: the two batch calls -- the per-window counts, then for W windows the head scores
// (f64) and picks of every row, the column norms / scores / picks of every head, then (count > 0) the gathered raw scores
// [W][count][max_rows][n_audio_ctx] f32 and the row statistics swx_align_weights_launch needs.  W == 0: the single-window calls
// -- no counts, picks sized for count = LH, no gathered rows (the caller's d_qk_sel receives them) and no row statistics.
struct HeadsBatchScratch { size_t cnt, score, sel, colnorm, nscore, top, gathered, rstat, total; };
static HeadsBatchScratch heads_batch_layout(const swx_model *m, int W, int max_n, int count)
{
    const size_t LH = (size_t)m->dims.n_text_layer * m->dims.n_text_head, w = W > 0 ? (size_t)W : 1, c = count > 0 ? (size_t)count : 0;
    HeadsBatchScratch L{};
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t at = off; off += align_up(bytes); return at; };
    L.cnt = take(W > 0 ? 3 * w * sizeof(int32_t) : 0);
    L.score = take(w * LH * max_n * sizeof(double));
    L.sel = take(W > 0 ? w * max_n * (c ? c : 1) * sizeof(int32_t) : LH * max_n * sizeof(int32_t));
    L.colnorm = take(w * LH * SWX_HS_MAXF * sizeof(float));
    L.nscore = take(w * LH * sizeof(float));
    L.top = take(w * LH * sizeof(int32_t));
    L.gathered = take(W > 0 ? w * c * max_n * m->dims.n_audio_ctx * sizeof(float) : 0);
    L.rstat = take(W > 0 ? w * c * max_n * sizeof(float2) : 0);
    L.total = off;
    return L;
}

size_t swx_heads_scratch_bytes(const swx_model *m, int max_n)
{
    if (!m || max_n <= 0) return 0;
    return heads_batch_layout(m, 0, max_n, 0).total;
}

// beside heads_batch_layout, which is private to this file
int swx_test_heads_layout(const swx_model *m, int W, int max_n, int count, int64_t *out)
{
    // the byte offsets the head-selection entries carve out of their scratch: heads_batch_layout, the function they call themselves
    if (!m || !out || W < 0 || max_n <= 0 || count < 0) return -1;
    const HeadsBatchScratch L = heads_batch_layout(m, W, max_n, W > 0 ? count : 0);
    const size_t v[9] = {L.cnt, L.score, L.sel, L.colnorm, L.nscore, L.top, L.gathered, L.rstat, L.total};
    for (int k = 0; k < 9; ++k) out[k] = (int64_t)v[k];
    return 0;
}

// dynamic_heads (timing.py:87-103): rows row0 .. row0 + n_rows - 1 of the pass; d_qk_sel [count][n_rows][ld_f] f32 receives the RAW
// scaled scores of the count heads picked per row -- the input layout of swx_align_weights (H = count, N = n_rows), which
// applies qk_scale / softmax / z-normalisation / median / head mean exactly as on the default path.  d_peaks: null (every row's
// own attention peak) or the n_rows jump midpoints of the previous DTW pass (f64).
int swx_heads_dynamic(swx_model *m, const void *d_q, int max_n, int row0, int n_rows, const void *d_xkv, int n_frames, float qk_scale,
                      int count, const double *d_peaks, float *d_qk_sel, int ld_f, void *d_scratch, size_t scratch_bytes, void *stream)
{
    if (!m || !m->arena) return -9;
    if (!d_q || !d_xkv || !d_qk_sel || !d_scratch) return -1;
    if (row0 < 0 || n_rows <= 0 || row0 + n_rows > max_n || ld_f < m->dims.n_audio_ctx) return -1;
    if (scratch_bytes < swx_heads_scratch_bytes(m, max_n)) return -8;
    const swx_dims &D = m->dims;
    const HeadsBatchScratch L = heads_batch_layout(m, 0, max_n, 0);
    unsigned char *p = (unsigned char *)d_scratch;
    double *score = (double *)(p + L.score);
    int32_t *sel = (int32_t *)(p + L.sel);
    int F = n_frames < 1 ? 1 : (n_frames > D.n_audio_ctx ? D.n_audio_ctx : n_frames);
    return swx_headsel_dynamic_launch(m->dtype, d_q, max_n, D.n_text_state, row0, n_rows, d_xkv, xkv_chunk_elems(m), D.n_text_layer,
                                      D.n_text_head, F, D.n_audio_ctx, qk_scale, count, d_peaks, score, sel, d_qk_sel, ld_f, S(stream));
}

// aligner = 'new' (timing.py:115-163) over the n_tok rows of the pass; d_neg_matrix [n_out][ld_f] f32 receives MINUS the
// column-normalised mean map of the topk sharpest heads for rows row0 .. row0 + n_out - 1 (= the DTW input, timing.py:194)
int swx_heads_new(swx_model *m, const void *d_q, int max_n, int n_tok, int row0, int n_out, const void *d_xkv, int n_frames,
                  float qk_scale, int medfilt_width, int topk, float w_colnorm, float w_rownorm, float w_coverage,
                  float *d_neg_matrix, int ld_f, void *d_scratch, size_t scratch_bytes, void *stream)
{
    if (!m || !m->arena) return -9;
    if (!d_q || !d_xkv || !d_neg_matrix || !d_scratch) return -1;
    if (n_tok <= 0 || n_tok > max_n) return -1;
    if (scratch_bytes < swx_heads_scratch_bytes(m, max_n)) return -8;
    const swx_dims &D = m->dims;
    const HeadsBatchScratch L = heads_batch_layout(m, 0, max_n, 0);
    unsigned char *p = (unsigned char *)d_scratch;
    float *colnorm = (float *)(p + L.colnorm);
    float *score = (float *)(p + L.nscore);
    int32_t *top = (int32_t *)(p + L.top);
    int F = n_frames < 1 ? 1 : (n_frames > D.n_audio_ctx ? D.n_audio_ctx : n_frames);
    return swx_headsel_new_launch(m->dtype, d_q, max_n, D.n_text_state, n_tok, row0, n_out, d_xkv, xkv_chunk_elems(m), D.n_text_layer,
                                  D.n_text_head, F, qk_scale, medfilt_width, topk, w_colnorm, w_rownorm, w_coverage, colnorm, score, top,
                                  d_neg_matrix, ld_f, S(stream));
}

// ---- the same three calls for W windows of one batch.  The pass writes d_q [L][W][max_n][d]; the cross-K/V is read in place:
// d_xkv points at the FIRST of the W windows inside a buffer of xkv_W windows (layer stride xkv_W * chunk, window stride chunk;
// xkv_W = 0 means W), so a sub-batch of a larger job is an offset, not a copy.
size_t swx_qcap_batch_bytes(const swx_model *m, int W, int max_n)
{
    if (!m || W <= 0 || max_n <= 0) return 0;
    return (size_t)W * swx_qcap_bytes(m, max_n);
}

int swx_score_q_batch(swx_model *m, const int32_t *d_tokens, const int32_t *h_n_tok, int W, int max_n, int n_sot, int eot,
                      const void *d_xkv, int xkv_W, float *d_token_probs, void *d_q, void *stream)
{
    if (!m || !m->arena || !m->ws) return -9;
    if (!d_q || !d_tokens || !h_n_tok || !d_xkv || W < 0 || xkv_W < 0 || (xkv_W && xkv_W < W)) return -1;
    if (W == 0) return 0;
    for (int w = 0; w < W; ++w) if (h_n_tok[w] - n_sot - 2 < 0) return -1;
    hipStream_t s = S(stream);
    SWX_TRY(score_forward(m, d_tokens, h_n_tok, W, max_n, 0, 0, max_n, d_xkv, false, s, d_q, xkv_W));
    if (d_token_probs) SWX_TRY(score_token_probs(m, d_tokens, W, max_n, n_sot, eot, d_token_probs, s));
    return 0;
}

// validates the per-window counts and puts [n_tok | n_rows | n_frames (clamped to [1, n_audio_ctx])] at the head of the scratch
static int heads_batch_counts(swx_model *m, int W, int max_n, int n_sot, const int32_t *h_n_tok, const int32_t *h_n_frames, int32_t *d_cnt,
                       hipStream_t s)
{
    const swx_dims &D = m->dims;
    std::vector<int32_t> hv(3 * (size_t)W);
    for (int w = 0; w < W; ++w) {
        if (h_n_tok[w] <= 0 || h_n_tok[w] > max_n || h_n_tok[w] - n_sot - 1 <= 0) return -1;
        hv[w] = h_n_tok[w];
        hv[W + w] = h_n_tok[w] - n_sot - 1;
        const int F = h_n_frames[w];
        hv[2 * W + w] = F < 1 ? 1 : (F > D.n_audio_ctx ? D.n_audio_ctx : F);
    }
    hipError_t er = hipMemcpyAsync(d_cnt, hv.data(), hv.size() * 4, hipMemcpyHostToDevice, s);
    if (er == hipSuccess) er = hipStreamSynchronize(s);      // hv is a stack-lifetime staging buffer
    return er == hipSuccess ? 0 : -100 - (int)er;
}

size_t swx_heads_batch_scratch_bytes(const swx_model *m, int W, int max_n, int count)
{
    if (!m || W <= 0 || max_n <= 0 || count < 0) return 0;
    return heads_batch_layout(m, W, max_n, count).total;
}

// dynamic_heads for the text-token rows (n_sot .. n_tok[w] - 2) of every window: score -> pick -> gather -> the default path's
// z-normalisation / median / head mean; d_neg_matrix f32 [W][max_n - n_sot - 1][ld_f] receives the NEGATED matrix (rows
// < n_tok[w] - n_sot - 1, frames < n_frames[w]; nothing else is written).  d_peaks: null or f64 [W][max_n - n_sot - 1].
int swx_heads_dynamic_batch(swx_model *m, const void *d_q, int W, int max_n, int n_sot, const int32_t *h_n_tok,
                            const int32_t *h_n_frames, const void *d_xkv, int xkv_W, float qk_scale, int medfilt_width, int count,
                            const double *d_peaks, float *d_neg_matrix, int ld_f, void *d_scratch, size_t scratch_bytes, void *stream)
{
    if (!m || !m->arena) return -9;
    if (!d_q || !d_xkv || !d_neg_matrix || !d_scratch || !h_n_tok || !h_n_frames) return -1;
    const swx_dims &D = m->dims;
    if (W < 0 || xkv_W < 0 || (xkv_W && xkv_W < W) || n_sot < 0 || max_n - n_sot - 1 <= 0 || max_n > D.n_text_ctx || count <= 0 ||
        ld_f != D.n_audio_ctx)
        return -1;
    if (W == 0) return 0;
    const HeadsBatchScratch L = heads_batch_layout(m, W, max_n, count);
    if (scratch_bytes < L.total) return -8;
    hipStream_t s = S(stream);
    unsigned char *p = (unsigned char *)d_scratch;
    int32_t *cnt = (int32_t *)(p + L.cnt);
    SWX_TRY(heads_batch_counts(m, W, max_n, n_sot, h_n_tok, h_n_frames, cnt, s));
    const int max_rows = max_n - n_sot - 1;
    const int64_t chunk = xkv_chunk_elems(m);
    float *gathered = (float *)(p + L.gathered);
    SWX_TRY(swx_headsel_dynamic_batch_launch(m->dtype, d_q, W, max_n, D.n_text_state, n_sot, cnt + W, 0, max_rows, d_xkv,
                                             (int64_t)(xkv_W ? xkv_W : W) * chunk, chunk, D.n_text_layer, D.n_text_head, cnt + 2 * W, 0,
                                             D.n_audio_ctx, qk_scale, count, d_peaks, (double *)(p + L.score), (int32_t *)(p + L.sel),
                                             gathered, ld_f, s));
    return swx_align_weights_launch(gathered, (float *)(p + L.rstat), nullptr, nullptr, W, count, max_rows, ld_f, cnt + W, cnt + 2 * W,
                                    qk_scale, medfilt_width, d_neg_matrix, max_rows, ld_f, s);
}

// aligner = 'new' for every window over its own n_tok[w] rows; d_neg_matrix f32 [W][max_n - n_sot - 1][ld_f] as above
int swx_heads_new_batch(swx_model *m, const void *d_q, int W, int max_n, int n_sot, const int32_t *h_n_tok, const int32_t *h_n_frames,
                        const void *d_xkv, int xkv_W, float qk_scale, int medfilt_width, int topk, float w_colnorm, float w_rownorm,
                        float w_coverage, float *d_neg_matrix, int ld_f, void *d_scratch, size_t scratch_bytes, void *stream)
{
    if (!m || !m->arena) return -9;
    if (!d_q || !d_xkv || !d_neg_matrix || !d_scratch || !h_n_tok || !h_n_frames) return -1;
    const swx_dims &D = m->dims;
    if (W < 0 || xkv_W < 0 || (xkv_W && xkv_W < W) || n_sot < 0 || max_n - n_sot - 1 <= 0 || max_n > D.n_text_ctx ||
        ld_f < D.n_audio_ctx)
        return -1;
    if (W == 0) return 0;
    const HeadsBatchScratch L = heads_batch_layout(m, W, max_n, 0);
    if (scratch_bytes < L.total) return -8;
    hipStream_t s = S(stream);
    unsigned char *p = (unsigned char *)d_scratch;
    int32_t *cnt = (int32_t *)(p + L.cnt);
    SWX_TRY(heads_batch_counts(m, W, max_n, n_sot, h_n_tok, h_n_frames, cnt, s));
    const int max_out = max_n - n_sot - 1;
    const int64_t chunk = xkv_chunk_elems(m);
    return swx_headsel_new_batch_launch(m->dtype, d_q, W, max_n, D.n_text_state, cnt, 0, n_sot, cnt + W, 0, max_out, d_xkv,
                                        (int64_t)(xkv_W ? xkv_W : W) * chunk, chunk, D.n_text_layer, D.n_text_head, cnt + 2 * W, 0,
                                        qk_scale, medfilt_width, topk, w_colnorm, w_rownorm, w_coverage, (float *)(p + L.colnorm),
                                        (float *)(p + L.nscore), (int32_t *)(p + L.top), d_neg_matrix, max_out, ld_f, s);
}

// ----------------------------------------------------------------------------- stand-alone alignment weights
size_t swx_align_weights_scratch_bytes(int W, int H, int N)
{
    if (W <= 0 || H <= 0 || N <= 0) return 0;
    return align_up((size_t)W * H * N * sizeof(float2)) + align_up((size_t)2 * W * sizeof(int32_t));
}

int swx_align_weights(const float *d_qk, int W, int H, int N, int ld_f, const int32_t *h_n_frames, float qk_scale,
                      int medfilt_width, float *d_neg_matrix, void *d_scratch, size_t scratch_bytes, void *stream)
{
    // stand-alone a7 (test hook / extra_models path).  Like every entry point it allocates nothing: the caller hands in
    // swx_align_weights_scratch_bytes(W, H, N) of device scratch (row statistics + the per-window counts)
    if (W <= 0) return 0;
    if (!d_scratch || scratch_bytes < swx_align_weights_scratch_bytes(W, H, N)) return -8;
    hipStream_t s = S(stream);
    float *rstat = (float *)d_scratch;
    int32_t *cnt = (int32_t *)((unsigned char *)d_scratch + align_up((size_t)W * H * N * sizeof(float2)));
    std::vector<int32_t> hv(2 * W);
    for (int w = 0; w < W; ++w) { hv[w] = N; hv[W + w] = h_n_frames[w]; }
    hipError_t er = hipMemcpyAsync(cnt, hv.data(), hv.size() * 4, hipMemcpyHostToDevice, s);
    if (er == hipSuccess) er = hipStreamSynchronize(s);      // hv is a stack-lifetime staging buffer
    if (er != hipSuccess) return -100 - (int)er;
    return swx_align_weights_launch(d_qk, rstat, nullptr, nullptr, W, H, N, ld_f, cnt, cnt + W, qk_scale, medfilt_width, d_neg_matrix,
                                    N, ld_f, s);
}

}  // extern "C"
