/* swx.h -- C ABI of libswx.so: the MI355X (gfx950) hot path of stable-ts.
 *
 * The reference (jianfch/stable-ts) has NO C ABI / FFI: its hot path is Python that calls the
 * un-vendored dependency openai-whisper (stable_whisper/whisper_compatibility.py:58-76).  The entry
 * points below are the native replacements for exactly the callables the reference's glue consumes
 * at that seam (seam B5); each one cites the reference call site it replaces.
 * INTEGRATION.md shows the ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer named d_* is a DEVICE pointer (HBM); h_* is a host pointer
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream)
 *   - return value: 0 = ok, negative = error (swx_strerror); no call blocks the host unless it says so
 *   - no hidden device allocation: the caller binds the weight arena and the workspace
 *   - compute dtype: SWX_F16 (fp16 storage + MFMA, fp32 accumulate/LN/softmax -- what the reference runs on
 *     a GPU, original_whisper.py:251-260) or SWX_F32 (exact-f32 MFMA; the strict parity mode that matches the
 *     reference's CPU path, which is always fp32)
 */
#ifndef SWX_H
#define SWX_H
#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SWX_F32 0
#define SWX_F16 1

#define SWX_N_SAMPLES 480000   /* whisper_compatibility.py:86  */
#define SWX_N_FRAMES 3000      /* whisper_compatibility.py:87  */
#define SWX_N_FFT 400
#define SWX_HOP 160

typedef struct swx_dims {      /* == whisper.model.ModelDimensions (read via model.dims.*, e.g. alignment.py:181) */
    int32_t n_mels, n_audio_ctx, n_audio_state, n_audio_head, n_audio_layer;
    int32_t n_vocab, n_text_ctx, n_text_state, n_text_head, n_text_layer;
} swx_dims;

typedef struct swx_model swx_model;   /* opaque */

const char *swx_strerror(int code);
int swx_version(void);

/* ---- model lifetime + weights (replaces whisper.load_model + model.to(device), original_whisper.py:995-1002) */
int swx_model_create(const swx_dims *dims, int dtype, swx_model **out);
void swx_model_destroy(swx_model *m);
/* size of the packed weight arena for this model/dtype */
size_t swx_weights_bytes(const swx_model *m);
int swx_bind_weights(swx_model *m, void *d_arena, size_t bytes);
/* a further handle (same dims and dtype) on the arena of `owner`, which stays the owner of the memory: the weights are
 * shared, nothing is cleared; each handle has its own workspace, alignment heads and stream, so host threads can drive
 * them concurrently (stream lanes) or with different head sets */
int swx_share_weights(swx_model *m, const swx_model *owner);
/* copy one checkpoint tensor (upstream state_dict key, fp32, device memory) into its packed slot,
 * converting/re-laying it out (QKV fusion, conv tap-major layout, fp16 cast) on the device */
int swx_load_tensor(swx_model *m, const char *name, const float *d_src, int64_t numel, void *stream);
/* 1 if every slot has been loaded; swx_missing_tensor writes the index-th missing name into buf (returns 0 at the end) */
int swx_weights_complete(const swx_model *m);
int swx_missing_tensor(const swx_model *m, int index, char *buf, int buflen);
/* the arena was filled from outside (rank 0's packed arena received over RCCL, parallel.py::broadcast_arena): mark every
 * tensor as present.  swx_weights_finalize: load-time preparation that depends on the complete set of tensors (the
 * LayerNorm-folded copies of the decoder projections the fused f16 decode step streams, csrc/swx_fold.hip); must be
 * called once after the last swx_load_tensor / after swx_weights_mark_loaded, before swx_decode. */
int swx_weights_mark_loaded(swx_model *m);
int swx_weights_finalize(swx_model *m, void *stream);
/* alignment heads (timing.py:105 reads model.alignment_heads.indices()): pairs (layer, head) */
int swx_set_alignment_heads(swx_model *m, const int32_t *h_layer_head_pairs, int n_pairs);
int swx_num_alignment_heads(const swx_model *m);

/* ---- workspace: max_windows = windows processed together by encode/score, max_rows = decoder sequences */
size_t swx_workspace_bytes(const swx_model *m, int max_windows, int max_rows);
int swx_bind_workspace(swx_model *m, void *d_ws, size_t bytes, int max_windows, int max_rows);

/* ---- a1: log-mel (replaces whisper.audio.log_mel_spectrogram at original_whisper.py:528-530, alignment.py:410-413)
 * d_pcm:  f32 [B][480000]  (caller zero-pads each <=30 s segment to exactly 480000 samples, as the reference does)
 * d_mel:  f32 [B][n_mels][3000]; the clamp floor uses the max over the WHOLE batch when per_item_max==0
 *         (upstream quirk inherited by refine) and per window when per_item_max!=0 */
int swx_log_mel(swx_model *m, const float *d_pcm, int B, float *d_mel, int per_item_max, void *stream);

/* log-mel of segments that are NOT zero-padded to 30 s, followed by pad_or_trim(mel, 3000): refine's inference
 * (alignment.py:660-661, padding 0) and locate (alignment.py:924-925, padding 201).
 * d_pcm f32 [B][480000] (only the first n_valid[b] samples of a row are read); n_valid / n_total: HOST int32 [B],
 * n_total = n_valid + the zero padding upstream appends (200 < n_total, n_total/160 <= 3008, n_valid <= 480000).
 * Frames t < n_total/160 are upstream's (reflection about n_total, clamp floor from the per-item max over all
 * n_total/160 frames, also those past 3000; over the whole batch when per_item_max==0, which is what upstream's
 * batched call in refine does); frames >= n_total/160 are 0.0.  Returns -2 on a length out of range. */
int swx_log_mel_ragged(swx_model *m, const float *d_pcm, const int32_t *n_valid, const int32_t *n_total, int B,
                       float *d_mel, int per_item_max, void *stream);
/* the same with the clamp floor shared by every `group` CONSECUTIVE items (B % group == 0, else "invalid argument"): refine in
 * lockstep puts the two audio copies of several word groups into one batch, and upstream's batched call takes the floor from
 * the pair (alignment.py:660).  group == 1 is per_item_max != 0, group == B is per_item_max == 0, bit for bit. */
int swx_log_mel_ragged_grouped(swx_model *m, const float *d_pcm, const int32_t *n_valid, const int32_t *n_total, int B,
                               float *d_mel, int group, void *stream);

/* ---- a2: encoder (replaces model.encoder(mel), decode.py:27-30, timing.py:59-60)
 * d_mel f32 [B][n_mels][3000] -> d_xa [B][1500][d] in the compute dtype */
int swx_encode(swx_model *m, const float *d_mel, int B, void *d_xa, void *stream);

/* ---- cross-attention K/V of every decoder layer for B windows (upstream recomputes them lazily through the
 * kv-cache hooks; here they are produced once per window and shared by decode + scoring)
 * d_xkv: compute dtype [L][B][ K: 1500 x d row-major | V^T: d x 1536 (per head [64][1536], keys contiguous, zero padded) ]
 *        (the decode-step cross-attention streams both operands as coalesced 16-byte MFMA fragments) */
size_t swx_cross_kv_bytes(const swx_model *m, int B);
int swx_cross_kv(swx_model *m, const void *d_xa, int B, void *d_xkv, void *stream);

/* ---- a3/a4: decoding (replaces DecodingTaskStable._main_loop, decode.py:33-65, and the upstream logit filters +
 * GreedyDecoder / BeamSearchDecoder it drives).  One decode job = W windows x G sequences per window
 * (G = beam_size or best_of or 1), all advanced in lockstep on the device, no per-step host sync. */
typedef struct swx_decode_cfg {
    int32_t n_windows;            /* W */
    int32_t n_group;              /* G */
    int32_t beam;                 /* 0 = greedy/sampling (GreedyDecoder), 1 = beam search (BeamSearchDecoder) */
    float temperature;            /* 0 = argmax */
    float patience;               /* beam: max_candidates = round(G * patience); <=0 -> 1.0 */
    int32_t sample_len;           /* max sampled tokens (n_text_ctx/2 = 224 by default) */
    int32_t sample_begin;         /* len(initial_tokens) of every window (per window: sample_begins below) */
    int32_t sot_index;            /* index of <|startoftranscript|> in the initial tokens */
    int32_t suppress_blank;       /* SuppressBlank */
    int32_t apply_timestamp_rules;/* ApplyTimestampRules (0 when without_timestamps) */
    int32_t max_initial_timestamp_index; /* -1 = None (stable-ts forces None, original_whisper.py:262-263) */
    int32_t eot, sot, no_timestamps, timestamp_begin, no_speech, blank_token; /* tokenizer ids (blank = encode(" ")[0]) */
    int32_t n_suppress;           /* SuppressTokens list length */
    int32_t min_tokens;           /* >0: EOT is suppressed until this many tokens were sampled (synthetic-weights
                                     benchmarking only; 0 = reference behaviour) */
    uint64_t seed;                /* sampling RNG seed (temperature > 0) */
    const int32_t *window_uid;    /* HOST array [W] or NULL: a stable identity of every window (e.g. its seek position).
                                     Sampling contract (temperature > 0): the draw of a sequence is a counter-based hash of
                                     (seed, window uid, slot within the window's group, step, token id) -- Gumbel-max over the
                                     filtered logits / T, i.e. a Categorical(logits / T) sample like upstream's GreedyDecoder,
                                     but NOT the reference's (framework Philox) random stream: a T > 0 retry is reproducible for a given (seed, uid)
                                     whatever the batch it is decoded in, and is not token-identical with the reference's.
                                     The variate by the top 24 bits k of the 32-bit hash word: u_k = (k + 0.5) * 2^-24, added
                                     to logits / T is -ln(-ln u_k) -- finite for every word (f32 holds u below 1 in the top
                                     bucket), so a masked id is never drawn.  The hash keys a row on uid * 0x9E3779B1 + slot.
                                     NULL: the row's index in this job is its key. */
    const float *noise;           /* DEVICE array [sample_len][W * G][n_vocab] f32 or NULL.  Non-NULL (greedy decoder, temperature > 0):
                                     the draw of row r at step t is argmax_i(logits[i] / T - log(noise[t][r][i])): upstream's
                                     Categorical(logits / T).sample() is a multinomial draw of one sample, which the framework
                                     computes as argmax(p / q) with q ~ Exp(1).  When the caller fills the array from the
                                     framework's generator -- one exponential call per step on [W * G][n_vocab], as the
                                     reference's decoding loop makes them -- the sampled tokens are the reference's for the
                                     same seed; the counter-based hash above is not used.  HBM cost: sample_len * W * G * n_vocab
                                     * 4 bytes (232 MB for large-v3 at sample_len 224, best_of 5), read once per step. */
    const int32_t *sample_begins; /* HOST array [W] or NULL: len(initial_tokens) of every window -- a RAGGED job, e.g. the windows of
                                     several recordings that each carry their own prompt.  NULL: every window has `sample_begin`
                                     tokens (arrays whose entries all agree are that job too: the same launches, the same captured
                                     graph).  With the array `sample_begin` is ignored and d_init_tokens is
                                     [W][max_w sample_begins[w]], rows padded with `eot`.  Every window computes what it computes
                                     as a job of its own: the step counter is shared (all windows sample their token i in the same
                                     unit), positions, the timestamp rules' view of tokens[sample_begin:], lengths and the
                                     context-full exit (decode.py:60: a window stops after sampling token
                                     n_text_ctx - sample_begins[w] and is finalized as at a loop exit, the others go on) are per
                                     window.  The job ends when every window is finished or context-full, or sample_len is used up.
                                     Each entry in [1, n_text_ctx], else "invalid argument". */
    const int32_t *sot_indices;   /* HOST array [W] or NULL (= `sot_index` for every window): index of <|startoftranscript|> in
                                     every window's initial tokens, in [0, sample_begins[w]), else "invalid argument" */
} swx_decode_cfg;

/* runs the whole loop; outputs (device):
 *  d_tokens_out  int32 [W][G_out][n_ctx+1]   final sequences incl. the initial tokens, eot-padded
 *  d_lens_out    int32 [W][G_out]            length up to (excluding) the first eot after the window's sample_begin
 *  d_sumlp_out   f32   [W][G_out]            sum_logprobs of each candidate
 *  d_nospeech    f32   [W]                   softmax(logits[sot_index])[no_speech] at step 0 (decode.py:42-44)
 *  G_out = G (greedy/best-of) or max(G, max_candidates) (beam)
 * inputs: d_init_tokens int32 [W][sample_begin] ([W][longest window], eot-padded, with cfg->sample_begins); d_suppress int32 [n_suppress];
 *         d_ts_mask uint8 [W][1501] or NULL (decode.py:14-16,54); d_xkv from swx_cross_kv for these W windows.
 * In a ragged job d_tokens_out[w] holds window w's own initial tokens followed by its samples (no padding in between).
 * Returns the number of steps executed (>=0) or a negative error.  Blocks until the loop has finished. */
int swx_decode(swx_model *m, const swx_decode_cfg *cfg, const int32_t *d_init_tokens, const int32_t *d_suppress,
               const uint8_t *d_ts_mask, const void *d_xkv, int32_t *d_tokens_out, int32_t *d_lens_out,
               float *d_sumlp_out, float *d_nospeech, void *stream);
int swx_decode_gout(const swx_decode_cfg *cfg);

/* ---- a6+a7: teacher-forced scoring pass + alignment matrix (replaces timing.py:41-67 _compute_qks and
 * timing.py:70-112 _compute_atten_weights + the head-mean/negation of timing.py:194-195)
 * For each window w: tokens d_tokens[w][0..n_tok[w]) = [*sot_sequence, no_timestamps, *text_tokens, eot].
 *  d_token_probs  f32 [W][max_n]      softmax(logits[n_sot-1+i? see DESIGN.md][:eot])[text_token_i], T values per window
 *  d_neg_matrix   f32 [W][max_n][1500] rows 0..T (T+1 rows), cols 0..n_frames[w): -(mean over alignment heads of
 *                 median7(znorm_tokens(softmax_frames(qk * qk_scale)))) -- the DTW input
 *  n_sot = len(sot_sequence); T[w] = n_tok[w] - n_sot - 2 */
int swx_score(swx_model *m, const int32_t *d_tokens, const int32_t *h_n_tok, int W, int max_n, int n_sot, int eot,
              const int32_t *h_n_frames, float qk_scale, int medfilt_width, const void *d_xkv,
              float *d_token_probs, float *d_neg_matrix, void *stream);

/* raw attention scores of the configured alignment heads from the same teacher-forced pass (what timing.py:41-67
 * _compute_qks hooks out of every cross-attention layer): a test / inspection hook since round 3 -- the head-selection variants
 * no longer materialise per-head scores (swx_score_q / swx_heads_* below).
 *  d_qk f32 [W][n_align][n_rows][1500]: (q * scale) . (k * scale) of token rows row0 .. row0+n_rows-1 (row0 + n_rows <= max_n),
 *       heads in the order of swx_set_alignment_heads sorted by (layer, head); pre-softmax, qk_scale not applied
 *  d_token_probs as in swx_score, or NULL */
int swx_score_qk(swx_model *m, const int32_t *d_tokens, const int32_t *h_n_tok, int W, int max_n, int n_sot, int eot,
                 int row0, int n_rows, const void *d_xkv, float *d_token_probs, float *d_qk, void *stream);

/* ---- head-selection variants of the alignment stage (reference: stable_whisper/timing.py:87-103 `dynamic_heads`,
 * :115-163 `aligner='new'`, :177-189 `extra_models`; csrc/swx_headsel.hip).  The reference hooks the scores of EVERY head out
 * of the pass ([L*H][tokens][1500] f32, 0.4-1.7 GB for large-v3) and runs tensor expressions over them; here the pass keeps
 * the cross-attention QUERIES of every layer and the kernels recompute a head's score row from q and the window's cross-K.
 *
 * swx_score_q: the teacher-forced pass of ONE window (timing.py:41-67).  d_q receives [n_text_layer][max_n][d] in the compute
 *   dtype (swx_qcap_bytes); d_token_probs as in swx_score (or NULL); d_xkv = the cross-K/V of that single window.
 * swx_heads_dynamic: rows row0 .. row0+n_rows-1; per row the `count` heads with the smallest sum_f |peak - f| / 1500 * p[f]
 *   (peak = the row's own argmax, or d_peaks[i] = the previous DTW pass's jump midpoint, f64); d_qk_sel f32
 *   [count][n_rows][ld_f] receives their RAW scaled scores = the input of swx_align_weights (H = count, N = n_rows).
 * swx_heads_new: over the n_tok rows: median filter -> * qk_scale -> softmax per head; score = w_colnorm * sum_f ||w[:, f]|| +
 *   w_rownorm * sum_i ||w[i, :]|| - w_coverage * penalty; the topk heads, column-normalised and averaged; d_neg_matrix f32
 *   [n_out][ld_f] receives MINUS that mean for rows row0 .. row0+n_out-1 (the DTW input).
 * swx_weighted_sum: d_out[e] = sum_j h_coef[j] * h_xs[j][e] (n_in <= 8 device arrays): pooling several models' head means.
 * d_scratch: swx_heads_scratch_bytes(m, max_n) of device memory; nothing is allocated inside. */
size_t swx_qcap_bytes(const swx_model *m, int max_n);
int swx_score_q(swx_model *m, const int32_t *d_tokens, const int32_t *h_n_tok, int max_n, int n_sot, int eot,
                const void *d_xkv, float *d_token_probs, void *d_q, void *stream);
size_t swx_heads_scratch_bytes(const swx_model *m, int max_n);
int swx_heads_dynamic(swx_model *m, const void *d_q, int max_n, int row0, int n_rows, const void *d_xkv, int n_frames,
                      float qk_scale, int count, const double *d_peaks, float *d_qk_sel, int ld_f, void *d_scratch,
                      size_t scratch_bytes, void *stream);
int swx_heads_new(swx_model *m, const void *d_q, int max_n, int n_tok, int row0, int n_out, const void *d_xkv, int n_frames,
                  float qk_scale, int medfilt_width, int topk, float w_colnorm, float w_rownorm, float w_coverage,
                  float *d_neg_matrix, int ld_f, void *d_scratch, size_t scratch_bytes, void *stream);
int swx_weighted_sum(const float *const *h_xs, const float *h_coef, int n_in, float *d_out, int64_t n, void *stream);

/* ---- the same stage for W windows of one batch in one call each (the kernels carry a window axis; a window's numbers are the
 * bits the single-window calls above give it).  Token counts h_n_tok[w] <= max_n and frame counts h_n_frames[w] (clamped to
 * [1, n_audio_ctx] inside) are ragged; the text-token rows of window w are n_sot .. n_tok[w] - 2 (max_rows = max_n - n_sot - 1).
 *
 * Cross-K/V: read IN PLACE from a batch buffer of xkv_W windows ([L][xkv_W][chunk], swx_cross_kv): d_xkv points at the chunk
 *   of the FIRST of the W windows in layer 0; layer stride = xkv_W chunks, window stride = one chunk.  xkv_W = 0 means W.
 * swx_score_q_batch: d_tokens int32 [W][max_n] (rows padded with eot), d_q receives [n_text_layer][W][max_n][d] in the compute
 *   dtype (swx_qcap_batch_bytes), d_token_probs f32 [W][max_n] or NULL.  Refuses (-1) a window with n_tok - n_sot - 2 < 0.
 *   Needs a workspace bound for >= W windows.
 * swx_heads_dynamic_batch: score -> pick -> gather -> z-normalisation / median / head mean (swx_align_weights' kernels) in one
 *   call; d_peaks f64 [W][max_rows] (the previous DTW pass's jump midpoints) or NULL (every row's own peak); d_neg_matrix f32
 *   [W][max_rows][ld_f] (ld_f = n_audio_ctx) receives the NEGATED matrix: rows < n_tok[w] - n_sot - 1 and frames < n_frames[w]
 *   of window w are written, nothing else.
 * swx_heads_new_batch: the same output layout for aligner = 'new' (options as swx_heads_new).
 * d_scratch: swx_heads_batch_scratch_bytes(m, W, max_n, count) of device memory (count = 0 for swx_heads_new_batch): the
 *   per-window counts, head scores and picks, column norms, and for count > 0 the gathered scores [W][count][max_rows][n_audio_ctx]
 *   with their row statistics.  Nothing is allocated inside.
 * Errors: -1 null / out-of-range arguments, -2 / -3 from the launchers (shape / median width), -8 short scratch or workspace. */
size_t swx_qcap_batch_bytes(const swx_model *m, int W, int max_n);
int swx_score_q_batch(swx_model *m, const int32_t *d_tokens, const int32_t *h_n_tok, int W, int max_n, int n_sot, int eot,
                      const void *d_xkv, int xkv_W, float *d_token_probs, void *d_q, void *stream);
size_t swx_heads_batch_scratch_bytes(const swx_model *m, int W, int max_n, int count);
int swx_heads_dynamic_batch(swx_model *m, const void *d_q, int W, int max_n, int n_sot, const int32_t *h_n_tok,
                            const int32_t *h_n_frames, const void *d_xkv, int xkv_W, float qk_scale, int medfilt_width, int count,
                            const double *d_peaks, float *d_neg_matrix, int ld_f, void *d_scratch, size_t scratch_bytes,
                            void *stream);
int swx_heads_new_batch(swx_model *m, const void *d_q, int W, int max_n, int n_sot, const int32_t *h_n_tok,
                        const int32_t *h_n_frames, const void *d_xkv, int xkv_W, float qk_scale, int medfilt_width, int topk,
                        float w_colnorm, float w_rownorm, float w_coverage, float *d_neg_matrix, int ld_f, void *d_scratch,
                        size_t scratch_bytes, void *stream);

/* full-sequence logits of a teacher-forced pass (model(mel, tokens) as used by refine/locate; also a test hook):
 * d_logits f32 [W][max_n][n_vocab].  Language detection (model.detect_language, original_whisper.py:329) is this call
 * with tokens = [[sot]]. */
int swx_forward_logits(swx_model *m, const int32_t *d_tokens, const int32_t *h_n_tok, int W, int max_n,
                       const void *d_xkv, float *d_logits, void *stream);

/* the same pass reduced to what refine's bisection reads (non_whisper/refinement.py:289-327): for every window w and row
 * j < n_tok[w] - 1, with x = the logits row swx_forward_logits defines and t = d_tokens[w][j + 1],
 *  d_prob f32   [W][max_n]  softmax(x[:n_vocab_used])[t] -- the arithmetic of swx_score's d_token_probs
 *  d_rank int32 [W][max_n]  #{v < n_vocab_used : x_v < x_t or (x_v == x_t and v < t)}: the position of t in an ascending sort
 *                           of the row on (logit, index), a total order.  The reference sorts the f32 PROBABILITIES with an
 *                           unstable sort; the two differ only where rounding to f32 probabilities ties another entry with the
 *                           target itself, and there the reference's position is arbitrary.
 * A target outside [0, n_vocab_used) gives prob 0, rank -1; entries j >= n_tok[w] - 1 are not written.  Output is O(W * max_n):
 * the projection runs in row chunks through the bound workspace and a reduction kernel finishes each chunk.  A window's
 * values do not depend on the batch it runs in. */
int swx_forward_token_ranks(swx_model *m, const int32_t *d_tokens, const int32_t *h_n_tok, int W, int max_n, int n_vocab_used,
                            const void *d_xkv, float *d_prob, int32_t *d_rank, void *stream);

/* the same pass reduced to what locate's greedy step reads (alignment.py:988-1010): for window w, x = the logits row
 * swx_forward_logits defines at position h_n_tok[w] - 1, restricted to ids 0 .. eot, with x[v] = -inf for every v in d_suppress
 * (ids outside [0, eot) in that list are ignored; d_suppress may be NULL when n_suppress == 0).
 *  d_top  int32 [W][2]  the largest and the second-largest entry of x[0 .. eot] in the total order on (logit, index) -- the order
 *                       of swx_forward_token_ranks; a tie goes to the higher index (the reference's unstable sort picks arbitrarily)
 *  d_prob f32   [W][3]  p = softmax(x[0 .. eot - 1]) (EOT excluded) at { d_target[w], d_top[w][0], d_top[w][1] }; 0 where the id
 *                       is outside [0, eot) (a target of -1, a top id equal to eot).  The arithmetic of d_token_probs.
 * Only the last row of every window goes through the final LayerNorm and the vocabulary projection (W rows, in fixed chunks of
 * 64 rows as in swx_forward_token_ranks: for M <= 64 the projection is one kernel on a grid that depends on n_vocab alone), and
 * one launch of the reduction finishes all W rows: no [W][max_n][n_vocab] tensor, 5 numbers per window out.  A pass with
 * max_n == 1 runs as a two-token pass (the token repeated; causal, so row 0 is unchanged), so that which kernels compute a window
 * never depends on the other windows: a window's outputs do not depend on the batch it runs in.  Only enqueues.  A NaN logit is
 * never selected (every comparison with it is false; the reference's sort ranks it highest).  Errors (nothing is launched): no
 * weights or workspace bound (-9); a null pointer, eot <= 0, eot >= n_vocab, n_suppress < 0, a token count outside [1, max_n]
 * (-1); max_n <= 0, a token row that is not a multiple of 16 bytes, a suppress mask beyond 48 KB of LDS (eot >= 393 184) (-2); W
 * above the bound workspace's windows (-8). */
int swx_forward_next_token(swx_model *m, const int32_t *d_tokens, const int32_t *h_n_tok, int W, int max_n, int eot,
                           const int32_t *d_suppress, int n_suppress, const int32_t *d_target,
                           const void *d_xkv, int32_t *d_top /*[W][2]*/, float *d_prob /*[W][3]*/, void *stream);

/* language identification on cross-K/V that is already resident (model.detect_language without the vocabulary projection):
 * the teacher-forced pass of the single token `sot` for W windows -- the pass swx_forward_logits makes with max_n = 1, through
 * the final LayerNorm, in the bound workspace -- then, per window, x_j = dot(hidden[w], E[d_lang_tokens[j]]) (f32 accumulation
 * in both dtypes), softmax over the n_lang values and the arg-max (ties: the lowest j).
 *  d_probs f32   [W][n_lang]   the probabilities, in the order of d_lang_tokens
 *  d_best  int32 [W]           the token id of the most probable language
 * Only enqueues: no allocation, no synchronisation, no [W][n_vocab] tensor; launch shapes depend on (W, n_lang, n_text_state),
 * and a window's values do not depend on the batch it runs in.  Errors (nothing is launched): n_lang <= 0 or > n_vocab, `sot`
 * outside the vocabulary, a null pointer (-1); W above the bound workspace's windows (-8).  The ids in d_lang_tokens are device
 * memory: one outside [0, n_vocab) is never dereferenced and gets probability 0; callers check their list before uploading
 * it. */
int swx_detect_language(swx_model *m, const void *d_xkv, int W, int sot, const int32_t *d_lang_tokens, int n_lang,
                        float *d_probs, int32_t *d_best, void *stream);

/* ---- a7 stand-alone (test hook + extra_models path): weights f32 [W][H][N][ld_f] raw qk ->
 * neg_matrix f32 [W][N][1500].  d_scratch: swx_align_weights_scratch_bytes(W, H, N) bytes of device memory (no entry point of
 * this library allocates device memory) */
size_t swx_align_weights_scratch_bytes(int W, int H, int N);
int swx_align_weights(const float *d_qk, int W, int H, int N, int ld_f, const int32_t *h_n_frames, float qk_scale,
                      int medfilt_width, float *d_neg_matrix, void *d_scratch, size_t scratch_bytes, void *stream);

/* ---- whisper.timing.median_filter (timing.py:110,138): f32 [rows][n] -> [rows][n], reflect padding */
int swx_median_filter(const float *d_x, int64_t rows, int n, int width, float *d_out, void *stream);

/* ---- device half of the non-VAD silence analysis (stabilization/nonvad.py:16-39 audio2loudness), on the PCM that is resident
 * for the spectrogram.  d_pcm f32 [W] windows pcm_stride samples apart; d_nk int32 [W][2] = {valid samples n, k};
 * d_idx int32 [W][n_idx] sample indices; d_out f32 [W][1 + n_idx]: out[w][0] = the k-th largest |x| of the window (the value
 * of the reference's `topk(|x|, k).values[-1]`, nonvad.py:22, found by a radix select: an element of the input, no arithmetic; NaN when
 * k == 0), out[w][1 + j] = |x[idx[w][j]]| (0 for an index outside [0, n)).  The floating-point part of the analysis stays in
 * host code on these values (stable_ts_amd/stabilization.py::loudness_from_probe). */
int swx_loudness_probe(const float *d_pcm, int64_t pcm_stride, const int32_t *d_nk, const int32_t *d_idx, int n_idx, int W,
                       float *d_out, void *d_scratch, size_t scratch_bytes, void *stream);
/* d_scratch (>= swx_loudness_probe_scratch_bytes(W) bytes, or NULL): with it and fewer than 16 windows the selection runs spread over
 * the chip (a forced-alignment pass analyses one window per call); without it one workgroup per window.  The same element either way. */
size_t swx_loudness_probe_scratch_bytes(int W);

/* ---- probe audio that stays on the device (refine_many): the edits of one bisection round applied to the probe rows in one launch.
 * d_probe f32 [n_rows] rows `stride` samples apart; probe row r belongs to clean row r >> 1 of d_clean f32 [(n_rows + 1) / 2] rows of
 * the same stride.  d_ops int32 [n_ops][4] = {row, a, b, kind} in DEVICE memory, stably sorted by row; d_row_start int32
 * [n_rows + 1] (device) = the offset of every row's ops in that list.  kind 0 writes +0.0f to [a, b) of the row, kind 1 copies
 * [a, b) from the row's clean row.  The ops are ordered writes: for every sample the LAST op of its row that covers it decides
 * its bits, a sample that no op covers keeps its bits.  An op whose row is not the row it is listed under (any row outside
 * [0, n_rows) is such an op) or whose kind is unknown is ignored; a, b are clamped to [0, stride]; nothing outside the two buffers
 * is dereferenced.  n_ops == 0 launches nothing.  The call only enqueues on `stream`: no synchronisation, no allocation. */
int swx_pcm_edit(const float *d_clean, float *d_probe, int64_t stride, int n_rows, const int32_t *d_ops,
                 const int32_t *d_row_start, int n_ops, void *stream);

/* ---- denoiser="noisereduce": non-stationary spectral gating of PCM on the device (csrc/swx_denoise.hip; the reference hands the
 * audio to the noisereduce package, stable_whisper/audio/noisereduce.py:38-87).  The statement that is implemented -- STFT with a
 * periodic Hann window, a moving mean of |X| over n_mean frames, a sigmoid mask, a triangular smoothing of the mask over
 * (2 n_grad_freq + 1) x (2 n_grad_time + 1) bins, inverse STFT, NaN -> 0 and +-inf -> +-FLT_MAX -- is written out in DESIGN.md
 * section 8.  d_pcm f32 [rows] rows pcm_stride samples apart, n >= 1 samples each, independent signals (the channels of a
 * recording); d_out f32 the same shape, out_stride apart, must not overlap d_pcm.  Arithmetic is f32; the output is the same bits
 * for every block size, row count and run.  d_scratch: swx_spectral_gate_scratch_bytes(rows, cfg) bytes, 16-byte aligned; the size
 * does not depend on n (the recording is walked in blocks of frames).  No model handle, no allocation, no host synchronisation,
 * every launch on `stream`.  A bad argument (a cfg outside the ranges below, too little scratch, overlapping buffers) returns
 * "invalid argument" before any launch. */
typedef struct swx_gate_cfg {
    int32_t n_fft;          /* 256, 512 or 1024; hop = n_fft / 4, window = n_fft */
    int32_t n_mean;         /* M >= 1: frames of the moving mean, (M - 1) / 2 of them before the frame */
    float   thresh, slope, prop_decrease;
    int32_t n_grad_freq, n_grad_time;   /* 1 .. 128 each; both 0 = no smoothing */
} swx_gate_cfg;
size_t swx_spectral_gate_scratch_bytes(int rows, const swx_gate_cfg *cfg);   /* 0 for a bad argument */
int swx_spectral_gate(const float *d_pcm, int64_t pcm_stride, int rows, int64_t n, const swx_gate_cfg *cfg, float *d_out,
                      int64_t out_stride, void *d_scratch, size_t scratch_bytes, void *stream);
/* tests only: output hops per block of the walk (0 = the default); changes swx_spectral_gate_scratch_bytes, never the output */
int swx_test_spectral_gate_block(int frames_per_block);

/* ---- f2 audio front-end: FLAC decoding on the HOST (no device work; csrc/swx_flac.hip).  The reference pipes every container
 * through an `ffmpeg -f s16le` child process (stable_whisper/audio/utils.py:63-125); offline boxes have no ffmpeg and the
 * reference's only real-speech fixture is test/jfk.flac, so native FLAC streams are decoded here: STREAMINFO + frames with
 * CONSTANT / VERBATIM / FIXED / LPC subframes, Rice / Rice2 residuals with escapes, wasted bits, left-side / side-right /
 * mid-side stereo, 4-32 bits per sample, up to 8 channels; CRC-8 and CRC-16 of every frame are verified.
 * swx_flac_probe: STREAMINFO only.  swx_flac_decode: h_out int32 [capacity_frames][channels] interleaved (sample values at the
 * stream's bit depth, not scaled), or NULL to count; returns the number of inter-channel sample frames decoded, or a negative
 * error (-20 not a FLAC stream, -21 corrupt stream / CRC mismatch, -22 unsupported stream, -23 truncated stream).  The MD5 in
 * `info` is the encoder's signature of the unencoded samples; the caller checks it (stable_ts_amd/audio_io.py::read_flac). */
typedef struct swx_flac_info {
    int32_t sample_rate, channels, bits_per_sample, min_block, max_block;
    int64_t total_samples;        /* per channel; 0 = unknown */
    uint8_t md5[16];
} swx_flac_info;
int swx_flac_probe(const uint8_t *h_data, size_t n_bytes, swx_flac_info *info);
int64_t swx_flac_decode(const uint8_t *h_data, size_t n_bytes, int32_t *h_out, int64_t capacity_frames, swx_flac_info *info);

/* ---- a8: DTW + backtrace (replaces whisper.timing.dtw at timing.py:195; CPU tie-break)
 * d_x f32 [W][ld_n][ld_m] (row-major; window w uses rows 0..N[w), cols 0..M[w));
 * outputs int32 [W][ld_n+ld_m] text/time indices in forward order and int32 [W] path lengths.
 * d_trace_ws: uint8 scratch of swx_dtw_workspace_bytes(W, ld_n, ld_m) */
size_t swx_dtw_workspace_bytes(int W, int ld_n, int ld_m);
int swx_dtw(const float *d_x, int W, int ld_n, int ld_m, const int32_t *d_N, const int32_t *d_M,
            int32_t *d_text_idx, int32_t *d_time_idx, int32_t *d_len, void *d_trace_ws, void *stream);

/* ---- measurement: per-kernel-class HIP-event timing on the launch stream (bench.py's roofline object).
 * classes: 0 gemm tiled (work=flops) 1 gemm skinny (bytes) 2 flash attention (flops) 3 rowwise attention (bytes)
 *          4 cached self-attention 5 select/beam 6 mel 7 align-weights 8 dtw 9 layernorm
 * swx_prof_collect: out[cls*3+{0,1,2}] = {launches, total ms, total algorithmic work}; returns the class count */
int swx_prof_enable(int on);
/* A/B switches for tests and scripts (SWX_FLAG_* = 1 << bit, all of them in SWX_FLAG_TABLE in csrc/swx_kernels.h, which fails the
 * build when two share a bit; bits 0..30 only, because a negative argument is the query): 1 = decode steps and small passes through the general
 * per-op path instead of the fused "dec" step (its reference), 2048 = decode cross-attention on the row-layout K / V^T
 * (reference of the fragment-ordered copy), 8192 = memory-walking logit filters (reference of the register kernel),
 * 16384 = decode loop without the captured step graph, 32768 = decode step without the cache prefetch of the next projection's
 * weights, 65536 / 131072 = tiled GEMM never on the ring / the 256 x 256 kernel (bit-identical either way), 2097152 = the decode step's
 * K-split projection reduces its slabs inside the GEMM launch (arrival tickets; bit-identical, measured slower in round 5),
 * 67108864 = f16 flash attention on round 6's software-pipelined tile (bit-identical, measured slower).  Default 0; nothing reads an environment variable.
 * flags < 0 only queries.  Returns the previous value. */
int swx_debug_flags(int flags);
int swx_prof_collect(double *out, int n_classes);
/* how swx_decode ran on this handle so far: out[0] = two-step graphs captured, out[1] = graph replays (2 decode steps each),
 * out[2] = decode steps launched eagerly, out[3] = 1 if a capture / replay failed at least once on this handle (that job ran
 * eagerly; the handle keeps trying graphs for later jobs and switches replay off for good after the third failure) */
int swx_graph_stats(const swx_model *m, int64_t *out);

/* ---- building blocks exported for the parity tests (same kernels the calls above launch) */
int swx_test_gemm(int dtype, const void *d_a, int64_t lda, const void *d_w, const float *d_bias, const void *d_res,
                  void *d_c, int64_t ldc, int M, int N, int K, int epilogue, int force_kernel, void *stream);
/* which f16 kernel swx_test_gemm's launch would get (host-only, no GPU): 0 register-staged tiled, 1 skinny, 2 / 3 direct-to-LDS
 * with 128 / 64-column tiles, 4 / 5 the LDS-DMA ring at 64 / 128 columns, 6 the 256 x 256 two-stage kernel; < 0: not offered */
int swx_test_gemm_plan(int M, int N, int K, int epilogue, int force_kernel, int flags);
/* decode-step "dec" GEMM (csrc/swx_decstep.hip), f16: epilogue bits 1 = LayerNorm fold (gamma / beta given, A = raw rows, K = full
 * row), 2 = GELU, 4 = residual update of d_x in place, 8 = QKV scatter (columns >= d go to the caches at pos0[m]), 16 = K-split
 * allowed, 64 = a multi-token pass (from 161 rows on the launch takes the tall kernel: register-resident weights, 16-row tiles; with
 * 8, rows are 7 tokens per sequence; bit-identical to the launch without it).  d_scratch: >= N*K*2 + 8N + slab bytes + 1 KiB. */
int swx_test_dec_gemm(const void *d_a, int64_t lda, const void *d_w, const float *d_gamma, const float *d_beta,
                      const float *d_bias, void *d_c, int64_t ldc, void *d_x, void *d_kcache, void *d_vcache,
                      const int32_t *d_pos0, int n_ctx, int d, int M, int N, int K, int epilogue, void *d_scratch,
                      size_t scratch_bytes, void *stream);
int swx_test_layernorm(int dtype, const void *d_x, const float *d_g, const float *d_b, void *d_y, int rows, int d,
                       void *stream);
/* vt_kp > 0: d_v is transposed per batch item, [H][64][vt_kp] (keys contiguous, zero padded) -- the cross-KV layout */
int swx_test_attention(int dtype, const void *d_q, int64_t ldq, const void *d_k, const void *d_v, int64_t ldkv,
                       void *d_o, int64_t ldo, int B, int H, int nq, int nk, int force_kernel, int vt_kp, void *stream);

/* swx_test_gemm with the arguments of the layout epilogues (csrc/swx_kernels.h: GemmArgs).  `epilogue` bits beyond swx_test_gemm's
 * 1 bias, 2 GELU, 4 residual d_res (row stride ldc), 8 f32 output:
 *   16  + d_resf[(m % res_mod)][n], f32 [res_mod][N] (the positional embedding behind conv2)
 *   64  C rows grouped in batch items of vt_s rows: row m at d_c + (m / vt_s) * vt_bs + (m % vt_s) * ldc
 *   32  C transposed per head: element (m, n) at d_c + (m / vt_s) * vt_bs + n * vt_kp + m % vt_s (n = head * 64 + dim)
 *   128 f16: columns [0, N/2) as 64 into d_c, columns [N/2, N) as 32 into d_c2 (column counted from N/2); with d_p also the
 *       fragment-ordered copy of both halves (batch item b at d_p + b * p_bs, per head ceil(vt_s / 32) * 4096 halfs,
 *       keys [vt_s, p_nkpad) zeroed; p_nkpad = vt_s rounded up to 32, p_vcol0 = N/2)
 *   256 f16: columns [0, 2N/3) plain into d_c, columns [2N/3, N) as 32 into d_c2; vt_zero_pad: keys [vt_s, vt_kp) of d_c2 zeroed
 * lda < K is allowed (the convolutions run as GEMMs over overlapping rows).  force_kernel goes to the launcher unchanged.  Returns -1
 * for a missing argument and -2 / -4 for a combination no kernel implements (nothing is launched): two layout bits at once; 128 / 256
 * in f32, on the skinny kernel, with a column split that is no multiple of the planned kernel's tile width, or with vt_s, vt_kp, vt_bs
 * or M no multiple of 4; d_p without 128 or with ldc, vt_bs or p_bs no multiple of 8; vt_zero_pad without 256. */
int swx_test_gemm_layout(int dtype, const void *d_a, int64_t lda, const void *d_w, int64_t ldw, const float *d_bias, const void *d_res,
                         const float *d_resf, int res_mod, void *d_c, int64_t ldc, void *d_c2, void *d_p, int64_t p_bs, int p_nkpad,
                         int p_vcol0, int vt_s, int vt_kp, int64_t vt_bs, int vt_zero_pad, int M, int N, int K, int epilogue,
                         int force_kernel, void *stream);
/* the stand-alone packer of the fragment-ordered cross-K/V copy (f16): d_k [B][nk][ldk] rows, d_vt [B][H][64][vt_kp] (zero padded past
 * nk), d_packed [B][H][per_head]; all three with `batch_stride` elements between batch items.  vt_kp >= nk rounded up to 32. */
int swx_test_xkv_pack(const void *d_k, const void *d_vt, void *d_packed, int B, int H, int nk, int ldk, int vt_kp, int64_t batch_stride,
                      void *stream);
/* swx_test_attention (f16, V transposed: vt_kp > 0) with explicit batch strides k_bs / v_bs (elements), the fragment-ordered copy
 * d_packed (batch stride k_bs; NULL: the row layout) and, with d_wq != NULL, the query projection inside the launch: q = LN(x) Wq^T + b
 * from the residual rows d_x [fq_rows][ldx] (window b owns rows b * nq ..), raw weights d_wq f16 [d][d], d = 64 H, folded into d_scratch
 * (>= d * d * 2 + 8 d + 1 KiB bytes) exactly as swx_test_dec_gemm folds them for its LayerNorm epilogue; d_q is not read then. */
int swx_test_attention_packed(const void *d_q, int64_t ldq, const void *d_k, const void *d_v, int64_t ldkv, int64_t k_bs, int64_t v_bs,
                              const void *d_packed, void *d_o, int64_t ldo, int B, int H, int nq, int nk, int vt_kp, int force_kernel,
                              const void *d_x, int64_t ldx, int fq_rows, const void *d_wq, const float *d_gamma, const float *d_beta,
                              const float *d_bias, void *d_scratch, size_t scratch_bytes, void *stream);
/* which form of the decode cross-attention kernel such a launch gets (host-only, no GPU; the function swx_attention itself executes):
 * family + 16 * QG + 256 * depth, family 0 = not the decode kernel (flash / row-wise), 1 = row-layout K / V^T, 2 = fragment-ordered
 * copy, 3 = fragment-ordered copy with the fused query projection (fq_k = 64 H); QG = groups of 16 query rows per workgroup (1, 2, 4);
 * depth = key blocks a wave keeps in flight (1, 2).  < 0: the call is refused. */
int swx_test_xattn_plan(int B, int H, int nq, int nk, int vt_kp, int has_packed, int has_fq, int force_kernel, int flags);

/* decode-step self-attention (f16): variant 0 = the single-token kernel without long-context code (positions < 128), 1 = the
 * single-token kernel, 2 = the general cached-attention kernel (their bit-identity reference).  d_q [R][d]; caches
 * [R_phys][n_ctx][d] with the new token's K / V already at position pos0[r] of row r; d_anc [R][n_ctx] or NULL; d_o [R][d]. */
int swx_test_self_attn_step(const void *d_q, void *d_kcache, void *d_vcache, const int32_t *d_anc, const int32_t *d_pos0,
                            int R, int H, int n_ctx, int d, int variant, void *d_o, void *stream);

/* multi-token self-attention of a teacher-forced pass (f16, no ancestor table, every row starts at position 0): mq = 0 the kernel
 * with one wave per (row, token, head) reading K / V from memory, mq = 1 several tokens of a (row, head) per workgroup with K / V
 * staged in LDS once (round 6; bit-identical).  d_q [R * n_new][d] (row stride d); caches [R][n_ctx][d] holding the tokens' K / V at
 * positions 0 .. n_new - 1; d_o [R * n_new][d].  Nothing in the reference corresponds to it. */
int swx_test_self_attn_multi(const void *d_q, void *d_kcache, void *d_vcache, int R, int H, int n_new, int n_ctx, int d, int mq,
                             void *d_o, void *stream);

/* decoder self-attention over the KV cache as swx_self_attention runs it outside the single-token step (f16 or f32; dtype 1 / 0):
 * d_qkv [R * n_new][ldqkv] with q at column 0 and, when skip_append == 0, k at column d and v at column 2 d (these are copied to
 * position pos0[r] + i of cache row r first); logical row of grid row ri is r = ri * row_mul (caches, d_pos0 and d_anc are indexed by r);
 * d_anc [rows][n_ctx] or NULL; pos0_all_zero: the caller states that d_pos0 holds zeros (f16 without a table then takes several tokens
 * per workgroup from 8 tokens on); d_o [R * n_new][d].  Launches nothing and returns a negative code when n_ctx > 512, n_new > n_ctx,
 * d != 64 H, row_mul < 1 or ldqkv < d (3 d when appending). */
int swx_test_self_attn_general(int dtype, const void *d_qkv, int64_t ldqkv, void *d_kcache, void *d_vcache, const int32_t *d_anc,
                               const int32_t *d_pos0, int R, int H, int n_new, int n_ctx, int d, int row_mul, int skip_append,
                               int pos0_all_zero, void *d_o, void *stream);
/* ---- layout of the decoder self-attention K cache (csrc/swx_kernels.h: KLayout).  A cache row is n_ctx * d elements; inside it
 * element (pos, h, dim) lies at (pos * H + h) * 64 + dim when row-major and at ((h * 8 + dim / 8) * n_ctx + pos) * 8 + dim % 8 when
 * chunked (k_chunked != 0: what the f16 decode engine keeps when swx_debug_flags bit 2 is set; A/B).  The V cache is row-major always.
 * swx_test_kcache_index: the library's own index function, host-only: element offset of dims 8 chunk .. 8 chunk + 7 of head h at pos
 * (< 0: arguments out of range).  swx_test_kcache_relayout: HOST buffers of `rows` cache rows, row-major -> chunked (to_chunked != 0)
 * or back, through the same function; src and dst must not overlap.
 * The *_kl calls are the test entry points of the same names with the layout of d_kcache as an argument (f16 only when chunked):
 *   swx_test_dec_gemm_kl        also rps > 0: rows per sequence of the QKV scatter (row m = sequence m / rps, token m % rps)
 *   swx_test_self_attn_general_kl  also step_variant: 0 the multi-token kernels; 1 / 2: n_new == 1 through the decode-step kernels with
 *                                  the position bound 128 / unknown (the long-context kernels) */
int swx_test_kcache_index(int k_chunked, int n_ctx, int d, int pos, int h, int chunk);
int swx_test_kcache_relayout(const void *h_src, void *h_dst, int64_t rows, int n_ctx, int d, int elem_bytes, int to_chunked);
int swx_test_dec_gemm_kl(const void *d_a, int64_t lda, const void *d_w, const float *d_gamma, const float *d_beta,
                         const float *d_bias, void *d_c, int64_t ldc, void *d_x, void *d_kcache, void *d_vcache,
                         const int32_t *d_pos0, int n_ctx, int d, int M, int N, int K, int epilogue, int rps, int k_chunked,
                         void *d_scratch, size_t scratch_bytes, void *stream);
int swx_test_self_attn_step_kl(const void *d_q, void *d_kcache, void *d_vcache, const int32_t *d_anc, const int32_t *d_pos0,
                               int R, int H, int n_ctx, int d, int variant, int k_chunked, void *d_o, void *stream);
int swx_test_self_attn_multi_kl(const void *d_q, void *d_kcache, void *d_vcache, int R, int H, int n_new, int n_ctx, int d, int mq,
                                int k_chunked, void *d_o, void *stream);
int swx_test_self_attn_general_kl(int dtype, const void *d_qkv, int64_t ldqkv, void *d_kcache, void *d_vcache, const int32_t *d_anc,
                                  const int32_t *d_pos0, int R, int H, int n_new, int n_ctx, int d, int row_mul, int skip_append,
                                  int pos0_all_zero, int step_variant, int k_chunked, void *d_o, void *stream);
/* which kernel swx_self_attention launches (host-only, no GPU; the function the launcher itself executes): 0 self_attn_cached<f16>,
 * 1 self_attn_cached<float>, 2 / 3 self_attn_cached_mq_f16<4 / 8>, 4 / 5 self_attn_step_f16<false> with 1 / 5 rows per workgroup,
 * 6 / 7 self_attn_step_f16<true> with 1 / 5 rows per workgroup, 8 self_attn_step_long_f16; < 0: the call is refused.
 * swx_test_self_attn_step's variants are step_cached = 1 with pos_bound = 128 (variant 0) or 0 (variant 1), and step_cached = 0. */
int swx_test_self_attn_plan(int dtype, int R, int H, int n_new, int n_ctx, int row_mul, int skip_append, int step_cached, int pos_bound,
                            int pos0_all_zero, int has_anc, int flags);
/* which kernel swx_test_dec_gemm's launch gets (host-only, no GPU; the function swx_gemm_dec itself executes), `epilogue` as there:
 * 0 gemm_dec_f16 with four-wave workgroups, 1 with single-wave workgroups, 2 / 3 gemm_dectall_f16 with four / eight waves; < 0: not offered */
int swx_test_dec_plan(int M, int N, int K, int epilogue, int flags);
/* where the head-selection entries keep their intermediates (host-only, no GPU; the function the entries themselves carve their
 * scratch with).  out[9] = byte offsets cnt, score, sel, colnorm, nscore, top, gathered, rstat and the total, which equals
 * swx_heads_batch_scratch_bytes(m, W, max_n, count).  With LH = n_text_layer * n_text_head, R = max_n - n_sot - 1 (the row stride
 * of a batch call) and 1536 = the frame stride of the column norms:
 *   cnt      int32 [3][W]            n_tok | text rows | frames (clamped to [1, n_audio_ctx]) of every window
 *   score    f64   [W][LH][R]        dynamic: head scores (timing.py:101), head l * n_text_head + h
 *   sel      int32 [W][R][count]     dynamic: the picked heads of every row, best first
 *   colnorm  f32   [W][LH][1536]     new: column norms over all n_tok rows, frames [0, F)
 *   nscore   f32   [W][LH]           new: head scores (timing.py:143-155)
 *   top      int32 [W][LH]           new: the first topk entries = the picked heads, best first
 *   gathered f32   [W][count][R][n_audio_ctx]   dynamic: raw scaled scores of slot k of every row, frames [0, n_audio_ctx)
 *   rstat    f32   [W][count][R][2]  dynamic: softmax row maximum and sum
 * W = 0: the single-window layout of swx_heads_dynamic / swx_heads_new (total = swx_heads_scratch_bytes(m, max_n); count is not
 * read): score [LH][n_rows] and sel [n_rows][count] with the call's own n_rows as the row stride, colnorm / nscore / top as above
 * with W = 1; cnt, gathered and rstat are empty (their offsets are those of the region that follows). */
int swx_test_heads_layout(const swx_model *m, int W, int max_n, int count, int64_t *out);

/* the bookkeeping behind every raise of a kernel's dynamic-LDS limit (csrc/swx_common.h::SwxLdsGrants: one table per kernel, one entry
 * per device 0..63; host-only, no GPU): on a fresh table, record (dev[i], ok[i] != 0 = granted, 0 = refused) for i = 0 .. n - 1 in
 * order, then state_out[d] for d = 0..63 = 0 unknown, 1 granted, -1 refused.  -5 and nothing written when a dev[i] lies outside 0..63. */
int swx_test_lds_grants(const int *dev, const int *ok, int n, int *state_out);

/* the VALU lane-exchange helpers of csrc/swx_common.h (v_permlane16/32_swap, DPP) against __shfl_xor, on n_waves waves of 64
 * u32 values: d_out[((w * 13 + k) * 64) + lane], k = 0..5 lane_xor<32, 16, 8, 4, 2, 1>, k = 6..11 the __shfl_xor of the same
 * offsets, k = 12 a bit mask of the derived forms that agreed with their shuffle form (1 wave_sum_d, 2 / 4 lane_xor16_max / 32_max,
 * 8 / 16 lane_xor16_add / 32_add, 32 wave_max, 64 wave_sum: 127 = all).  Nothing in the reference corresponds to it. */
int swx_test_lane_xor(const uint32_t *d_in, uint32_t *d_out, int n_waves, void *stream);

/* the reduction kernel of swx_forward_next_token alone, on the CALLER'S logits: d_logits f32 [W][ld] (ld > eot), the other
 * arguments and the outputs as there.  Reads nothing past column eot of a row. */
int swx_test_next_token_reduce(const float *d_logits, int64_t ld, int W, int eot, const int32_t *d_suppress, int n_suppress,
                               const int32_t *d_target, int32_t *d_top, float *d_prob, void *stream);

/* csrc/swx_common.h::gelu_erf2 (the GELU of the tiled / dec GEMM epilogues: two values on packed f32 instructions, both sides of
 * erff's branch) against gelu_erf (the device library's erff) over ALL 2^32 f32 bit patterns: d_out[0] = values whose results differ
 * (NaN results with different payloads not counted), d_out[1] = the lowest such bit pattern (0xffffffff if none), d_out[2] = NaN
 * results whose payloads differ.  Nothing in the reference corresponds to it. */
int swx_test_gelu_pair(uint64_t *d_out, void *stream);

/* the selection path of swx_decode on the CALLER'S logits (csrc/swx_decode.hip: the logit filters, token selection, beam update,
 * step finish and finalize kernels), with no model and no forward pass: swx_decode_init, swx_decode_after_prefill on
 * d_prefill_logits, then per step [copy the step's slice of the script into the logits rows -> selection of token i] launched
 * eagerly, and finalize.  The loop ends by the conditions of swx_decode (one shared host function): context full, every window
 * done (polled every 8 steps once min_tokens have been sampled), sample_len used up.  n_vocab and n_ctx are free (the token
 * buffers are n_ctx + 1 wide); cfg is read as by swx_decode (sample_begins: a ragged job; window_uid: HOST [W], keys the built-in
 * draw as there, NULL = row index; sot_index / sot_indices are not used; noise: DEVICE [sample_len][W * G][n_vocab]); debug flag 8192 selects the memory-walking kernel as in swx_decode.
 *  d_init_tokens int32 [W][longest window]; d_suppress int32 [n_suppress] or NULL; d_ts_mask uint8 [W][1501] or NULL
 *  d_prefill_logits f32 [W][2][n_vocab]  row 0: the SOT position (no-speech probability), row 1: the logits token 0 is selected from
 *  d_script f32 [n_script][W * G][n_vocab]  slice i - 1: the logits token i is selected from ("size out of range" when the loop
 *           needs a slice past n_script)
 *  outputs as swx_decode's (d_nospeech may be NULL), and, both optional: d_anc_out int32 [W * G][n_ctx], the final ancestor table
 *  (written when G > 1), d_pos0_out int32 [W * G].  d_ws: swx_test_decode_script_ws_bytes(cfg, n_vocab, n_ctx) bytes of device
 *  memory, 256-byte aligned.  Returns the number of steps executed or a negative error; blocks until the loop has finished. */
size_t swx_test_decode_script_ws_bytes(const swx_decode_cfg *cfg, int n_vocab, int n_ctx);
int swx_test_decode_script(const swx_decode_cfg *cfg, int n_vocab, int n_ctx, const int32_t *d_init_tokens,
                           const int32_t *d_suppress, const uint8_t *d_ts_mask, const float *d_prefill_logits,
                           const float *d_script, int n_script, int32_t *d_tokens_out, int32_t *d_lens_out, float *d_sumlp_out,
                           float *d_nospeech, int32_t *d_anc_out, int32_t *d_pos0_out, void *d_ws, size_t ws_bytes, void *stream);

/* the built-in sampling draw of the selection kernels (cfg.seed / cfg.window_uid above), through the functions those kernels call.
 * swx_test_sampler_words: for ids id0 .. id0 + n - 1 of (seed, row_uid, step) the 32-bit hash words (d_words uint32 [n]) and the f32
 * variates added to logits / T (d_variates f32 [n]).  swx_test_sampler_buckets: the variate of every bucket k = word >> 8 in
 * [k0, k0 + n), k0 + n <= 2^24 (one launch may cover all 2^24: 64 MB).  row_uid is taken mod 2^32; step, id0, k0 >= 0.  Asynchronous on `stream`; 0 or a negative error. */
int swx_test_sampler_words(uint64_t seed, int64_t row_uid, int step, int id0, int n, uint32_t *d_words, float *d_variates, void *stream);
int swx_test_sampler_buckets(int k0, int n, float *d_variates, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SWX_H */
