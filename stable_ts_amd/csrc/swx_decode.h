// swx_decode.h -- device-resident bookkeeping of one decode job (W windows x G sequences)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/swx.h"

struct DecodeBufs {
    swx_decode_cfg cfg;
    int W, G, M, V, TS, n_ctx, n_init;
    int max_cand, fin_cap;
    int32_t *tokens[2];        // [M][TS] (double buffered for the beam gather)
    int32_t *anc[2];           // [M][n_ctx] ancestor tables (null when G == 1)
    int32_t *pos0;             // [M] position of the token the next forward pass embeds
    const int32_t *begin;      // [W] initial tokens per window of a ragged job (n_init is then the longest: the row stride of the
                               //     initial-token array and the bound the host plans with), or null: every window has n_init
    float *sum_lp, *sum_lp_next;   // [M]
    int32_t *row_done;         // [M]
    int32_t *win_done, *win_done_prev;   // [W]
    int32_t *n_done;           // [1]
    int32_t *step_dev;         // [1] number of tokens sampled so far: read by the selection kernels, advanced by the step-finish
                               //     kernel -- the step index is device state so that a captured step graph can be replayed
    int32_t *fin_tokens;       // [W][fin_cap][TS]
    float *fin_score;          // [W][fin_cap]
    int32_t *fin_len;          // [W][fin_cap]
    int32_t *fin_count;        // [W]
    float *cand_lp;            // [M][G+1]
    int32_t *cand_tok;         // [M][G+1]
    float *logits;             // [M][V] f32
    const int32_t *suppress;   // [n_suppress]
    const uint8_t *ts_mask;    // [W][1501] or null
    const int32_t *win_uid;    // [W] stable window identities for the sampling RNG, or null (= window index)
};

// ---- the built-in sampling draw (temperature > 0, cfg.noise == NULL): one Gumbel variate per (seed, row_uid, step, token id).
// Here, not in swx_decode.hip, so that the test hooks (swx_test_sampler_words / _buckets) run the very functions the selection
// kernels call.  Contract (swx.h, tests/sampler_ref.py): bucket k = word >> 8, u_k = (k + 0.5) * 2^-24, variate -ln(-ln u_k).
__device__ __forceinline__ unsigned hash32(unsigned x)
{
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

__device__ __forceinline__ unsigned sampler_word(uint64_t seed, unsigned row_uid, unsigned step, unsigned idx)
{
    const unsigned h = hash32((unsigned)seed ^ hash32(idx + 0x9e3779b9u * (step + 1u)));
    return hash32(h ^ hash32(row_uid * 0x85ebca6bu + (unsigned)(seed >> 32)));
}

// f32 has no 24-bit bucket centre from 0.5 up (k + 0.5f rounds to even there), and in the top bucket the rounded centre is 1.0f,
// whose variate would be +inf: u is held at the largest f32 below 1.  Every other bucket's bits are what they always were.
__device__ __forceinline__ float sampler_variate(unsigned word)
{
    const float u = fminf(((float)(word >> 8) + 0.5f) * (1.0f / 16777216.0f), 0x1.fffffep-1f);   // (0,1)
    return -logf(-logf(u));
}

__device__ __forceinline__ float gumbel(uint64_t seed, unsigned row_uid, unsigned step, unsigned idx)
{
    return sampler_variate(sampler_word(seed, row_uid, step, idx));
}

int swx_decode_init(const DecodeBufs &b, const int32_t *init_tokens, hipStream_t s);
int swx_decode_after_prefill(const DecodeBufs &b, const float *lg2, float *nospeech, hipStream_t s);
int swx_decode_select(const DecodeBufs &b, int cur, hipStream_t s);
int swx_decode_finalize(const DecodeBufs &b, int cur, int n_steps, int32_t *tokens_out, int32_t *lens_out,
                        float *sumlp_out, int G_out, hipStream_t s);
