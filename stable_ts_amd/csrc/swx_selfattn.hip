// swx_selfattn.hip -- the decoder's cached self-attention (d_head = 64), split off swx_attn.hip.
//
// Upstream: whisper/model.py::MultiHeadAttention.qkv_attention with the causal mask and the kv_cache hooks, reached from
// stable_whisper/decode.py:40 (decoder steps) and timing.py:58-61 (the teacher-forced pass).
//
//   self_attn_cached    decoder self-attention over the KV cache; beams address the cache through an ancestor table
//                       (position -> physical row) so that a beam reorder never copies K/V.  One arithmetic order for the whole
//                       family: self_attn_cached_mq_f16 (several tokens per workgroup), self_attn_step_f16 and
//                       self_attn_step_long_f16 (the decode step) are bit-identical to it.
//   qk_capture          raw scaled q.k of the alignment heads only (what timing.py:50-56 hooks out of every layer).
#include "swx_common.h"
#include "swx_kernels.h"
#include "swx_attn.h"

namespace {

// ========================================================================================== cached self-attn
template <typename T>
__global__ __launch_bounds__(256) void kv_append_kernel(SelfAttnArgs a, int row_mul)
{
    // grid (n_new, R): copy k,v of token i of row r into the cache at position pos0[r] + i
    const int i = blockIdx.x, ri = blockIdx.y;
    const int r = ri * row_mul;
    const int pos = a.pos0[r] + i;
    const T *src = (const T *)a.qkv + ((size_t)ri * a.n_new + i) * a.ldqkv;
    T *kc = (T *)a.kcache + (size_t)r * a.n_ctx * a.d;
    T *vc = (T *)a.vcache + ((size_t)r * a.n_ctx + pos) * a.d;
    for (int c = threadIdx.x; c < a.d; c += 256) { kc[swx_kidx(a.kl, pos, c >> 6, (c >> 3) & 7) + (c & 7)] = src[a.d + c]; vc[c] = src[2 * a.d + c]; }
}

// CH (all readers below): the K cache rows are chunked (a.kl, swx_kernels.h: KLayout); false: row-major, the strides are the
// compile-time ones (sc = 8 elements -> the eight 16-byte loads of a key are one address + immediate offsets)
template <bool CH>
__device__ __forceinline__ KLayout k_layout_of(KLayout kl, int d) { return CH ? kl : KLayout{d, DH, 8}; }

// first element of head h's key at `pos` of cache row `row`.  Row-major, a position is one more "row" of d elements: the address is formed as
// ((row * n_ctx + pos) * d + head offset), one 64-bit multiply, which is what keeps the step kernels at their register counts
template <bool CH, typename T>
__device__ __forceinline__ const T *k_key_ptr(const T *kc, int n_ctx, int d, KLayout kl, int row, int pos, int h)
{
    if (CH) return kc + (size_t)row * n_ctx * d + swx_kidx(kl, pos, h, 0);
    return kc + ((size_t)row * n_ctx + pos) * d + swx_kidx(kl, 0, h, 0);
}

template <typename T, bool CH = false>
__global__ __launch_bounds__(64) void self_attn_cached(SelfAttnArgs a, int row_mul)
{
    const KLayout kl = k_layout_of<CH>(a.kl, a.d);
    // grid (n_new, H, R): one wave per (row, new token, head); causal over positions [0, pos0 + i]
    __shared__ float qs[DH];
    __shared__ float ps[512];
    const int lane = threadIdx.x;
    const int i = blockIdx.x, h = blockIdx.y, ri = blockIdx.z;
    const int r = ri * row_mul;
    const int pos = a.pos0[r] + i;
    const T *qp = (const T *)a.qkv + ((size_t)ri * a.n_new + i) * a.ldqkv + h * DH;
    qs[lane] = to_f32<T>(qp[lane]);
    __syncthreads();
    const int32_t *anc = a.anc ? a.anc + (size_t)r * a.n_ctx : nullptr;
    float mx = -__builtin_inff();
    for (int j = lane; j <= pos; j += 64) {
        const int pr = anc ? anc[j] : r;
        const T *kr = k_key_ptr<CH>((const T *)a.kcache, a.n_ctx, a.d, kl, pr, j, h);
        float acc = 0.f;
#pragma unroll 2
        for (int d0 = 0; d0 < DH; d0 += 8) {
            float kv[8];
            load8<T>(kr + (d0 >> 3) * kl.sc, kv);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc = fmaf(qs[d0 + e], kv[e], acc);
        }
        acc *= 0.125f;
        ps[j] = acc;
        mx = fmaxf(mx, acc);
    }
    mx = wave_max(mx);
    float sum = 0.f;
    for (int j = lane; j <= pos; j += 64) { const float e = expf(ps[j] - mx); ps[j] = e; sum += e; }
    sum = wave_sum(sum);
    __syncthreads();
    const float inv = 1.0f / sum;
    // P.V : lane = (key group kg = lane>>3, 8-wide d chunk dc = lane&7): 16-byte V loads, 8 keys per wave instruction
    const int kg = lane >> 3, dc = (lane & 7) * 8;
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
    for (int j = kg; j <= pos; j += 8) {
        const int pr = anc ? anc[j] : r;
        const T *vr = (const T *)a.vcache + ((size_t)pr * a.n_ctx + j) * a.d + h * DH + dc;
        float vv[8];
        load8<T>(vr, vv);
        const float pj = ps[j] * inv;
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = fmaf(pj, vv[e], acc[e]);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        acc[e] += lane_xor<8>(acc[e], lane);
        acc[e] = lane_xor16_add(acc[e]);
        acc[e] = lane_xor32_add(acc[e]);
    }
    if (kg == 0) {
        T *op = (T *)a.o + ((size_t)ri * a.n_new + i) * a.ldo + h * DH + dc;
#pragma unroll
        for (int e = 0; e < 8; ++e) op[e] = from_f32<T>(acc[e]);
    }
}

// ------------------------------------------------------------------ multi-token self-attention, several tokens per workgroup (round 6)
// self_attn_cached gives every (row, token, head) its own wave, which reads positions 0 .. pos of the head's K and V from L2 again: a 113-token
// scoring pass moves 655 MB per layer through the L1s for 11.6 MB of cache (80 us per layer at 20 windows).  Here a workgroup of NQW waves takes NQW
// CONSECUTIVE tokens of one (row, head): the K and V rows up to its last token's position are staged in LDS ONCE (rows padded to 144 B: a quarter
// wave's 16-byte reads fall on 64 different banks) and every wave runs self_attn_cached's arithmetic on its own token from there -- per score the
// same fmaf chain over d, the same expf, per output element the same key order per lane group and the same lane reduction: bit-identical
// (tests/test_gpu_kernels.py).  f16, no ancestor table, rows that start at position 0 (teacher-forced passes and prefills: the host knows it).
template <int NQW, bool CH = false>
__global__ __launch_bounds__(64 * NQW) void self_attn_cached_mq_f16(SelfAttnArgs a, int row_mul, int lds_rows)
{
    const KLayout kl = k_layout_of<CH>(a.kl, a.d);
    extern __shared__ __attribute__((aligned(16))) unsigned char mq_smem[];   // K [lds_rows][72] | V [lds_rows][72] f16 | qs [NQW][64] | ps [NQW][lds_rows] f32
    constexpr int LD = 72;
    f16 *Ks = (f16 *)mq_smem, *Vs = Ks + (size_t)lds_rows * LD;
    float *qs_all = (float *)(Vs + (size_t)lds_rows * LD), *ps_all = qs_all + NQW * DH;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i0 = blockIdx.x * NQW, h = blockIdx.y, ri = blockIdx.z;
    const int r = ri * row_mul;
    const int i_last = (i0 + NQW < a.n_new ? i0 + NQW : a.n_new) - 1;       // rows start at position 0: token i attends to positions 0 .. i
    {
        const f16 *kg_ = (const f16 *)a.kcache + (size_t)r * a.n_ctx * a.d;
        const f16 *vg_ = (const f16 *)a.vcache + (size_t)r * a.n_ctx * a.d + h * DH;
        for (int c = tid; c < (i_last + 1) * 8; c += 64 * NQW) {
            const int j = c >> 3, c8 = (c & 7) * 8;
            *(f16x8 *)(Ks + j * LD + c8) = *(const f16x8 *)(kg_ + swx_kidx(kl, j, h, c & 7));
            *(f16x8 *)(Vs + j * LD + c8) = *(const f16x8 *)(vg_ + (size_t)j * a.d + c8);
        }
    }
    const bool live = i0 + wave < a.n_new;
    const int i = live ? i0 + wave : a.n_new - 1;      // a wave past the last token repeats it (every wave reaches the barriers) and stores nothing
    const int pos = i;
    float *qs = qs_all + wave * DH, *ps = ps_all + (size_t)wave * lds_rows;
    qs[lane] = (float)((const f16 *)a.qkv)[((size_t)ri * a.n_new + i) * a.ldqkv + h * DH + lane];
    __syncthreads();
    float mx = -__builtin_inff();
    for (int j = lane; j <= pos; j += 64) {
        const f16 *kr = Ks + j * LD;
        float acc = 0.f;
#pragma unroll 2
        for (int d0 = 0; d0 < DH; d0 += 8) {
            const f16x8 t = *(const f16x8 *)(kr + d0);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc = fmaf(qs[d0 + e], (float)t[e], acc);
        }
        acc *= 0.125f;
        ps[j] = acc;
        mx = fmaxf(mx, acc);
    }
    mx = wave_max(mx);
    float sum = 0.f;
    for (int j = lane; j <= pos; j += 64) { const float e = expf(ps[j] - mx); ps[j] = e; sum += e; }
    sum = wave_sum(sum);
    __syncthreads();
    const float inv = 1.0f / sum;
    const int kg = lane >> 3, dc = (lane & 7) * 8;
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
    for (int j = kg; j <= pos; j += 8) {
        const f16x8 t = *(const f16x8 *)(Vs + j * LD + dc);
        const float pj = ps[j] * inv;
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = fmaf(pj, (float)t[e], acc[e]);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        acc[e] += lane_xor<8>(acc[e], lane);
        acc[e] = lane_xor16_add(acc[e]);
        acc[e] = lane_xor32_add(acc[e]);
    }
    if (kg == 0 && live) {
        f16 *op = (f16 *)a.o + ((size_t)ri * a.n_new + i) * a.ldo + h * DH + dc;
#pragma unroll
        for (int e = 0; e < 8; ++e) op[e] = (f16)acc[e];
    }
}

// ------------------------------------------------------------------------------------------ decode-step self-attention
// One wave per (row, head) of a single-token decode step, f16: q comes from the QKV projection's output (a.qkv, row stride
// ldqkv), the new token's K / V are ALREADY in the cache at position pos0[r] of row r (the projection's epilogue scattered
// them).  The dependent-load chain is 3 round trips: {pos0} -> {ancestor ids} -> {K rows, V fragments} -> math; the V
// fragments of the first 128 positions are requested together with the K rows (ancestor ids travel between lanes by
// shuffles).  Arithmetic order is self_attn_cached's, so both paths agree bit for bit.
// HBM traffic: K and V of every cached position of every row once = R * (pos + 1) * d * 2 * 2 bytes per launch (57 MB at
// position 111 for 100 rows of large-v3: at the end of a window's decode this kernel is bandwidth-, not latency-bound).
// WPB (round 6 experiment, SWX_FLAG_SELFATTN_WG5): waves per workgroup -- WPB consecutive rows of one head (the beams of a window)
// share a workgroup, i.e. a CU's L1 and one workgroup dispatch; every wave still does exactly its row's arithmetic.
template <bool LONG, int WPB = 1, bool CH = false>
__global__ __launch_bounds__(64 * WPB) void self_attn_step_f16(SelfAttnArgs a)
{
    const KLayout kl = k_layout_of<CH>(a.kl, a.d);
    constexpr int PF = 16;                   // prefetched V fragments per lane (keys kg + 8 i, i < PF  <=>  j < 128)
    __shared__ float qs_all[WPB][DH];
    __shared__ float ps_all[WPB][512];
    const int lane = threadIdx.x & 63, wave_in_wg = threadIdx.x >> 6, h = blockIdx.x;
    const int r_raw = blockIdx.y * WPB + wave_in_wg;
    const bool r_live = r_raw < a.R;
    const int r = r_live ? r_raw : a.R - 1;  // a wave past the last row repeats it (every wave reaches the barriers) and does not store
    float *qs = qs_all[wave_in_wg], *ps = ps_all[wave_in_wg];
    const int d = a.d;
    const int pos = a.pos0[r];
    const int32_t *anc = a.anc ? a.anc + (size_t)r * a.n_ctx : nullptr;
    const f16 *kc = (const f16 *)a.kcache, *vc = (const f16 *)a.vcache;
    const int j0 = lane, j1 = lane + 64;
    const bool has0 = j0 <= pos, has1 = j1 <= pos;         // positions that live in the cache (the new one included)
    // ancestor ids: clamped unconditional loads + select (a predicated load would cost its own round trip)
    const int32_t *ap = anc ? anc : a.pos0;
    const bool old0 = j0 < pos, old1 = j1 < pos;           // the ancestor table covers the older positions; the new one is row r's own
    const int t0 = ap[(anc && old0) ? j0 : 0], t1 = ap[(anc && old1) ? j1 : 0];
    const int pr0 = (anc && old0) ? t0 : r, pr1 = (anc && old1) ? t1 : r;
    qs[lane] = (float)((const f16 *)a.qkv)[(size_t)r * a.ldqkv + h * DH + lane];
    // ---- K rows of positions lane, lane + 64 and the V fragments of positions < 128: one batch of loads
    f16x8 k0[8], k1[8];
    {
        const f16 *kr0 = k_key_ptr<CH>(kc, a.n_ctx, a.d, kl, has0 ? pr0 : r, has0 ? j0 : 0, h);   // clamped, never predicated
#pragma unroll
        for (int e = 0; e < 8; ++e) k0[e] = *(const f16x8 *)(kr0 + e * kl.sc);
        if (pos >= 64) {
            const f16 *kr1 = k_key_ptr<CH>(kc, a.n_ctx, a.d, kl, has1 ? pr1 : r, has1 ? j1 : 0, h);
#pragma unroll
            for (int e = 0; e < 8; ++e) k1[e] = *(const f16x8 *)(kr1 + e * kl.sc);
        }
    }
    const int kg = lane >> 3, dc = (lane & 7) * 8;
    f16x8 vpre[PF];
#pragma unroll
    for (int i = 0; i < PF; ++i) {
        if (i * 8 <= pos) {                                  // uniform: some key of this group of 8 is in the cache
            const int j = kg + 8 * i;
            const int src = j & 63;
            const int pa = __shfl(pr0, src, 64), pb = __shfl(pr1, src, 64);
            const int prj = j < 64 ? pa : pb;                       // (pr0 / pr1 are r for the new position)
            const bool ok = j <= pos;
            vpre[i] = *(const f16x8 *)(vc + ((size_t)(ok ? prj : r) * a.n_ctx + (ok ? j : 0)) * d + h * DH + dc);
        }
    }
    __syncthreads();                                        // qs visible
    // ---- scores (each lane owns whole keys)
    auto dot_regs = [&](const f16x8 *kk) {
        float acc = 0.f;
#pragma unroll
        for (int c = 0; c < 8; ++c)
#pragma unroll
            for (int e = 0; e < 8; ++e) acc = fmaf(qs[c * 8 + e], (float)kk[c][e], acc);
        return acc;
    };
    float mx = -__builtin_inff();
    if (j0 <= pos) {
        const float sc = dot_regs(k0) * 0.125f;
        ps[j0] = sc; mx = fmaxf(mx, sc);
    }
    if (pos >= 64 && j1 <= pos) {
        const float sc = dot_regs(k1) * 0.125f;
        ps[j1] = sc; mx = fmaxf(mx, sc);
    }
    // positions >= 128 (a decode that started from a long prompt: sequential transcribe() carries up to 223 tokens over).  The
    // plain loop here was two dependent round trips per 64 positions (ancestor id -> K row); now the ancestor ids of every
    // remaining chunk are requested in one batch and then all K rows in one batch.  Per key the dot product is the same
    // expression, so the scores are bit-identical (the maximum is order-independent).
    if (LONG && pos >= 128) {
        constexpr int KT = 6;                               // 128 + 5 * 64 = 448 = n_text_ctx (six slots: three pairs)
        int prt[KT];
#pragma unroll
        for (int c = 0; c < KT; ++c) {
            const int j = lane + 128 + 64 * c;
            const bool old = anc && j < pos;
            const int t = ap[old ? j : 0];
            prt[c] = old ? t : r;
        }
#pragma unroll
        for (int c2 = 0; c2 < KT; c2 += 2) {                // two chunks of K rows in flight at a time (64 registers, like k0 / k1)
            if (128 + 64 * c2 <= pos) {                     // uniform
                f16x8 kt[2][8];
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int c = c2 + u;
                    if (128 + 64 * c <= pos) {              // uniform: the chunk holds a cached position
                        const int j = lane + 128 + 64 * c;
                        const bool has = j <= pos;
                        const f16 *kr = k_key_ptr<CH>(kc, a.n_ctx, a.d, kl, has ? prt[c] : r, has ? j : 0, h);
#pragma unroll
                        for (int e = 0; e < 8; ++e) kt[u][e] = *(const f16x8 *)(kr + e * kl.sc);
                    }
                }
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int c = c2 + u;
                    const int j = lane + 128 + 64 * c;
                    if (128 + 64 * c <= pos && j <= pos) {
                        const float sc = dot_regs(kt[u]) * 0.125f;
                        ps[j] = sc; mx = fmaxf(mx, sc);
                    }
                }
            }
        }
    }
    mx = wave_max(mx);
    float sum = 0.f;
    for (int j = lane; j <= pos; j += 64) { const float e = expf(ps[j] - mx); ps[j] = e; sum += e; }
    sum = wave_sum(sum);
    __syncthreads();
    const float inv = 1.0f / sum;
    // ---- P.V : lane = (key group kg, 8-wide d chunk dc); keys in ascending order per lane like the generic kernel
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
#pragma unroll
    for (int i = 0; i < PF; ++i) {
        const int j = kg + 8 * i;
        if (i * 8 <= pos && j <= pos) {
            const float pj = ps[j] * inv;
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] = fmaf(pj, (float)vpre[i][e], acc[e]);
        }
    }
    // keys >= 128: batches of 8 keys per lane group -- ancestor ids in one batch, V fragments in one batch, then the
    // multiply-adds in ascending key order exactly as the one-key-at-a-time loop did them (bit-identical)
    for (int jb = kg + 8 * PF; LONG && jb <= pos; jb += 64) {
        int prv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int j = jb + 8 * u;
            const bool old = anc && j < pos;
            const int t = ap[old ? j : 0];
            prv[u] = old ? t : r;
        }
        f16x8 vb[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int j = jb + 8 * u;
            const bool ok = j <= pos;
            vb[u] = *(const f16x8 *)(vc + ((size_t)(ok ? prv[u] : r) * a.n_ctx + (ok ? j : 0)) * d + h * DH + dc);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int j = jb + 8 * u;
            if (j <= pos) {
                const float pj = ps[j] * inv;
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] = fmaf(pj, (float)vb[u][e], acc[e]);
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        acc[e] += lane_xor<8>(acc[e], lane);
        acc[e] = lane_xor16_add(acc[e]);
        acc[e] = lane_xor32_add(acc[e]);
    }
    if (kg == 0 && r_live) {
        f16 *op = (f16 *)a.o + (size_t)r * a.ldo + h * DH + dc;
#pragma unroll
        for (int e = 0; e < 8; ++e) op[e] = (f16)acc[e];
    }
}


// ---------------------------------------------------------------------------- decode-step self-attention, long context, few waves
// Round 6.  A decode that starts from a carried-over prompt (the reference's sequential flow: `model.transcribe(audio)` decodes ONE
// window per call, positions 228-340) runs self_attn_step_f16<true> as R x H = 100 waves, each a chain of DEPENDENT round trips:
// pos0 -> ancestor ids -> K rows of positions < 128 -> K rows 128-255 -> K rows 256-383 -> [softmax] -> per 64 keys (ancestor ids ->
// V fragments): 13 trips at position 340 = the launch's 13 us.  With at most one wave per SIMD there is no neighbour to hide them
// behind and the whole register file belongs to the wave, so this variant requests EVERYTHING a row needs in two batches:
//   1. the ancestor ids of all seven 64-position chunks;
//   2. K rows of positions < 256, the V fragments of positions < 128 -- and, behind them in the queue, K rows of positions 256-447 and
//      the V fragments of positions 128-447 (their ancestor ids travel between lanes by shuffles instead of being loaded again).
// = pos0 + two round trips.  Per score and per output element the expressions and their ORDER are self_attn_step_f16's (one lane owns
// a key's whole dot product; a lane group accumulates its keys in ascending order), so the result is bit-identical
// (tests/hw_checks/self_attn_check.py, tests/test_gpu_model.py).  Dispatched for R x H <= 1024 (SWX_FLAG_SELFATTN_NO_DEEP: A/B).
template <bool CH = false>
__global__ __launch_bounds__(64) void self_attn_step_long_f16(SelfAttnArgs a)
{
    const KLayout kl = k_layout_of<CH>(a.kl, a.d);
    constexpr int PF = 16;                   // V fragments per lane of positions < 128 (keys kg + 8 i)
    constexpr int NC = 5;                    // 64-position chunks past 128: 128 + 64 * 5 = 448 = n_text_ctx
    __shared__ float qs[DH];
    __shared__ float ps[512];
    const int lane = threadIdx.x, h = blockIdx.x, r = blockIdx.y;
    const int d = a.d;
    const int pos = a.pos0[r];
    const int32_t *anc = a.anc ? a.anc + (size_t)r * a.n_ctx : nullptr;
    const f16 *kc = (const f16 *)a.kcache, *vc = (const f16 *)a.vcache;
    const int32_t *ap = anc ? anc : a.pos0;
    // ---- batch 1: ancestor ids of every chunk (clamped unconditional loads + select; the new position is row r's own)
    int pr[2 + NC];
#pragma unroll
    for (int c = 0; c < 2 + NC; ++c) {
        const int j = lane + 64 * c;
        const bool old = anc && j < pos;
        const int t = ap[old ? j : 0];
        pr[c] = old ? t : r;
    }
    qs[lane] = (float)((const f16 *)a.qkv)[(size_t)r * a.ldqkv + h * DH + lane];
    // ---- batch 2: K rows (a lane owns whole keys) and V fragments (lane = key group kg, 8-wide d chunk dc)
    auto load_k = [&](int c, f16x8 (&kk)[8]) {
        const int j = lane + 64 * c;
        const bool has = j <= pos;
        const f16 *kr = k_key_ptr<CH>(kc, a.n_ctx, a.d, kl, has ? pr[c] : r, has ? j : 0, h);     // clamped, never predicated
#pragma unroll
        for (int e = 0; e < 8; ++e) kk[e] = *(const f16x8 *)(kr + e * kl.sc);
    };
    // the V side's ancestor ids (lane group kg reads keys kg + 8 u of every chunk: the id sits in lane kg + 8 u): all 56 exchanges as ONE
    // batch in front of the loads -- inside the guarded load blocks each exchange is an LDS round trip of its own in front of its load
    const int kg = lane >> 3, dc = (lane & 7) * 8;
    int pv[2 + NC][8];
#pragma unroll
    for (int c = 0; c < 2 + NC; ++c)
#pragma unroll
        for (int u = 0; u < 8; ++u) pv[c][u] = __shfl(pr[c], kg + 8 * u, 64);
    __builtin_amdgcn_sched_barrier(0);
    f16x8 kA[4][8];
#pragma unroll
    for (int c = 0; c < 4; ++c)
        if (64 * c <= pos) load_k(c, kA[c]);                // uniform: the chunk holds a cached position
    f16x8 vpre[PF];
#pragma unroll
    for (int i = 0; i < PF; ++i) {
        if (i * 8 <= pos) {                                  // uniform
            const int j = kg + 8 * i;
            const int prj = pv[i >> 3][i & 7];
            const bool ok = j <= pos;
            vpre[i] = *(const f16x8 *)(vc + ((size_t)(ok ? prj : r) * a.n_ctx + (ok ? j : 0)) * d + h * DH + dc);
        }
    }
    constexpr int NE = 3;                    // V batches / K chunk requested up front: positions < 320; the rest (320-447) after the first scores
    f16x8 kE[8];
    if (64 * 4 <= pos) load_k(4, kE);
    auto load_vb = [&](int b, f16x8 (&vv)[8]) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int j = kg + 128 + 64 * b + 8 * u;
            const int prj = pv[2 + b][u];
            const bool ok = j <= pos;
            vv[u] = *(const f16x8 *)(vc + ((size_t)(ok ? prj : r) * a.n_ctx + (ok ? j : 0)) * d + h * DH + dc);
        }
    };
    f16x8 vb[NC][8];
#pragma unroll
    for (int b = 0; b < NE; ++b)
        if (128 + 64 * b <= pos) load_vb(b, vb[b]);          // uniform
    __syncthreads();                                        // qs visible
    // ---- scores
    auto dot_regs = [&](const f16x8 *kk) {
        float acc = 0.f;
#pragma unroll
        for (int c = 0; c < 8; ++c)
#pragma unroll
            for (int e = 0; e < 8; ++e) acc = fmaf(qs[c * 8 + e], (float)kk[c][e], acc);
        return acc;
    };
    float mx = -__builtin_inff();
    auto score = [&](int c, const f16x8 *kk) {
        const int j = lane + 64 * c;
        if (64 * c <= pos && j <= pos) {
            const float sc = dot_regs(kk) * 0.125f;
            ps[j] = sc; mx = fmaxf(mx, sc);
        }
    };
#pragma unroll
    for (int c = 0; c < 4; ++c) score(c, kA[c]);
    // positions >= 320 (never reached by the sequential flow's 223-token prompts + 112 steps; one more round trip when they are): their
    // K rows and V fragments take over the registers of the rows just multiplied
    __builtin_amdgcn_sched_barrier(0);
    f16x8 kL[2][8];
#pragma unroll
    for (int c = 5; c < 2 + NC; ++c)
        if (64 * c <= pos) load_k(c, kL[c - 5]);
#pragma unroll
    for (int b = NE; b < NC; ++b)
        if (128 + 64 * b <= pos) load_vb(b, vb[b]);
    score(4, kE);
#pragma unroll
    for (int c = 5; c < 2 + NC; ++c) score(c, kL[c - 5]);
    mx = wave_max(mx);
    float sum = 0.f;
    for (int j = lane; j <= pos; j += 64) { const float e = expf(ps[j] - mx); ps[j] = e; sum += e; }
    sum = wave_sum(sum);
    __syncthreads();
    const float inv = 1.0f / sum;
    // ---- P.V : keys in ascending order per lane group
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
#pragma unroll
    for (int i = 0; i < PF; ++i) {
        const int j = kg + 8 * i;
        if (i * 8 <= pos && j <= pos) {
            const float pj = ps[j] * inv;
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] = fmaf(pj, (float)vpre[i][e], acc[e]);
        }
    }
#pragma unroll
    for (int b = 0; b < NC; ++b)
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int j = kg + 128 + 64 * b + 8 * u;
            if (128 + 64 * b <= pos && j <= pos) {
                const float pj = ps[j] * inv;
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] = fmaf(pj, (float)vb[b][u][e], acc[e]);
            }
        }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        acc[e] += lane_xor<8>(acc[e], lane);
        acc[e] = lane_xor16_add(acc[e]);
        acc[e] = lane_xor32_add(acc[e]);
    }
    if (kg == 0) {
        f16 *op = (f16 *)a.o + (size_t)r * a.ldo + h * DH + dc;
#pragma unroll
        for (int e = 0; e < 8; ++e) op[e] = (f16)acc[e];
    }
}


// =============================================================================================== qk capture
template <typename T>
__global__ __launch_bounds__(256) void qk_capture_kernel(const T *__restrict__ q, int64_t ldq, int q_rows_per_w, int row0,
                                                         const T *__restrict__ k, int64_t ldk, int64_t k_bs, int nk,
                                                         const int32_t *__restrict__ heads, int head_slot0, int slots_total,
                                                         float *__restrict__ out, int out_ld_n, int out_ld_f)
{
    // grid (n_rows, n_heads, W)
    __shared__ float qs[DH];
    const int i = blockIdx.x, hs = blockIdx.y, w = blockIdx.z;
    const int head = heads[hs];
    const T *qp = q + ((size_t)w * q_rows_per_w + row0 + i) * ldq + head * DH;
    if (threadIdx.x < DH) qs[threadIdx.x] = to_f32<T>(qp[threadIdx.x]);
    __syncthreads();
    float *orow = out + (((size_t)w * slots_total + head_slot0 + hs) * out_ld_n + i) * out_ld_f;
    for (int f = threadIdx.x; f < nk; f += 256) {
        const T *kr = k + (size_t)w * k_bs + (size_t)f * ldk + head * DH;
        float acc = 0.f;
#pragma unroll 2
        for (int d0 = 0; d0 < DH; d0 += 8) {
            float kv[8];
            load8<T>(kr + d0, kv);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc = fmaf(qs[d0 + e], kv[e], acc);
        }
        orow[f] = acc * 0.125f;
    }
}

}  // namespace

int swx_self_attn_plan(int dtype, const SelfAttnArgs &a, int row_mul, int flags)
{
    if (a.n_ctx > 512) return -5;
    if (a.step_cached) {       // single-token step, q in a.qkv, the new K / V already in the cache
        if (dtype != SWX_F16 || a.n_new != 1 || row_mul != 1 || !a.skip_append) return -5;
        // (a decode whose positions stay below 128 -- no prompt carried over -- takes the variant without the long-context code:
        // 157 instead of 211 registers, three waves per SIMD)
        const bool wg5 = (flags & SWX_FLAG_SELFATTN_WG5) != 0;       // A/B: five rows (a window's beams) per workgroup
        if (a.pos_bound > 0 && a.pos_bound <= 128) return wg5 ? SWX_SA_K_STEP_WG5 : SWX_SA_K_STEP;
        // few waves (one window of the sequential flow: 100): every load of a row in two batches (bit-identical)
        const bool deep = !wg5 && (int64_t)a.R * a.H <= 1024 && a.n_ctx <= 448 && !(flags & SWX_FLAG_SELFATTN_NO_DEEP);
        return deep ? SWX_SA_K_STEP_DEEP : wg5 ? SWX_SA_K_STEP_LONG_WG5 : SWX_SA_K_STEP_LONG;
    }
    if (dtype != SWX_F16) return SWX_SA_K_CACHED_F32;
    // several tokens of a (row, head) per workgroup, K / V staged in LDS once (bit-identical; SWX_FLAG_SELFATTN_NO_MQ: A/B)
    if (a.pos0_all_zero && !a.anc && a.n_new >= 8 && a.n_new <= a.n_ctx && !(flags & SWX_FLAG_SELFATTN_NO_MQ))
        return a.n_new >= 32 ? SWX_SA_K_MQ8 : SWX_SA_K_MQ4;
    return SWX_SA_K_CACHED_F16;
}

// self_attn_cached_mq_f16<NQW, CH>: K / V rows [lds_rows][72] f16 + qs / ps per wave, past 64 KB from n_new = 193 on at NQW = 8.
// Each of the four instantiations holds a grant of its own (swx_common.h: the kernel is the template argument).  The generic lambda
// this replaces kept ONE flag for all four -- they decay to one function-pointer type -- so only the first one launched was ever
// granted its LDS.
template <int NQW, bool CH>
static int launch_mq(const SelfAttnArgs &a, int row_mul, hipStream_t s)
{
    const int lds_rows = ((a.n_new + 7) / 8) * 8;
    const size_t lds = (size_t)lds_rows * 72 * 2 * 2 + (size_t)NQW * 64 * 4 + (size_t)NQW * lds_rows * 4;
    return swx_launch_lds<self_attn_cached_mq_f16<NQW, CH>>(dim3(cdiv(a.n_new, NQW), a.H, a.R), dim3(64 * NQW), lds, SWX_LDS_MAX, s, a,
                                                            row_mul, lds_rows);
}

int swx_self_attention(int dtype, const SelfAttnArgs &a_in, int row_mul, hipStream_t s)
{
    if (a_in.R <= 0 || a_in.n_new <= 0) return 0;
    SelfAttnArgs a = a_in;
    if (!a.kl.sp) a.kl = swx_klayout(0, a.n_ctx, a.d);
    if (dtype != SWX_F16 && a.kl.sp != a.d) return -5;      // the chunked K cache is the f16 engine's
    const int kid = swx_self_attn_plan(dtype, a, row_mul, swx_flags());
    if (kid < 0) return kid;
    // algorithmic bytes: K and V of every cached position of every row once (+ q in, o out); the positions are device state --
    // the decode loop passes the one it knows (step_pos), multi-token passes attend to n_new positions on average n_new / 2 + 1
    const double npos = a.step_pos > 0 ? a.step_pos + 1 : (a.n_new + 1) * 0.5;
    SwxProfScope prof(PC_SELF_ATTN, (double)a.R * a.n_new * a.d * (dtype == SWX_F16 ? 2 : 4) * (2.0 * npos + 2.0), s);
    dim3 g1(a.n_new, a.R);
    dim3 g2(a.n_new, a.H, a.R);
    const bool ch = a.kl.sp != a.d;           // chunked K cache rows: the CH instantiation of the reader
#define SWX_SA_LAUNCH(K0, K1, grid, block, ...) \
    do { if (ch) hipLaunchKernelGGL((K1), grid, block, 0, s, __VA_ARGS__); else hipLaunchKernelGGL((K0), grid, block, 0, s, __VA_ARGS__); } while (0)
    switch (kid) {
        case SWX_SA_K_STEP_WG5: SWX_SA_LAUNCH((self_attn_step_f16<false, 5, false>), (self_attn_step_f16<false, 5, true>), dim3(a.H, cdiv(a.R, 5)), dim3(320), a); break;
        case SWX_SA_K_STEP: SWX_SA_LAUNCH((self_attn_step_f16<false, 1, false>), (self_attn_step_f16<false, 1, true>), dim3(a.H, a.R), dim3(64), a); break;
        case SWX_SA_K_STEP_DEEP: SWX_SA_LAUNCH((self_attn_step_long_f16<false>), (self_attn_step_long_f16<true>), dim3(a.H, a.R), dim3(64), a); break;
        case SWX_SA_K_STEP_LONG_WG5: SWX_SA_LAUNCH((self_attn_step_f16<true, 5, false>), (self_attn_step_f16<true, 5, true>), dim3(a.H, cdiv(a.R, 5)), dim3(320), a); break;
        case SWX_SA_K_STEP_LONG: SWX_SA_LAUNCH((self_attn_step_f16<true, 1, false>), (self_attn_step_f16<true, 1, true>), dim3(a.H, a.R), dim3(64), a); break;
        case SWX_SA_K_MQ4:
        case SWX_SA_K_MQ8: {
            if (!a.skip_append) hipLaunchKernelGGL(kv_append_kernel<f16>, g1, dim3(256), 0, s, a, row_mul);
            const int rc = kid == SWX_SA_K_MQ8 ? (ch ? launch_mq<8, true>(a, row_mul, s) : launch_mq<8, false>(a, row_mul, s))
                                               : (ch ? launch_mq<4, true>(a, row_mul, s) : launch_mq<4, false>(a, row_mul, s));
            if (rc < 0) return rc;
            break;
        }
        case SWX_SA_K_CACHED_F16:
            if (!a.skip_append) hipLaunchKernelGGL(kv_append_kernel<f16>, g1, dim3(256), 0, s, a, row_mul);
            SWX_SA_LAUNCH((self_attn_cached<f16, false>), (self_attn_cached<f16, true>), g2, dim3(64), a, row_mul);
            break;
        case SWX_SA_K_CACHED_F32:
            if (!a.skip_append) hipLaunchKernelGGL(kv_append_kernel<float>, g1, dim3(256), 0, s, a, row_mul);
            hipLaunchKernelGGL((self_attn_cached<float, false>), g2, dim3(64), 0, s, a, row_mul);
            break;
        default: return -5;
    }
#undef SWX_SA_LAUNCH
    SWX_CHECK_LAUNCH();
    return 0;
}

int swx_qk_capture(int dtype, const void *q, int64_t ldq, int q_rows_per_w, int row0, int n_rows, const void *k,
                   int64_t ldk, int64_t k_bs, int nk, const int32_t *heads, int n_heads, int head_slot0, int slots_total, int W,
                   float *out, int out_ld_n, int out_ld_f, hipStream_t s)
{
    if (n_rows <= 0 || n_heads <= 0 || W <= 0) return 0;
    dim3 g(n_rows, n_heads, W);
    if (dtype == SWX_F16)
        hipLaunchKernelGGL(qk_capture_kernel<f16>, g, dim3(256), 0, s, (const f16 *)q, ldq, q_rows_per_w, row0, (const f16 *)k, ldk, k_bs, nk, heads, head_slot0, slots_total, out, out_ld_n, out_ld_f);
    else
        hipLaunchKernelGGL(qk_capture_kernel<float>, g, dim3(256), 0, s, (const float *)q, ldq, q_rows_per_w, row0, (const float *)k, ldk, k_bs, nk, heads, head_slot0, slots_total, out, out_ld_n, out_ld_f);
    SWX_CHECK_LAUNCH();
    return 0;
}
