// swx_testhooks.hip -- the swx_test_* entries of the C ABI that reach single launchers and plan functions, and the two whole-chip
// self-check kernels.  (A hook that needs a file-private function lives beside it: swx_decjob.hip, swx_score.hip.)
#include <cstring>
#include "swx_model.h"

// lane-exchange helpers vs __shfl_xor (swx_test_lane_xor)
__global__ __launch_bounds__(64) void lane_xor_check_kernel(const uint32_t *__restrict__ in, uint32_t *__restrict__ out)
{
    const int lane = threadIdx.x;
    const uint32_t x = in[blockIdx.x * 64 + lane];
    uint32_t *o = out + (size_t)blockIdx.x * 13 * 64 + lane;
    o[0 * 64] = lane_xor_u32<32>(x, lane); o[1 * 64] = lane_xor_u32<16>(x, lane); o[2 * 64] = lane_xor_u32<8>(x, lane);
    o[3 * 64] = lane_xor_u32<4>(x, lane);  o[4 * 64] = lane_xor_u32<2>(x, lane);  o[5 * 64] = lane_xor_u32<1>(x, lane);
    o[6 * 64] = (uint32_t)__shfl_xor((int)x, 32, 64); o[7 * 64] = (uint32_t)__shfl_xor((int)x, 16, 64);
    o[8 * 64] = (uint32_t)__shfl_xor((int)x, 8, 64);  o[9 * 64] = (uint32_t)__shfl_xor((int)x, 4, 64);
    o[10 * 64] = (uint32_t)__shfl_xor((int)x, 2, 64); o[11 * 64] = (uint32_t)__shfl_xor((int)x, 1, 64);
    double v = (double)__uint_as_float(x);
    double ref = v;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) ref += __shfl_xor(ref, off, 64);
    const double got = wave_sum_d(v);
    unsigned ok = (__double_as_longlong(got) == __double_as_longlong(ref)) ? 1u : 0u;
    // the select-free forms for commutative operations, on finite values
    const float f = (float)(int)(x >> 9) * 1.1920929e-7f - 0.37f;
    ok |= (__float_as_uint(lane_xor16_max(f)) == __float_as_uint(fmaxf(f, __shfl_xor(f, 16, 64)))) ? 2u : 0u;
    ok |= (__float_as_uint(lane_xor32_max(f)) == __float_as_uint(fmaxf(f, __shfl_xor(f, 32, 64)))) ? 4u : 0u;
    ok |= (__float_as_uint(lane_xor16_add(f)) == __float_as_uint(f + __shfl_xor(f, 16, 64))) ? 8u : 0u;
    ok |= (__float_as_uint(lane_xor32_add(f)) == __float_as_uint(f + __shfl_xor(f, 32, 64))) ? 16u : 0u;
    float wm = f, ws = f;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { wm = fmaxf(wm, __shfl_xor(wm, off, 64)); ws += __shfl_xor(ws, off, 64); }
    ok |= (__float_as_uint(wave_max(f)) == __float_as_uint(wm)) ? 32u : 0u;
    ok |= (__float_as_uint(wave_sum(f)) == __float_as_uint(ws)) ? 64u : 0u;
    o[12 * 64] = ok;
}

// gelu_erf2 (packed, both sides of erff's branch) vs gelu_erf (the device library's erff) over EVERY f32 bit pattern (swx_test_gelu_pair)
__global__ __launch_bounds__(256) void gelu_pair_check_kernel(unsigned long long *__restrict__ out)
{
    const unsigned base = (blockIdx.x * 256u + threadIdx.x) * 32u;          // 2^27 threads x 32 values = 2^32
    unsigned bad = 0, nan_bits = 0, first = 0xffffffffu;
#pragma unroll 4
    for (unsigned j = 0; j < 32; j += 2) {
        const unsigned u0 = base + j, u1 = base + j + 1;
        const f32x2 x = {__uint_as_float(u0), __uint_as_float(u1)};
        const f32x2 got = gelu_erf2(x);
        const float r0 = gelu_erf(x[0]), r1 = gelu_erf(x[1]);
        const unsigned g0 = __float_as_uint(got[0]), g1 = __float_as_uint(got[1]), e0 = __float_as_uint(r0), e1 = __float_as_uint(r1);
        if (g0 != e0) { if (r0 != r0 && got[0] != got[0]) ++nan_bits; else { ++bad; first = first < u0 ? first : u0; } }
        if (g1 != e1) { if (r1 != r1 && got[1] != got[1]) ++nan_bits; else { ++bad; first = first < u1 ? first : u1; } }
    }
    if (bad) { atomicAdd(out, (unsigned long long)bad); atomicMin(out + 1, (unsigned long long)first); }
    if (nan_bits) atomicAdd(out + 2, (unsigned long long)nan_bits);
}

// the built-in sampling draw (swx_decode.h) as the selection kernels call it: the word and its variate of ids id0 .. id0 + n - 1
// (swx_test_sampler_words), the variate of every bucket k0 .. k0 + n - 1 (swx_test_sampler_buckets)
__global__ __launch_bounds__(256) void sampler_words_kernel(uint64_t seed, unsigned row_uid, unsigned step, unsigned id0, unsigned n,
                                                            uint32_t *__restrict__ words, float *__restrict__ variates)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    words[i] = sampler_word(seed, row_uid, step, id0 + i);
    variates[i] = gumbel(seed, row_uid, step, id0 + i);
}

__global__ __launch_bounds__(256) void sampler_buckets_kernel(unsigned k0, unsigned n, float *__restrict__ variates)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    variates[i] = sampler_variate((k0 + i) << 8);
}

extern "C" {

// ------------------------------------------------------------------------------------------------ test hooks
int swx_test_sampler_words(uint64_t seed, int64_t row_uid, int step, int id0, int n, uint32_t *d_words, float *d_variates, void *stream)
{
    if (!d_words || !d_variates || n <= 0 || step < 0 || id0 < 0 || (int64_t)id0 + n > (int64_t)1 << 31) return -1;
    hipLaunchKernelGGL(sampler_words_kernel, dim3(((unsigned)n + 255u) / 256u), dim3(256), 0, S(stream), seed, (unsigned)(uint64_t)row_uid,
                       (unsigned)step, (unsigned)id0, (unsigned)n, d_words, d_variates);
    SWX_CHECK_LAUNCH();
    return 0;
}

int swx_test_sampler_buckets(int k0, int n, float *d_variates, void *stream)
{
    if (!d_variates || n <= 0 || k0 < 0 || (int64_t)k0 + n > (int64_t)1 << 24) return -1;
    hipLaunchKernelGGL(sampler_buckets_kernel, dim3(((unsigned)n + 255u) / 256u), dim3(256), 0, S(stream), (unsigned)k0, (unsigned)n, d_variates);
    SWX_CHECK_LAUNCH();
    return 0;
}

int swx_test_gemm(int dtype, const void *d_a, int64_t lda, const void *d_w, const float *d_bias, const void *d_res,
                  void *d_c, int64_t ldc, int M, int N, int K, int epilogue, int force_kernel, void *stream)
{
    GemmArgs g = swx_gemm_args(d_a, lda, d_w, K, d_bias, d_c, ldc, M, N, K, epilogue);
    g.R = d_res; g.ldr = ldc;
    return swx_gemm(dtype, g, force_kernel, S(stream));
}

// the f16 kernel swx_gemm picks for a launch (contiguous, 16-byte aligned operands assumed): 0 register-staged tiled, 1 skinny,
// 2 / 3 direct-to-LDS at 128 / 64 columns, 4 / 5 ring at 64 / 128 columns, 6 the 256 x 256 kernel; < 0 = not offered.  No GPU needed.
int swx_test_gemm_plan(int M, int N, int K, int epilogue, int force_kernel, int flags)
{
    return swx_gemm_plan_f16(M, N, K, epilogue, N, N, true, force_kernel, flags);
}

int swx_test_dec_gemm(const void *d_a, int64_t lda, const void *d_w, const float *d_gamma, const float *d_beta, const float *d_bias,
                      void *d_c, int64_t ldc, void *d_x, void *d_kcache, void *d_vcache, const int32_t *d_pos0, int n_ctx, int d,
                      int M, int N, int K, int epilogue, void *d_scratch, size_t scratch_bytes, void *stream)
{
    return swx_test_dec_gemm_kl(d_a, lda, d_w, d_gamma, d_beta, d_bias, d_c, ldc, d_x, d_kcache, d_vcache, d_pos0, n_ctx, d, M, N, K, epilogue,
                                0, 0, d_scratch, scratch_bytes, stream);
}

int swx_test_dec_gemm_kl(const void *d_a, int64_t lda, const void *d_w, const float *d_gamma, const float *d_beta, const float *d_bias,
                         void *d_c, int64_t ldc, void *d_x, void *d_kcache, void *d_vcache, const int32_t *d_pos0, int n_ctx, int d,
                         int M, int N, int K, int epilogue, int rps, int k_chunked, void *d_scratch, size_t scratch_bytes, void *stream)
{
    if (k_chunked && (epilogue & DEC_QKV) && (n_ctx <= 0 || d <= 0 || d % 64)) return -2;
    // d_scratch: N*K halfs (folded weights) + 2N floats (c1, c2) + the slab floats of the shape, 256-byte aligned pieces
    hipStream_t s = S(stream);
    unsigned char *p = (unsigned char *)d_scratch;
    const size_t slab_b = align_up(swx_dec_slab_floats(M, N, K) * 4 + 256);
    const size_t need = align_up((size_t)N * K * 2) + 2 * align_up((size_t)N * 4) + slab_b + (size_t)SWX_DEC_TICKETS * 4;
    if (scratch_bytes < need) return -8;
    f16 *wf = (f16 *)p; p += align_up((size_t)N * K * 2);
    float *c1 = (float *)p; p += align_up((size_t)N * 4);
    float *c2 = (float *)p; p += align_up((size_t)N * 4);
    float *slabs = (float *)p; p += slab_b;
    int *ticket = (int *)p;
    // bit 7 of `epilogue`: the caller zeroed the counters ONCE and keeps one scratch buffer over its calls -- what the decode path does
    // (swx_bind_workspace zeroes, the last arriver of every launch resets); without it every call starts from fresh counters
    if (!(epilogue & 128)) { hipError_t e = hipMemsetAsync(ticket, 0, (size_t)SWX_DEC_TICKETS * 4, s); if (e != hipSuccess) return -100 - (int)e; }
    DecGemmArgs g{};
    g.A = (const f16 *)d_a; g.lda = lda; g.M = M; g.N = N; g.K = K; g.epi = epilogue; g.ldw = K;
    g.C = (f16 *)d_c; g.ldc = ldc; g.X = (f16 *)d_x; g.ldx = ldc; g.slabs = slabs; g.ticket = ticket;
    g.kcache = (f16 *)d_kcache; g.vcache = (f16 *)d_vcache; g.pos0 = d_pos0; g.n_ctx = n_ctx; g.d = d;
    g.epi = epilogue & 31;
    g.tall = (epilogue & 64) ? 1 : 0;                 // bit 6: a multi-token pass (the tall kernel from 161 rows on)
    g.rps = (epilogue & 64) && (epilogue & DEC_QKV) ? 7 : 0;      // (QKV scatter of the tall test: 7 rows per sequence)
    if (rps > 0 && (epilogue & DEC_QKV)) g.rps = rps;
    g.kl = swx_klayout(k_chunked ? 1 : 0, n_ctx, d);
    if ((epilogue & DEC_LN) && (epilogue & 32)) {     // bit 5: d_w is already folded, d_gamma / d_beta are c1 / c2 (timing runs)
        g.W = (const f16 *)d_w; g.c1 = d_gamma; g.c2 = d_beta;
    } else if (epilogue & DEC_LN) {
        SWX_TRY(swx_fold_ln(d_w, d_gamma, d_beta, d_bias, wf, c1, c2, N, K, s));
        g.W = wf; g.c1 = c1; g.c2 = c2;
    } else if (epilogue & 32) {                       // timing runs: d_w is taken as packed already
        g.W = (const f16 *)d_w; g.c2 = d_bias;
    } else {
        SWX_TRY(swx_fold_ln(d_w, nullptr, nullptr, nullptr, wf, nullptr, nullptr, N, K, s));      // re-pack only
        g.W = wf; g.c2 = d_bias;
    }
    return swx_gemm_dec(g, s);
}

int swx_test_self_attn_step(const void *d_q, void *d_kcache, void *d_vcache, const int32_t *d_anc, const int32_t *d_pos0,
                            int R, int H, int n_ctx, int d, int variant, void *d_o, void *stream)
{
    return swx_test_self_attn_step_kl(d_q, d_kcache, d_vcache, d_anc, d_pos0, R, H, n_ctx, d, variant, 0, d_o, stream);
}

int swx_test_self_attn_step_kl(const void *d_q, void *d_kcache, void *d_vcache, const int32_t *d_anc, const int32_t *d_pos0,
                               int R, int H, int n_ctx, int d, int variant, int k_chunked, void *d_o, void *stream)
{
    if (d != 64 * H) return -2;
    SelfAttnArgs sa{};
    sa.kl = swx_klayout(k_chunked ? 1 : 0, n_ctx, d);
    sa.qkv = d_q; sa.ldqkv = d; sa.kcache = d_kcache; sa.vcache = d_vcache; sa.anc = (int32_t *)d_anc; sa.pos0 = d_pos0;
    sa.o = d_o; sa.ldo = d; sa.R = R; sa.n_new = 1; sa.H = H; sa.n_ctx = n_ctx; sa.d = d; sa.skip_append = 1;
    sa.step_cached = variant < 2 ? 1 : 0;
    sa.pos_bound = variant == 0 ? 128 : 0;
    return swx_self_attention(SWX_F16, sa, 1, S(stream));
}

int swx_test_self_attn_multi(const void *d_q, void *d_kcache, void *d_vcache, int R, int H, int n_new, int n_ctx, int d, int mq,
                             void *d_o, void *stream)
{
    return swx_test_self_attn_multi_kl(d_q, d_kcache, d_vcache, R, H, n_new, n_ctx, d, mq, 0, d_o, stream);
}

int swx_test_self_attn_multi_kl(const void *d_q, void *d_kcache, void *d_vcache, int R, int H, int n_new, int n_ctx, int d, int mq,
                                int k_chunked, void *d_o, void *stream)
{
    static int32_t *d_zeros = nullptr;           // every row starts at position 0
    static int zeros_n = 0;
    if (R <= 0 || n_new <= 0 || n_new > n_ctx) return -2;
    if (zeros_n < R) {
        if (d_zeros) (void)hipFree(d_zeros);
        zeros_n = 0; d_zeros = nullptr;
        if (hipMalloc((void **)&d_zeros, (size_t)R * 4) != hipSuccess) return -3;
        zeros_n = R;
    }
    hipError_t e = hipMemsetAsync(d_zeros, 0, (size_t)R * 4, S(stream));
    if (e != hipSuccess) return -100 - (int)e;
    SelfAttnArgs sa{};
    sa.qkv = d_q; sa.ldqkv = d; sa.kcache = d_kcache; sa.vcache = d_vcache; sa.anc = nullptr; sa.pos0 = d_zeros;
    sa.o = d_o; sa.ldo = d; sa.R = R; sa.n_new = n_new; sa.H = H; sa.n_ctx = n_ctx; sa.d = d; sa.skip_append = 1;
    sa.pos0_all_zero = mq ? 1 : 0;
    if (k_chunked && d != 64 * H) return -2;
    sa.kl = swx_klayout(k_chunked ? 1 : 0, n_ctx, d);
    return swx_self_attention(SWX_F16, sa, 1, S(stream));
}

int swx_test_self_attn_general(int dtype, const void *d_qkv, int64_t ldqkv, void *d_kcache, void *d_vcache, const int32_t *d_anc,
                               const int32_t *d_pos0, int R, int H, int n_new, int n_ctx, int d, int row_mul, int skip_append,
                               int pos0_all_zero, void *d_o, void *stream)
{
    return swx_test_self_attn_general_kl(dtype, d_qkv, ldqkv, d_kcache, d_vcache, d_anc, d_pos0, R, H, n_new, n_ctx, d, row_mul, skip_append,
                                         pos0_all_zero, 0, 0, d_o, stream);
}

// step_variant: 0 = the multi-token kernels; 1 / 2 = n_new == 1 through the decode-step kernels with pos_bound 128 / unknown (the long-context
// kernels: with R * H <= 1024 the one that requests every load in two batches)
int swx_test_self_attn_general_kl(int dtype, const void *d_qkv, int64_t ldqkv, void *d_kcache, void *d_vcache, const int32_t *d_anc,
                                  const int32_t *d_pos0, int R, int H, int n_new, int n_ctx, int d, int row_mul, int skip_append,
                                  int pos0_all_zero, int step_variant, int k_chunked, void *d_o, void *stream)
{
    if (dtype != SWX_F16 && dtype != SWX_F32) return -1;
    if (k_chunked && dtype != SWX_F16) return -2;
    if (!d_qkv || !d_kcache || !d_vcache || !d_pos0 || !d_o) return -1;
    if (R <= 0 || H <= 0 || n_new <= 0 || n_ctx <= 0 || n_ctx > 512 || n_new > n_ctx || d != 64 * H || row_mul < 1) return -2;
    if (ldqkv < (skip_append ? d : 3 * d)) return -2;
    SelfAttnArgs sa{};
    sa.qkv = d_qkv; sa.ldqkv = ldqkv; sa.kcache = d_kcache; sa.vcache = d_vcache; sa.anc = (int32_t *)d_anc; sa.pos0 = d_pos0;
    sa.o = d_o; sa.ldo = d; sa.R = R; sa.n_new = n_new; sa.H = H; sa.n_ctx = n_ctx; sa.d = d; sa.skip_append = skip_append ? 1 : 0;
    sa.pos0_all_zero = pos0_all_zero ? 1 : 0;
    if (step_variant) { sa.step_cached = 1; sa.pos_bound = step_variant == 1 ? 128 : 0; }
    sa.kl = swx_klayout(k_chunked ? 1 : 0, n_ctx, d);
    return swx_self_attention(dtype, sa, row_mul, S(stream));
}

int swx_test_kcache_index(int k_chunked, int n_ctx, int d, int pos, int h, int chunk)
{
    if (n_ctx <= 0 || d <= 0 || d % 64 || pos < 0 || pos >= n_ctx || h < 0 || h >= d / 64 || chunk < 0 || chunk >= 8) return -1;
    return swx_kidx(swx_klayout(k_chunked ? 1 : 0, n_ctx, d), pos, h, chunk);
}

int swx_test_kcache_relayout(const void *h_src, void *h_dst, int64_t rows, int n_ctx, int d, int elem_bytes, int to_chunked)
{
    if (!h_src || !h_dst || h_src == h_dst || rows < 0 || n_ctx <= 0 || d <= 0 || d % 64 || elem_bytes <= 0) return -1;
    const KLayout rm = swx_klayout(0, n_ctx, d), ch = swx_klayout(1, n_ctx, d);
    const KLayout &from = to_chunked ? rm : ch, &to = to_chunked ? ch : rm;
    const size_t cb = (size_t)8 * elem_bytes, row_b = (size_t)n_ctx * d * elem_bytes;
    for (int64_t r = 0; r < rows; ++r)
        for (int pos = 0; pos < n_ctx; ++pos)
            for (int h = 0; h < d / 64; ++h)
                for (int c = 0; c < 8; ++c)
                    memcpy((unsigned char *)h_dst + r * row_b + (size_t)swx_kidx(to, pos, h, c) * elem_bytes,
                           (const unsigned char *)h_src + r * row_b + (size_t)swx_kidx(from, pos, h, c) * elem_bytes, cb);
    return 0;
}

int swx_test_self_attn_plan(int dtype, int R, int H, int n_new, int n_ctx, int row_mul, int skip_append, int step_cached, int pos_bound,
                            int pos0_all_zero, int has_anc, int flags)
{
    static int32_t some_table;                   // only whether a.anc is set matters to the plan
    SelfAttnArgs sa{};
    sa.anc = has_anc ? &some_table : nullptr;
    sa.R = R; sa.n_new = n_new; sa.H = H; sa.n_ctx = n_ctx; sa.d = 64 * H; sa.skip_append = skip_append;
    sa.step_cached = step_cached; sa.pos_bound = pos_bound; sa.pos0_all_zero = pos0_all_zero;
    return swx_self_attn_plan(dtype, sa, row_mul, flags);
}

int swx_test_dec_plan(int M, int N, int K, int epilogue, int flags)
{
    // `epilogue` as swx_test_dec_gemm reads it (bit 6: a multi-token pass); the hook hands in a ticket buffer always and X with bit 2
    int mt = 1, ks2 = 1;
    bool ticket = false;
    return swx_dec_kernel_plan(M, N, K, epilogue & 31, (epilogue & 64) ? 1 : 0, (epilogue & DEC_RES) != 0, flags, &mt, &ks2, &ticket);
}

int swx_test_layernorm(int dtype, const void *d_x, const float *d_g, const float *d_b, void *d_y, int rows, int d, void *stream)
{
    return swx_layernorm(dtype, d_x, d, d_g, d_b, d_y, d, rows, d, S(stream));
}

int swx_test_attention(int dtype, const void *d_q, int64_t ldq, const void *d_k, const void *d_v, int64_t ldkv, void *d_o,
                       int64_t ldo, int B, int H, int nq, int nk, int force_kernel, int vt_kp, void *stream)
{
    AttnArgs a{};
    a.q = d_q; a.ldq = ldq; a.k = d_k; a.v = d_v; a.ldkv = ldkv; a.o = d_o; a.ldo = ldo;
    a.k_bs = (int64_t)nk * ldkv; a.vt_kp = vt_kp;
    a.v_bs = vt_kp ? (int64_t)H * 64 * vt_kp : (int64_t)nk * ldkv;
    a.B = B; a.H = H; a.nq = nq; a.nk = nk; a.q_rows_per_batch = nq;
    return swx_attention(dtype, a, force_kernel, S(stream));
}

// swx_test_gemm with every field of GemmArgs the layout epilogues read.  A combination the kernels do not implement is refused here
// (-2) instead of launched: the column split of EPI_KV / EPI_QKV_VT has to fall on a tile boundary of the kernel the plan picks, both
// are f16 tiled-kernel epilogues, and the fragment-ordered copy is written by EPI_KV's fast paths only.
int swx_test_gemm_layout(int dtype, const void *d_a, int64_t lda, const void *d_w, int64_t ldw, const float *d_bias, const void *d_res,
                         const float *d_resf, int res_mod, void *d_c, int64_t ldc, void *d_c2, void *d_p, int64_t p_bs, int p_nkpad,
                         int p_vcol0, int vt_s, int vt_kp, int64_t vt_bs, int vt_zero_pad, int M, int N, int K, int epilogue,
                         int force_kernel, void *stream)
{
    if (dtype != SWX_F16 && dtype != SWX_F32) return -1;
    if (!d_a || !d_w || !d_c || M <= 0 || N <= 0 || K <= 0 || lda <= 0 || ldw < K) return -1;
    if ((epilogue & EPI_BIAS) && !d_bias) return -1;
    if ((epilogue & EPI_RES) && !d_res) return -1;
    if ((epilogue & EPI_RESF32MOD) && (!d_resf || res_mod <= 0)) return -1;
    const int layout = epilogue & (EPI_CBATCH | EPI_STORE_VT | EPI_KV | EPI_QKV_VT);
    if (layout && vt_s <= 0) return -1;
    if ((epilogue & (EPI_STORE_VT | EPI_KV | EPI_QKV_VT)) && vt_kp < vt_s) return -1;
    if (layout & (layout - 1)) return -2;                       // one layout epilogue per launch
    if (epilogue & (EPI_KV | EPI_QKV_VT)) {
        if (dtype != SWX_F16 || !d_c2) return -2;
        if ((epilogue & EPI_KV) ? N % 2 != 0 : N % 3 != 0) return -2;
        const int split = (epilogue & EPI_KV) ? N / 2 : (N / 3) * 2;
        const bool ptr16 = (uintptr_t)d_a % 16 == 0 && (uintptr_t)d_w % 16 == 0;
        const int plan = swx_gemm_plan_f16(M, N, K, epilogue, 1, 1, ptr16, force_kernel, swx_flags());
        if (plan < 0) return plan;
        if (plan == SWX_GEMM_SKINNY || plan == SWX_GEMM_BIG) return -2;
        const int width = (plan == SWX_GEMM_GLDS64 || plan == SWX_GEMM_RING64) ? 64 : 128;
        if (split % width != 0) return -2;
        // the transposed half and the key padding are written by the 4-row column-wise path only
        if (vt_s % 4 != 0 || vt_kp % 4 != 0 || vt_bs % 4 != 0 || M % 4 != 0) return -2;
    } else if (vt_zero_pad) return -2;
    if (d_p) {
        // ... and the copy's K pieces by the 16-byte row path only
        if (!(epilogue & EPI_KV) || ldc % 8 != 0 || vt_bs % 8 != 0 || p_bs % 8 != 0 || p_vcol0 != N / 2) return -2;
        if (p_nkpad != ((vt_s + 31) / 32) * 32 || (epilogue & (EPI_RES | EPI_GELU | EPI_OUT_F32 | EPI_RESF32MOD))) return -2;
    }
    GemmArgs g = swx_gemm_args(d_a, lda, d_w, ldw, d_bias, d_c, ldc, M, N, K, epilogue);
    g.R = d_res; g.ldr = ldc; g.Rf = d_resf; g.res_mod = res_mod > 0 ? res_mod : 1;
    g.C2 = d_c2; g.P = d_p; g.p_bs = p_bs; g.p_nkpad = p_nkpad; g.p_vcol0 = p_vcol0;
    g.vt_s = vt_s; g.vt_kp = vt_kp; g.vt_bs = vt_bs; g.vt_zero_pad = vt_zero_pad ? 1 : 0;
    return swx_gemm(dtype, g, force_kernel, S(stream));
}

int swx_test_xkv_pack(const void *d_k, const void *d_vt, void *d_packed, int B, int H, int nk, int ldk, int vt_kp, int64_t batch_stride,
                      void *stream)
{
    if (!d_k || !d_vt || !d_packed || B <= 0 || H <= 0 || nk <= 0) return -1;
    if (ldk < 64 * H || ldk % 8 != 0 || vt_kp % 8 != 0 || batch_stride % 8 != 0) return -2;
    return swx_xkv_pack(d_k, d_vt, d_packed, B, H, nk, ldk, vt_kp, batch_stride, S(stream));
}

// swx_test_attention (f16, transposed V) with the batch strides, the fragment-ordered copy and the fused query projection as arguments.
// d_wq != null: q = LN(x) Wq^T + b inside the launch -- the raw weights [d][d] (d = 64 H) are folded into d_scratch (d * d halfs +
// 2 d floats, 256-byte aligned pieces) as swx_test_dec_gemm_kl folds them for DEC_LN; d_q is not read; no prefetch target.
int swx_test_attention_packed(const void *d_q, int64_t ldq, const void *d_k, const void *d_v, int64_t ldkv, int64_t k_bs, int64_t v_bs,
                              const void *d_packed, void *d_o, int64_t ldo, int B, int H, int nq, int nk, int vt_kp, int force_kernel,
                              const void *d_x, int64_t ldx, int fq_rows, const void *d_wq, const float *d_gamma, const float *d_beta,
                              const float *d_bias, void *d_scratch, size_t scratch_bytes, void *stream)
{
    if (!d_o || B <= 0 || H <= 0 || nq <= 0 || nk <= 0 || vt_kp <= 0) return -1;
    if (!d_packed && (!d_k || !d_v)) return -1;
    if (!d_wq && !d_q) return -1;
    if (vt_kp % 8 != 0 || vt_kp < ((nk + 31) / 32) * 32 || k_bs % 8 != 0 || v_bs % 8 != 0 || ldo < 64 * H) return -2;
    if (d_k && (ldkv < 64 * H || ldkv % 8 != 0)) return -2;
    hipStream_t s = S(stream);
    AttnArgs a{};
    a.q = d_q; a.ldq = ldq; a.k = d_k; a.v = d_v; a.ldkv = ldkv; a.o = d_o; a.ldo = ldo;
    a.k_bs = k_bs; a.v_bs = v_bs; a.vt_kp = vt_kp; a.kv_packed = d_packed;
    a.B = B; a.H = H; a.nq = nq; a.nk = nk; a.q_rows_per_batch = nq;
    if (d_wq) {
        const int d = 64 * H;
        if (!d_x || !d_gamma || !d_beta || !d_bias || !d_scratch) return -1;
        if (ldx < d || ldx % 8 != 0 || fq_rows < (B - 1) * nq + 1) return -2;
        if (scratch_bytes < align_up((size_t)d * d * 2) + 2 * align_up((size_t)d * 4)) return -8;
        unsigned char *p = (unsigned char *)d_scratch;
        f16 *wf = (f16 *)p; p += align_up((size_t)d * d * 2);
        float *c1 = (float *)p; p += align_up((size_t)d * 4);
        float *c2 = (float *)p;
        SWX_TRY(swx_fold_ln(d_wq, d_gamma, d_beta, d_bias, wf, c1, c2, d, d, s));
        a.fq_x = (const f16 *)d_x; a.fq_ldx = ldx; a.fq_rows = fq_rows; a.fq_w = wf; a.fq_c1 = c1; a.fq_c2 = c2; a.fq_k = d;
    } else if (ldq < 64 * H || ldq % 8 != 0) return -2;
    return swx_attention(SWX_F16, a, force_kernel, s);
}

int swx_test_xattn_plan(int B, int H, int nq, int nk, int vt_kp, int has_packed, int has_fq, int force_kernel, int flags)
{
    static const _Float16 some_memory[1] = {};   // only whether a.kv_packed / a.fq_w are set matters to the plan
    if (B <= 0 || H <= 0 || nq <= 0 || nk <= 0) return -1;
    AttnArgs a{};
    a.B = B; a.H = H; a.nq = nq; a.nk = nk; a.vt_kp = vt_kp; a.q_rows_per_batch = nq;
    a.kv_packed = has_packed ? some_memory : nullptr;
    if (has_fq) { a.fq_w = some_memory; a.fq_k = 64 * H; }
    const SwxXattnPlan p = swx_xattn_plan(SWX_F16, a, force_kernel, flags);
    return p.family < 0 ? p.family : p.family + 16 * p.qg + 256 * p.depth;
}

int swx_test_lds_grants(const int *dev, const int *ok, int n, int *state_out)
{
    if (n < 0 || (n > 0 && (!dev || !ok)) || !state_out) return -1;
    for (int i = 0; i < n; ++i)
        if (!SwxLdsGrants::tracked(dev[i])) return -5;
    SwxLdsGrants t;
    for (int i = 0; i < n; ++i) t.record(dev[i], ok[i] != 0);
    for (int d = 0; d < 64; ++d) state_out[d] = t.state(d);
    return 0;
}

int swx_test_lane_xor(const uint32_t *d_in, uint32_t *d_out, int n_waves, void *stream)
{
    if (!d_in || !d_out || n_waves <= 0) return -1;
    hipLaunchKernelGGL(lane_xor_check_kernel, dim3(n_waves), dim3(64), 0, S(stream), d_in, d_out);
    SWX_CHECK_LAUNCH();
    return 0;
}

int swx_test_gelu_pair(uint64_t *d_out, void *stream)
{
    if (!d_out) return -1;
    hipStream_t s = S(stream);
    const unsigned long long init[3] = {0ull, 0xffffffffull, 0ull};
    hipError_t e = hipMemcpyAsync(d_out, init, sizeof(init), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);            // `init` is a stack-lifetime staging buffer
    if (e != hipSuccess) return -100 - (int)e;
    hipLaunchKernelGGL(gelu_pair_check_kernel, dim3(1u << 19), dim3(256), 0, s, (unsigned long long *)d_out);
    SWX_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
