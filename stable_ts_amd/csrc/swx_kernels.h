// swx_kernels.h -- internal launcher prototypes shared by the translation units of libswx.so
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/swx.h"

#define EPI_BIAS 1
#define EPI_GELU 2
#define EPI_RES 4
#define EPI_OUT_F32 8
#define EPI_RESF32MOD 16
#define EPI_CBATCH 64        // C rows are grouped in batch items of vt_s rows, vt_bs elements apart (row-major inside an item)
#define EPI_STORE_VT 32     // store C transposed per head: C[((row / vt_s) * (N/64) + col/64) * 64 + col%64][row % vt_s] with row stride vt_kp
#define EPI_KV 128          // f16 tiled kernels only: ONE launch for the cross-attention K and V projections of a layer (fused weight rows
                            // [2d][d]): columns [0, N/2) are stored like EPI_CBATCH into C, columns [N/2, N) like EPI_STORE_VT into C2
                            // (column index relative to N/2); N/2 is a multiple of the tile width, so a tile is one or the other

#define EPI_QKV_VT 256      // f16 tiled kernels only (round 6): the encoder's fused Q|K|V projection with V stored TRANSPOSED per head for the
                            // flash kernel -- columns [0, 2N/3) plain into C, columns [2N/3, N) like EPI_STORE_VT into C2 (column index relative
                            // to 2N/3; vt_zero_pad: the key padding [vt_s, vt_kp) of every column is zeroed by the tile that ends a batch item)

struct GemmArgs {
    const void *A; int64_t lda;     // [M][K] compute dtype
    const void *W; int64_t ldw;     // [N][K] compute dtype
    const float *bias;              // [N] or null
    const void *R; int64_t ldr;     // residual, compute dtype (may alias C)
    const float *Rf; int res_mod;   // f32 residual [res_mod][N], row index = m % res_mod
    void *C; int64_t ldc;           // compute dtype, or f32 with EPI_OUT_F32
    void *C2;                       // EPI_KV: base of the transposed half
    void *P; int64_t p_bs;          // EPI_KV, optional (round 6): the fragment-ordered copy of K / V^T the decode-step cross-attention streams
    int p_nkpad, p_vcol0;           // (swx_xkv_packed_elems_per_head) written by the same epilogue instead of by swx_xkv_pack: base of batch item
                                    // 0, batch stride in elements, keys per head rounded up to 32 (the padding keys are zeroed), first V column
    int M, N, K;
    int epi;
    int vt_s, vt_kp; int64_t vt_bs;   // EPI_STORE_VT: rows per batch item, padded key stride, element stride between batch items
    int vt_zero_pad;                  // EPI_STORE_VT fast path: also write zeros to keys [vt_s, vt_kp) of the columns it stores
    int tile_order;                   // gemm_f16_big8 only, set by swx_gemm: 0 = row-major, 1 = an XCD's concurrent tiles share a band of
                                      // weights that fits its L2 (groups of 4 column tiles, walked along M; SWX_FLAG_BIG8_GROUPED)
};
int swx_gemm(int dtype, const GemmArgs &g, int force_kernel, hipStream_t s);
// the f16 kernel a launch gets (swx_gemm.hip; a pure function of the shape, the epilogue and the switches)
enum { SWX_GEMM_TILED_REG = 0, SWX_GEMM_SKINNY = 1, SWX_GEMM_GLDS128 = 2, SWX_GEMM_GLDS64 = 3, SWX_GEMM_RING64 = 4, SWX_GEMM_RING128 = 5,
       SWX_GEMM_BIG = 6 };
int swx_gemm_plan_f16(int M, int N, int K, int epi, int64_t ldc, int64_t ldr, bool ptr16, int force_kernel, int flags);

// ---- run-time A/B switches (swx_debug_flags(); tests and scripts only -- no environment variable reads them).  Each one
//      selects the bit-identity / parity REFERENCE of a kernel class; the superseded generations these flags used to keep
//      alive (split-K decode step, flash attention v1, DTW generation 2, the tiled-GEMM variants that lost) were deleted in
//      round 3.
//      ONE list, (name, bit index) in bit order: SWX_FLAG_<name> = 1 << bit.  The static_asserts below it fail the build when two
//      entries share a bit or an index leaves 0..30 (swx_debug_flags(-1) is the "read" sentinel, so bit 31 cannot be a switch).
//      Free: 3, 12, 29, 30.  bench.py --debug-flags / --ab-flags, the tests and the recorded profiles name switches by their
//      integers, so an entry keeps its bit for good.
#define SWX_FLAG_TABLE(X) \
    X(NO_FAST_STEP, 0)        /* decode steps / small passes go through the generic per-op path (LayerNorm launches, row-major weights, \
                                 skinny / tiled GEMMs): the reference of the fused "dec" step */ \
    X(KCACHE_CHUNKED, 1)      /* f16 decode: the self-attention K cache in position-contiguous 16-byte chunks per head (KLayout below) instead of \
                                 row-major [n_ctx][d] like the V cache.  Bit-identical.  Measured: the step kernel 9.67 vs 9.75 us in the headline \
                                 pass, whose passes it does not separate (407.5-408.5 vs 406.2-407.4 ms); sequential mode 4 600-4 610 vs \
                                 4 650-4 689 ms; stand-alone 15 % slower when neighbouring keys come from different beams, 14 % faster when \
                                 from one row.  Off by default (profiles/kcache_layout_*) */ \
    X(SELFATTN_NO_DEEP, 2)    /* decode-step self-attention, long context at <= 1 024 waves: the chunk-by-chunk kernel instead of every load in \
                                 two batches (A/B; bit-identical) */ \
    X(DEC_NO_W1, 4)           /* decode-step GEMM at <= 80 workgroups: four-wave workgroups instead of single-wave ones (A/B; bit-identical) */ \
    X(TALL_NO_W8, 5)          /* tall dec GEMM: four waves = one 64-column panel per workgroup (rounds 4-5) instead of eight waves = two panels \
                                 (A/B; bit-identical) */ \
    X(FLASH_NO_QB1, 6)        /* f16 flash attention of launches with <= 256 workgroups at 32 queries per wave: 32 queries per wave (rounds 3-5) \
                                 instead of 16 (A/B; bit-identical) */ \
    X(XKV_PACK_SEPARATE, 7)   /* cross-K/V: the fragment-ordered copy by its own launch (swx_xkv_pack, rounds 2-5) instead of by the \
                                 projection's epilogue (A/B; the same bytes) */ \
    X(SELFATTN_NO_MQ, 8)      /* multi-token self-attention: one wave per (row, token, head) reading K / V from L2 (rounds 1-5) instead of 4-8 \
                                 tokens per workgroup from LDS (A/B; bit-identical) */ \
    X(XQ_FULL_TILE, 9)        /* decode cross-attention's fused query projection: DMA all 16 rows of the residual tile instead of the window's \
                                 nq rows (A/B; bit-identical) */ \
    X(DEC_W1_FULL_TILE, 10)   /* single-wave dec GEMM workgroups: DMA all 16 rows of the activation tile (rows past M clamped) instead of the \
                                 rows that exist (A/B; bit-identical).  Shared bit 8 with SELFATTN_NO_MQ when round 6 measured it */ \
    X(NO_PACKED_XKV, 11)      /* decode cross-attention reads the row-layout K / V^T instead of the fragment-ordered copy */ \
    X(SELECT_MEM, 13)         /* logit filters + token selection: the kernel that walks the row in memory (reference of the register-resident \
                                 kernel, and its fallback for vocabularies > 51 * 1024) */ \
    X(NO_GRAPH, 14)           /* decode loop: launch every step eagerly instead of replaying the captured two-step graph */ \
    X(NO_PREFETCH, 15)        /* decode step: no cache prefetch of the next projection's weights (A/B; no functional effect) */ \
    X(NO_RING, 16)            /* tiled GEMM: never the ring kernel for launches with few tiles (A/B; results are bit-identical) */ \
    X(NO_BIG_TILE, 17)        /* tiled GEMM: never the 256 x 256 kernel (A/B; results are bit-identical) */ \
    X(SCORE_TILED, 18)        /* multi-token decoder passes above 160 rows on the tiled GEMMs + flash attention (round 3's dispatch: faster at \
                                 >= 2 windows, but a window's rounding then depends on its batch) -- A/B only */ \
    X(NO_TALL, 19)            /* multi-token passes: never the tall dec GEMM (register-resident weights, 16-row tiles): A/B, bit-identical */ \
    X(NO_FUSED_XQ, 20)        /* decode step: cross-attention query projection as a launch of its own instead of inside the cross-attention \
                                 kernel (A/B; bit-identical) */ \
    X(TICKET, 21)             /* decode step: the K-split projection's slabs reduced INSIDE the GEMM launch by the last-arriving K slice \
                                 (DEC_TICKET) instead of by dec_slab_finish.  Built and measured in round 5 in two forms, both bit-identical: \
                                 plain slab stores + agent-scope release / acquire fences 451.8 vs 432.6 ms per headline pass (the launch \
                                 17.0 us against 8.2 + 5.0); write-through `sc1` slab stores + drained ticket + `sc1` reads (the form kept) \
                                 432.4 vs 430.1 ms -- break-even at best, so off by default; kept for A/B \
                                 (profiles/r05_c5_bench_ticket_ab.json, r05_c12_bench_ticket_sc1_ab.json). */ \
    X(BIG8_GROUPED, 22)       /* 256 x 256 GEMM: tiles listed in groups of 4 column tiles walked along M instead of row-major (A/B; \
                                 bit-identical).  Built in round 6 to cut the N = 5120 launch's 3.8x fabric traffic: measured neutral to 3 % \
                                 SLOWER at every encoder shape (profiles/r06_c2_kb_gemm_big_tile_order.txt), so off by default */ \
    X(XKV_TWO_LAUNCHES, 23)   /* cross-K/V projection as two launches (K, then V) instead of one over the fused weight rows (A/B; bit-identical) */ \
    X(LOUDNESS_ONE_WG, 24)    /* silence analysis probe: always the one-workgroup-per-window selection kernel (A/B; the same element) */ \
    X(XATTN_R5, 25)           /* decode cross-attention: one key block per wave in flight, default load policy (rounds 2-5) instead of two + nt \
                                 (A/B; bit-identical) */ \
    X(FLASH_PIPELINED, 26)    /* f16 flash attention: the software-pipelined tile attn_flash3_f16 (round 6: bit-identical, measured 4 % SLOWER \
                                 than generation 2 -- DESIGN.md section 7) instead of attn_flash2_f16 */ \
    X(SELFATTN_WG5, 27)       /* decode-step self-attention: five rows (the beams of a window) per workgroup instead of one wave per workgroup \
                                 (A/B; the same arithmetic per row) */ \
    X(QKV_SEPARATE_VT, 28)    /* encoder at few windows: V transposed by its own launch instead of by the QKV projection's epilogue (A/B; \
                                 bit-identical) */
#define SWX_FLAG_DEFINE(name, bit) constexpr int SWX_FLAG_##name = 1 << (bit);
SWX_FLAG_TABLE(SWX_FLAG_DEFINE)
#undef SWX_FLAG_DEFINE
#define SWX_FLAG_IN_RANGE(name, bit) && (bit) >= 0 && (bit) <= 30
#define SWX_FLAG_OR(name, bit) | (int64_t(1) << (bit))
#define SWX_FLAG_SUM(name, bit) + (int64_t(1) << (bit))
static_assert(true SWX_FLAG_TABLE(SWX_FLAG_IN_RANGE), "SWX_FLAG_TABLE: a bit index outside 0..30");
static_assert((int64_t(0) SWX_FLAG_TABLE(SWX_FLAG_OR)) == (int64_t(0) SWX_FLAG_TABLE(SWX_FLAG_SUM)), "SWX_FLAG_TABLE: two switches share a bit");
#undef SWX_FLAG_IN_RANGE
#undef SWX_FLAG_OR
#undef SWX_FLAG_SUM
#define SWX_DEFAULT_FLAGS 0
int swx_flags();

// ---- layout of a row of the decoder self-attention K cache.  A row is always n_ctx * d elements at row * n_ctx * d; what the
//      descriptor says is where element (pos, h, dim) lies INSIDE it, as three element strides:
//        row-major [n_ctx][d]        sp = d, sh = 64,         sc = 8          (the V cache, the f32 engine, the scoring-pass cache)
//        chunked   [H][8][n_ctx][8]  sp = 8, sh = 64 * n_ctx, sc = 8 * n_ctx  (the f16 decode cache under SWX_FLAG_KCACHE_CHUNKED)
//      The step kernels give lane j key j and fetch its head's 128 bytes as eight 16-byte loads: row-major, one wave-instruction
//      touches 64 cache lines 2 d bytes apart; chunked, load e of lane j is base(row, h) + e * n_ctx * 16 + 16 j -- 1 024
//      contiguous bytes per run of lanes that share an ancestor row.  Every reader and writer of the K cache computes its
//      addresses with swx_kidx (the readers' row-major instantiations with its strides as compile-time constants); sp == 0 (a
//      zero-initialised descriptor) means row-major and is filled in by the launchers.
struct KLayout { int sp, sh, sc; };      // element strides: position, head, 8-dim chunk of a head
__host__ __device__ inline KLayout swx_klayout(int chunked, int n_ctx, int d)
{
    return chunked ? KLayout{8, 64 * n_ctx, 8 * n_ctx} : KLayout{d, 64, 8};
}
// element offset inside a cache row of the first of the 8 dims of chunk `chunk` (dims 8 chunk .. 8 chunk + 7) of head h at `pos`
__host__ __device__ inline int swx_kidx(const KLayout &L, int pos, int h, int chunk) { return h * L.sh + chunk * L.sc + pos * L.sp; }

// ---- decode-step GEMM (swx_decstep.hip): M split over workgroups, K whole -> the kernel finishes its own outputs (no f32
//      slabs, no finish launch), LayerNorm folded into the consumer (statistics from the staged tile)
#define DEC_LN 1        // out = rstd[m] * (acc - mean[m] * c1[n]) + c2[n]   (A = raw residual stream, W = gamma-folded weights)
#define DEC_GELU 2
#define DEC_RES 4       // X[m][n] = f16(X + c2[n] + acc)   (in place)
#define DEC_QKV 8       // columns [0,d) -> C, [d,2d) -> kcache[m][pos0[m]], [2d,3d) -> vcache[m][pos0[m]]
#define DEC_SLAB 16     // K-split allowed: f32 partials to slabs + dec_slab_finish (needs DEC_RES)
#define DEC_TICKET 32   // (launcher-internal, with DEC_SLAB | DEC_RES) the slab reduction INSIDE the launch: the K slices of a (panel, row
                        // group) draw a ticket after publishing their slab; the last arriver reduces (dec_slab_finish's arithmetic)
// The packed weights of the projection that runs NEXT in the decode step, for the cache prefetch the current kernel issues: a few
// loads per wave whose results nobody reads, one per 128-byte line, dealt over the lanes of the launch in order.  What gets warm
// is the memory-side Infinity Cache (the consumer's FETCH_SIZE does not drop, its latency does: section 5 of DESIGN.md), so
// where a line's load is issued from does not matter.  No functional effect.  base == null: nothing to prefetch.
struct DecPrefetch {
    const void *base;                    // packed weights, N * K halfs, contiguous
    int lines;                           // N * K * 2 / 128
};
DecPrefetch swx_dec_prefetch_of(const void *packed_w, int M, int N, int K, int epi);

struct DecGemmArgs {
    const _Float16 *A; int64_t lda;      // [M][K]
    const _Float16 *W; int64_t ldw;      // PACKED weights (swx_fold_ln: [N/16][K/32][64][8], MFMA fragment order); ldw unused
    int M, N, K;
    int epi;
    const float *c2;                     // [N] bias (or folded bias with DEC_LN)
    const float *c1;                     // [N] column sums of the folded weights (DEC_LN)
    _Float16 *C; int64_t ldc;
    _Float16 *X; int64_t ldx;
    float *slabs;                        // swx_dec_slab_floats(M, N, K) floats when the shape runs K-split
    int *ticket;                         // K-split shapes of the decode-step kernel: SWX_DEC_TICKETS zeroed ints (self-resetting arrival
                                         // counters per (panel, row group)) -> the slab reduction runs inside the launch; null: dec_slab_finish
    _Float16 *kcache, *vcache; const int32_t *pos0; int n_ctx, d;
    KLayout kl;                          // DEC_QKV: layout of a K cache row (zeros: row-major)
    int rps;                             // DEC_QKV: rows per sequence (0 / 1: one new token per row); row m = sequence m / rps, token m % rps
    int row_mul;                         // DEC_QKV: cache row (and pos0 index) of sequence q = q * row_mul (0 / 1: q itself; the prefill writes row w * G)
    int ks2, kslice, n_rg; int64_t slab_stride;   // filled by the launcher
    int tall;                            // caller: 1 = a multi-token pass (rows may run into the thousands): from 161 rows on the launcher takes the
                                         // kernel that keeps the weights in registers and walks 16-row tiles (same arithmetic per element)
    int tps;                             // launcher (tall kernel): 16-row tiles per workgroup; n_rg = row splits
    DecPrefetch pf;                      // cache prefetch of the NEXT projection's weights (pf.base == null: none)
    int w1_full_tile;               // single-wave workgroups: stage the whole 16-row tile although fewer rows exist (A/B: SWX_FLAG_DEC_W1_FULL_TILE)
};
#define SWX_DEC_TICKETS 4096
int swx_dec_plan(int M, int N, int K, int epi, int *mt, int *ks2);    // <0: shape not supported by this generation
size_t swx_dec_slab_floats(int M, int N, int K);
int swx_gemm_dec(DecGemmArgs g, hipStream_t s);
// which kernel swx_gemm_dec launches (pure: the function the launcher itself executes; swx_test_dec_plan).  `epi`: the DEC_* bits of the
// call, `tall`: DecGemmArgs::tall, `ticket_ok`: a ticket buffer and X were handed in, `flags`: swx_debug_flags.  < 0: shape not offered.
enum SwxDecKernel { SWX_DEC_K_W4 = 0,        // gemm_dec_f16, four-wave workgroups (1-3 row tiles per workgroup)
                    SWX_DEC_K_W1 = 1,        // gemm_dec_f16, single-wave workgroups
                    SWX_DEC_K_TALL4 = 2,     // gemm_dectall_f16, four waves = one panel per workgroup
                    SWX_DEC_K_TALL8 = 3 };   // gemm_dectall_f16, eight waves = two panels per workgroup
int swx_dec_kernel_plan(int M, int N, int K, int epi, int tall, bool ticket_ok, int flags, int *mt, int *ks2, bool *ticket);
// load-time LayerNorm fold + re-pack into MFMA fragment order: Wf = pack(f16(W * gamma)), c1[n] = sum_k Wf[n][k],
// c2[n] = bias[n] + sum_k beta[k] W[n][k];  gamma == null: plain re-pack of W (c1 / c2 untouched)
int swx_fold_ln(const void *W, const float *gamma, const float *beta, const float *bias, void *Wf, float *c1, float *c2,
                int N, int K, hipStream_t s);

// ---- in-library kernel timing (HIP events on the launch stream), used by bench.py for the roofline object
enum SwxProfClass { PC_GEMM_TILED = 0, PC_GEMM_SKINNY = 1, PC_ATTN_FLASH = 2, PC_ATTN_ROWWISE = 3, PC_SELF_ATTN = 4,
                    PC_SELECT = 5, PC_MEL = 6, PC_ALIGN = 7, PC_DTW = 8, PC_NORM = 9, PC_COUNT = 10 };
bool swx_prof_on();
void swx_prof_begin(int cls, double work, hipStream_t s);   // work = algorithmic flops (MFMA classes) or bytes (HBM classes)
void swx_prof_end(hipStream_t s);
struct SwxProfScope {
    hipStream_t s; bool on;
    SwxProfScope(int cls, double work, hipStream_t st) : s(st), on(swx_prof_on()) { if (on) swx_prof_begin(cls, work, st); }
    ~SwxProfScope() { if (on) swx_prof_end(s); }
};

// ---- swx_norm.hip
int swx_layernorm(int dtype, const void *x, int64_t ldx, const float *gamma, const float *beta, void *y, int64_t ldy,
                  int rows, int d, hipStream_t s);
// melT[b][t+1][c] (c < Cp, zero padded; rows 0 and 3001 zero) <- mel[b][c][t]
int swx_mel_transpose(int dtype, const float *mel, int B, int n_mels, int Cp, void *melT, hipStream_t s);
int swx_fill_zero(void *p, size_t bytes, hipStream_t s);
// x[r][i] = tok_emb[tokens[r*ld_tok + i]] + pos_emb[pos0[r] + i]  for i < n_new[r] (rows of d)
int swx_embed(int dtype, const int32_t *tokens, int64_t ld_tok, const int32_t *tok_off, const int32_t *pos0, int R, int n_new,
              const void *tok_emb, const float *pos_emb, int d, void *x, hipStream_t s);
int swx_convert_f32(int dtype, const float *src, void *dst, int64_t n, hipStream_t s);
// strided/re-laid-out weight copies used by swx_load_tensor
int swx_copy_rows(int dtype, const float *src, int64_t src_ld, void *dst, int64_t dst_ld, int64_t rows, int64_t cols,
                  hipStream_t s);
int swx_copy_conv_w(int dtype, const float *src, int out_c, int in_c, int in_cp, void *dst, hipStream_t s);

// ---- swx_attn.hip
struct AttnArgs {
    const void *q; int64_t ldq;      // [B*nq][...] head h at column h*64
    const void *k; const void *v; int64_t ldkv;   // row stride of K (and of V when it is row-major); head h at column h*64
    int64_t k_bs, v_bs;              // element stride between batch items of K / V
    int vt_kp;                       // 0: V row-major [nk][ldkv]; >0: V transposed per batch item [H][64][vt_kp] (keys contiguous)
    void *o; int64_t ldo;
    int B, H, nq, nk;
    int q_rows_per_batch;            // rows of q per batch item (== nq unless grouped)
    const void *kv_packed;           // decode cross-attention: K and V^T of batch item 0 in MFMA fragment order (swx_xkv_pack),
                                     // batch stride k_bs; null = read a.k / a.v
    // decode step only (nq <= 16, packed K / V^T): the cross-attention QUERY projection folded into the attention launch --
    // q = LN(x) Wcq^T + b computed per (window, head) from the raw residual rows with the decode-step GEMM's arithmetic
    // (packed LayerNorm-folded weights, swx_fold_ln), instead of a launch of its own; a.q is not read then.  fq_w == null: off.
    const _Float16 *fq_x; int64_t fq_ldx; int fq_rows;      // residual stream [fq_rows][d]; window b owns rows b * q_rows_per_batch ..
    const _Float16 *fq_w; const float *fq_c1, *fq_c2; int fq_k;   // packed folded weights [d][fq_k], column constants
    const void *fq_pf; int fq_pf_lines;                     // weights to touch for the NEXT projection (cache prefetch), or null
    int fq_full_tile;                                       // A/B (SWX_FLAG_XQ_FULL_TILE): stage all 16 rows of the residual tile, not only the nq that exist
    // strict f32: take the query-block kernel also at nq <= 16.  nq is the LONGEST window's token count in a multi-token pass: with
    // the key-split kernel below 17 queries, a short window's numbers would depend on the windows it shares the pass with
    int f32_no_split;
};
#define SWX_VT_KP 1536               // padded key count of the transposed cross-attention V (64-key tiles never run off a row)
// dense (non-causal) attention over nk keys: encoder self-attention and cross-attention
int swx_attention(int dtype, const AttnArgs &a, int force_kernel, hipStream_t s);
// V [B][n][ldv] -> per-head transposed V^T [B][H][64][kp] (keys contiguous, zero padded): feeds the MFMA flash kernel's vector path
int swx_transpose_v(const void *v, int64_t ldv, int64_t v_bs, int n, void *vt, int kp, int64_t vt_bs, int B, int H, hipStream_t s);
int swx_pad_zero(void *base, int64_t row_bytes, int64_t batch_bytes, int off_bytes, int pad_bytes, int rows, int nb, hipStream_t s);

// ---- swx_xattn.hip: the decode-step cross-attention behind swx_attention
// fragment-ordered copy of one layer's cross K / V^T for the decode-step cross-attention: per (window, head)
// [K: blocks of 32 keys x 4 fragments x 64 lanes x 8 halfs | V^T: the same], zero padded past nk
__host__ __device__ inline int64_t swx_xkv_packed_elems_per_head(int nk) { return (int64_t)((nk + 31) / 32) * 4 * 512 * 2; }
int swx_xkv_pack(const void *k, const void *vt, void *packed, int B, int H, int nk, int ldk, int vt_kp, int64_t batch_stride,
                 hipStream_t s);
// whether swx_attention runs a launch on the decode cross-attention kernel, and on which form of it (pure: the function the launcher
// itself executes; swx_test_xattn_plan).  Reads the scalar fields of `a` and whether a.kv_packed / a.fq_w are set, no memory.
// `flags`: swx_debug_flags.  family < 0: the error swx_attention returns.
enum SwxXattnFamily { SWX_XA_NOT_DECODE = 0,     // flash / f32 / row-wise kernels
                      SWX_XA_ROW = 1,            // attn_decode_cross_f16<false, QG>: row-layout K / V^T
                      SWX_XA_PACKED = 2,         // attn_decode_cross2_f16<true, QG> (depth 2) / attn_decode_cross_f16<true, QG> (depth 1)
                      SWX_XA_PACKED_FQ = 3 };    // attn_decode_cross_xq2_f16<FQ> (depth 2) / attn_decode_cross_xq_f16<FQ> (depth 1)
struct SwxXattnPlan { int family, qg, depth; };  // qg: groups of 16 query rows per workgroup; depth: key blocks of a wave in flight
SwxXattnPlan swx_xattn_plan(int dtype, const AttnArgs &a, int force_kernel, int flags);
// the launch of a decode family (p.family > 0) of that plan.  Called by swx_attention alone, after its own checks of the shape and
// of the plan's error (their order decides the code of a doubly invalid input, so they stay there)
int swx_xattn_launch(const SwxXattnPlan &p, const AttnArgs &a, hipStream_t s);

// ---- swx_selfattn.hip
// decoder self-attention over the per-row KV cache with ancestor indirection
struct SelfAttnArgs {
    const void *qkv; int64_t ldqkv;  // [R*n_new][3d]: q | k | v of the new tokens
    void *kcache; void *vcache;      // [Mphys][n_ctx][d]
    int32_t *anc;                    // [rows][n_ctx] cache row holding position p of a logical row (null = identity)
    const int32_t *pos0;             // [R] position of the first new token of each row
    void *o; int64_t ldo;            // [R*n_new][d]
    int R, n_new, H, n_ctx, d;
    int skip_append;                 // K/V of the new tokens were already scattered into the cache (QKV projection's epilogue)
    int step_cached;                 // n_new == 1, f16: q at a.qkv (row stride ldqkv), the new K/V already appended -> the
                                     // latency-optimised single-token kernel of the decode step
    int step_pos;                    // profiler only: position of the new token when the host knows it (decode loop), else 0
    int pos_bound;                   // decode step: an upper bound of every row's position known to the host (initial tokens + sample
                                     // budget), or 0 = unknown.  <= 128: the kernel variant without the code for positions >= 128
    int pos0_all_zero;               // multi-token pass: the host knows that every row starts at position 0 (a.pos0 is the zeros array):
                                     // several tokens of a (row, head) per workgroup with K / V staged in LDS (self_attn_cached_mq_f16)
    KLayout kl;                      // layout inside a K cache row (zeros: row-major); the V cache is always row-major
};
// logical row of grid index ri is ri * row_mul (prefill of beam groups computes one row per window)
int swx_self_attention(int dtype, const SelfAttnArgs &a, int row_mul, hipStream_t s);
// which kernel swx_self_attention launches for these arguments (pure: the function the launcher itself executes; swx_test_self_attn_plan).
// Reads the scalar fields of `a` and whether a.anc is set, no memory.  `flags`: swx_debug_flags.  < 0: the error swx_self_attention returns.
enum SwxSelfAttnKernel { SWX_SA_K_CACHED_F16 = 0,      // self_attn_cached<f16> (after kv_append_kernel<f16> unless skip_append)
                         SWX_SA_K_CACHED_F32 = 1,      // self_attn_cached<float> (the same)
                         SWX_SA_K_MQ4 = 2,             // self_attn_cached_mq_f16<4>
                         SWX_SA_K_MQ8 = 3,             // self_attn_cached_mq_f16<8>
                         SWX_SA_K_STEP = 4,            // self_attn_step_f16<false, 1>
                         SWX_SA_K_STEP_WG5 = 5,        // self_attn_step_f16<false, 5>
                         SWX_SA_K_STEP_LONG = 6,       // self_attn_step_f16<true, 1>
                         SWX_SA_K_STEP_LONG_WG5 = 7,   // self_attn_step_f16<true, 5>
                         SWX_SA_K_STEP_DEEP = 8 };     // self_attn_step_long_f16
int swx_self_attn_plan(int dtype, const SelfAttnArgs &a, int row_mul, int flags);
// raw scaled qk of selected heads: out[w][hi][i][f] = 0.125 * q[w][row0+i][head] . k[w][f][head]
int swx_qk_capture(int dtype, const void *q, int64_t ldq, int q_rows_per_w, int row0, int n_rows, const void *k,
                   int64_t ldk, int64_t k_bs, int nk, const int32_t *heads, int n_heads, int head_slot0, int slots_total, int W,
                   float *out, int out_ld_n, int out_ld_f, hipStream_t s);

// ---- swx_align.hip / swx_mel.hip
int swx_align_weights_launch(const float *d_qk, float *d_p, float *d_mean, float *d_sd, int W, int H, int N, int ld_f,
                             const int *d_n_rows, const int *d_n_frames, float qk_scale, int medfilt_width,
                             float *d_neg_matrix, int out_ld_n, int out_ld_f, hipStream_t s);
int swx_mel_launch(const float *d_pcm, int B, const float *d_hann, const double2 *d_twiddle, const float *d_filters,
                   int n_mels, float *d_mel, unsigned *d_gmax, int per_item_max, hipStream_t s);
int swx_mel_ragged_launch(const float *d_pcm, const int *d_lens, int B, const float *d_hann, const double2 *d_twiddle,
                          const float *d_filters, int n_mels, float *d_mel, unsigned *d_gmax, int group,
                          hipStream_t s);

// ---- swx_headsel.hip: the head-selection variants of the word-timestamp stage from the captured cross-attention queries
//      qcap [L][max_n][d] and the window's cross-K (row layout, layer stride in elements); see the file header
constexpr int SWX_HS_MAXF = 1536;
int swx_headsel_dynamic_launch(int dtype, const void *qcap, int max_n, int d, int row0, int n_rows, const void *xkv,
                               int64_t layer_stride, int L, int H, int F, int nk, float qk_scale, int count, const double *d_peaks,
                               double *d_score, int32_t *d_sel, float *d_out, int out_ld_f, hipStream_t s);
int swx_headsel_new_launch(int dtype, const void *qcap, int max_n, int d, int n, int row0, int n_out, const void *xkv,
                           int64_t layer_stride, int L, int H, int F, float qk_scale, int medfilt_width, int topk, float w_col,
                           float w_row, float w_cov, float *d_colnorm, float *d_score, int32_t *d_top, float *d_out, int out_ld_f,
                           hipStream_t s);
// the same kernels over a window axis: qcap [L][W][max_n][d], cross-K of (layer l, window w) at xkv + l * layer_stride +
// w * win_stride (elements), per-window counts in device int32 [W] arrays (or null with W = 1 and the scalar next to it).
// dynamic: d_score f64 [W][L*H][row_ld], d_sel [W][row_ld][count], d_peaks f64 [W][row_ld] or null, d_out [W][count][row_ld][out_ld_f].
// new: d_colnorm [W][L*H][SWX_HS_MAXF], d_score / d_top [W][L*H], d_out [W][out_ld_n][out_ld_f] (negated mean).
int swx_headsel_dynamic_batch_launch(int dtype, const void *qcap, int W, int max_n, int d, int row0, const int32_t *d_n_rows,
                                     int n_rows1, int row_ld, const void *xkv, int64_t layer_stride, int64_t win_stride, int L, int H,
                                     const int32_t *d_n_frames, int F1, int nk, float qk_scale, int count, const double *d_peaks,
                                     double *d_score, int32_t *d_sel, float *d_out, int out_ld_f, hipStream_t s);
int swx_headsel_new_batch_launch(int dtype, const void *qcap, int W, int max_n, int d, const int32_t *d_n_tok, int n1, int row0,
                                 const int32_t *d_n_out, int n_out1, int max_out, const void *xkv, int64_t layer_stride,
                                 int64_t win_stride, int L, int H, const int32_t *d_n_frames, int F1, float qk_scale, int medfilt_width,
                                 int topk, float w_col, float w_row, float w_cov, float *d_colnorm, float *d_score, int32_t *d_top,
                                 float *d_out, int out_ld_n, int out_ld_f, hipStream_t s);
int swx_weighted_sum_launch(const float *const *h_xs, const float *h_coef, int n_in, float *d_out, int64_t n, hipStream_t s);

// ---- swx_decode.hip
struct DecodeState;   // device-resident bookkeeping, defined in swx_decode.hip
