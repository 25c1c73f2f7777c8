// swx_xattn.hip -- decode-step cross-attention (d_head = 64), split off swx_attn.hip: reached through swx_attention, whose
// dispatcher asks swx_xattn_plan and hands the decode families to swx_xattn_launch.
//
// Upstream: whisper/model.py::MultiHeadAttention.qkv_attention, reached from stable_whisper/decode.py:40 (decoder steps) and
// timing.py:58-61 (small teacher-forced passes).
//
//   attn_decode_cross_* K / V^T of a (window, head) streamed straight into MFMA operands (HBM-bound), from the row layout or from
//                       the fragment-ordered copy; with the cross-attention query projection inside the launch (_xq).
//   xkv_pack_kernel     writes that fragment-ordered copy (swx_xkv_pack; the cross-K/V projection's epilogue writes the same bytes).
#include "swx_common.h"
#include "swx_kernels.h"
#include "swx_attn.h"

namespace {

// ============================================================================================ decode cross
// Decode-step cross-attention: <= 16 queries (the G beams of one window) against the window's 1500 encoder positions.
// HBM-bound: the only traffic that matters is ONE pass over this (window, head)'s K [1500][64] and V^T [64][kp]
// (384 KB in fp16), so nothing is staged in LDS -- every MFMA fragment is a coalesced 16-byte global load:
//   S^T[16 keys][16 q] = K-frag . Q^T        (K rows gathered so that a lane ends up holding 8 CONSECUTIVE keys)
//   O^T[64 d][16 q]   += V^T-frag . P^T      (V^T rows are key-contiguous: 16-byte loads again)
// 4 waves split the keys (32-key blocks, round-robin) with a private online softmax each and merge through LDS once.
// PACKED: K and V^T come from the fragment-ordered copy (swx_xkv_pack): every MFMA operand fragment of a 32-key block is one
// contiguous 1 KB piece, so a wave instruction reads 8 full 128-byte lines instead of 16 separate 64-byte row pieces (the
// per-CU address path, not HBM, bounds the row-layout variant at ~4.2 TB/s: same finding as for the decode GEMM weights).
// QG: groups of 16 query rows one workgroup carries through a single pass over the head's K / V^T (1 for a decode step; up to 4
// for a multi-token pass over many windows, where one workgroup per group would re-stream the head's 384 KB once per group --
// 8 times for a ~113-row scoring pass: measured +14 ms per 20-window pass).  Every group's arithmetic is the one-group
// kernel's (same key order per wave, same merge), so the result does not depend on QG.
// FQ > 0 (decode step, PACKED, QG = 1): FQ = d / 32 k-steps of the cross-attention QUERY projection run inside this launch (AttnArgs::fq_*).
// The workgroup of (window b, head h) DMAs the 16-row tile of the raw residual stream that starts at the window's first row into
// LDS, its four waves take the head's four 16-column panels of the packed LayerNorm-folded weights (all FQ fragments of a wave in
// flight at once, like gemm_dec_f16), compute the rows' LayerNorm statistics from the tile, run the FQ MFMAs and leave
// f16(rstd (acc - mean c1) + c2) in a 2 KB LDS tile the attention part reads its query fragments from -- the statistics, the
// k-step order and the epilogue expression of swx_decstep.hip::gemm_dec_f16<1, FQ, DEC_LN>, so q is bit-identical to the separate
// launch (tests: test_decode_f16_fused_cross_query_is_bit_identical).  The first K / V^T block is requested before any of it.
template <bool PACKED, int QG, int FQ, int XV = 0>     // XV: 0 one key block per wave in flight (rounds 2-5); 1: two, with nt loads (round 6)
__device__ __forceinline__ void attn_decode_cross_body(const AttnArgs &a)
{
    constexpr bool NT = XV == 1 && PACKED;
    constexpr int DEPTH = XV == 0 ? 1 : 2;
    __shared__ float sm_m[4][16], sm_l[4][16];
    __shared__ float sm_o[4][DH][17];
    extern __shared__ __attribute__((aligned(1024))) unsigned char fq_smem[];   // FQ: [16][FQ * 32] f16 | float2 stat[16] | f16 q[16][64]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = blockIdx.x, b = blockIdx.y;
    // blockIdx.z = QG groups of 16 query rows of this (window, head): a teacher-forced pass of ~100 rows over ONE window has 20
    // flash workgroups to offer 256 CUs; as groups of 16 rows on this kernel it has 100-160, each streaming the head's K / V^T
    // (384 KB, L2-resident after the first group) with its 4 waves splitting the keys
    const int q_base0 = blockIdx.z * 16 * QG;
    const int qn = lane & 15, g = lane >> 4;
    const f16 *Q = (const f16 *)a.q;
    const f16 *Kp = (const f16 *)a.k + (size_t)b * a.k_bs + h * DH;
    const f16 *Vp = (const f16 *)a.v + (size_t)b * a.v_bs + (size_t)h * DH * a.vt_kp;

    f32x4 o[QG][4];
    float m_run[QG], l_run[QG];
#pragma unroll
    for (int u = 0; u < QG; ++u) {
#pragma unroll
        for (int t = 0; t < 4; ++t) o[u][t] = (f32x4){0.f, 0.f, 0.f, 0.f};
        m_run[u] = -__builtin_inff(); l_run[u] = 0.f;
    }
    const int nblk = (a.nk + 31) >> 5;
    // A-row i of S^T tile t  <->  key k0 + (i>>2)*8 + (i&3) + 4t, so that lane (q, g) owns keys k0 + g*8 + 0..7
    const int krow = (qn >> 2) * 8 + (qn & 3);

    const int64_t per_head = swx_xkv_packed_elems_per_head(a.nk);
    const f16 *Kpk = PACKED ? (const f16 *)a.kv_packed + (size_t)b * a.k_bs + (size_t)h * per_head + lane * 8 : nullptr;
    const f16 *Vpk = PACKED ? Kpk + per_head / 2 : nullptr;
    auto load_blk = [&](int cb, f16x8 (&kf)[4], f16x8 (&vf)[4]) {
        if constexpr (PACKED) {
            const int blk = cb < nblk ? cb : nblk - 1;
#pragma unroll
            for (int f = 0; f < 4; ++f) {
                const f16x8 *kp_ = (const f16x8 *)(Kpk + ((size_t)blk * 4 + f) * 512);
                kf[f] = NT ? __builtin_nontemporal_load(kp_) : *kp_;
            }
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const f16x8 *vp_ = (const f16x8 *)(Vpk + ((size_t)blk * 4 + t) * 512);
                vf[t] = NT ? __builtin_nontemporal_load(vp_) : *vp_;
            }
            return;
        }
        const int k0 = (cb < nblk ? cb : nblk - 1) << 5;    // tail prefetch re-reads the last block: loads are never predicated
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int key = k0 + krow + 4 * t;
            const f16 *kr = Kp + (size_t)(key < a.nk ? key : a.nk - 1) * a.ldkv + g * 8;   // rows past nk are masked to -inf below
            kf[2 * t] = *(const f16x8 *)(kr);
            kf[2 * t + 1] = *(const f16x8 *)(kr + 32);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) vf[t] = *(const f16x8 *)(Vp + (size_t)(t * 16 + qn) * a.vt_kp + k0 + g * 8);
    };
    // the first key block of this wave is requested before q is assembled, so its latency overlaps the q loads
    f16x8 kA[4], vA[4];
    load_blk(wave, kA, vA);

    f16x8 qf[QG][2];
    if constexpr (FQ > 0) {
        static_assert(QG == 1 && FQ % 4 == 0, "fused query projection: one group of <= 16 rows");
        typedef __attribute__((address_space(3))) void lds_void;
        typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
        typedef _Float16 f16x4v __attribute__((ext_vector_type(4)));
        constexpr int kslice = FQ * 32, SPR = kslice >> 3, RS = kslice * 2;
        const int li = lane & 15, lg = lane >> 4;
        const int row0 = b * a.q_rows_per_batch;
        // residual tile -> LDS: only the instructions that hold one of the window's nq rows (5 beams = 13 of the 16-row tile's FQ = 40; round 6:
        // the tile was 40 KB of the ~590 KB a workgroup pulls through its CU).  Rows past nq stay whatever LDS held: their projections are
        // never read (qok below).  A run-time loop: no instruction under a branch of its own; a.fq_full_tile (A/B) stages all 16 rows
        {
            const int n_need = a.fq_full_tile ? FQ : (a.nq * SPR + 63) >> 6;
            for (int qi = wave; qi < n_need; qi += 4) {
                const int p = qi * 64 + lane;
                const int row = p / SPR, ps = p - row * SPR;
                const int kslot = ps ^ (row & 15);
                const int gr = row0 + row < a.fq_rows ? row0 + row : a.fq_rows - 1;
                __builtin_amdgcn_global_load_lds(a.fq_x + (size_t)gr * a.fq_ldx + kslot * 8, (lds_void *)(fq_smem + qi * 1024), 16, 0, 0);
            }
        }
        const f16 *wp = a.fq_w + ((size_t)(h * 4 + wave) * FQ) * 512 + lane * 8;
        f16x8 wf[FQ];
#pragma unroll
        for (int ks = 0; ks < FQ; ++ks) wf[ks] = *(const f16x8 *)(wp + (size_t)ks * 512);
        const int ncol = h * DH + wave * 16 + lg * 4;
        const f32x4 c2 = *(const f32x4 *)(a.fq_c2 + ncol), c1 = *(const f32x4 *)(a.fq_c1 + ncol);
        unsigned pfv = 0;
        if (a.fq_pf) {      // cache prefetch of the next projection's weights: one 128-byte line per thread, result never read
            int line = ((b * a.H + h) * 4 + wave) * 64 + lane;
            line = line < a.fq_pf_lines ? line : a.fq_pf_lines - 1;
            pfv = *(const volatile unsigned *)((const unsigned char *)a.fq_pf + (size_t)line * 128);
        }
        __syncthreads();                                    // tile landed (hipcc drains every load of the wave in front of it)
        float2 *stat = (float2 *)(fq_smem + 16 * RS);
        f16 *qt = (f16 *)(fq_smem + 16 * RS + 16 * sizeof(float2));
        f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
        const unsigned char *abase = fq_smem + (size_t)li * RS;
        {
            constexpr int PF = 8;                           // fragment reads eight k-steps ahead of their MFMA (one MFMA per step)
            f16x8 af[PF];
#pragma unroll
            for (int ks = 0; ks < PF; ++ks) af[ks] = *(const f16x8 *)(abase + (((ks * 4 + lg) ^ li) << 4));
#pragma unroll
            for (int ks = 0; ks < FQ; ++ks) {
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[ks], af[ks % PF], acc, 0, 0, 0);
                if (ks + PF < FQ) af[ks % PF] = *(const f16x8 *)(abase + ((((ks + PF) * 4 + lg) ^ li) << 4));
                __builtin_amdgcn_sched_barrier(0);          // (the scheduler sinks each read back in front of its MFMA otherwise)
            }
        }
        // (the statistics after the MFMAs: their row registers do not have to live next to the 40 weight fragments)
        {
            const f16x2 one2 = {(f16)1.f, (f16)1.f};
            const int rb = wave * 4 + lg;
            const unsigned char *rp = fq_smem + (size_t)rb * RS + li * 16;
            f16x8 v[SPR / 16];
#pragma unroll
            for (int i = 0; i < SPR / 16; ++i) v[i] = *(const f16x8 *)(rp + i * 256);
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int i = 0; i < SPR / 16; ++i)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const f16x2 pr = {v[i][2 * e], v[i][2 * e + 1]};
                    s1 = __builtin_amdgcn_fdot2(pr, one2, s1, false);
                    s2 = __builtin_amdgcn_fdot2(pr, pr, s2, false);
                }
#pragma unroll
            for (int o2 = 0; o2 < 1; ++o2) {     // 1, 2, 4, 8 in this order (DPP exchanges: swx_common.h)
                s1 += lane_xor<1>(s1, lane); s2 += lane_xor<1>(s2, lane); s1 += lane_xor<2>(s1, lane); s2 += lane_xor<2>(s2, lane);
                s1 += lane_xor<4>(s1, lane); s2 += lane_xor<4>(s2, lane); s1 += lane_xor<8>(s1, lane); s2 += lane_xor<8>(s2, lane);
            }
            if (li == 0) {
                const float inv = 1.0f / (float)kslice;
                const float mean = s1 * inv;
                float var = s2 * inv - mean * mean;
                var = var > 0.f ? var : 0.f;
                stat[rb] = make_float2(mean, 1.0f / sqrtf(var + 1e-5f));
            }
        }
        __syncthreads();                                    // stat[] visible
        {
            const float2 st = stat[li];
            f16x4v o4;
#pragma unroll
            for (int e = 0; e < 4; ++e) o4[e] = (f16)(st.y * (acc[e] - st.x * c1[e]) + c2[e]);
            *(f16x4v *)(qt + li * DH + wave * 16 + lg * 4) = o4;
        }
        __syncthreads();
        const bool qok = qn < a.nq;
        qf[0][0] = qok ? *(const f16x8 *)(qt + qn * DH + g * 8) : (f16x8)(f16)0;
        qf[0][1] = qok ? *(const f16x8 *)(qt + qn * DH + 32 + g * 8) : (f16x8)(f16)0;
        asm volatile("" ::"v"(pfv));
    } else {
#pragma unroll
    for (int u = 0; u < QG; ++u) {
        const bool qok = q_base0 + u * 16 + qn < a.nq;
        const f16 *qp = Q + ((size_t)b * a.q_rows_per_batch + (qok ? q_base0 + u * 16 + qn : 0)) * a.ldq + h * DH + g * 8;
        qf[u][0] = qok ? *(const f16x8 *)(qp) : (f16x8)(f16)0;
        qf[u][1] = qok ? *(const f16x8 *)(qp + 32) : (f16x8)(f16)0;
    }
    }

    auto compute_blk = [&](int cb, const f16x8 (&kf)[4], const f16x8 (&vf)[4]) {
        const int k0 = cb << 5;
#pragma unroll
        for (int u = 0; u < QG; ++u) {
            f32x4 s[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                s[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
                s[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[2 * t], qf[u][0], s[t], 0, 0, 0);
                s[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[2 * t + 1], qf[u][1], s[t], 0, 0, 0);
            }
            float tmax = -__builtin_inff();
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int key = k0 + g * 8 + 4 * t + r;
                    const float v = (key < a.nk) ? s[t][r] * 0.125f : -__builtin_inff();
                    s[t][r] = v;
                    tmax = fmaxf(tmax, v);
                }
            tmax = lane_xor16_max_lds(tmax);            // (through the LDS crossbar on purpose in this HBM-streaming kernel: swx_common.h)
            tmax = lane_xor32_max_lds(tmax);
            const float m_new = fmaxf(m_run[u], tmax);
            const float alpha = __expf(m_run[u] - m_new);
            float psum = 0.f;
            f16x8 pb;
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float p = __expf(s[t][r] - m_new);
                    psum += p;
                    pb[4 * t + r] = (f16)p;
                }
            psum = lane_xor16_add_lds(psum);
            psum = lane_xor32_add_lds(psum);
            l_run[u] = l_run[u] * alpha + psum;
            m_run[u] = m_new;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                o[u][t][0] *= alpha; o[u][t][1] *= alpha; o[u][t][2] *= alpha; o[u][t][3] *= alpha;
                o[u][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf[t], pb, o[u][t], 0, 0, 0);
            }
        }
    };
    if constexpr (DEPTH > 1) {
        // Round 6: DEPTH key blocks in flight per wave.  The loop below issues a block's eight loads and waits for them in the same
        // iteration (the compiled loop: 8 loads, vmcnt(7) .. vmcnt(0), 8 MFMAs), so a wave pays one memory round trip per block --
        // twelve per launch -- and the launch has W x H x 4 waves x 8 KB = 12.8 MB in flight: by Little's law ~5.5 TB/s at the ~2.3 us
        // a loaded round trip takes, which is what the kernel measures.  Here block n + DEPTH of the wave is requested before block
        // n + 1 is multiplied.  Same blocks in the same order per wave: bit-identical.  Loads past the wave's last block re-read it
        // (clamped, never predicated: a predicated load costs a drained join).  The stages are unconditional inside the loop and the
        // remainder follows it: with a stage under an `if` the wait in front of the first stage has to assume the shorter path and
        // drains the younger blocks' loads too (seen in the ISA of the first form).  Measured on the headline pass, A/B in one process
        // (profiles/r06_c12_*): two blocks + nt 427.3 ms, two blocks 429.8, three blocks + nt 428.9, one block (round 5) 432.9.
        f16x8 kS[DEPTH][4], vS[DEPTH][4];
#pragma unroll
        for (int f = 0; f < 4; ++f) { kS[0][f] = kA[f]; vS[0][f] = vA[f]; }
#pragma unroll
        for (int dd = 1; dd < DEPTH; ++dd) load_blk(wave + 4 * dd, kS[dd], vS[dd]);
        int cb = wave;
        for (; cb + 4 * (DEPTH - 1) < nblk; cb += 4 * DEPTH) {
#pragma unroll
            for (int dd = 0; dd < DEPTH; ++dd) {
                compute_blk(cb + 4 * dd, kS[dd], vS[dd]);
                load_blk(cb + 4 * (DEPTH + dd), kS[dd], vS[dd]);
            }
        }
#pragma unroll
        for (int dd = 0; dd < DEPTH - 1; ++dd)
            if (cb + 4 * dd < nblk) compute_blk(cb + 4 * dd, kS[dd], vS[dd]);
    } else {
        compute_blk(wave, kA, vA);                           // nblk >= 4: every wave owns at least one block
#pragma unroll 2
        for (int cb = wave + 4; cb < nblk; cb += 4) {
            f16x8 kf[4], vf[4];
            load_blk(cb, kf, vf);
            compute_blk(cb, kf, vf);
        }
    }

    // merge the four partial softmaxes, one group at a time: o[u][t][r] is O^T[d = t*16 + g*4 + r][q = qn]
#pragma unroll
    for (int u = 0; u < QG; ++u) {
        const int q_base = q_base0 + u * 16;
        if (q_base >= a.nq) break;
        if (u > 0) __syncthreads();
        if (g == 0) { sm_m[wave][qn] = m_run[u]; sm_l[wave][qn] = l_run[u]; }
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) sm_o[wave][t * 16 + g * 4 + r][qn] = o[u][t][r];
        __syncthreads();
        const int nq_here = a.nq - q_base < 16 ? a.nq - q_base : 16;
        for (int i = tid; i < nq_here * DH; i += 256) {
            const int q = i >> 6, d = i & 63;
            const float M = fmaxf(fmaxf(sm_m[0][q], sm_m[1][q]), fmaxf(sm_m[2][q], sm_m[3][q]));
            float L = 0.f, O = 0.f;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const float f = __expf(sm_m[w][q] - M);
                L += sm_l[w][q] * f;
                O += sm_o[w][d][q] * f;
            }
            ((f16 *)a.o)[((size_t)b * a.q_rows_per_batch + q_base + q) * a.ldo + h * DH + d] = (f16)(O / L);
        }
    }
}

template <bool PACKED, int QG>
__global__ __launch_bounds__(256) void attn_decode_cross_f16(AttnArgs a) { attn_decode_cross_body<PACKED, QG, 0>(a); }
// with the query projection inside: the 40 weight fragments of a wave must not cost the launch its second workgroup per CU
// (W x H = 400 workgroups stream K / V^T concurrently; at one per CU they would run in two rounds) -- two blocks per CU = 256 registers
template <int FQ>
__global__ __launch_bounds__(256, 2) void attn_decode_cross_xq_f16(AttnArgs a) { attn_decode_cross_body<true, 1, FQ>(a); }
// round 6: the K / V^T stream -- 384 KB per (window, head) that ONE workgroup reads once per step and nobody reads again for 5 GB of
// other traffic -- with two key blocks of a wave in flight and the non-temporal load policy (MI355X_MICROARCH.md, row `nt-weights`);
// SWX_FLAG_XATTN_R5 keeps the one-block loop above as its bit-identity reference
template <int FQ>
__global__ __launch_bounds__(256, 2) void attn_decode_cross_xq2_f16(AttnArgs a) { attn_decode_cross_body<true, 1, FQ, 1>(a); }
// (QG = 4: two workgroups per CU -- the four-group form of a many-window scoring pass compiled to 280 registers = ONE workgroup = one wave per SIMD = 64 KB
// in flight per CU without the bound; held to 256 it has 234, no spill: 98 -> 68 us per layer of the 20-window scoring pass, profiles/r06_c34_*)
template <bool PACKED, int QG>
__global__ __launch_bounds__(256, QG == 4 ? 2 : 1) void attn_decode_cross2_f16(AttnArgs a) { attn_decode_cross_body<PACKED, QG, 0, 1>(a); }

// ================================================================================================ xkv pack
// One workgroup per (32-key block, head, window): the block's K rows (32 x 64) and V^T columns (64 x 32) are copied into the
// fragment order attn_decode_cross_f16 consumes (index maps: see load_blk / compute_blk there).
__global__ __launch_bounds__(256) void xkv_pack_kernel(const f16 *__restrict__ K, const f16 *__restrict__ VT, f16 *__restrict__ P,
                                                       int nk, int ldk, int vt_kp, int64_t bs)
{
    const int blk = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63, frag = tid >> 6;           // 4 fragments x 64 lanes for K, then for V^T
    const int qn = lane & 15, g = lane >> 4;
    const int64_t per_head = swx_xkv_packed_elems_per_head(nk);
    f16 *out = P + (size_t)b * bs + (size_t)h * per_head + ((size_t)blk * 4 + frag) * 512 + lane * 8;
    {   // K fragment f = 2t + kk: lane (qn, g) holds dims 32 kk + 8 g .. + 8 of key 32 blk + (qn >> 2) * 8 + (qn & 3) + 4 t
        const int t = frag >> 1, kk = frag & 1;
        const int key = blk * 32 + (qn >> 2) * 8 + (qn & 3) + 4 * t;
        f16x8 v = (f16x8)(f16)0;
        if (key < nk) v = *(const f16x8 *)(K + (size_t)b * bs + (size_t)key * ldk + h * DH + kk * 32 + g * 8);
        *(f16x8 *)out = v;
    }
    {   // V^T fragment t: lane (qn, g) holds keys 32 blk + 8 g .. + 8 of row d = 16 t + qn (zero padded past nk in the source)
        const int t = frag;
        const f16x8 v = *(const f16x8 *)(VT + (size_t)b * bs + ((size_t)h * DH + t * 16 + qn) * vt_kp + blk * 32 + g * 8);
        *(f16x8 *)(out + per_head / 2) = v;
    }
}

}  // namespace

int swx_xkv_pack(const void *k, const void *vt, void *packed, int B, int H, int nk, int ldk, int vt_kp, int64_t batch_stride,
                 hipStream_t s)
{
    if (B <= 0) return 0;
    if (((nk + 31) / 32) * 32 > vt_kp) return -5;
    hipLaunchKernelGGL(xkv_pack_kernel, dim3((nk + 31) / 32, H, B), dim3(256), 0, s, (const f16 *)k, (const f16 *)vt, (f16 *)packed,
                       nk, ldk, vt_kp, batch_stride);
    SWX_CHECK_LAUNCH();
    return 0;
}

SwxXattnPlan swx_xattn_plan(int dtype, const AttnArgs &a, int force_kernel, int flags)
{
    SwxXattnPlan p{SWX_XA_NOT_DECODE, 1, 1};
    // the decode kernel also takes a SMALL multi-row pass (align(): one window of ~100 rows) as groups of 16 rows, when the
    // fragment-ordered K / V^T copy exists and the flash grid would be tiny
    const int ngrp = cdiv(a.nq, 16);
    const bool by_batch = flags & SWX_FLAG_SCORE_TILED;       // round 3's size-dependent choice (A/B only)
    const bool small_pass = a.nq > 16 && a.kv_packed && !(flags & SWX_FLAG_NO_PACKED_XKV) && force_kernel == 0 &&
                            (!by_batch || (a.nq <= 160 && (int64_t)a.B * a.H * ngrp <= 1024));
    const bool dec = (dtype == SWX_F16) && a.vt_kp > 0 && (a.nq <= 16 || small_pass) && a.nk >= 128 && (force_kernel == 3 || force_kernel == 0);
    if (force_kernel == 3 && !dec) { p.family = -5; return p; }
    if (!dec) return p;
    // groups of 16 query rows per workgroup: one while the launch is small (a decode step; align(): one window = 100-160
    // workgroups), up to four when many windows share the pass (the head's K / V^T is then streamed once per 64 rows)
    const int64_t wgs1 = (int64_t)a.B * a.H * ngrp;
    p.qg = (a.nq <= 16 || wgs1 <= 512) ? 1 : (ngrp >= 4 && wgs1 > 2048) ? 4 : 2;
    const bool packed = a.kv_packed && !(flags & SWX_FLAG_NO_PACKED_XKV);     // else row-layout K / V^T: the reference
    const bool r5_loop = (flags & SWX_FLAG_XATTN_R5) != 0;                    // one key block per wave in flight (A/B)
    if (packed && a.fq_w && p.qg == 1 && a.nq <= 16) {
        const int fq = a.fq_k / 32;
        const bool offered = a.fq_k % 32 == 0 && (fq == 12 || fq == 16 || fq == 20 || fq == 24 || fq == 32 || fq == 40);
        p.family = offered ? SWX_XA_PACKED_FQ : -5;
        p.depth = r5_loop ? 1 : 2;
    } else if (a.fq_w) {
        p.family = -5;                  // the fused query projection exists on the packed single-group kernel only
    } else if (packed) {
        p.family = SWX_XA_PACKED;
        p.depth = r5_loop ? 1 : 2;
    } else {
        p.family = SWX_XA_ROW;          // attn_decode_cross_f16<false, QG>: one key block per wave in flight
    }
    return p;
}

int swx_xattn_launch(const SwxXattnPlan &xp, const AttnArgs &a_in, hipStream_t s)
{
    const AttnArgs &a = a_in;
    constexpr size_t esz = 2;                              // f16: the only dtype the plan offers these kernels to
    SwxProfScope prof(PC_ATTN_ROWWISE, (double)a.B * a.H * 64 * esz * (2.0 * a.nk + 2.0 * a.nq) +
                                           (a.fq_w ? 2.0 * a.H * 64 * a.fq_k + 2.0 * a.fq_rows * a.fq_k : 0.0), s);
    const int ngrp = cdiv(a.nq, 16), qg = xp.qg;
    dim3 gd(a.H, a.B, cdiv(ngrp, qg));
    const bool packed = xp.family == SWX_XA_PACKED;
    const bool r5_loop = xp.depth == 1;                    // one key block per wave in flight (A/B: SWX_FLAG_XATTN_R5)
    if (xp.family == SWX_XA_PACKED_FQ) {
        // fused query projection: + [16][K] residual tile, statistics, q tile in dynamic LDS
        AttnArgs a = a_in;
        a.fq_full_tile = (swx_flags() & SWX_FLAG_XQ_FULL_TILE) ? 1 : 0;
        const int fq = a.fq_k / 32;
        const size_t lds = (size_t)16 * a.fq_k * 2 + 16 * sizeof(float2) + 16 * DH * 2;
#define SWX_XQ(FQ_) do { \
        const int rc_ = r5_loop ? swx_launch_lds<attn_decode_cross_xq_f16<FQ_>>(gd, dim3(256), lds, 96 * 1024, s, a) \
                                : swx_launch_lds<attn_decode_cross_xq2_f16<FQ_>>(gd, dim3(256), lds, 96 * 1024, s, a); \
        if (rc_ < 0) return rc_; } while (0)
        switch (fq) {
            case 12: SWX_XQ(12); break; case 16: SWX_XQ(16); break; case 20: SWX_XQ(20); break;
            case 24: SWX_XQ(24); break; case 32: SWX_XQ(32); break; case 40: SWX_XQ(40); break;
            default: return -5;
        }
#undef SWX_XQ
    } else if (packed) {
        if (r5_loop) {
            if (qg == 1) hipLaunchKernelGGL((attn_decode_cross_f16<true, 1>), gd, dim3(256), 0, s, a);
            else if (qg == 2) hipLaunchKernelGGL((attn_decode_cross_f16<true, 2>), gd, dim3(256), 0, s, a);
            else hipLaunchKernelGGL((attn_decode_cross_f16<true, 4>), gd, dim3(256), 0, s, a);
        } else {
            if (qg == 1) hipLaunchKernelGGL((attn_decode_cross2_f16<true, 1>), gd, dim3(256), 0, s, a);
            else if (qg == 2) hipLaunchKernelGGL((attn_decode_cross2_f16<true, 2>), gd, dim3(256), 0, s, a);
            else hipLaunchKernelGGL((attn_decode_cross2_f16<true, 4>), gd, dim3(256), 0, s, a);
        }
    } else {      // SWX_XA_ROW
        if (qg == 1) hipLaunchKernelGGL((attn_decode_cross_f16<false, 1>), gd, dim3(256), 0, s, a);
        else if (qg == 2) hipLaunchKernelGGL((attn_decode_cross_f16<false, 2>), gd, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((attn_decode_cross_f16<false, 4>), gd, dim3(256), 0, s, a);
    }
    SWX_CHECK_LAUNCH();
    return 0;
}
