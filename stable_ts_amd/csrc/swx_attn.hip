// swx_attn.hip -- dense (non-causal) attention kernels (d_head = 64 for every Whisper size) and the dispatcher of swx_attention.
//
// Upstream: whisper/model.py::MultiHeadAttention.qkv_attention (q,k each scaled by d_head^-0.25, fp32 softmax),
// reached from stable_whisper/decode.py:40 (decoder steps), decode.py:27-30 (encoder) and timing.py:58-61 (the
// teacher-forced pass whose cross-attention qk the word-timestamp code reads).
//
//   attn_flash2_f16     MFMA flash attention, non-causal, for the MFMA-bound cases (encoder self-attention,
//                       1500x1500 per head; cross-attention of the scoring pass).  One wave = 32 queries,
//                       K tile [64 keys][64] and V^T tile [64][64 keys] double-buffered in LDS per 4-wave workgroup.
//   attn_flash_f32      the same on the exact-f32 matrix instruction (strict f32 mode).
//   attn_dense_rowwise  VALU kernel (any dtype): 8 queries that share one K/V (same window, same head) per workgroup;
//                       K and V are streamed once per workgroup.  What the strict f32 mode runs where attn_flash_f32 is not offered.
// The decode-step cross-attention (attn_decode_cross_*, reached through swx_attention) lives in swx_xattn.hip, the decoder's
// cached self-attention and qk_capture in swx_selfattn.hip.
#include <type_traits>
#include "swx_common.h"
#include "swx_kernels.h"
#include "swx_attn.h"

namespace {

// ================================================================================================ flash f16
constexpr int FL_KT = 64;            // keys per tile
constexpr int FL_LD = 72;            // halfs per LDS row (144 B: keeps b128 / b64 fragment reads aligned)

// ================================================================================================ flash f16 (generation 2)
// Swapped QK^T (S^T = K.Q^T), so a lane's accumulator registers all belong to ONE query: the online-softmax row statistics are
// lane-local + two shuffles and the exponentiated tile is already laid out as the B operand of O^T += V^T.P^T (no LDS round
// trip for P).  Against the first kernel (16 queries per wave, single-buffered tiles: 0.10 of the MFMA peak, deleted in round 3):
//   * a wave owns QB 16-query blocks (QB = 2: 32 queries; QB = 4: 64 queries for long query axes): every K / V^T fragment read
//     from LDS feeds QB MFMAs -- 24 fragment reads per 16 QB MFMAs per wave and tile -- and a workgroup covers 64 QB queries per
//     barrier;
//   * K / V^T tiles are double-buffered in LDS, the global loads of tile t+1 are issued into registers BEFORE the MFMAs of
//     tile t and written to the other buffer after them: one barrier per tile, no exposed load latency;
//   * with VT (V already transposed per head in HBM: cross-KV layout, and the encoder's V through swx_transpose_v) both
//     tiles are written with 16-byte vector stores; the row-major-V form (scalar transposing stores) is kept for the callers
//     that have no transposed copy.
template <bool VT, int QB>
__global__ __launch_bounds__(256, 2) void attn_flash2_f16(AttnArgs a)
{
    __shared__ __attribute__((aligned(16))) f16 Ks[2][FL_KT][FL_LD];   // [buf][key][d]
    __shared__ __attribute__((aligned(16))) f16 Vt[2][DH][FL_LD];      // [buf][d][key]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.z, h = blockIdx.y;
    const int q0 = blockIdx.x * (QB * 64) + wave * (QB * 16);
    const int qn = lane & 15, g = lane >> 4;
    const f16 *Q = (const f16 *)a.q;
    const f16 *K = (const f16 *)a.k + (size_t)b * a.k_bs + h * DH;
    const f16 *V = (const f16 *)a.v + (size_t)b * a.v_bs + (VT ? (size_t)h * DH * a.vt_kp : (size_t)h * DH);

    f16x8 qf[QB][2];
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
        const int qi = q0 + qb * 16 + qn;
        const f16 *qp = Q + ((size_t)b * a.q_rows_per_batch + (qi < a.nq ? qi : a.nq - 1)) * a.ldq + h * DH + g * 8;   // clamped
        qf[qb][0] = *(const f16x8 *)(qp);
        qf[qb][1] = *(const f16x8 *)(qp + 32);
    }
    f32x4 o[QB][4];
    float m_run[QB], l_run[QB];
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
        m_run[qb] = -__builtin_inff(); l_run[qb] = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t) o[qb][t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }

    // staging registers of one tile: chunk c = tid + 256 i  ->  K row c>>3, dims (c&7)*8 ; V^T row c>>3, keys (c&7)*8
    f16x8 rk[2], rv[2];
    auto load_tile = [&](int kt0) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int c = tid + 256 * i, r = c >> 3, c8 = (c & 7) * 8;
            const int kg = kt0 + r;
            const int kgc = kg < a.nk ? kg : a.nk - 1;                      // clamped, never predicated
            rk[i] = *(const f16x8 *)(K + (size_t)kgc * a.ldkv + c8);
            if (kg >= a.nk) rk[i] = (f16x8)(f16)0;
            if constexpr (VT) {
                rv[i] = *(const f16x8 *)(V + (size_t)r * a.vt_kp + kt0 + c8);           // zero padded past nk in the source
            } else {
                rv[i] = *(const f16x8 *)(V + (size_t)kgc * a.ldkv + c8);
                if (kg >= a.nk) rv[i] = (f16x8)(f16)0;
            }
        }
    };
    auto store_tile = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int c = tid + 256 * i, r = c >> 3, c8 = (c & 7) * 8;
            *(f16x8 *)&Ks[buf][r][c8] = rk[i];
            if constexpr (VT) {
                *(f16x8 *)&Vt[buf][r][c8] = rv[i];
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) Vt[buf][c8 + e][r] = rv[i][e];
            }
        }
    };

    const int ntile = (a.nk + FL_KT - 1) / FL_KT;
    load_tile(0);
    store_tile(0);
    __syncthreads();
    for (int t = 0; t < ntile; ++t) {
        const int cur = t & 1, kt0 = t * FL_KT;
        if (t + 1 < ntile) load_tile(kt0 + FL_KT);
        // K fragments of this tile, shared by the QB query blocks
        f16x8 kf[4][2];
#pragma unroll
        for (int tt = 0; tt < 4; ++tt)
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) kf[tt][kk] = *(const f16x8 *)&Ks[cur][tt * 16 + qn][kk * 32 + g * 8];
        f16x8 pb[QB][2];
#pragma unroll
        for (int qb = 0; qb < QB; ++qb) {
            f32x4 sc[4];
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) {
                sc[tt] = (f32x4){0.f, 0.f, 0.f, 0.f};
                sc[tt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[tt][0], qf[qb][0], sc[tt], 0, 0, 0);
                sc[tt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[tt][1], qf[qb][1], sc[tt], 0, 0, 0);
            }
            // softmax bookkeeping on the RAW scores (the 1/8 scale is positive: max commutes with it) and in the exp2 domain:
            // per element one max, one fma, one v_exp_f32, one add -- the key-range mask only on the last tile.  This loop,
            // not the MFMAs, bounds the kernel (32 MFMAs = 512 cycles against ~350 VALU operations = 1400 cycles per 64-key
            // tile and wave before; ~200 now).
            constexpr float SC2 = 0.125f * 1.4426950408889634f;
            if (kt0 + FL_KT > a.nk) {
#pragma unroll
                for (int tt = 0; tt < 4; ++tt)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (kt0 + tt * 16 + g * 4 + r >= a.nk) sc[tt][r] = -__builtin_inff();
            }
            float tmax = -__builtin_inff();
#pragma unroll
            for (int tt = 0; tt < 4; ++tt)
#pragma unroll
                for (int r = 0; r < 4; ++r) tmax = fmaxf(tmax, sc[tt][r]);
            tmax = lane_xor16_max(tmax);                // (VALU row swaps, not ds_bpermute: swx_common.h)
            tmax = lane_xor32_max(tmax);
            const float m_new = fmaxf(m_run[qb], tmax);                               // raw units
            const float alpha = __builtin_amdgcn_exp2f((m_run[qb] - m_new) * SC2);    // m_run = -inf on the first tile -> 0
            const float mc = m_new * SC2;
            float psum = 0.f;
#pragma unroll
            for (int tt = 0; tt < 4; ++tt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(sc[tt][r], SC2, -mc));
                    sc[tt][r] = p;
                    psum += p;
                }
            psum = lane_xor16_add(psum);
            psum = lane_xor32_add(psum);
            l_run[qb] = l_run[qb] * alpha + psum;
            m_run[qb] = m_new;
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) { o[qb][tt][0] *= alpha; o[qb][tt][1] *= alpha; o[qb][tt][2] *= alpha; o[qb][tt][3] *= alpha; }
            // P^T as the B operand: k-slot (g, j) of k-block c <-> key 32c + (j<4 ? g*4+j : 16 + g*4 + j-4)
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int r = 0; r < 4; ++r) { pb[qb][c][r] = (f16)sc[2 * c][r]; pb[qb][c][4 + r] = (f16)sc[2 * c + 1][r]; }
        }
        // O^T += V^T . P^T : every V^T fragment feeds all QB query blocks
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) {
                const f16x4 lo = *(const f16x4 *)&Vt[cur][tt * 16 + qn][32 * c + g * 4];
                const f16x4 hi = *(const f16x4 *)&Vt[cur][tt * 16 + qn][32 * c + 16 + g * 4];
                f16x8 va;
#pragma unroll
                for (int e = 0; e < 4; ++e) { va[e] = lo[e]; va[4 + e] = hi[e]; }
#pragma unroll
                for (int qb = 0; qb < QB; ++qb) o[qb][tt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(va, pb[qb][c], o[qb][tt], 0, 0, 0);
            }
        if (t + 1 < ntile) store_tile(cur ^ 1);
        __syncthreads();
    }

#pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
        const int qi = q0 + qb * 16 + qn;
        if (qi < a.nq) {
            const float inv = 1.0f / l_run[qb];
            f16 *op = (f16 *)a.o + ((size_t)b * a.q_rows_per_batch + qi) * a.ldo + h * DH;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                f16x4 ov;
#pragma unroll
                for (int r = 0; r < 4; ++r) ov[r] = (f16)(o[qb][t][r] * inv);
                *(f16x4 *)(op + t * 16 + g * 4) = ov;
            }
        }
    }
}

// ================================================================================================ flash f16 (generation 3, round 6)
// MEASURED SLOWER, kept behind SWX_FLAG_FLASH_PIPELINED as the record of the experiment.
// The arithmetic of attn_flash2_f16<true, QB> operation for operation (bit-identical: tests/test_gpu_kernels.py::
// test_flash3_is_bit_identical_to_flash2), re-staged so that the matrix pipe and the VALU of ONE wave could overlap.  Generation 2's
// key tile is  for qb: { 8 QK^T MFMAs -> softmax of that block (~100 VALU + 17 v_exp on the MFMA results) }  then 32 PV MFMAs, and
// hipcc keeps that order: every wave alternates between MFMA-only and VALU-only stretches (0.25 MFMA utilisation by counters at two
// waves per SIMD).  Here the tile is ONE basic block (the key-range mask lives in a peeled instantiation for the last tile, the
// next tile's loads / stores are unconditional) laid out as a software pipeline over the query blocks:
//     QK(0) | softmax(0) + QK(1) | softmax(1) + QK(2) + PV(0) | softmax(2) + QK(3) + PV(1) | softmax(3) + PV(2) | PV(3)
// with sched_group_barrier pipelines that put one MFMA in front of every few VALU instructions of a softmax (seen in the ISA).
// Result on hardware (profiles/r06_c14_flash3_ab.json): 391-406 us against 376-387 us per encoder layer at 20 windows, 42.9 against
// 37.4 us at one window; headline pass 428.6 vs 427.5 ms, align() 916 vs 902 ms.  What MI355X_MICROARCH.md says of two waves per
// SIMD holds: VALU placed beside a wave's own dependency-paced MFMAs delays them, and the second wave of the SIMD already fills
// generation 2's MFMA-only and VALU-only stretches -- moving work between the two is zero- or negative-sum.
template <int QB>
__global__ __launch_bounds__(256, 2) void attn_flash3_f16(AttnArgs a)
{
    __shared__ __attribute__((aligned(16))) f16 Ks[2][FL_KT][FL_LD];   // [buf][key][d]
    __shared__ __attribute__((aligned(16))) f16 Vt[2][DH][FL_LD];      // [buf][d][key]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.z, h = blockIdx.y;
    const int q0 = blockIdx.x * (QB * 64) + wave * (QB * 16);
    const int qn = lane & 15, g = lane >> 4;
    const f16 *Q = (const f16 *)a.q;
    const f16 *K = (const f16 *)a.k + (size_t)b * a.k_bs + h * DH;
    const f16 *V = (const f16 *)a.v + (size_t)b * a.v_bs + (size_t)h * DH * a.vt_kp;

    f16x8 qf[QB][2];
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
        const int qi = q0 + qb * 16 + qn;
        const f16 *qp = Q + ((size_t)b * a.q_rows_per_batch + (qi < a.nq ? qi : a.nq - 1)) * a.ldq + h * DH + g * 8;   // clamped
        qf[qb][0] = *(const f16x8 *)(qp);
        qf[qb][1] = *(const f16x8 *)(qp + 32);
    }
    f32x4 o[QB][4];
    float m_run[QB], l_run[QB];
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
        m_run[qb] = -__builtin_inff(); l_run[qb] = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t) o[qb][t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    const int ntile = (a.nk + FL_KT - 1) / FL_KT;
    f16x8 rk[2], rv[2];
    auto load_tile = [&](int kt0) {           // (past the last tile: the last tile again -- never predicated, never stored to a live buffer)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int c = tid + 256 * i, r = c >> 3, c8 = (c & 7) * 8;
            const int kg = kt0 + r;
            const int kgc = kg < a.nk ? kg : a.nk - 1;
            rk[i] = *(const f16x8 *)(K + (size_t)kgc * a.ldkv + c8);
            if (kg >= a.nk) rk[i] = (f16x8)(f16)0;
            rv[i] = *(const f16x8 *)(V + (size_t)r * a.vt_kp + kt0 + c8);               // zero padded past nk in the source
        }
    };
    auto store_tile = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int c = tid + 256 * i, r = c >> 3, c8 = (c & 7) * 8;
            *(f16x8 *)&Ks[buf][r][c8] = rk[i];
            *(f16x8 *)&Vt[buf][r][c8] = rv[i];
        }
    };
    constexpr float SC2 = 0.125f * 1.4426950408889634f;

    auto tile = [&](auto mask_tag, int cur, int kt0) {
        constexpr bool MASK = decltype(mask_tag)::value;
        f16x8 kf[4][2], va[2][4];
#pragma unroll
        for (int tt = 0; tt < 4; ++tt)
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) kf[tt][kk] = *(const f16x8 *)&Ks[cur][tt * 16 + qn][kk * 32 + g * 8];
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) {
                const f16x4 lo = *(const f16x4 *)&Vt[cur][tt * 16 + qn][32 * c + g * 4];
                const f16x4 hi = *(const f16x4 *)&Vt[cur][tt * 16 + qn][32 * c + 16 + g * 4];
#pragma unroll
                for (int e = 0; e < 4; ++e) { va[c][tt][e] = lo[e]; va[c][tt][4 + e] = hi[e]; }
            }
        f32x4 sc[2][4];
        f16x8 pb[2][2];
        auto qk = [&](int qb, f32x4 (&s4)[4]) {
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) {
                s4[tt] = (f32x4){0.f, 0.f, 0.f, 0.f};
                s4[tt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[tt][0], qf[qb][0], s4[tt], 0, 0, 0);
                s4[tt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[tt][1], qf[qb][1], s4[tt], 0, 0, 0);
            }
        };
        auto pv = [&](int qb, const f16x8 (&p2)[2]) {
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int tt = 0; tt < 4; ++tt) o[qb][tt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(va[c][tt], p2[c], o[qb][tt], 0, 0, 0);
        };
        auto softmax = [&](int qb, f32x4 (&s4)[4], f16x8 (&p2)[2]) {
            if constexpr (MASK) {
#pragma unroll
                for (int tt = 0; tt < 4; ++tt)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (kt0 + tt * 16 + g * 4 + r >= a.nk) s4[tt][r] = -__builtin_inff();
            }
            float tmax = -__builtin_inff();
#pragma unroll
            for (int tt = 0; tt < 4; ++tt)
#pragma unroll
                for (int r = 0; r < 4; ++r) tmax = fmaxf(tmax, s4[tt][r]);
            tmax = lane_xor16_max(tmax);
            tmax = lane_xor32_max(tmax);
            const float m_new = fmaxf(m_run[qb], tmax);
            const float alpha = __builtin_amdgcn_exp2f((m_run[qb] - m_new) * SC2);
            const float mc = m_new * SC2;
            float psum = 0.f;
#pragma unroll
            for (int tt = 0; tt < 4; ++tt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s4[tt][r], SC2, -mc));
                    s4[tt][r] = p;
                    psum += p;
                }
            psum = lane_xor16_add(psum);
            psum = lane_xor32_add(psum);
            l_run[qb] = l_run[qb] * alpha + psum;
            m_run[qb] = m_new;
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) { o[qb][tt][0] *= alpha; o[qb][tt][1] *= alpha; o[qb][tt][2] *= alpha; o[qb][tt][3] *= alpha; }
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int r = 0; r < 4; ++r) { p2[c][r] = (f16)s4[2 * c][r]; p2[c][4 + r] = (f16)s4[2 * c + 1][r]; }
        };
        qk(0, sc[0]);
        auto stage = [&](auto qb_tag) {
            constexpr int qb = decltype(qb_tag)::value;
            if constexpr (qb + 1 < QB) qk(qb + 1, sc[(qb + 1) & 1]);
            if constexpr (qb >= 1) pv(qb - 1, pb[(qb - 1) & 1]);
            softmax(qb, sc[qb & 1], pb[qb & 1]);
            // one MFMA in front of every few VALU instructions of this stage's softmax (8 or 16 MFMAs per stage, ~115 VALU)
            constexpr int NM = (qb + 1 < QB ? 8 : 0) + (qb >= 1 ? 8 : 0);
#pragma unroll
            for (int i = 0; i < NM; ++i) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x002, NM == 16 ? 7 : 14, 0);
            }
        };
        stage(std::integral_constant<int, 0>{});
        if constexpr (QB > 1) stage(std::integral_constant<int, 1>{});
        if constexpr (QB > 2) stage(std::integral_constant<int, 2>{});
        if constexpr (QB > 3) stage(std::integral_constant<int, 3>{});
        static_assert(QB <= 4, "stages are listed by hand");
        pv(QB - 1, pb[(QB - 1) & 1]);
    };

    load_tile(0);
    store_tile(0);
    __syncthreads();
    for (int t = 0; t + 1 < ntile; ++t) {
        load_tile((t + 1) * FL_KT);
        tile(std::false_type{}, t & 1, t * FL_KT);
        store_tile((t & 1) ^ 1);
        __syncthreads();
    }
    if (ntile * FL_KT > a.nk) tile(std::true_type{}, (ntile - 1) & 1, (ntile - 1) * FL_KT);
    else tile(std::false_type{}, (ntile - 1) & 1, (ntile - 1) * FL_KT);

#pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
        const int qi = q0 + qb * 16 + qn;
        if (qi < a.nq) {
            const float inv = 1.0f / l_run[qb];
            f16 *op = (f16 *)a.o + ((size_t)b * a.q_rows_per_batch + qi) * a.ldo + h * DH;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                f16x4 ov;
#pragma unroll
                for (int r = 0; r < 4; ++r) ov[r] = (f16)(o[qb][t][r] * inv);
                *(f16x4 *)(op + t * 16 + g * 4) = ov;
            }
        }
    }
}

// V [B][n][ldv] (head h at column h*64) -> V^T [B][H][64][kp] per head, keys contiguous, zero padded up to kp: LDS tile
// transpose, 16-byte accesses on both sides.  One workgroup per (64-key tile, head, batch item).
__global__ __launch_bounds__(256) void transpose_v_kernel(const f16 *__restrict__ V, int64_t ldv, int64_t v_bs, int n, f16 *__restrict__ VT,
                                                          int kp, int64_t vt_bs)
{
    __shared__ __attribute__((aligned(16))) f16 T[DH][FL_LD];      // [d][key]
    const int kt0 = blockIdx.x * 64, h = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int c = tid + 256 * i, key = c >> 3, c8 = (c & 7) * 8;
        const int kg = kt0 + key;
        f16x8 v = *(const f16x8 *)(V + (size_t)b * v_bs + (size_t)(kg < n ? kg : n - 1) * ldv + h * DH + c8);
        if (kg >= n) v = (f16x8)(f16)0;
#pragma unroll
        for (int e = 0; e < 8; ++e) T[c8 + e][key] = v[e];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int c = tid + 256 * i, dr = c >> 3, k8 = (c & 7) * 8;
        if (kt0 + k8 < kp) *(f16x8 *)(VT + (size_t)b * vt_bs + ((size_t)h * DH + dr) * kp + kt0 + k8) = *(const f16x8 *)&T[dr][k8];
    }
}

// ================================================================================================ flash f32 (round 5)
// Strict-f32 mode on the exact-f32 matrix instruction (v_mfma_f32_16x16x4_f32: f32 operands, f32 accumulate).  Until round 5 every
// f32 attention ran on the VALU kernel below -- 23.8 ms per encoder layer at 20 windows (9.7 TFLOP/s) and 118 us per decode-step
// cross-attention (2.6 TB/s): 1.2 s of the 3.1-s strict pass (profiles/r05_c1_f32pass_kernels.csv).  Same structure as the f16
// kernel: swapped QK^T (S^T = K.Q^T: a lane's four accumulator values belong to ONE query, row statistics = lane-local + two
// shuffles, the exponentiated tile is already the B operand of O^T += V^T.P^T), K / V tiles of 64 keys double-buffered in LDS,
// the next tile's global loads in registers under the current tile's MFMAs.  The k index of a 16 x 16 x 4 instruction is a
// summation index: k-slot g of step (t, e) stands for d = 16 g + 4 t + e (QK^T: one 16-byte LDS read per lane and t) and for
// key 4 g + e of the 16-key block (PV: the S^T accumulator element e IS that key's probability).
//   SPLIT = false: a wave owns 32 queries (two 16-query blocks), the workgroup 128; every wave walks all four 16-key blocks.
//   SPLIT = true (nq <= 16: the decode step's cross-attention, HBM-bound): the four waves share ONE 16-query block and take one
//   16-key block of every tile each; the four partial (max, sum, O) states are merged through LDS at the end.
// V row-major [key][d] (encoder: the fused QKV buffer) or transposed [d][key] (VT: the cross-K/V layout, keys zero padded).
constexpr int F32_KT = 64;           // keys per tile
constexpr int F32_LD = 68;           // floats per LDS row: 16-byte fragment reads of 16 consecutive rows cover all 64 banks
constexpr size_t F32_LDS_BYTES = (size_t)4 * F32_KT * F32_LD * sizeof(float);

template <bool VT, bool SPLIT>
__global__ __launch_bounds__(256, 2) void attn_flash_f32(AttnArgs a)
{
    constexpr int QB = SPLIT ? 1 : 2;            // 16-query blocks per wave
    constexpr int KB = SPLIT ? 1 : 4;            // 16-key blocks of a tile per wave
    extern __shared__ __attribute__((aligned(16))) float f32_smem[];
    float (*Ks)[F32_KT][F32_LD] = (float (*)[F32_KT][F32_LD])f32_smem;                                   // [buf][key][d]
    float (*Vs)[F32_KT][F32_LD] = (float (*)[F32_KT][F32_LD])(f32_smem + 2 * F32_KT * F32_LD);           // [buf][key][d] or, VT, [buf][d][key]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.z, h = blockIdx.y;
    const int q0 = SPLIT ? blockIdx.x * 16 : blockIdx.x * 128 + wave * 32;
    const int qn = lane & 15, g = lane >> 4;
    const float *Q = (const float *)a.q;
    const float *K = (const float *)a.k + (size_t)b * a.k_bs + h * DH;
    const float *V = (const float *)a.v + (size_t)b * a.v_bs + (VT ? (size_t)h * DH * a.vt_kp : (size_t)h * DH);

    f32x4 qf[QB][4];                              // Q[query qn][d = 16 g + 4 t + e]
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
        const int qi = q0 + qb * 16 + qn;
        const float *qp = Q + ((size_t)b * a.q_rows_per_batch + (qi < a.nq ? qi : a.nq - 1)) * a.ldq + h * DH + g * 16;   // clamped
#pragma unroll
        for (int t = 0; t < 4; ++t) qf[qb][t] = *(const f32x4 *)(qp + 4 * t);
    }
    f32x4 o[QB][4];
    float m_run[QB], l_run[QB];                   // l_run: this LANE's share of the row sum (its four keys per block), reduced at the end
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
        m_run[qb] = -__builtin_inff(); l_run[qb] = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t) o[qb][t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }

    // staging registers of one tile: thread -> rows (tid >> 4) + 16 i, floats (tid & 15) * 4 .. + 3
    const int sr = tid >> 4, sc4 = (tid & 15) * 4;
    f32x4 rk[4], rv[4];
    const f32x4 zero4 = (f32x4){0.f, 0.f, 0.f, 0.f};
    auto load_tile = [&](int kt0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = sr + 16 * i;
            const int kg = kt0 + r;
            const int kgc = kg < a.nk ? kg : a.nk - 1;                      // clamped, never predicated
            rk[i] = *(const f32x4 *)(K + (size_t)kgc * a.ldkv + sc4);
            if (kg >= a.nk) rk[i] = zero4;
            if constexpr (VT) {
                rv[i] = *(const f32x4 *)(V + (size_t)r * a.vt_kp + kt0 + sc4);          // row = d; zero padded past nk in the source
            } else {
                rv[i] = *(const f32x4 *)(V + (size_t)kgc * a.ldkv + sc4);
                if (kg >= a.nk) rv[i] = zero4;
            }
        }
    };
    auto store_tile = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            *(f32x4 *)&Ks[buf][sr + 16 * i][sc4] = rk[i];
            *(f32x4 *)&Vs[buf][sr + 16 * i][sc4] = rv[i];
        }
    };

    const int ntile = (a.nk + F32_KT - 1) / F32_KT;
    const bool active = SPLIT || q0 < a.nq;       // wave-uniform: a wave without queries only stages tiles
    load_tile(0);
    store_tile(0);
    __syncthreads();
    for (int t = 0; t < ntile; ++t) {
        const int cur = t & 1, kt0 = t * F32_KT;
        if (t + 1 < ntile) load_tile(kt0 + F32_KT);
        if (active) {
            f32x4 sc[QB][KB];
#pragma unroll
            for (int kbi = 0; kbi < KB; ++kbi) {
                const int kb = SPLIT ? wave : kbi;
                f32x4 kf[4];
#pragma unroll
                for (int tt = 0; tt < 4; ++tt) kf[tt] = *(const f32x4 *)&Ks[cur][kb * 16 + qn][g * 16 + 4 * tt];
#pragma unroll
                for (int qb = 0; qb < QB; ++qb) {
                    f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int tt = 0; tt < 4; ++tt)
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[tt][e], qf[qb][tt][e], acc, 0, 0, 0);
                    sc[qb][kbi] = acc;             // S^T[key kb*16 + 4 g + r][query qn], r = 0..3
                }
            }
#pragma unroll
            for (int qb = 0; qb < QB; ++qb) {
                float tmax = -__builtin_inff();
#pragma unroll
                for (int kbi = 0; kbi < KB; ++kbi) {
                    const int kb = SPLIT ? wave : kbi;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float v = sc[qb][kbi][r] * 0.125f;
                        if (kt0 + kb * 16 + g * 4 + r >= a.nk) v = -__builtin_inff();
                        sc[qb][kbi][r] = v;
                        tmax = fmaxf(tmax, v);
                    }
                }
                tmax = SPLIT ? lane_xor16_max_lds(tmax) : lane_xor16_max(tmax);     // (SPLIT = the HBM-streaming decode step: swx_common.h)
                tmax = SPLIT ? lane_xor32_max_lds(tmax) : lane_xor32_max(tmax);
                const float m_new = fmaxf(m_run[qb], tmax);
                const float m_use = m_new == -__builtin_inff() ? 0.f : m_new;      // a wave whose keys are all masked so far (SPLIT)
                const float alpha = expf(m_run[qb] - m_use);                        // m_run = -inf -> 0
                float psum = 0.f;
#pragma unroll
                for (int kbi = 0; kbi < KB; ++kbi)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float p = expf(sc[qb][kbi][r] - m_use);
                        sc[qb][kbi][r] = p;
                        psum += p;
                    }
                l_run[qb] = l_run[qb] * alpha + psum;
                m_run[qb] = m_new;
#pragma unroll
                for (int tt = 0; tt < 4; ++tt) { o[qb][tt][0] *= alpha; o[qb][tt][1] *= alpha; o[qb][tt][2] *= alpha; o[qb][tt][3] *= alpha; }
            }
            // O^T[d][query] += V^T[d][key] P^T[key][query]: k-slot g of step r <-> key kb*16 + 4 g + r
#pragma unroll
            for (int kbi = 0; kbi < KB; ++kbi) {
                const int kb = SPLIT ? wave : kbi;
#pragma unroll
                for (int tt = 0; tt < 4; ++tt) {
                    f32x4 vf;
                    if constexpr (VT) {
                        vf = *(const f32x4 *)&Vs[cur][tt * 16 + qn][kb * 16 + g * 4];
                    } else {
#pragma unroll
                        for (int r = 0; r < 4; ++r) vf[r] = Vs[cur][kb * 16 + g * 4 + r][tt * 16 + qn];
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r)
#pragma unroll
                        for (int qb = 0; qb < QB; ++qb)
                            o[qb][tt] = __builtin_amdgcn_mfma_f32_16x16x4f32(vf[r], sc[qb][kbi][r], o[qb][tt], 0, 0, 0);
                }
            }
        }
        if (t + 1 < ntile) store_tile(cur ^ 1);
        __syncthreads();
    }

    if constexpr (!SPLIT) {
#pragma unroll
        for (int qb = 0; qb < QB; ++qb) {
            float l = l_run[qb];
            l = lane_xor16_add(l);
            l = lane_xor32_add(l);
            const int qi = q0 + qb * 16 + qn;
            if (active && qi < a.nq) {
                const float inv = 1.0f / l;
                float *op = (float *)a.o + ((size_t)b * a.q_rows_per_batch + qi) * a.ldo + h * DH;
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    f32x4 ov;
#pragma unroll
                    for (int r = 0; r < 4; ++r) ov[r] = o[qb][t][r] * inv;
                    *(f32x4 *)(op + t * 16 + g * 4) = ov;          // O^T[d = 16 t + 4 g + r][query qn]
                }
            }
        }
    } else {
        // merge the four waves' states (the loop's last barrier has passed: the tiles are dead) -- [wave][18][64]: max, lane sum, O
        float *sm = f32_smem;
        sm[(wave * 18 + 0) * 64 + lane] = m_run[0];
        sm[(wave * 18 + 1) * 64 + lane] = l_run[0];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) sm[(wave * 18 + 2 + t * 4 + r) * 64 + lane] = o[0][t][r];
        __syncthreads();
        float mw[4], M = -__builtin_inff();
#pragma unroll
        for (int w = 0; w < 4; ++w) { mw[w] = sm[(w * 18 + 0) * 64 + lane]; M = fmaxf(M, mw[w]); }
        float l = 0.f;
        f32x4 ov = (f32x4){0.f, 0.f, 0.f, 0.f};                    // this wave finishes d-tile `wave`
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const float sc_w = expf(mw[w] - M);                     // -inf (nothing seen) -> 0
            l += sm[(w * 18 + 1) * 64 + lane] * sc_w;
#pragma unroll
            for (int r = 0; r < 4; ++r) ov[r] += sm[(w * 18 + 2 + wave * 4 + r) * 64 + lane] * sc_w;
        }
        l = lane_xor16_add_lds(l);                  // (the SPLIT form keeps its LDS exchanges: swx_common.h)
        l = lane_xor32_add_lds(l);
        const int qi = q0 + qn;
        if (qi < a.nq) {
            const float inv = 1.0f / l;
#pragma unroll
            for (int r = 0; r < 4; ++r) ov[r] *= inv;
            *(f32x4 *)((float *)a.o + ((size_t)b * a.q_rows_per_batch + qi) * a.ldo + h * DH + wave * 16 + g * 4) = ov;
        }
    }
}

// ============================================================================================ dense rowwise
constexpr int RW_QB = 8;
constexpr int RW_MAXK = 1536;

template <typename T>
__global__ __launch_bounds__(256) void attn_dense_rowwise(AttnArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *qs = smem;                       // [RW_QB][64]
    float *sc = smem + RW_QB * DH;          // [RW_QB][nk_pad]
    const int nkp = (a.nk + 3) & ~3;
    float *part = sc + RW_QB * nkp;         // [4][RW_QB][64]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.z, h = blockIdx.y, q0 = blockIdx.x * RW_QB;
    const int nqb = min(RW_QB, a.nq - q0);
    const T *Q = (const T *)a.q;
    const T *K = (const T *)a.k + (size_t)b * a.k_bs + h * DH;
    const T *V = (const T *)a.v + (size_t)b * a.v_bs + (a.vt_kp ? (size_t)h * DH * a.vt_kp : (size_t)h * DH);

    for (int i = tid; i < RW_QB * DH; i += 256) {
        const int qi = i >> 6, d = i & 63;
        qs[i] = (qi < nqb) ? to_f32<T>(Q[((size_t)b * a.q_rows_per_batch + q0 + qi) * a.ldq + h * DH + d]) : 0.f;
    }
    __syncthreads();

    // scores
    for (int j = tid; j < a.nk; j += 256) {
        const T *kr = K + (size_t)j * a.ldkv;
        float acc[RW_QB];
#pragma unroll
        for (int qi = 0; qi < RW_QB; ++qi) acc[qi] = 0.f;
#pragma unroll 2
        for (int d0 = 0; d0 < DH; d0 += 8) {
            float kv[8];
            load8<T>(kr + d0, kv);
#pragma unroll
            for (int e = 0; e < 8; ++e)
#pragma unroll
                for (int qi = 0; qi < RW_QB; ++qi) acc[qi] = fmaf(qs[qi * DH + d0 + e], kv[e], acc[qi]);
        }
#pragma unroll
        for (int qi = 0; qi < RW_QB; ++qi) sc[qi * nkp + j] = acc[qi] * 0.125f;
    }
    __syncthreads();

    // softmax: wave handles queries wave, wave+4
    for (int qi = wave; qi < nqb; qi += 4) {
        float *row = sc + qi * nkp;
        float mx = -__builtin_inff();
        for (int j = lane; j < a.nk; j += 64) mx = fmaxf(mx, row[j]);
        mx = wave_max(mx);
        float sum = 0.f;
        for (int j = lane; j < a.nk; j += 64) { const float e = expf(row[j] - mx); row[j] = e; sum += e; }
        sum = wave_sum(sum);
        const float inv = 1.0f / sum;
        for (int j = lane; j < a.nk; j += 64) row[j] *= inv;
    }
    __syncthreads();

    // out = P V : thread (slice = wave, d = lane)
    float acc[RW_QB];
#pragma unroll
    for (int qi = 0; qi < RW_QB; ++qi) acc[qi] = 0.f;
    if (a.vt_kp) {
        // transposed V: lane = d streams its own key row, wave = contiguous quarter of the keys
        const int per = ((a.nk + 31) / 32) * 8;
        const int j_lo = wave * per, j_hi = min(a.nk, j_lo + per);
        const T *vr = V + (size_t)lane * a.vt_kp;
        for (int j0 = j_lo; j0 < j_hi; j0 += 8) {
            float vv[8];
            load8<T>(vr + j0, vv);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                if (j0 + e < j_hi) {
#pragma unroll
                    for (int qi = 0; qi < RW_QB; ++qi) acc[qi] = fmaf(sc[qi * nkp + j0 + e], vv[e], acc[qi]);
                }
            }
        }
    } else {
        for (int j = wave; j < a.nk; j += 4) {
            const float vv = to_f32<T>(V[(size_t)j * a.ldkv + lane]);
#pragma unroll
            for (int qi = 0; qi < RW_QB; ++qi) acc[qi] = fmaf(sc[qi * nkp + j], vv, acc[qi]);
        }
    }
#pragma unroll
    for (int qi = 0; qi < RW_QB; ++qi) part[(wave * RW_QB + qi) * DH + lane] = acc[qi];
    __syncthreads();
    for (int i = tid; i < nqb * DH; i += 256) {
        const int qi = i >> 6, d = i & 63;
        const float v = part[(0 * RW_QB + qi) * DH + d] + part[(1 * RW_QB + qi) * DH + d] +
                        part[(2 * RW_QB + qi) * DH + d] + part[(3 * RW_QB + qi) * DH + d];
        ((T *)a.o)[((size_t)b * a.q_rows_per_batch + q0 + qi) * a.ldo + h * DH + d] = from_f32<T>(v);
    }
}

}  // namespace

// The dynamic-LDS grant of the four attn_flash_f32 instantiations (swx_common.h: once per kernel and device).  False when the
// device cannot grant 68 KB: the caller then takes the VALU kernel instead of failing.
static bool f32_flash_ready(bool vt, bool split)
{
    constexpr int need = (int)F32_LDS_BYTES;
    const hipError_t e = vt ? (split ? swx_lds_grant<attn_flash_f32<true, true>>(need) : swx_lds_grant<attn_flash_f32<true, false>>(need))
                            : (split ? swx_lds_grant<attn_flash_f32<false, true>>(need) : swx_lds_grant<attn_flash_f32<false, false>>(need));
    return e == hipSuccess;
}

int swx_attention(int dtype, const AttnArgs &a, int force_kernel, hipStream_t s)
{
    if (a.B <= 0 || a.nq <= 0 || a.nk <= 0) return 0;
    if (a.nk > RW_MAXK) return -5;
    const bool flash = (dtype == SWX_F16) && (force_kernel == 2 || (force_kernel >= 4 && force_kernel <= 6) || (force_kernel == 0 && a.nq >= 32));
    const size_t esz = dtype == SWX_F16 ? 2 : 4;
    const SwxXattnPlan xp = swx_xattn_plan(dtype, a, force_kernel, swx_flags());
    if (xp.family < 0) return xp.family;
    if (xp.family != SWX_XA_NOT_DECODE) return swx_xattn_launch(xp, a, s);
    if (flash) {
        if (dtype != SWX_F16) return -5;
        SwxProfScope prof(PC_ATTN_FLASH, 4.0 * a.B * a.H * (double)a.nq * a.nk * 64, s);
        // queries per wave: 64 when the query axis is long (encoder self-attention: 1 500 queries) AND the launch still has a
        // workgroup for every CU that way (at one window 64 queries per wave are 6 x 20 = 120 workgroups), 32 otherwise;
        // force_kernel 4 / 6 / 5 pin 32 / 48 / 64 (scripts/kernel_bench.py --flash-kernel, --only flash_small)
        const bool wide_fills = (int64_t)a.B * a.H * cdiv(a.nq, 256) >= 256;
        // ... and 16 while 32 per wave would leave the launch at one workgroup per CU or less (the encoder of ONE window: 12 x 20 = 240 workgroups
        // = one wave per SIMD on a kernel whose softmax and MFMA stretches want a second wave to fill them; 24 x 20 = 480 that way).  A
        // query block's arithmetic does not depend on how many blocks its wave carries: bit-identical (SWX_FLAG_FLASH_NO_QB1: A/B)
        const bool narrow_fills = a.vt_kp && force_kernel == 0 && a.nq >= 256 && (int64_t)a.B * a.H * cdiv(a.nq, 128) <= 256 &&
                                  !(swx_flags() & SWX_FLAG_FLASH_NO_QB1);
        const int qb = !a.vt_kp ? 2 : narrow_fills ? 1 : force_kernel == 4 ? 2 : force_kernel == 6 ? 3 : (force_kernel == 5 || (a.nq >= 1024 && wide_fills)) ? 4 : 2;
        dim3 g(cdiv(a.nq, 64 * qb), a.H, a.B);
        const bool gen3 = a.vt_kp && (swx_flags() & SWX_FLAG_FLASH_PIPELINED);  // round 6's software-pipelined tile: bit-identical, slower (A/B only)
        if (!a.vt_kp) hipLaunchKernelGGL((attn_flash2_f16<false, 2>), g, dim3(256), 0, s, a);
        else if (gen3 && qb == 4) hipLaunchKernelGGL((attn_flash3_f16<4>), g, dim3(256), 0, s, a);
        else if (gen3 && qb == 3) hipLaunchKernelGGL((attn_flash3_f16<3>), g, dim3(256), 0, s, a);
        else if (gen3 && qb == 2) hipLaunchKernelGGL((attn_flash3_f16<2>), g, dim3(256), 0, s, a);
        else if (qb == 4) hipLaunchKernelGGL((attn_flash2_f16<true, 4>), g, dim3(256), 0, s, a);
        else if (qb == 3) hipLaunchKernelGGL((attn_flash2_f16<true, 3>), g, dim3(256), 0, s, a);
        else if (qb == 1) hipLaunchKernelGGL((attn_flash2_f16<true, 1>), g, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((attn_flash2_f16<true, 2>), g, dim3(256), 0, s, a);
    } else if (dtype == SWX_F32 && (force_kernel == 0 || force_kernel == 7) && a.vt_kp % F32_KT == 0 &&
               // a transposed V is read as V[d][kt0 .. kt0 + 63] for every key tile: its row pitch must cover the padded key axis
               (a.vt_kp == 0 || a.vt_kp >= cdiv(a.nk, F32_KT) * F32_KT) && f32_flash_ready(a.vt_kp != 0, a.nq <= 16 && !a.f32_no_split)) {
        // strict f32 on the exact-f32 matrix instruction: queries <= 16 per batch item (decode step: HBM-bound, the four waves split
        // the keys) or blocks of 128 queries (encoder self-attention, scoring pass: MFMA-bound).  Where the 68 KB of dynamic LDS
        // cannot be granted (f32_flash_ready: not gfx950) the launch falls through to the VALU kernel below.
        const bool split = a.nq <= 16 && !a.f32_no_split;
        SwxProfScope prof(split ? PC_ATTN_ROWWISE : PC_ATTN_FLASH,
                          split ? (double)a.B * a.H * 64 * esz * (2.0 * a.nk + 2.0 * a.nq) : 4.0 * a.B * a.H * (double)a.nq * a.nk * 64, s);
        dim3 gd(split ? 1 : cdiv(a.nq, 128), a.H, a.B);
        if (a.vt_kp) {
            if (split) hipLaunchKernelGGL((attn_flash_f32<true, true>), gd, dim3(256), F32_LDS_BYTES, s, a);
            else hipLaunchKernelGGL((attn_flash_f32<true, false>), gd, dim3(256), F32_LDS_BYTES, s, a);
        } else {
            if (split) hipLaunchKernelGGL((attn_flash_f32<false, true>), gd, dim3(256), F32_LDS_BYTES, s, a);
            else hipLaunchKernelGGL((attn_flash_f32<false, false>), gd, dim3(256), F32_LDS_BYTES, s, a);
        }
    } else {
        if (force_kernel == 7) return -5;
        // algorithmic bytes: K and V of every (window, head) once + q in + o out
        SwxProfScope prof(PC_ATTN_ROWWISE, (double)a.B * a.H * 64 * esz * (2.0 * a.nk + 2.0 * a.nq), s);
        dim3 g(cdiv(a.nq, RW_QB), a.H, a.B);
        const int nkp = (a.nk + 3) & ~3;
        const size_t smem = sizeof(float) * ((size_t)RW_QB * DH + (size_t)RW_QB * nkp + (size_t)4 * RW_QB * DH);
        if (dtype == SWX_F16) hipLaunchKernelGGL(attn_dense_rowwise<f16>, g, dim3(256), smem, s, a);
        else hipLaunchKernelGGL(attn_dense_rowwise<float>, g, dim3(256), smem, s, a);
    }
    SWX_CHECK_LAUNCH();
    return 0;
}

int swx_transpose_v(const void *v, int64_t ldv, int64_t v_bs, int n, void *vt, int kp, int64_t vt_bs, int B, int H, hipStream_t s)
{
    if (B <= 0 || n <= 0) return 0;
    if (kp % 8 != 0 || kp < n) return -5;
    hipLaunchKernelGGL(transpose_v_kernel, dim3(cdiv(kp, 64), H, B), dim3(256), 0, s, (const f16 *)v, ldv, v_bs, n, (f16 *)vt, kp, vt_bs);
    SWX_CHECK_LAUNCH();
    return 0;
}

// zeroes `pad_bytes` at byte offset `off_bytes` of each of `rows` rows (row stride `row_bytes`) of `nb` batch items (stride
// `batch_bytes`): the key padding of the transposed cross-attention V (columns n .. kp of every [64 x kp] head block), which
// is multiplied by exact-zero probabilities and therefore has to be finite.  (Filling the whole cross-K/V buffer with zeros
// first -- 9.8 GB per 20-window batch -- cost 1.9 ms per pass.)
__global__ __launch_bounds__(256) void pad_zero_kernel(unsigned char *base, int64_t row_bytes, int64_t batch_bytes, int off_bytes,
                                                       int pad_bytes, int rows)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    unsigned char *p = base + (size_t)blockIdx.y * batch_bytes + (size_t)r * row_bytes + off_bytes;
    if ((((uintptr_t)p) & 7) == 0 && (pad_bytes & 7) == 0) {
        for (int i = 0; i < pad_bytes; i += 8) *(unsigned long long *)(p + i) = 0ull;
    } else {
        for (int i = 0; i < pad_bytes; ++i) p[i] = 0;
    }
}

int swx_pad_zero(void *base, int64_t row_bytes, int64_t batch_bytes, int off_bytes, int pad_bytes, int rows, int nb, hipStream_t s)
{
    if (rows <= 0 || nb <= 0 || pad_bytes <= 0) return 0;
    hipLaunchKernelGGL(pad_zero_kernel, dim3(cdiv(rows, 256), nb), dim3(256), 0, s, (unsigned char *)base, row_bytes, batch_bytes,
                       off_bytes, pad_bytes, rows);
    SWX_CHECK_LAUNCH();
    return 0;
}
