// swx_gemm.hip -- C = epilogue(A[M,K] * W[N,K]^T) on gfx950 MFMA.
//
// Every Linear / Conv1d of the Whisper encoder and decoder (upstream whisper/model.py, reached from
// stable_whisper/decode.py:27-30,40 and timing.py:59-61) goes through these kernels.  Weights keep the
// checkpoint's [out, in] layout, so both operands are K-contiguous ("B^T input") and each MFMA fragment is one
// 16-byte load.  This file holds the dispatch -- swx_gemm_plan_f16 (which f16 kernel a launch gets) and swx_gemm -- and the skinny
// kernel; every other family has a file of its own with its launch function (swx_gemm_tile.h declares them and holds what they share):
//   swx_gemm_tiled.hip
//   * tiled f16, register-staged   128x128x64 tile, 4 waves (2x2), 4x4 v_mfma_f32_16x16x32_f16 per wave: K % 64 != 0, and the
//                                  bit-identity reference of the four below
//   * gemm_f16_glds_128 / _64      the same tile filled by LDS-DMA, one operand buffer, three workgroups per CU overlap each other
//   * gemm_f16_ring<64|128, 3>     launches with <= 1 workgroup per CU: three LDS stages, LDS-DMA from inline asm, counted waits
//   swx_gemm_big.hip
//   * gemm_f16_big8                256x256 tile, 8 waves, LDS-DMA into a ring of eight half-tile slots, four phases per K tile, the
//                                  two row groups of waves half a phase apart: launches that fill whole rounds of the 256 CUs
//   swx_gemm_f32.hip
//   * tiled f32, f32 rows64        the 128x128 tiling on v_mfma_f32_16x16x4_f32 (exact f32 fma chain), and its restaging for
//                                  launches of at most 128 rows                                            (strict-parity mode)
//   here
//   * skinny f16                   M <= 128 rows: one 16-column weight panel per workgroup, K split over its 4 waves, weights
//                                  streamed straight from HBM into MFMA fragments (no LDS), LDS reduction
// Epilogue (f32): +bias, GELU(erf), +f32 residual indexed by row % res_mod (positional embedding), +T residual,
// store as T or f32.
#include "swx_gemm_tile.h"

namespace {

// ----------------------------------------------------------------------------------------------- skinny f16
// HBM-bound weight streaming for the decode steps.  Workgroup = one 16-column weight panel, its 4 waves split K.
// Per wave the K slice is walked in chunks of CH k-steps with a two-deep register pipeline: the 16-byte weight
// fragments (HBM) and the MT activation fragments (L2-resident, re-read by every panel) of chunk c+1 are in flight
// while the MFMAs of chunk c issue -- without it each k-step exposes a full memory round trip (measured 40 us per
// launch at M=100 before, rocprof r01 v0).
template <int MT>
__global__ __launch_bounds__(256) void gemm_f16_skinny(GemmArgs g)
{
    constexpr int NKS_MAX = 10;      // k-steps (of 32) per wave: the launcher keeps K / 128 <= 10
    __shared__ f32x4 red[3][MT][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n0 = blockIdx.x * 16;
    const f16 *A = (const f16 *)g.A;
    const f16 *W = (const f16 *)g.W;
    const int fr = lane & 15, fk = (lane >> 4) * 8;
    // K is split over the 4 waves
    const int kslice = g.K / 4;
    const int nks = kslice / 32;
    const int kb = wave * kslice;
    const int n = n0 + fr;
    const bool nok = n < g.N;
    const f16 *wp = W + (size_t)(nok ? n : 0) * g.ldw + kb + fk;
    const f16x8 zero8 = (f16x8)(f16)0;

    // HBM side first: every weight fragment of this wave's K slice is put in flight at once (<= 10 x 1 KB per wave);
    // the bandwidth-delay product of the chip (~10 MB) needs tens of KB outstanding per CU, which a double-buffered
    // weight load cannot provide
    f16x8 wf[NKS_MAX];
#pragma unroll
    for (int ks = 0; ks < NKS_MAX; ++ks) {
        const f16x8 v = *(const f16x8 *)(wp + (ks < nks ? ks : nks - 1) * 32);
        wf[ks] = (nok && ks < nks) ? v : zero8;
    }

    f32x4 acc[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const f16 *ap[MT];
    bool aok[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) {
        const int m = t * 16 + fr;
        aok[t] = m < g.M;
        ap[t] = A + (size_t)(aok[t] ? m : 0) * g.lda + kb + fk;
    }
    // L2 side: activation fragments, two k-steps deep
    f16x8 af[2][MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) { const f16x8 v = *(const f16x8 *)(ap[t]); af[0][t] = aok[t] ? v : zero8; }
#pragma unroll
    for (int ks = 0; ks < NKS_MAX; ++ks) {
        if (ks < nks) {
            if (ks + 1 < nks) {
#pragma unroll
                for (int t = 0; t < MT; ++t) { const f16x8 v = *(const f16x8 *)(ap[t] + (ks + 1) * 32); af[(ks + 1) & 1][t] = aok[t] ? v : zero8; }
            }
#pragma unroll
            for (int t = 0; t < MT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[ks & 1][t], wf[ks], acc[t], 0, 0, 0);
        }
    }

    if (wave > 0) {
#pragma unroll
        for (int t = 0; t < MT; ++t) red[wave - 1][t][lane] = acc[t];
    }
    __syncthreads();
    if (wave == 0) {
        const int col = n0 + (lane & 15), row_l = (lane >> 4) * 4;
#pragma unroll
        for (int t = 0; t < MT; ++t) {
            f32x4 v = acc[t];
#pragma unroll
            for (int w = 0; w < 3; ++w) {
                const f32x4 o = red[w][t][lane];
                v[0] += o[0]; v[1] += o[1]; v[2] += o[2]; v[3] += o[3];
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) epilogue_store<f16>(g, t * 16 + row_l + r, col, v[r]);
        }
    }
}

// gemm_f16_skinny<mt> for mt = 1 .. 7 row tiles, <8> for more
template <int MT = 1>
void launch_skinny(int mt, const GemmArgs &g, hipStream_t s)
{
    if constexpr (MT < 8) {
        if (mt > MT) return launch_skinny<MT + 1>(mt, g, s);
    }
    hipLaunchKernelGGL(gemm_f16_skinny<MT>, dim3(cdiv(g.N, 16)), dim3(256), 0, s, g);
}

}  // namespace

// Which f16 kernel a launch gets.  One pure function (no device state) so that the rule is testable without a GPU
// (tests/test_gemm_plan_cpu.py restates the benchmarked shapes) and is what swx_gemm executes.  `ptr16` = A, W (and C / R for
// the big kernel's vector epilogue) are 16-byte aligned; `force_kernel`: 0 dispatch, 1 register-staged, 2 skinny, 7 direct-to-LDS
// with occupancy overlap (8 / 9: its 64-column tiles always / never), 10 / 11 ring at 64 / 128 columns, 12 the 256 x 256 kernel.
int swx_gemm_plan_f16(int M, int N, int K, int epi, int64_t ldc, int64_t ldr, bool ptr16, int force_kernel, int flags)
{
    if (K % 32 != 0) return -4;                                            // tiled: K % 32, skinny: K % 128
    const bool skinny_ok = M <= 128 && K % 128 == 0 && K / 128 <= 10 && N <= 16384;   // vocabulary-sized N: tiled
    if (force_kernel == 2) return skinny_ok ? SWX_GEMM_SKINNY : -4;
    if (skinny_ok && force_kernel != 1 && force_kernel < 7) return SWX_GEMM_SKINNY;
    const bool glds_ok = K % 64 == 0 && ptr16;
    if (force_kernel >= 7 && !glds_ok) return -4;
    if (force_kernel == 1 || !glds_ok) return SWX_GEMM_TILED_REG;          // K % 64 != 0, and the bit-identity reference
    const int64_t t128 = (int64_t)cdiv(N, BN) * cdiv(M, BM);
    // 64-column tiles when 128-wide ones would leave CUs idle (encoder at one window: M = 1500, N = 1280 is 120 tiles of
    // 128 x 128 for 256 CUs)
    const bool narrow = force_kernel == 8 || (force_kernel != 9 && N % 64 == 0 && t128 < 224);
    // the 256 x 256 kernel: plain epilogues, when its tiles fill whole rounds of the 256 CUs -- one workgroup per CU, so a last
    // round that is 30 % full costs a full round (M = 6000, N = 3840: 360 tiles, 769 against 885 TFLOP/s) -- or nearly so with
    // a long K to amortise prologue and epilogue (M = 30 000, N = 1280, K = 5120: 590 tiles, 979 against 892); not for K < 512
    // (profiles/r03_kb_gemm_big.txt)
    const bool big_ok = !(epi & ~(EPI_BIAS | EPI_GELU | EPI_RES)) && ldc % 8 == 0 && (!(epi & EPI_RES) || ldr % 8 == 0);
    if (force_kernel == 12) return big_ok && K >= 128 ? SWX_GEMM_BIG : -4;      // (its prologue keeps two K tiles in flight)
    const int64_t t256 = (int64_t)cdiv(M, BG) * cdiv(N, BG);
    const double fill = (double)t256 / (double)(((t256 + 255) / 256) * 256);
    if (force_kernel == 0 && big_ok && t256 >= 200 && K >= 512 && (fill >= 0.9 || (fill >= 0.75 && K >= 2560)) &&
        !(flags & SWX_FLAG_NO_BIG_TILE))
        return SWX_GEMM_BIG;
    // the ring kernel for launches of at most one workgroup per CU (the encoder / cross-K/V at one window: 64-column tiles when
    // `narrow`, else 128-column ones up to 256 tiles); from ~1.5 workgroups per CU on, gemm_f16_glds -- three resident
    // workgroups, epilogues overlapped with the neighbours' MFMAs -- is as fast or faster (N = 3840 / 5120 at M = 1500: 29.3 /
    // 29.6 us against 33.4 / 35.9; profiles/r03_kb_gemm_ring.txt).  Not the one-row-tile logits GEMM (133 MB of weights).
    const bool ring_ok = K >= 128;
    if (force_kernel == 10 || force_kernel == 11) return !ring_ok ? -4 : force_kernel == 10 ? SWX_GEMM_RING64 : SWX_GEMM_RING128;
    if (force_kernel == 0 && ring_ok && M > 256 && (narrow || t128 <= 256) && !(flags & SWX_FLAG_NO_RING))
        return narrow ? SWX_GEMM_RING64 : SWX_GEMM_RING128;
    return narrow ? SWX_GEMM_GLDS64 : SWX_GEMM_GLDS128;
}

int swx_gemm(int dtype, const GemmArgs &g, int force_kernel, hipStream_t s)
{
    if (g.M <= 0 || g.N <= 0) return 0;
    if (dtype == SWX_F16) {
        if (g.lda % 8 != 0 || g.ldw % 8 != 0) return -4;
        const bool ptr16 = (uintptr_t)g.A % 16 == 0 && (uintptr_t)g.W % 16 == 0;
        // (C / R alignment only matters to the big kernel's 16-byte epilogue: withheld from it by an unaligned leading dimension)
        const bool cr16 = (uintptr_t)g.C % 16 == 0 && (!(g.epi & EPI_RES) || (uintptr_t)g.R % 16 == 0);
        const int plan = swx_gemm_plan_f16(g.M, g.N, g.K, g.epi, cr16 ? g.ldc : 1, cr16 ? g.ldr : 1, ptr16, force_kernel, swx_flags());
        if (plan < 0) return plan;
        if (plan == SWX_GEMM_SKINNY) {
            SwxProfScope prof(PC_GEMM_SKINNY, 2.0 * ((double)g.N * g.K + (double)g.M * g.K) + (double)g.M * g.N * ((g.epi & EPI_OUT_F32) ? 4 : 2), s);
            launch_skinny(cdiv(g.M, 16), g, s);
        } else {
            SwxProfScope prof(PC_GEMM_TILED, 2.0 * (double)g.M * g.N * g.K, s);
            // (a refused dynamic-LDS grant of the ring / 256 x 256 kernels comes back as -100 - its error)
            if (const int rc = plan == SWX_GEMM_BIG ? swx_gemm_launch_big8(g, s) : swx_gemm_launch_tiled(plan, g, s)) return rc;
        }
    } else {
        if (g.K % 16 != 0 || g.lda % 4 != 0 || g.ldw % 4 != 0) return -4;
        SwxProfScope prof(PC_GEMM_TILED, 2.0 * (double)g.M * g.N * g.K, s);
        swx_gemm_launch_f32(g, force_kernel, s);
    }
    SWX_CHECK_LAUNCH();
    return 0;
}
