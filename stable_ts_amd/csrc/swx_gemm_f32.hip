// swx_gemm_f32.hip -- the two GEMM kernels of the strict-f32 mode, on v_mfma_f32_16x16x4_f32 (an exact f32 fma chain per output element):
// gemm_f32_tiled (128 x 128, 64 x 32 and 64 x 16 tiles) and gemm_f32_rows64 (at most 128 rows, 64-deep K chunks).  Element-wise
// epilogue (swx_gemm_tile.h::epilogue_store).  swx_gemm_launch_f32 at the end of the file says which launch gets which.
#include "swx_gemm_tile.h"

namespace {

// ------------------------------------------------------------------------------------------------ tiled f32
constexpr int BK32 = 16, LD32 = BK32 + 1;

// BMT x BNT = tile (128 x 128; 64 x 32 / 64 x 16 for launches with few rows, where 128-wide tiles leave N / 128 = 10-40 workgroups on
// 256 CUs and one CU's exact-f32 MFMA rate bounds the launch), ST = K
// steps of operands held in REGISTERS ahead of the one being multiplied.  Round 4: with ST = 2 (one step ahead) every 16-deep K
// step waited out a global round trip -- 2.6 us per step, 210 us for a K = 1280 launch at 100 rows: the decode-step projections of
// the strict-f32 mode, 3.9 s of its 5.8-s pass.  Operands now travel ST - 1 steps ahead.  Per output element the arithmetic is
// unchanged in every variant (one accumulator, K ascending in steps of 4), so all variants are bit-identical.
template <int BMT, int BNT, int ST>
__global__ __launch_bounds__(256) void gemm_f32_tiled(GemmArgs g)
{
    constexpr int WN = BNT >= 128 ? 2 : 1, WM = 4 / WN;                             // waves across the tile's columns / rows
    constexpr int WROWS = BMT / WM, WCOLS = BNT / WN;                                // a wave's share of the BMT x BNT tile
    constexpr int NI = WROWS / 16, NJ = WCOLS / 16;
    constexpr int NA = (BMT * 4 + 255) / 256, NB = (BNT * 4 + 255) / 256;            // float4 loads of the A / B tile per thread
    static_assert(NI >= 1 && NJ >= 1, "a wave owns at least one 16 x 16 fragment");
    __shared__ float As[2][BMT][LD32];
    __shared__ float Bs[2][BNT][LD32];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = WN == 2 ? wave >> 1 : wave, wn = WN == 2 ? wave & 1 : 0;
    const int m0 = blockIdx.y * BMT, n0 = blockIdx.x * BNT;
    const float *A = (const float *)g.A;
    const float *W = (const float *)g.W;

    f32x4 acc[NI][NJ];
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    f32x4 ra[ST][NA], rb[ST][NB];
    auto load_regs = [&](int st, int k0) {
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int c = tid + 256 * i, row = c >> 2, kc = (c & 3) * 4;
            const int gm = m0 + row;
            ra[st][i] = (row < BMT && gm < g.M) ? *(const f32x4 *)(A + (size_t)gm * g.lda + k0 + kc) : (f32x4){0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int c = tid + 256 * i, row = c >> 2, kc = (c & 3) * 4;
            const int gn = n0 + row;
            rb[st][i] = (row < BNT && gn < g.N) ? *(const f32x4 *)(W + (size_t)gn * g.ldw + k0 + kc) : (f32x4){0.f, 0.f, 0.f, 0.f};
        }
    };
    auto store_lds = [&](int st, int buf) {
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int c = tid + 256 * i, row = c >> 2, kc = (c & 3) * 4;
            if (row < BMT) {
#pragma unroll
                for (int e = 0; e < 4; ++e) As[buf][row][kc + e] = ra[st][i][e];
            }
        }
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int c = tid + 256 * i, row = c >> 2, kc = (c & 3) * 4;
            if (row < BNT) {
#pragma unroll
                for (int e = 0; e < 4; ++e) Bs[buf][row][kc + e] = rb[st][i][e];
            }
        }
    };
    auto compute = [&](int cur) {
        const int fr = lane & 15, fk = lane >> 4;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            float a[NI], b[NJ];
#pragma unroll
            for (int i = 0; i < NI; ++i) a[i] = As[cur][wm * WROWS + i * 16 + fr][kk * 4 + fk];
#pragma unroll
            for (int j = 0; j < NJ; ++j) b[j] = Bs[cur][wn * WCOLS + j * 16 + fr][kk * 4 + fk];
#pragma unroll
            for (int i = 0; i < NI; ++i)
#pragma unroll
                for (int j = 0; j < NJ; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
    };

    const int KT = g.K / BK32;
    // register stage of K step kt is kt % ST; steps 0 .. ST - 2 are requested up front
#pragma unroll
    for (int st = 0; st < ST - 1; ++st) if (st < KT) load_regs(st, st * BK32);
    store_lds(0, 0);
    __syncthreads();
    for (int kt0 = 0; kt0 < KT; kt0 += ST) {
#pragma unroll
        for (int u = 0; u < ST; ++u) {                       // (unrolled: the register stages are compile-time indices)
            const int kt = kt0 + u;
            if (kt < KT) {
                const int cur = kt & 1;
                if (kt + ST - 1 < KT) load_regs((u + ST - 1) % ST, (kt + ST - 1) * BK32);
                compute(cur);
                if (kt + 1 < KT) store_lds((u + 1) % ST, cur ^ 1);
                __syncthreads();
            }
        }
    }

    const int col_l = lane & 15, row_l = (lane >> 4) * 4;
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                epilogue_store<float>(g, m0 + wm * WROWS + i * 16 + row_l + r, n0 + wn * WCOLS + j * 16 + col_l, acc[i][j][r]);
}

// ------------------------------------------------------------------------------------------------ f32, few rows (round 5)
// The strict-f32 launches with at most 128 rows (decode step at 100 rows, prefill, one window's scoring pass) on 64 x 16 NJ tiles:
// the arithmetic of gemm_f32_tiled element for element (one accumulator, K ascending in steps of 4, k-slot g of step s = k 4 s + g:
// bit-identical, tests/test_gpu_kernels.py), restaged.  gemm_f32_tiled<64, 16 | 32> spent a barrier, a scalar LDS round trip and
// 17-word rows on every 16-deep K step (4 MFMAs = 128 MFMA clocks per ~1 000-clock step: 36-64 us for a K = 1280 launch, 1.2 s of
// the 3.1-s strict pass, profiles/r05_c1_f32pass_kernels.csv).  Here a K chunk is 64 deep (16 NJ MFMAs per wave and barrier), a
// thread stages 16 consecutive k of one row (four 16-byte loads, two chunks ahead in registers) and writes them TRANSPOSED 4 x 4
// in registers -- LDS position 16 t + 4 g + e holds k = 16 t + 4 e + g -- so that the four steps 4 t .. 4 t + 3 of a lane's k-slot
// are ONE 16-byte LDS read; rows of 68 words keep those reads and the 16-byte writes conflict-free.
constexpr int R64_LD = 68;
template <int NJ>
__global__ __launch_bounds__(256) void gemm_f32_rows64(GemmArgs g)
{
    constexpr int BNT = 16 * NJ;
    __shared__ __attribute__((aligned(16))) float As[2][64][R64_LD];
    __shared__ __attribute__((aligned(16))) float Bs[2][BNT][R64_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 15, fg = lane >> 4;
    const int m0 = blockIdx.y * 64, n0 = blockIdx.x * BNT;
    const float *A = (const float *)g.A;
    const float *W = (const float *)g.W;
    // staging: A tile: thread -> (row = tid >> 2, 16-k group = tid & 3), four 16-byte loads, written 4 x 4 transposed with 16-byte
    // LDS stores; B tile (16 NJ rows): thread -> (row = tid >> 4 [+ 16], k = 4 (tid & 15) .. + 3), ONE 16-byte load per 16 rows,
    // four scalar LDS stores -- every thread does the same work: no divergent branch around a load or its wait
    const int srow = tid >> 2, sgrp = tid & 3;
    const bool a_ok = m0 + srow < g.M;
    const float *ap = A + (size_t)(a_ok ? m0 + srow : g.M - 1) * g.lda + sgrp * 16;
    const int brow = tid >> 4, bc4 = tid & 15;
    bool b_ok[NJ];
    const float *wp[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        b_ok[j] = n0 + j * 16 + brow < g.N;
        wp[j] = W + (size_t)(b_ok[j] ? n0 + j * 16 + brow : g.N - 1) * g.ldw + bc4 * 4;
    }
    const int bpos = 16 * (bc4 >> 2) + (bc4 & 3);       // k = 16 t + 4 e + i (t = bc4 >> 2, e = bc4 & 3) -> position 16 t + 4 i + e
    const f32x4 zero4 = (f32x4){0.f, 0.f, 0.f, 0.f};

    f32x4 acc[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[j] = zero4;
    f32x4 ra[2][4], rb[2][NJ];
#pragma unroll
    for (int st = 0; st < 2; ++st) {
#pragma unroll
        for (int e = 0; e < 4; ++e) ra[st][e] = zero4;
#pragma unroll
        for (int j = 0; j < NJ; ++j) rb[st][j] = zero4;
    }
    // Clamped addresses, never a predicated load; the zero-select of rows past M / N only when the registers go to LDS; and the
    // loads themselves in inline asm behind a hand-counted wait.  What hipcc made of ordinary loads here, seen in the ISA one form
    // after the other: a conditional load = a branch whose join waits vmcnt(0); a select right behind the load waits for it at
    // once; a prefetch under `if (c + 2 < KC)` makes the wait for chunk c + 1 valid for the path WITHOUT new loads, i.e. drains
    // them; and with everything unconditional the loop header still got a vmcnt(0) for the stage carried around the back edge.
    // Each form drained the two-chunk prefetch once per chunk (first hardware run: 22 us per K = 1280 launch).  Loads return in
    // issue order: chunk c + 1 has landed once only the NL loads of chunk c + 2 are pending.
    constexpr int NL = 4 + NJ;                     // loads per thread and chunk
    auto load_regs = [&](int st, int k0) {
#pragma unroll
        for (int e = 0; e < 4; ++e) asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(ra[st][e]) : "v"(ap + k0 + 4 * e) : "memory");
#pragma unroll
        for (int j = 0; j < NJ; ++j) asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(rb[st][j]) : "v"(wp[j] + k0) : "memory");
    };
    auto wait_stage = [&](int st) {                // stage st is the OLDER of the two in flight
        if constexpr (NJ == 1)
            asm volatile("s_waitcnt vmcnt(%5)" : "+v"(ra[st][0]), "+v"(ra[st][1]), "+v"(ra[st][2]), "+v"(ra[st][3]), "+v"(rb[st][0]) : "n"(NL) : "memory");
        else
            asm volatile("s_waitcnt vmcnt(%6)" : "+v"(ra[st][0]), "+v"(ra[st][1]), "+v"(ra[st][2]), "+v"(ra[st][3]), "+v"(rb[st][0]), "+v"(rb[st][NJ - 1]) : "n"(NL) : "memory");
    };
    auto store_lds = [&](int st, int buf) {
        // registers hold k = 16 sgrp + 4 e + i as ra[st][e][i]; LDS position 16 sgrp + 4 i + e
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const f32x4 va = (f32x4){ra[st][0][i], ra[st][1][i], ra[st][2][i], ra[st][3][i]};
            *(f32x4 *)&As[buf][srow][16 * sgrp + 4 * i] = a_ok ? va : zero4;
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i) Bs[buf][j * 16 + brow][bpos + 4 * i] = b_ok[j] ? rb[st][j][i] : 0.f;
    };
    auto compute = [&](int buf) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const f32x4 a4 = *(const f32x4 *)&As[buf][wave * 16 + fr][16 * t + 4 * fg];
            f32x4 b4[NJ];
#pragma unroll
            for (int j = 0; j < NJ; ++j) b4[j] = *(const f32x4 *)&Bs[buf][j * 16 + fr][16 * t + 4 * fg];
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int j = 0; j < NJ; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[e], b4[j][e], acc[j], 0, 0, 0);
        }
    };

    const int KC = g.K / 64;
    load_regs(0, 0);
    load_regs(1, KC > 1 ? 64 : 0);
    wait_stage(0);
    store_lds(0, 0);
    __syncthreads();
    for (int c0 = 0; c0 < KC; c0 += 2) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {                       // (unrolled: the register stages are compile-time indices)
            const int c = c0 + u;
            if (c < KC) {
                // stage u went to LDS at the end of step c - 1.  Issued unconditionally (past the end: the last chunk again, never
                // stored): under a condition hipcc's wait for chunk c + 1 must hold on the path WITHOUT new loads and drains them
                load_regs(u, (c + 2 < KC ? c + 2 : KC - 1) * 64);
                compute(c & 1);
                if (c + 1 < KC) { wait_stage(u ^ 1); store_lds(u ^ 1, (c + 1) & 1); }
                __syncthreads();
            }
        }
    }
    // The idle re-loads of the last chunk are still in flight, and hipcc believes their destination registers dead (no store
    // follows): without the statements below it hands them out to the epilogue's address arithmetic while the loads land in them
    // (first hardware run of this form: wrong results and a memory fault).  Every staging register stays allocated up to the wait.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int st = 0; st < 2; ++st) {
#pragma unroll
        for (int e = 0; e < 4; ++e) asm volatile("" ::"v"(ra[st][e]));
#pragma unroll
        for (int j = 0; j < NJ; ++j) asm volatile("" ::"v"(rb[st][j]));
    }
    const int col_l = lane & 15, row_l = (lane >> 4) * 4;
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) epilogue_store<float>(g, m0 + wave * 16 + row_l + r, n0 + j * 16 + col_l, acc[j][r]);
}

}  // namespace

void swx_gemm_launch_f32(const GemmArgs &g, int force_kernel, hipStream_t s)
{
    // few rows (decode step, prefill, a single window's scoring pass): 64 x 32 or 64 x 16 tiles spread the launch over
    // 160-320 workgroups instead of N / 128 = 10-40 (one CU's exact-f32 MFMA rate is 0.6 TFLOP/s); bit-identical either way,
    // so the choice may depend on the launch
    if (g.M <= BM && g.N >= 256 && g.K % 64 == 0 && force_kernel != 8) {
        // (round 5) the same tiles on 64-deep K chunks; force_kernel 8 keeps the 16-deep generation as its bit-identity reference
        if (g.N >= 2560) hipLaunchKernelGGL((gemm_f32_rows64<2>), dim3(cdiv(g.N, 32), cdiv(g.M, 64)), dim3(256), 0, s, g);
        else hipLaunchKernelGGL((gemm_f32_rows64<1>), dim3(cdiv(g.N, 16), cdiv(g.M, 64)), dim3(256), 0, s, g);
    } else if (g.M <= BM && g.N >= 256) {
        if (g.N >= 2560) hipLaunchKernelGGL((gemm_f32_tiled<64, 32, 4>), dim3(cdiv(g.N, 32), cdiv(g.M, 64)), dim3(256), 0, s, g);
        else hipLaunchKernelGGL((gemm_f32_tiled<64, 16, 4>), dim3(cdiv(g.N, 16), cdiv(g.M, 64)), dim3(256), 0, s, g);
    } else {
        hipLaunchKernelGGL((gemm_f32_tiled<128, 128, 4>), dim3(cdiv(g.N, BN), cdiv(g.M, BM)), dim3(256), 0, s, g);
    }
}
