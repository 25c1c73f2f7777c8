// swx_gemm_big.hip -- gemm_f16_big8: the f16 GEMM on a 256 x 256 tile with 8 waves, and nothing else (swx_gemm.hip::swx_gemm_plan_f16 says
// which launches get it; swx_gemm_launch_big8 at the end of the file launches it).
#include <type_traits>
#include "swx_gemm_tile.h"

namespace {

// ------------------------------------------------------------------------------------ tiled f16, 256 x 256 tile, 8 waves
// The large-M shapes (encoder at 20 windows: M = 30 000).  The 128 x 128 tile (swx_gemm_tiled.hip) reads 16 KB of fragments from LDS per wave
// and K step for 32 MFMAs -- 64 KB per workgroup against an LDS port of 128 B/clk: exactly as many LDS cycles as MFMA cycles,
// which is what holds that kernel at 0.29-0.34 of the MFMA peak however it is scheduled.  Here a wave owns 128 x 64 of a
// 256 x 256 tile (8 waves as 2 x 4): 24 fragment reads feed 64 MFMAs, 0.75 LDS cycles per MFMA cycle.  One workgroup per CU
// (two waves per SIMD, 128 accumulator registers each), 128 KB of operand stages filled by the ring kernel's asm LDS-DMA.  Plain
// epilogues only (bias, GELU, f16 residual, f16 rows with 16-byte aligned leading dimensions): the encoder's four projections;
// everything else stays on the 128-row kernels.  Same MFMA order per accumulator: bit-identical results
// (tests/hw_checks/gemm_glds_check.py, gemm_big8_check.py).
constexpr int BG_CLD = BG + 4;                            // f32 epilogue row

// Epilogue of the 256 x 256 kernel: four passes of 64 rows through a f32 tile in LDS, 16-byte row-contiguous stores.
// acc[i][j] = rows wm * 128 + i * 16 + ..., columns wn * 64 + j * 16 + ... of the tile.
// (restates the plain path of swx_gemm_tile.h::tile_epilogue_f16_one for 512 threads and four passes: a fix here belongs there too)
__device__ __forceinline__ void big_tile_epilogue(const GemmArgs &g, unsigned char *ring, f32x4 (&acc)[8][4], int m0, int n0, int tid,
                                                  int lane, int wm, int wn)
{
    float (*Cs)[BG_CLD] = (float (*)[BG_CLD])ring;
    const int col_l = lane & 15, row_l = (lane >> 4) * 4;
    const int c8 = (tid & 31) * 8, rb = tid >> 5, gn = n0 + c8;
    const bool col_ok = gn < g.N, full = gn + 8 <= g.N;
    float bv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) bv[e] = ((g.epi & EPI_BIAS) && gn + e < g.N) ? g.bias[gn + e] : 0.f;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        f16x8 rv[4];
        if (g.epi & EPI_RES) {
#pragma unroll
            for (int it = 0; it < 4; ++it) {
                const int gm = m0 + p * 64 + it * 16 + rb;
                rv[it] = (gm < g.M && full) ? *(const f16x8 *)((const f16 *)g.R + (size_t)gm * g.ldr + gn) : (f16x8)(f16)0;
            }
        }
        if (wm == (p >> 1)) {
#pragma unroll
            for (int ii = 0; ii < 4; ++ii)
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) Cs[ii * 16 + row_l + r][wn * 64 + j * 16 + col_l] = acc[(p & 1) * 4 + ii][j][r];
        }
        __syncthreads();
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int row = it * 16 + rb, gm = m0 + p * 64 + row;
            if (gm >= g.M || !col_ok) continue;
            const f32x4 lo = *(const f32x4 *)&Cs[row][c8], hi = *(const f32x4 *)&Cs[row][c8 + 4];
            float v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] += bv[e];
            if (g.epi & EPI_GELU) {
                gelu_erf_n<8>(v);
            }
            f16 *cp = (f16 *)g.C + (size_t)gm * g.ldc + gn;
            if (full) {
                if (g.epi & EPI_RES) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] += (float)rv[it][e];
                }
                f16x8 o;
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] = (f16)v[e];
                *(f16x8 *)cp = o;
            } else {
                for (int e = 0; e < 8 && gn + e < g.N; ++e) {
                    float t = v[e];
                    if (g.epi & EPI_RES) t += (float)((const f16 *)g.R)[(size_t)gm * g.ldr + gn + e];
                    cp[e] = (f16)t;
                }
            }
        }
        if (p < 3) __syncthreads();
    }
}

// ------------------------------------------------------ tiled f16, 256 x 256 tile, 8 waves, half-tile ring, staggered wave groups
// Generation 1 of this kernel (round 3: two 64 KB K-step stages, one `vmcnt(0)` + barrier per step; deleted in round 4) left the
// MFMA pipe idle twice per K step: its one LDS-DMA stage in flight was issued at the start of the step whose MFMAs (2 048 clocks
// for 64 KB) are shorter than a loaded fabric round trip, and its eight waves read fragments and multiplied in lockstep (1 536
// clocks of LDS reads per step that no MFMA covered).  This generation keeps the tile, the swizzle, the wave -> accumulator map
// and the MFMA order per accumulator (bit-identical results) and changes the schedule (cdna_hip_programming.md, "The 256^2
// 8-phase template").  Measured against generation 1 (profiles/r04_kb_gemm_big8.txt, M = 30 000, TFLOP/s): N = 3840: 962 -> 1 039;
// N = 5120 + GELU: 840 -> 882; K = 5120: 919 -> 1 044; N = 2560: 974 -> 1 035; in the headline pass 562 / 428 / 297 -> 545 / 388 /
// 280 us per launch (profiles/r04_big8_pass_kernels.csv).  Still 0.35 - 0.42 of the MFMA peak: four to five half-tiles in flight
// per CU (16 MB over the chip) cover ~2 us of fabric latency at the 7.8 TB/s of operand traffic 1 000 TFLOP/s needs -- LDS
// capacity (128 of 160 KB), not the schedule, bounds the depth.
//  * the two 64 KB operand buffers are eight HALF-TILE slots (A0 A1 B0 B1 of an even and an odd K tile).  Half h of A = the 64
//    rows each row group of waves multiplies in its phases with that half (tile rows wm * 128 + h * 64 + ..), half h of B = the
//    32 columns of each column group (wn * 64 + h * 32 + ..): a phase needs whole halves, and a slot is refilled as soon as its
//    last fragment read has retired.  Loads are issued in consumption order S_k = A0 B0 B1 A1 of tile k / 4; phase P issues
//    S_(P+7), so four to five half-tiles (64 - 80 KB per CU) are in flight at any time instead of 0 - 64 KB;
//  * a K tile is four phases = the four quadrants of a wave's 8 x 4 accumulators, (A0,B0) (A0,B1) (A1,B1) (A1,B0): 12 / 4 / 8 / 0
//    fragment reads (B0 stays in registers) for 16 MFMAs each.  Phase P of a wave:
//        R_P  fragment reads            W_P  s_waitcnt vmcnt(8): the halves phase P + 1 reads have landed (this wave's part)
//        X_P  barrier                   s_waitcnt lgkmcnt(0)     I_P  issue S_(P+7)          M_P  16 MFMAs          Y_P  barrier
//  * the row groups wm = 0 / 1 (the two waves of every SIMD) run half a phase apart: group 1 passes one extra barrier before
//    its first phase, so its R / W section runs under group 0's MFMAs and the other way round.
// Ordering, by construction (nothing here is "seen to work"): RAW -- a half read in R_(P+1) was retired by EVERY wave's W_P
// before that wave's X_P; a reader passes its Y_P first, which completes only after all waves of the other group called X_P
// (group 0 reads) or X_(P+1) (group 1 reads).  WAR -- I_P rewrites the slot of S_(P-1), whose last fragment reads are in
// R_(P-1) or earlier (A0: R_(P-1); B0, B1, A1: R_(P-2)); every wave retires its reads (lgkmcnt(0)) before its M of the same
// phase, i.e. before its Y_(P-1), and I_P follows X_P, which completes after the other group called Y_(P-1) (group 0 issues) or
// Y_P (group 1 issues).  The last tile's waits count what is really in flight (4, 2, 0).  K >= 128.
constexpr int B8_HALF = 128 * 128;                        // bytes per half-tile: 128 rows x 64 halfs
constexpr int B8_BUF = 4 * B8_HALF;                       // A0 | A1 | B0 | B1 of one K tile

template <int N>
__device__ __forceinline__ void b8_wait_vm()
{
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
__device__ __forceinline__ void b8_barrier()
{
    asm volatile("s_barrier" ::: "memory");
}
__device__ __forceinline__ void b8_wait_lds()
{
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

__global__ __launch_bounds__(512) void gemm_f16_big8(GemmArgs g)
{
    extern __shared__ __attribute__((aligned(1024))) unsigned char ring[];     // 2 x 4 half-tiles = 128 KB; the epilogue's f32 tile after
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    const int wm = wave >> 2, wn = wave & 3;
    const int wm_u = wave_u >> 2;
    int bx = blockIdx.x, by = blockIdx.y;
    {
        // Workgroup `orig` runs on XCD orig % 8 (round-robin dispatch); XCD x takes the contiguous range [start(x), start(x + 1)) of
        // a tile LIST, its k-th workgroup the k-th entry of that range -- so the ~32 tiles an XCD runs at one time are 32 neighbours
        // of the list.  The list is row-major.  At N = 5120 (20 column tiles) those 32 neighbours span every column, i.e. the whole
        // 13.1 MB weight matrix streams through the XCD's 4 MB L2 once per 256-row band (counters, round 5: 1.49 GB per launch for
        // 397 MB algorithmic).  Round 6 built the alternative (tile_order 1, SWX_FLAG_BIG8_GROUPED): GROUPS of 4 column tiles walked
        // along M, the last group taking the remainder -- 32 neighbours = 8 row bands x 4 column bands, the group's weight bands
        // (2.6 MB at K = 1280) resident in L2 for the whole walk.  A pure renumbering, bit-identical
        // (tests/hw_checks/gemm_big8_check.py runs both orders) -- and NOT faster: 458 vs 453 us at N = 5120 + GELU, 384 vs 372 us at
        // K = 5120, 291 vs 284 us at N = 3840 (profiles/r06_c2_kb_gemm_big_tile_order.txt), 427.0 vs 425.5 ms per headline pass.  The
        // re-streamed operands come out of the 256 MB Infinity Cache, whose bandwidth the launch does not exhaust: the extra
        // fabric traffic costs nothing, so the default stays row-major.
        const int gx = gridDim.x, gy = gridDim.y, nwg = gx * gy, orig = by * gx + bx;
        const int xcd = orig & 7, q = nwg >> 3, r = nwg & 7;
        const int wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (orig >> 3);
        if (g.tile_order != 1 || gx <= 4) { bx = wg % gx; by = wg / gx; }
        else {
            constexpr int GN = 4;
            const int nfull = gx / GN, per = GN * gy;            // tiles per full group
            const int grp = wg / per;
            if (grp < nfull) { const int rem = wg - grp * per; by = rem / GN; bx = grp * GN + (rem - by * GN); }
            else { const int gl = gx - nfull * GN, rem = wg - nfull * per; by = rem / gl; bx = nfull * GN + (rem - by * gl); }
        }
    }
    const int m0 = by * BG, n0 = bx * BG;
    const f16 *A = (const f16 *)g.A;
    const f16 *W = (const f16 *)g.W;

    f32x4 acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // a wave stages two 8-row chunks of a half-tile (local rows lr = (wave * 2 + c) * 8 + lane / 8; rows past M / N clamped)
    const f16 *sA[2][2], *sB[2][2];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int lr = (wave * 2 + c) * 8 + (lane >> 3);
            const int slot = (lane & 7) ^ ((lr >> 1) & 7);
            const int ra = (lr >> 6) * 128 + h * 64 + (lr & 63);
            const int rb = (lr >> 5) * 64 + h * 32 + (lr & 31);
            const int gm = m0 + ra < g.M ? m0 + ra : g.M - 1;
            const int gn = n0 + rb < g.N ? n0 + rb : g.N - 1;
            sA[h][c] = A + (size_t)gm * g.lda + slot * 8;
            sB[h][c] = W + (size_t)gn * g.ldw + slot * 8;
        }
    typedef __attribute__((address_space(3))) void lds_void;
    const unsigned ring0 = (unsigned)(uintptr_t)(lds_void *)ring;
    // half-tile `which` (0 A0, 1 B0, 2 B1, 3 A1: the consumption order) of K tile kt into its slot
    auto issue = [&](int kt, auto which_c) {
        constexpr int which = decltype(which_c)::value;
        constexpr bool isA = which == 0 || which == 3;
        constexpr int h = which >= 2 ? 1 : 0;
        constexpr int off = (isA ? 0 : 2 * B8_HALF) + h * B8_HALF;
        const unsigned dst = ring0 + (kt & 1) * B8_BUF + off + wave_u * 2048;
#pragma unroll
        for (int c = 0; c < 2; ++c) glds16_asm((isA ? sA[h][c] : sB[h][c]) + kt * 64, dst + c * 1024);
    };
    using I0 = std::integral_constant<int, 0>; using I1 = std::integral_constant<int, 1>;
    using I2 = std::integral_constant<int, 2>; using I3 = std::integral_constant<int, 3>;

    const int KT = g.K / 64;                              // the launcher guarantees KT >= 2
    const int fr = lane & 15, fs = lane >> 4;
    f16x8 fa[4][2], fb0[2][2], fb1[2][2];                 // [fragment][kk]: the current A half, B0, B1
    auto read_a = [&](int buf, int h) {
        const unsigned char *t = ring + buf * B8_BUF + h * B8_HALF;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int lr = wm * 64 + i * 16 + fr;
                fa[i][kk] = *(const f16x8 *)(t + lr * 128 + (((kk * 4 + fs) ^ ((lr >> 1) & 7)) << 4));
            }
    };
    auto read_b = [&](int buf, int h, f16x8 (&fb)[2][2]) {
        const unsigned char *t = ring + buf * B8_BUF + 2 * B8_HALF + h * B8_HALF;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int lr = wn * 32 + j * 16 + fr;
                fb[j][kk] = *(const f16x8 *)(t + lr * 128 + (((kk * 4 + fs) ^ ((lr >> 1) & 7)) << 4));
            }
    };
    // 16 MFMAs of quadrant (ih, jh); per accumulator kk = 0 then 1, K tiles ascending: the order of every tiled f16 kernel
    auto quad = [&](auto ih_c, auto jh_c, const f16x8 (&fb)[2][2]) {
        constexpr int ih = decltype(ih_c)::value, jh = decltype(jh_c)::value;
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[ih * 4 + i][jh * 2 + j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[i][kk], fb[j][kk], acc[ih * 4 + i][jh * 2 + j], 0, 0, 0);
        __builtin_amdgcn_s_setprio(0);
    };
    // MODE 0: a tile with at least two tiles after it; 1: the second-last tile; 2: the last tile
    auto tile = [&](auto mode_c, int t) {
        constexpr int MODE = decltype(mode_c)::value;
        const int buf = t & 1;
        // phase 1: (A0, B0)
        read_a(buf, 0);
        read_b(buf, 0, fb0);
        b8_wait_vm<MODE == 2 ? 2 : 8>();                  // B1 of this tile
        b8_barrier();
        b8_wait_lds();
        if (MODE < 2) issue(t + 1, I3());                 // A1 of tile t + 1 (slot last read in phase 3 of tile t - 1)
        quad(I0(), I0(), fb0);
        b8_barrier();
        // phase 2: (A0, B1)
        read_b(buf, 1, fb1);
        b8_wait_vm<MODE == 2 ? 0 : 8>();                  // A1 of this tile
        b8_barrier();
        b8_wait_lds();
        if (MODE == 0) issue(t + 2, I0());                // A0 of tile t + 2 (slot last read in phase 1 of this tile)
        quad(I0(), I1(), fb1);
        b8_barrier();
        // phase 3: (A1, B1)
        read_a(buf, 1);
        b8_barrier();
        b8_wait_lds();
        if (MODE == 0) issue(t + 2, I1());                // B0 of tile t + 2 (slot last read in phase 1 of this tile)
        quad(I1(), I1(), fb1);
        b8_barrier();
        // phase 4: (A1, B0)
        if (MODE == 0) b8_wait_vm<8>();                   // A0, B0 of tile t + 1
        if (MODE == 1) b8_wait_vm<4>();
        b8_barrier();
        if (MODE == 0) issue(t + 2, I2());                // B1 of tile t + 2 (slot last read in phase 2 of this tile)
        quad(I1(), I0(), fb0);
        b8_barrier();
    };

    issue(0, I0()); issue(0, I1()); issue(0, I2()); issue(0, I3());
    issue(1, I0()); issue(1, I1()); issue(1, I2());
    b8_wait_vm<10>();                                     // A0, B0 of tile 0
    b8_barrier();
    if (wm_u == 1) b8_barrier();                          // row group 1 runs half a phase behind
    int t = 0;
    for (; t < KT - 2; ++t) tile(I0(), t);
    tile(I1(), t);
    tile(I2(), t + 1);
    if (wm_u == 0) b8_barrier();                          // pairs with row group 1's last barrier: every wave is done with the ring
    big_tile_epilogue(g, ring, acc, m0, n0, tid, lane, wm, wn);
}

}  // namespace

// 2 * B8_BUF = 128 KB of dynamic LDS: above the 64 KB a launch gets unasked, so through the grant
int swx_gemm_launch_big8(const GemmArgs &g, hipStream_t s)
{
    GemmArgs gb = g;
    gb.tile_order = (swx_flags() & SWX_FLAG_BIG8_GROUPED) ? 1 : 0;
    return swx_launch_lds<gemm_f16_big8>(dim3(cdiv(g.N, BG), cdiv(g.M, BG)), dim3(512), 2 * B8_BUF, 2 * B8_BUF, s, gb);
}
