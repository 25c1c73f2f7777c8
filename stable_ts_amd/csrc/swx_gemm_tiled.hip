// swx_gemm_tiled.hip -- the f16 GEMM kernels on the 128-row tile (4 waves as 2 x 2, 4 x NJ v_mfma_f32_16x16x32_f16 per wave and 32 of K):
// gemm_f16_tiled (register-staged, the bit-identity reference), gemm_f16_glds_128 / _64 (LDS-DMA, occupancy overlap) and
// gemm_f16_ring<64|128, 3> (LDS-DMA ring for launches of at most one workgroup per CU).  One epilogue: swx_gemm_tile.h::tile_epilogue_f16.
// swx_gemm.hip::swx_gemm_plan_f16 says which launch gets which; swx_gemm_launch_tiled at the end of the file launches them.
#include "swx_gemm_tile.h"

namespace {

// ------------------------------------------------------------------------------------------------ tiled f16
__global__ __launch_bounds__(256) void gemm_f16_tiled(GemmArgs g)
{
    // one allocation: [A tiles | B tiles] during the K loop, reused as the f32 C tile of the coalesced epilogue
    __shared__ __attribute__((aligned(16))) unsigned char smem[2 * 2 * BM * LD16 * 2];
    f16 (*As)[BM][LD16] = (f16 (*)[BM][LD16])smem;
    f16 (*Bs)[BN][LD16] = (f16 (*)[BN][LD16])(smem + 2 * BM * LD16 * 2);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
    const f16 *A = (const f16 *)g.A;
    const f16 *W = (const f16 *)g.W;

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    f16x8 ra[4], rb[4];
    auto load_regs = [&](int k0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = tid + 256 * i, row = c >> 3, kc = (c & 7) * 8;
            const int gm = m0 + row, gn = n0 + row;
            const bool kok = k0 + kc < g.K;          // K may end in the middle of a 64-wide step (K % 32 == 0)
            // predicated loads here: the clamped-address form measured 10-15 % slower on this kernel (profiles r01 v5)
            ra[i] = (gm < g.M && kok) ? *(const f16x8 *)(A + (size_t)gm * g.lda + k0 + kc) : (f16x8)(f16)0;
            rb[i] = (gn < g.N && kok) ? *(const f16x8 *)(W + (size_t)gn * g.ldw + k0 + kc) : (f16x8)(f16)0;
        }
    };
    auto store_lds = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = tid + 256 * i, row = c >> 3, kc = (c & 7) * 8;
            *(f16x8 *)&As[buf][row][kc] = ra[i];
            *(f16x8 *)&Bs[buf][row][kc] = rb[i];
        }
    };

    const int KT = (g.K + BK16 - 1) / BK16;
    load_regs(0);
    store_lds(0);
    __syncthreads();
    for (int kt = 0; kt < KT; ++kt) {
        const int cur = kt & 1;
        if (kt + 1 < KT) load_regs((kt + 1) * BK16);
        const int fr = lane & 15, fk = (lane >> 4) * 8;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            f16x8 a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = *(const f16x8 *)&As[cur][wm * 64 + i * 16 + fr][kk * 32 + fk];
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = *(const f16x8 *)&Bs[cur][wn * 64 + j * 16 + fr][kk * 32 + fk];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        if (kt + 1 < KT) store_lds(cur ^ 1);
        __syncthreads();
    }

    tile_epilogue_f16<4>(g, smem, acc, m0, n0, tid, lane, wm, wn);
}

// ------------------------------------------------------------------------------------- tiled f16, direct-to-LDS
// Same 128 x 128 x 64 tile and 4 x 4 accumulator grid per wave as gemm_f16_tiled, but the operand tiles go
// global -> LDS with `global_load_lds` (16 bytes per lane, 1 KiB per wave instruction): no staging VGPRs and no
// ds_write pass, which is what bounds the register-staged kernel (8 ds_write_b128 per thread and K tile at ~79 B/clk/CU
// are as many LDS cycles as the tile's MFMAs; cdna_hip_programming.md section 5, ladder step 2 -> 3).
// LDS image: a wave instruction writes base + lane * 16, i.e. 8 consecutive 128-byte tile rows; rows are NOT padded.
// Bank conflicts of the fragment reads (16 lanes = 16 tile rows at one 16-byte column slot) are removed by an XOR swizzle
// of the slot with (row >> 1) & 7, applied on the SOURCE address of the load (the LDS destination is fixed by the
// hardware) and on the read address.  Blocks are renumbered so that each XCD (private L2) works on neighbouring tiles.
// Requires K % 64 == 0; rows past M / N are clamped to the last valid row (their results are never stored).
//
// Generation 2 (round 2).  What the K = 1280 shapes of the encoder showed for the first kernel (double buffered, one barrier
// per K step, 67.6 KB of f32 epilogue staging -> two workgroups per CU; profiles/r02_kb_gemm_glds.txt): time = 103 us per
// 1280 of K + 79 us that do not depend on K -- at M = 30000, N = 1280 the fixed part was 43 % of the launch: the epilogue's
// dependent bias / residual loads (see tile_epilogue_f16), with only one other workgroup on the CU to hide them.
// Now: one operand buffer, two barriers per K step, 33.8 KB of LDS -> three workgroups per CU: the occupancy, not a software
// pipeline, overlaps one workgroup's loads and epilogue with its neighbours' MFMAs.  Measured at M = 30000
// (profiles/r02_kb_gemm_gen2.txt, TFLOP/s, first kernel -> double buffer, 2 per CU -> single buffer, 4 per CU -> single buffer,
// 3 per CU = this kernel): N = K = 1280: 522 -> 737 -> 783 -> 768; N = 3840: 536 -> 704 -> 754 -> 737; N = 5120: 523 -> 748 ->
// 809 -> 788; K = 5120: 715 -> 783 -> 816 -> 854.  The variants that lost were deleted in round 3.  Bit-identical to the
// register-staged kernel (same MFMA order per accumulator, same f32 epilogue arithmetic; tests/hw_checks/gemm_glds_check.py).
template <int BNT>     // BNT = tile width: 128, or 64 for shapes whose 128-wide tiles would not fill the chip
__device__ __forceinline__ void gemm_f16_glds_body(const GemmArgs &g)
{
    constexpr int NJ = BNT / 32;                       // 16-column fragments per wave (2 x 2 waves: 64 rows x BNT / 2 columns each)
    constexpr int TB = BNT * 128;                      // bytes of the B operand tile (BNT rows x 64 halfs)
    constexpr int STAGE = GL_TILE + TB;
    constexpr int MAIN = STAGE;
    constexpr int EPI_ = 64 * (BNT + 4) * 4;
    __shared__ __attribute__((aligned(1024))) unsigned char smem[MAIN > EPI_ ? MAIN : EPI_];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    int bx = blockIdx.x, by = blockIdx.y;
    {
        const int gx = gridDim.x, nwg = gx * gridDim.y, orig = by * gx + bx;
        const int xcd = orig & 7, q = nwg >> 3, r = nwg & 7;
        const int wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (orig >> 3);
        bx = wg % gx; by = wg / gx;
    }
    const int m0 = by * BM, n0 = bx * BNT;
    const f16 *A = (const f16 *)g.A;
    const f16 *W = (const f16 *)g.W;

    f32x4 acc[4][NJ];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // per-lane source rows of the 8-row chunks this wave stages: four of A, NJ of W (chunk = wave * n + c)
    const f16 *srcA[4], *srcW[NJ];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int r = (wave * 4 + c) * 8 + (lane >> 3);
        const int slot = (lane & 7) ^ ((r >> 1) & 7);
        const int gm = m0 + r < g.M ? m0 + r : g.M - 1;
        srcA[c] = A + (size_t)gm * g.lda + slot * 8;
    }
#pragma unroll
    for (int c = 0; c < NJ; ++c) {
        const int r = (wave * NJ + c) * 8 + (lane >> 3);
        const int slot = (lane & 7) ^ ((r >> 1) & 7);
        const int gn = n0 + r < g.N ? n0 + r : g.N - 1;
        srcW[c] = W + (size_t)gn * g.ldw + slot * 8;
    }
    typedef __attribute__((address_space(3))) void lds_void;
    auto stage = [&](int kt, int buf) {
        unsigned char *ta = smem + buf * STAGE, *tb = ta + GL_TILE;
#pragma unroll
        for (int c = 0; c < 4; ++c)
            __builtin_amdgcn_global_load_lds(srcA[c] + kt * 64, (lds_void *)(ta + (wave * 4 + c) * 1024), 16, 0, 0);
#pragma unroll
        for (int c = 0; c < NJ; ++c)
            __builtin_amdgcn_global_load_lds(srcW[c] + kt * 64, (lds_void *)(tb + (wave * NJ + c) * 1024), 16, 0, 0);
    };
    const int KT = g.K / 64;
    const int fr = lane & 15, fs = lane >> 4;
    auto compute = [&](int buf) {
        const unsigned char *ta = smem + buf * STAGE, *tb = ta + GL_TILE;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            f16x8 a[4], b[NJ];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = wm * 64 + i * 16 + fr;
                a[i] = *(const f16x8 *)(ta + row * 128 + (((kk * 4 + fs) ^ ((row >> 1) & 7)) << 4));
            }
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int row = wn * (BNT / 2) + j * 16 + fr;
                b[j] = *(const f16x8 *)(tb + row * 128 + (((kk * 4 + fs) ^ ((row >> 1) & 7)) << 4));
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < NJ; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[i], b[j], acc[i][j], 0, 0, 0);
        }
    };
    for (int kt = 0; kt < KT; ++kt) {       // one operand buffer, two barriers per K step: three workgroups per CU overlap each other
        stage(kt, 0);
        __syncthreads();
        compute(0);
        __syncthreads();
    }
    tile_epilogue_f16<NJ>(g, smem, acc, m0, n0, tid, lane, wm, wn);
}

// the instantiations in use (second launch bound = workgroups per CU the register allocation must allow)
__global__ __launch_bounds__(256, 3) void gemm_f16_glds_128(GemmArgs g) { gemm_f16_glds_body<128>(g); }
__global__ __launch_bounds__(256, 3) void gemm_f16_glds_64(GemmArgs g) { gemm_f16_glds_body<64>(g); }

// ------------------------------------------------------------------------------- tiled f16, direct-to-LDS ring
// The kernel above hides a K step's memory round trip behind the OTHER workgroups of its CU (three resident).  Shapes with
// fewer than ~two tiles per CU have nobody to hide behind -- the encoder at batch 1 (align(): M = 1500; N = 1280 is 240 tiles
// of 128 x 64) runs stage -> wait -> compute serially, ~0.9 us per K step for 0.1-0.2 us of MFMAs: 18.6 us at K = 1280,
// 65.8 us at K = 5120 (profiles/r02_kb_gemm_narrow_tiles.txt).  Here ONE workgroup keeps NST - 1 K steps in flight: a ring
// of NST = 3 operand stages in LDS (72 / 96 KB), filled by LDS-DMA issued from inline asm (swx_gemm_tile.h::glds16_asm: a DMA hipcc can see
// makes it wait vmcnt(0) before the next LDS read and inside __syncthreads(); cdna_hip_programming.md "glds with >1 tile in flight"), retired by counted
// `s_waitcnt vmcnt(n)` + a raw `s_barrier`.  Per K step: [wait until stage kt has landed for this wave (the NST - 2 younger
// stages stay in flight) and this wave's LDS reads of step kt - 1 are back] -> barrier (now true for every wave) -> refill
// the stage step kt - 1 used -> MFMAs of step kt.  A DMA's data is read one barrier after the wait that retires it, a stage
// is rewritten one barrier after its last read returned.  Same tile, swizzle, MFMA order per accumulator and epilogue as
// the kernel above: bit-identical results (tests/hw_checks/gemm_glds_check.py).
template <int N>
__device__ __forceinline__ void ring_wait_barrier()
{
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(N) : "memory");
}

template <int BNT, int NST>
__device__ __forceinline__ void gemm_f16_ring_body(const GemmArgs &g)
{
    constexpr int NJ = BNT / 32;
    constexpr int TB = BNT * 128;
    constexpr int STAGE = GL_TILE + TB;
    constexpr int L = 4 + NJ;                            // DMA instructions per wave and stage
    static_assert(NST == 3 || NST == 4, "ring depth");      // depth 4 measured no better than 3 anywhere and was not kept
    static_assert((NST - 2) * L < 64, "vmcnt is a 6-bit field");
    extern __shared__ __attribute__((aligned(1024))) unsigned char ring[];     // NST stages; the f32 epilogue tile afterwards
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    const int wm = wave >> 1, wn = wave & 1;
    int bx = blockIdx.x, by = blockIdx.y;
    {
        const int gx = gridDim.x, nwg = gx * gridDim.y, orig = by * gx + bx;
        const int xcd = orig & 7, q = nwg >> 3, r = nwg & 7;
        const int wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (orig >> 3);
        bx = wg % gx; by = wg / gx;
    }
    const int m0 = by * BM, n0 = bx * BNT;
    const f16 *A = (const f16 *)g.A;
    const f16 *W = (const f16 *)g.W;

    f32x4 acc[4][NJ];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const f16 *srcA[4], *srcW[NJ];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int r = (wave * 4 + c) * 8 + (lane >> 3);
        const int slot = (lane & 7) ^ ((r >> 1) & 7);
        const int gm = m0 + r < g.M ? m0 + r : g.M - 1;
        srcA[c] = A + (size_t)gm * g.lda + slot * 8;
    }
#pragma unroll
    for (int c = 0; c < NJ; ++c) {
        const int r = (wave * NJ + c) * 8 + (lane >> 3);
        const int slot = (lane & 7) ^ ((r >> 1) & 7);
        const int gn = n0 + r < g.N ? n0 + r : g.N - 1;
        srcW[c] = W + (size_t)gn * g.ldw + slot * 8;
    }
    typedef __attribute__((address_space(3))) void lds_void;
    const unsigned ring0 = (unsigned)(uintptr_t)(lds_void *)ring;
    auto stage = [&](int kt, int buf) {
        const unsigned ta = ring0 + buf * STAGE, tb = ta + GL_TILE;
#pragma unroll
        for (int c = 0; c < 4; ++c) glds16_asm(srcA[c] + kt * 64, ta + (wave_u * 4 + c) * 1024);
#pragma unroll
        for (int c = 0; c < NJ; ++c) glds16_asm(srcW[c] + kt * 64, tb + (wave_u * NJ + c) * 1024);
    };
    const int KT = g.K / 64;                             // the launcher guarantees KT >= NST - 1
    const int fr = lane & 15, fs = lane >> 4;
    auto compute = [&](int buf) {
        const unsigned char *ta = ring + buf * STAGE, *tb = ta + GL_TILE;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            f16x8 a[4], b[NJ];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = wm * 64 + i * 16 + fr;
                a[i] = *(const f16x8 *)(ta + row * 128 + (((kk * 4 + fs) ^ ((row >> 1) & 7)) << 4));
            }
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int row = wn * (BNT / 2) + j * 16 + fr;
                b[j] = *(const f16x8 *)(tb + row * 128 + (((kk * 4 + fs) ^ ((row >> 1) & 7)) << 4));
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < NJ; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[i], b[j], acc[i][j], 0, 0, 0);
        }
    };
#pragma unroll
    for (int st = 0; st < NST - 1; ++st) stage(st, st);
    int buf = 0, nbuf = NST - 1;                         // stage of step kt, stage the next refill goes to
    for (int kt = 0; kt < KT; ++kt) {
        const int ahead = KT - 1 - kt;                   // K steps after this one: min(ahead, NST - 2) stages may stay in flight
        if (ahead >= NST - 2) ring_wait_barrier<(NST - 2) * L>();
        else if (NST == 4 && ahead == 1) ring_wait_barrier<L>();
        else ring_wait_barrier<0>();
        if (kt + NST - 1 < KT) stage(kt + NST - 1, nbuf);
        compute(buf);
        buf = buf + 1 == NST ? 0 : buf + 1;
        nbuf = nbuf + 1 == NST ? 0 : nbuf + 1;
    }
    __syncthreads();                                     // every wave is done with the ring: it becomes the epilogue's f32 tile
    tile_epilogue_f16<NJ>(g, ring, acc, m0, n0, tid, lane, wm, wn);
}

template <int BNT, int NST>
__global__ __launch_bounds__(256) void gemm_f16_ring(GemmArgs g) { gemm_f16_ring_body<BNT, NST>(g); }

// 72 KB (BNT = 64) / 96 KB (BNT = 128) of dynamic LDS: above the 64 KB a launch gets unasked, so through the grant
template <int BNT, int NST>
static int launch_ring(const GemmArgs &g, hipStream_t s)
{
    constexpr int stage_bytes = GL_TILE + BNT * 128, epi_bytes = 64 * (BNT + 4) * 4;
    constexpr int lds = NST * stage_bytes > epi_bytes ? NST * stage_bytes : epi_bytes;
    return swx_launch_lds<gemm_f16_ring<BNT, NST>>(dim3(cdiv(g.N, BNT), cdiv(g.M, BM)), dim3(256), lds, lds, s, g);
}

}  // namespace

int swx_gemm_launch_tiled(int plan, const GemmArgs &g, hipStream_t s)
{
    const dim3 grid(cdiv(g.N, BN), cdiv(g.M, BM));
    switch (plan) {
        case SWX_GEMM_RING64: return launch_ring<64, 3>(g, s);
        case SWX_GEMM_RING128: return launch_ring<128, 3>(g, s);
        case SWX_GEMM_GLDS64: hipLaunchKernelGGL(gemm_f16_glds_64, dim3(cdiv(g.N, 64), grid.y), dim3(256), 0, s, g); break;
        case SWX_GEMM_GLDS128: hipLaunchKernelGGL(gemm_f16_glds_128, grid, dim3(256), 0, s, g); break;
        default: hipLaunchKernelGGL(gemm_f16_tiled, grid, dim3(256), 0, s, g); break;
    }
    return 0;
}
