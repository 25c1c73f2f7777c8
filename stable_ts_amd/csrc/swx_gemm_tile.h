// swx_gemm_tile.h -- what more than one kernel family of swx_gemm*.hip uses: the tile constants, the element-wise epilogue, the tile
// epilogue of the 128-row f16 kernels with its layout maps, the asm LDS-DMA, and the launch functions swx_gemm.hip dispatches to.
// Private to those files; everything device-side sits in an anonymous namespace like the kernels that inline it.
#pragma once
#include "swx_common.h"
#include "swx_kernels.h"

// One launch function per family file: grid arithmetic and LDS grant live with the kernel.  0, or -100 - the error of a refused
// dynamic-LDS grant (swx_common.h::swx_launch_lds); launch errors are swx_gemm's SWX_CHECK_LAUNCH.  Internal to libswx.so.
#define SWX_GEMM_LOCAL __attribute__((visibility("hidden")))
SWX_GEMM_LOCAL int swx_gemm_launch_tiled(int plan, const GemmArgs &g, hipStream_t s);       // swx_gemm_tiled.hip: every SWX_GEMM_* plan but SKINNY and BIG
SWX_GEMM_LOCAL int swx_gemm_launch_big8(const GemmArgs &g, hipStream_t s);                  // swx_gemm_big.hip
SWX_GEMM_LOCAL void swx_gemm_launch_f32(const GemmArgs &g, int force_kernel, hipStream_t s);    // swx_gemm_f32.hip (no dynamic LDS: nothing to refuse)

constexpr int BM = 128, BN = 128;           // tile of the 128 x 128 kernels (f16 and f32)
constexpr int BK16 = 64, LD16 = BK16 + 8;   // halfs; 144-byte rows keep every fragment read 16-byte aligned
constexpr int GL_TILE = 128 * 128;          // bytes of one LDS-DMA operand tile: 128 rows x 64 halfs
constexpr int BG = 256;                     // tile edge of the 256 x 256 kernel

namespace {

template <typename T>
__device__ __forceinline__ void epilogue_store(const GemmArgs &g, int row, int col, float v)
{
    if (row >= g.M || col >= g.N) return;
    if (g.epi & EPI_BIAS) v += g.bias[col];
    if (g.epi & EPI_GELU) v = gelu_erf(v);
    if (g.epi & EPI_RESF32MOD) v += g.Rf[(size_t)(row % g.res_mod) * g.N + col];
    if (g.epi & EPI_RES) v += to_f32<T>(((const T *)g.R)[(size_t)row * g.ldr + col]);
    if (g.epi & EPI_STORE_VT) {
        const int w = row / g.vt_s, sidx = row - w * g.vt_s;
        ((T *)g.C)[(size_t)w * g.vt_bs + (size_t)col * g.vt_kp + sidx] = from_f32<T>(v);   // col = h*64 + dd
    } else if (g.epi & EPI_CBATCH) {
        const int w = row / g.vt_s, sidx = row - w * g.vt_s;
        ((T *)g.C)[(size_t)w * g.vt_bs + (size_t)sidx * g.ldc + col] = from_f32<T>(v);
    } else if (g.epi & EPI_OUT_F32) ((float *)g.C)[(size_t)row * g.ldc + col] = v;
    else ((T *)g.C)[(size_t)row * g.ldc + col] = from_f32<T>(v);
}

// LDS-DMA of 16 bytes per lane from inline asm (gemm_f16_ring, gemm_f16_big8): a DMA hipcc can see makes it wait vmcnt(0) before the
// next LDS read and inside __syncthreads(), so kernels with more than one tile in flight issue it here and retire it by counted waits
__device__ __forceinline__ void glds16_asm(const void *gsrc, unsigned lds_dst)
{
    unsigned keep;     // M0 is the DMA's LDS base and belongs to hipcc: saved and restored inside the statement
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}

// EPI_KV with GemmArgs::P (round 6): the decode-step cross-attention's fragment-ordered copy (swx_xattn.hip::xkv_pack_kernel's index maps)
// written from the projection's epilogue.  K: the 16-byte piece (key, head, dims 8 c .. 8 c + 7) is lane (g = c & 3, qn) of fragment 2 t + (c >> 2)
// of the key's 32-key block, key % 32 = (qn >> 2) * 8 + 4 t + (qn & 3).  V^T: the 8-byte piece (4 keys from key0 = a multiple of 4, head, dim) is
// half (key0 % 8) / 4 of lane (g = (key0 % 32) / 8, qn = dim % 16) of fragment dim / 16.  Keys [vt_s, p_nkpad) of a head are zeros.
__device__ __forceinline__ f16 *xkv_packed_k_piece(const GemmArgs &g, int wb, int key, int col)
{
    const int h = col >> 6, c = (col & 63) >> 3, kq = key & 31;
    const int frag = (((kq >> 2) & 1) << 1) + (c >> 2), lane_ = (c & 3) * 16 + (kq >> 3) * 4 + (kq & 3);
    return (f16 *)g.P + (size_t)wb * g.p_bs + (size_t)h * swx_xkv_packed_elems_per_head(g.vt_s) + ((size_t)(key >> 5) * 4 + frag) * 512 + lane_ * 8;
}
__device__ __forceinline__ f16 *xkv_packed_v_piece(const GemmArgs &g, int wb, int key0, int vcol)
{
    const int h = vcol >> 6, dd = vcol & 63, kq = key0 & 31;
    const int64_t per_head = swx_xkv_packed_elems_per_head(g.vt_s);
    return (f16 *)g.P + (size_t)wb * g.p_bs + (size_t)h * per_head + per_head / 2 + ((size_t)(key0 >> 5) * 4 + (dd >> 4)) * 512 +
           ((kq >> 3) * 16 + (dd & 15)) * 8 + ((kq & 7) >> 2) * 4;
}

// Shared tile epilogue of the 128-row f16 kernels (gemm_f16_tiled, gemm_f16_glds, gemm_f16_ring): special layouts element-wise,
// otherwise accumulators -> f32 tile in LDS
// (two halves of 64 rows, 33.8 KB) -> 16-byte row-contiguous stores with bias / GELU / residual in f32.  The bias (the same
// 8 columns for every row group of a thread) and the residual rows of a half are requested BEFORE the accumulators are
// staged: loaded per row group after the previous group's store (a store through a f16 pointer may alias the f32 bias, so
// hipcc keeps the order) they were eight dependent L2 round trips per tile -- 43 % of a K = 1280 launch (swx_gemm_tiled.hip,
// gemm_f16_glds).
template <int NJ>      // NJ 16-column fragments per wave: tile width BNT = 32 NJ (128 or 64 columns)
__device__ __forceinline__ void tile_epilogue_f16_one(const GemmArgs &g, unsigned char *smem, f32x4 (&acc)[4][NJ], int m0, int n0,
                                                         int tid, int lane, int wm, int wn)
{
    constexpr int BNT = 32 * NJ, WN = 16 * NJ;        // tile width, columns per wave
    constexpr int CLD_ = BNT + 4;
    const int col_l = lane & 15, row_l = (lane >> 4) * 4;
    // EPI_STORE_VT (the cross-attention V, stored transposed per head: element (row, col) at [col][row within the window]):
    // through LDS like the plain path, but read back COLUMN-wise -- a thread takes 4 consecutive rows of one column (8 bytes in
    // the transposed layout; window boundaries and M are multiples of 4), 16 lanes cover 64 consecutive rows of a column
    // (128 contiguous bytes).  The element-wise path (a 2-byte store, a bias load and an integer division per element) cost
    // 61-83 us against 30 us for the same shape with a plain epilogue.
    if ((g.epi & EPI_STORE_VT) && !(g.epi & (EPI_RES | EPI_GELU | EPI_OUT_F32 | EPI_RESF32MOD | EPI_CBATCH)) && g.vt_s % 4 == 0 &&
        g.vt_kp % 4 == 0 && g.vt_bs % 4 == 0 && g.M % 4 == 0) {
        constexpr int CLV = BNT + 1;                         // odd pitch: the column-wise read-back is 2-way conflicted at worst
        float (*Cv)[CLV] = (float (*)[CLV])smem;            // 64 x 129 x 4 B = 33.0 KB per half
        const int rg = tid & 15, cq = tid >> 4;
        constexpr int NKV = BNT / 16;
        float bvt[NKV];                                      // this thread's columns: requested before any store
#pragma unroll
        for (int k = 0; k < NKV; ++k) bvt[k] = ((g.epi & EPI_BIAS) && n0 + cq + 16 * k < g.N) ? g.bias[n0 + cq + 16 * k] : 0.f;
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            if (wm == half) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < NJ; ++j)
#pragma unroll
                        for (int r = 0; r < 4; ++r) Cv[i * 16 + row_l + r][wn * WN + j * 16 + col_l] = acc[i][j][r];
            }
            __syncthreads();
            const int gm = m0 + half * 64 + rg * 4;
            if (gm < g.M) {
                const int wb = gm / g.vt_s, sidx = gm - wb * g.vt_s;
                f16 *cbase = (f16 *)g.C + (size_t)wb * g.vt_bs + sidx;
#pragma unroll
                for (int k = 0; k < NKV; ++k) {
                    const int col = cq + 16 * k, gn = n0 + col;
                    if (gn >= g.N) continue;
                    const float b = bvt[k];
                    f16x4 o;
#pragma unroll
                    for (int r = 0; r < 4; ++r) o[r] = (f16)(Cv[rg * 4 + r][col] + b);
                    *(f16x4 *)(cbase + (size_t)gn * g.vt_kp) = o;
                    if (g.P) {                                          // ... and the fragment-ordered copy (with its zeroed key padding)
                        *(f16x4 *)xkv_packed_v_piece(g, wb, sidx, gn - g.p_vcol0) = o;
                        if (sidx + 4 == g.vt_s) {
                            const f16x4 z = {(f16)0.f, (f16)0.f, (f16)0.f, (f16)0.f};
                            for (int kz = g.vt_s; kz < g.p_nkpad; kz += 4) *(f16x4 *)xkv_packed_v_piece(g, wb, kz, gn - g.p_vcol0) = z;
                        }
                    }
                    if (g.vt_zero_pad && sidx + 4 == g.vt_s) {          // the row group that ends a batch item: its columns' key padding
                        const f16x4 z = {(f16)0.f, (f16)0.f, (f16)0.f, (f16)0.f};
                        for (int zp = 4; sidx + zp < g.vt_kp; zp += 4) *(f16x4 *)(cbase + (size_t)gn * g.vt_kp + zp) = z;
                    }
                }
            }
            if (half == 0) __syncthreads();
        }
        return;
    }
    // EPI_CBATCH (rows scattered per batch item: the cross-attention K of every window behind one GEMM) keeps rows contiguous,
    // so it takes the coalesced path with a per-row base; the element-wise path cost 55-98 us against 30 us for the same
    // shape with a plain epilogue (M = 1500, N = K = 1280)
    const bool plain = !(g.epi & (EPI_STORE_VT | EPI_OUT_F32 | EPI_RESF32MOD)) && (g.ldc % 8 == 0) &&
                       (!(g.epi & EPI_RES) || g.ldr % 8 == 0) &&
                       (!(g.epi & EPI_CBATCH) || (g.vt_bs % 8 == 0 && !(g.epi & EPI_RES)));
    if (!plain) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    epilogue_store<f16>(g, m0 + wm * 64 + i * 16 + row_l + r, n0 + wn * WN + j * 16 + col_l, acc[i][j][r]);
        return;
    }
    // (swx_gemm_big.hip::big_tile_epilogue restates the rest of this function for the 256-wide tile: a fix here belongs there too)
    float (*Cs)[CLD_] = (float (*)[CLD_])smem;          // 64 x 132 x 4 B = 33.8 KB per half (BNT = 128)
    constexpr int TPR = BNT / 8, RPI = 256 / TPR, NIT = 64 / RPI;    // threads per row, rows per iteration, iterations per half
    const int c8 = (tid % TPR) * 8, rb = tid / TPR, gn = n0 + c8;
    const bool col_ok = gn < g.N, full = gn + 8 <= g.N;
    float bv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) bv[e] = ((g.epi & EPI_BIAS) && gn + e < g.N) ? g.bias[gn + e] : 0.f;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        f16x8 rv[NIT];
        if (g.epi & EPI_RES) {
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const int gm = m0 + half * 64 + it * RPI + rb;
                rv[it] = (gm < g.M && full) ? *(const f16x8 *)((const f16 *)g.R + (size_t)gm * g.ldr + gn) : (f16x8)(f16)0;
            }
        }
        if (wm == half) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < NJ; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) Cs[i * 16 + row_l + r][wn * WN + j * 16 + col_l] = acc[i][j][r];
        }
        __syncthreads();
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int row = it * RPI + rb, gm = m0 + half * 64 + row;
            if (gm >= g.M || !col_ok) continue;
            const f32x4 lo = *(const f32x4 *)&Cs[row][c8], hi = *(const f32x4 *)&Cs[row][c8 + 4];
            float v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] += bv[e];
            if (g.epi & EPI_GELU) {
                gelu_erf_n<8>(v);
            }
            f16 *cp = (f16 *)g.C + (size_t)gm * g.ldc + gn;
            if (g.epi & EPI_CBATCH) {
                const int wb = gm / g.vt_s;
                cp = (f16 *)g.C + (size_t)wb * g.vt_bs + (size_t)(gm - wb * g.vt_s) * g.ldc + gn;
            }
            if (full) {
                if (g.epi & EPI_RES) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] += (float)rv[it][e];
                }
                f16x8 o;
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] = (f16)v[e];
                *(f16x8 *)cp = o;
                if (g.P && (g.epi & EPI_CBATCH)) {                      // K of the cross-attention: ... and the fragment-ordered copy
                    const int wb = gm / g.vt_s, key = gm - wb * g.vt_s;
                    *(f16x8 *)xkv_packed_k_piece(g, wb, key, gn) = o;
                    if (key + 1 == g.vt_s)
                        for (int kz = g.vt_s; kz < g.p_nkpad; ++kz) *(f16x8 *)xkv_packed_k_piece(g, wb, kz, gn) = (f16x8)(f16)0;
                }
            } else {
                for (int e = 0; e < 8 && gn + e < g.N; ++e) {
                    float t = v[e];
                    if (g.epi & EPI_RES) t += (float)((const f16 *)g.R)[(size_t)gm * g.ldr + gn + e];
                    cp[e] = (f16)t;
                }
            }
        }
        if (half == 0) __syncthreads();
    }
}

// EPI_KV (round 6): the K and the V projection of a decoder layer's cross-attention as ONE launch over the fused weight rows -- a
// tile left of N / 2 takes the K epilogue (rows grouped per window), a tile right of it the V epilogue (transposed per head into
// C2, columns counted from N / 2).  Workgroup-uniform; per element the arithmetic of the two separate launches.
template <int NJ>
__device__ __forceinline__ void tile_epilogue_f16(const GemmArgs &g, unsigned char *smem, f32x4 (&acc)[4][NJ], int m0, int n0,
                                                     int tid, int lane, int wm, int wn)
{
    if (g.epi & EPI_QKV_VT) {
        // the encoder's fused Q | K | V projection: V (the last third of the columns; the third is a multiple of the tile width)
        // leaves transposed per head -- what swx_transpose_v did in a launch of its own; per element the plain epilogue's value
        GemmArgs h = g;
        const int split = (g.N / 3) * 2;
        h.epi = g.epi & ~EPI_QKV_VT;
        if (n0 >= split) { h.epi |= EPI_STORE_VT; h.C = (f16 *)g.C2 - (size_t)split * g.vt_kp; h.bias = g.bias; }
        tile_epilogue_f16_one<NJ>(h, smem, acc, m0, n0, tid, lane, wm, wn);
        return;
    }
    if (!(g.epi & EPI_KV)) { tile_epilogue_f16_one<NJ>(g, smem, acc, m0, n0, tid, lane, wm, wn); return; }
    GemmArgs h = g;
    const int half = g.N >> 1;
    if (n0 >= half) {
        h.epi = (g.epi & ~(EPI_KV | EPI_CBATCH)) | EPI_STORE_VT;
        h.C = (f16 *)g.C2 - (size_t)half * g.vt_kp;          // the V epilogue addresses by the absolute column
    } else {
        h.epi = (g.epi & ~(EPI_KV | EPI_STORE_VT)) | EPI_CBATCH;
    }
    tile_epilogue_f16_one<NJ>(h, smem, acc, m0, n0, tid, lane, wm, wn);
}

}  // namespace
