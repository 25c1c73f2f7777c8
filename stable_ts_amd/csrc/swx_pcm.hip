// Probe audio that stays on the device (refine_many): the bisection of refine() changes a probe in at most one interval per
// unfinished word between two rounds -- `probe[row, a:b] = 0` or `probe[row, a:b] = clean[0, a:b]` -- so the host sends the
// round's edits instead of rebuilding and uploading 1.9 MB per window.
//
// The edits are ORDERED WRITES, not a set of muted intervals: two words can write to the same row and a restore can overwrite
// another word's mute, so for every sample the LAST op of its row that covers it decides its bits, and a sample no op covers
// keeps its bits.  The list comes stably sorted by row with the offsets of every row (d_row_start).
//
// One launch, grid (sample span, row).  A thread owns fixed sample positions (PE_VEC groups of 4 consecutive samples) and walks
// its row's ops in order with the pending values in registers: no two threads ever write the same sample, so the result is exact
// without atomics or barriers across workgroups, and the probe row is never read.  The op list goes through LDS once per
// workgroup, PE_BATCH ops at a time, each clipped to the workgroup's span as it is staged; a workgroup whose span meets no op of
// its row exits after reading the list.  A group of 4 that is written whole and lies on a 16-byte boundary leaves as one
// 16-byte store (and a restore reads clean the same way); the ragged ends, and rows whose stride puts them off that boundary,
// go scalar per lane.
#include "swx_common.h"
#include "swx_kernels.h"

namespace {

constexpr int PE_T = 256;                       // threads per workgroup
constexpr int PE_VEC = 4;                       // groups of 4 samples per thread
constexpr int PE_SPAN = PE_T * PE_VEC * 4;      // 4096 samples per workgroup (stable_ts_amd.engine.PCM_EDIT_SPAN)
constexpr int PE_BATCH = 128;                   // ops staged in LDS at a time (stable_ts_amd.engine.PCM_EDIT_BATCH)

__global__ __launch_bounds__(PE_T) void pcm_edit_kernel(const float *__restrict__ clean, float *__restrict__ probe, int64_t stride,
                                                        const int32_t *__restrict__ ops, const int32_t *__restrict__ row_start,
                                                        int n_ops)
{
    __shared__ int sh_a[PE_BATCH], sh_b[PE_BATCH], sh_kind[PE_BATCH];
    const int tid = threadIdx.x, row = blockIdx.y;
    const int64_t span_lo = (int64_t)blockIdx.x * PE_SPAN;
    const int64_t span_hi = span_lo + PE_SPAN < stride ? span_lo + PE_SPAN : stride;
    int s0 = row_start[row], s1 = row_start[row + 1];
    s0 = s0 < 0 ? 0 : (s0 > n_ops ? n_ops : s0);
    s1 = s1 < s0 ? s0 : (s1 > n_ops ? n_ops : s1);
    if (s0 == s1) return;
    const float *c_row = clean + (size_t)(row >> 1) * (size_t)stride;
    float *p_row = probe + (size_t)row * (size_t)stride;

    float val[PE_VEC][4];
    unsigned dirty[PE_VEC];
#pragma unroll
    for (int v = 0; v < PE_VEC; ++v) {
        dirty[v] = 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) val[v][j] = 0.f;
    }
    bool any = false;

    for (int base = s0; base < s1; base += PE_BATCH) {
        const int nb = s1 - base < PE_BATCH ? s1 - base : PE_BATCH;
        __syncthreads();                                                // the walk of the batch before is over
        bool live = false;
        if (tid < nb) {
            const int32_t *op = ops + (size_t)(base + tid) * 4;
            const int o_row = op[0], kind = op[3];
            int64_t a = op[1], b = op[2];
            a = a < span_lo ? span_lo : a;                              // span_lo >= 0, span_hi <= stride: the clamp to [0, stride]
            b = b > span_hi ? span_hi : b;
            live = o_row == row && (kind == 0 || kind == 1) && a < b;
            sh_a[tid] = live ? (int)a : 0;
            sh_b[tid] = live ? (int)b : 0;
            sh_kind[tid] = kind;
        }
        if (__syncthreads_or(live)) {
            any = true;
            for (int k = 0; k < nb; ++k) {
                const int a = sh_a[k], b = sh_b[k];
                if (a >= b) continue;
                const int kind = sh_kind[k];
#pragma unroll
                for (int v = 0; v < PE_VEC; ++v) {
                    const int64_t p64 = span_lo + ((int64_t)v * PE_T + tid) * 4;
                    if (p64 >= b || p64 + 4 <= a) continue;
                    const int p = (int)p64;
                    if (kind == 1) {
                        if (a <= p && p + 4 <= b && (((uintptr_t)(c_row + p)) & 15u) == 0) {
                            const float4 c = *(const float4 *)(c_row + p);
                            val[v][0] = c.x; val[v][1] = c.y; val[v][2] = c.z; val[v][3] = c.w;
                            dirty[v] = 15u;
                        } else {
#pragma unroll
                            for (int j = 0; j < 4; ++j)
                                if (p + j >= a && p + j < b) { val[v][j] = c_row[p + j]; dirty[v] |= 1u << j; }
                        }
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (p + j >= a && p + j < b) { val[v][j] = 0.f; dirty[v] |= 1u << j; }
                    }
                }
            }
        }
    }
    if (!any) return;
#pragma unroll
    for (int v = 0; v < PE_VEC; ++v) {
        if (!dirty[v]) continue;
        const int64_t p = span_lo + ((int64_t)v * PE_T + tid) * 4;       // a dirty lane lies below span_hi <= stride by construction
        if (dirty[v] == 15u && (((uintptr_t)(p_row + p)) & 15u) == 0) {
            *(float4 *)(p_row + p) = make_float4(val[v][0], val[v][1], val[v][2], val[v][3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (dirty[v] & (1u << j)) p_row[p + j] = val[v][j];
        }
    }
}

}  // namespace

extern "C" int swx_pcm_edit(const float *d_clean, float *d_probe, int64_t stride, int n_rows, const int32_t *d_ops,
                            const int32_t *d_row_start, int n_ops, void *stream)
{
    if (n_ops == 0) return 0;
    if (!d_clean || !d_probe || !d_ops || !d_row_start || n_ops < 0 || n_rows <= 0 || n_rows > 65535 || stride <= 0 ||
        stride > 0x7FFFFFFF - PE_SPAN)
        return -1;
    hipLaunchKernelGGL(pcm_edit_kernel, dim3(cdiv(stride, PE_SPAN), n_rows), dim3(PE_T), 0, (hipStream_t)stream, d_clean, d_probe,
                       stride, d_ops, d_row_start, n_ops);
    SWX_CHECK_LAUNCH();
    return 0;
}
