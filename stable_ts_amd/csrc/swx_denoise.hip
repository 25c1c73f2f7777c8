// Non-stationary spectral gating of PCM on the device: denoiser="noisereduce" (stable_whisper/audio/noisereduce.py hands the
// audio to the noisereduce package with n_fft = 512, stationary = False).  The algorithm is published and model-free; the statement
// this file implements is written out in DESIGN.md section 8 and restated on the CPU in tests/spectral_gate_ref.py:
//
//   1. STFT, periodic Hann window of n_fft, hop n_fft / 4, centred frames, zeros outside the signal
//   2. S = moving mean of |X| over n_mean frames along time (zeros outside the frame grid)
//   3. m = sigmoid(((|X| - S) / (S + 1e-6) - thresh) * slope), then prop_decrease * (m - 1) + 1
//   4. m smoothed by a triangular filter over frequency and time (zeros outside the grid)
//   5. inverse STFT of X m: inverse real DFT, window, overlap-add, division by the overlap-added squared window
//
// The recording is walked in blocks of output hops so that the scratch does not grow with its length.  Per block, five launches:
//
//   sg_stft_kernel   one wave per frame: windowed frame -> LDS, n_fft real points as an n_fft / 2-point complex radix-2 Stockham
//                    FFT in padded LDS planes, split into the n_fft / 2 + 1 bins, X[frame][bin] and |X| out with 16-byte stores
//   sg_mask_kernel   one thread per frame and 4 bins: the moving mean as a direct sum in ascending frame order (16-byte loads that
//                    are coalesced along the bins, so nothing is transposed), the mask
//   sg_synth_kernel  one wave per frame: the two smoothing passes (time from global, frequency through LDS with a zero halo),
//                    X m, the inverse transform, the window; the windowed frame out with 16-byte stores
//   sg_ola_kernel    one thread per 4 output samples: the (at most four) covering frames gathered in ascending frame order
//
// Every value is a function of absolute frame / sample indices only and every sum has a fixed order, so the output is the same bits
// for every block size, every row count and every run: no atomics, no running sums.  A block recomputes the frames of its halo
// (n_mean - 1 + 2 n_grad_time + 3 of them).  The twiddle and window tables are computed in f64 by a kernel of the same stream at the
// start of the call (the call has no handle to keep them in, and copies from host memory would tie the stream to the host).
#include <float.h>
#include "swx_common.h"
#include "swx_kernels.h"

namespace {

constexpr int SG_PL = 544;              // floats per LDS plane: sg_pad(512) + 1 = 529, rounded up
constexpr int SG_MAXG = 128;            // largest smoothing half-width
constexpr int SG_DEFAULT_BLOCK = 4096;  // output hops per block
constexpr int SG_MAX_MEAN = 1 << 20;

int g_block = 0;                        // swx_test_spectral_gate_block

// one dword of padding per 32: the stride-2 accesses of the first butterfly stage and of the bin split fall on distinct banks
__device__ __forceinline__ int sg_pad(int j) { return j + (j >> 5); }

__global__ void sg_tables_kernel(float2 *__restrict__ tw, float *__restrict__ win, int n_fft)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_fft) return;
    double s, c;
    sincospi(2.0 * (double)i / (double)n_fft, &s, &c);
    win[i] = (float)(0.5 - 0.5 * c);
    if (i < n_fft / 2) tw[i] = make_float2((float)c, (float)(-s));          // exp(-2 pi i / n_fft)
}

// nn-point complex FFT of the workgroup's (one wave's) frame, natural order in and out: radix-2 Stockham, ping-pong between the two
// buffers.  In: buf[0].  Returns the buffer that holds the result.  conj = -1 runs the conjugate twiddles (unnormalised inverse).
__device__ __forceinline__ int sg_fft(float (*buf)[2][SG_PL], int nn, int n_fft, const float2 *__restrict__ tw, float conj, int lane)
{
    int cur = 0;
    const int T = nn >> 1;
    for (int p = 1; p < nn; p <<= 1) {
        __syncthreads();
        const float *xr = buf[cur][0], *xi = buf[cur][1];
        float *yr = buf[cur ^ 1][0], *yi = buf[cur ^ 1][1];
        const int tstride = n_fft / (2 * p);                               // tw[k tstride] = exp(-i pi k / p)
        for (int t = lane; t < T; t += 64) {
            const int k = t & (p - 1);
            const float2 w = tw[k * tstride];
            const float wr = w.x, wi = conj * w.y;
            const float ar = xr[sg_pad(t)], ai = xi[sg_pad(t)];
            const float br = xr[sg_pad(t + T)], bi = xi[sg_pad(t + T)];
            const float cr = br * wr - bi * wi, ci = br * wi + bi * wr;
            const int j = (t << 1) - k;
            yr[sg_pad(j)] = ar + cr;
            yi[sg_pad(j)] = ai + ci;
            yr[sg_pad(j + p)] = ar - cr;
            yi[sg_pad(j + p)] = ai - ci;
        }
        cur ^= 1;
    }
    __syncthreads();
    return cur;
}

// grid (frames of the block's wide range, rows), 64 threads.  Frame fa0 + blockIdx.x -> X [row][Wf][ldk] complex, A = |X| [row][Wf][ldk]
__global__ __launch_bounds__(64) void sg_stft_kernel(const float *__restrict__ pcm, int64_t pcm_stride, int64_t n, int64_t fa0, int n_fft,
                                                     const float2 *__restrict__ tw, const float *__restrict__ win,
                                                     float *__restrict__ X, float *__restrict__ A, int Wf, int ldk)
{
    __shared__ float buf[2][2][SG_PL];
    const int lane = threadIdx.x, fi = blockIdx.x, row = blockIdx.y;
    const int nn = n_fft >> 1, hop = n_fft >> 2;
    const float *x = pcm + (int64_t)row * pcm_stride;
    const int64_t s0 = (fa0 + fi) * hop - nn;
    const bool aligned = (((uintptr_t)x + (uintptr_t)(s0 * 4)) & 15u) == 0;
    for (int q = lane; q < (n_fft >> 2); q += 64) {
        const int64_t s = s0 + 4 * q;
        float v[4];
        if (aligned && s >= 0 && s + 4 <= n) {
            const float4 t = *(const float4 *)(x + s);
            v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = (s + e >= 0 && s + e < n) ? x[s + e] : 0.f;
        }
        const float4 w = *(const float4 *)(win + 4 * q);
        buf[0][0][sg_pad(2 * q)] = v[0] * w.x;
        buf[0][1][sg_pad(2 * q)] = v[1] * w.y;
        buf[0][0][sg_pad(2 * q + 1)] = v[2] * w.z;
        buf[0][1][sg_pad(2 * q + 1)] = v[3] * w.w;
    }
    const int cur = sg_fft(buf, nn, n_fft, tw, 1.f, lane);
    const float *zr = buf[cur][0], *zi = buf[cur][1];
    float *xrow = X + ((int64_t)row * Wf + fi) * ldk * 2;
    float *arow = A + ((int64_t)row * Wf + fi) * ldk;
    // Z = FFT of (even samples + i odd samples): X[k] = E[k] + W^k O[k], E = (Z[k] + conj Z[nn - k]) / 2, O = (Z[k] - conj Z[nn - k]) / 2i
    for (int q = lane; q < (nn >> 1); q += 64) {
        float o[4], a[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int k = 2 * q + e, kk = (nn - k) & (nn - 1);
            const float ar = zr[sg_pad(k)], ai = zi[sg_pad(k)];
            const float br = zr[sg_pad(kk)], bi = -zi[sg_pad(kk)];
            const float er = 0.5f * (ar + br), ei = 0.5f * (ai + bi);
            const float pr = 0.5f * (ai - bi), pi = -0.5f * (ar - br);
            const float2 w = tw[k];
            const float xr = er + (pr * w.x - pi * w.y), xi = ei + (pr * w.y + pi * w.x);
            o[2 * e] = xr; o[2 * e + 1] = xi;
            a[e] = sqrtf(xr * xr + xi * xi);
        }
        *(float4 *)(xrow + 4 * q) = make_float4(o[0], o[1], o[2], o[3]);
        *(float2 *)(arow + 2 * q) = make_float2(a[0], a[1]);
    }
    if (lane == 0) {
        const float xr = zr[0] - zi[0];                                      // the Nyquist bin: E[0] - O[0]
        xrow[2 * nn] = xr; xrow[2 * nn + 1] = 0.f;
        arow[nn] = fabsf(xr);
        for (int k = nn + 1; k < ldk; ++k) { xrow[2 * k] = 0.f; xrow[2 * k + 1] = 0.f; arow[k] = 0.f; }
    }
}

__device__ __forceinline__ float sg_mask_value(float a, float sum, float n_mean, float thresh, float slope, float prop)
{
    const float S = sum / n_mean;
    const float r = (a - S) / (S + 1e-6f);
    const float m = 1.f / (1.f + expf(-((r - thresh) * slope)));
    return prop * (m - 1.f) + 1.f;
}

// grid (ceil(nm ldk / 4 / 256), rows).  Mask frame fm0 + i (zeros outside [0, F)) -> Mk [row][Wm][ldk]
__global__ __launch_bounds__(256) void sg_mask_kernel(const float *__restrict__ A, float *__restrict__ Mk, int64_t F, int64_t fa0, int64_t fm0,
                                                      int nm, int ldk, int Wf, int Wm, int n_mean, int L, float thresh, float slope,
                                                      float prop)
{
    const int ldk4 = ldk >> 2, row = blockIdx.y;
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gid >= (int64_t)nm * ldk4) return;
    const int fmi = (int)(gid / ldk4), g = (int)(gid - (int64_t)fmi * ldk4);
    const int64_t f = fm0 + fmi;
    float4 m = make_float4(0.f, 0.f, 0.f, 0.f);
    if (f >= 0 && f < F) {
        const int64_t lo = f - L > 0 ? f - L : 0;
        const int64_t hi = f - L + n_mean < F ? f - L + n_mean : F;
        const float *a = A + ((int64_t)row * Wf + (lo - fa0)) * ldk + 4 * g;
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int64_t j = lo; j < hi; ++j, a += ldk) {
            const float4 v = *(const float4 *)a;
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
        const float4 c = *(const float4 *)(A + ((int64_t)row * Wf + (f - fa0)) * ldk + 4 * g);
        const float nm_f = (float)n_mean;
        m.x = sg_mask_value(c.x, s.x, nm_f, thresh, slope, prop);
        m.y = sg_mask_value(c.y, s.y, nm_f, thresh, slope, prop);
        m.z = sg_mask_value(c.z, s.z, nm_f, thresh, slope, prop);
        m.w = sg_mask_value(c.w, s.w, nm_f, thresh, slope, prop);
    }
    *(float4 *)(Mk + ((int64_t)row * Wm + fmi) * ldk + 4 * g) = m;
}

// grid (frames fy0 .. of the block, rows), 64 threads: the windowed output frame -> Yf [row][Wy][n_fft]
__global__ __launch_bounds__(64) void sg_synth_kernel(const float *__restrict__ X, const float *__restrict__ Mk, float *__restrict__ Yf,
                                                      int64_t fy0, int64_t fa0, int64_t fm0, int n_fft, int ldk, int Wf, int Wm, int Wy,
                                                      int nf, int nt, const float2 *__restrict__ tw, const float *__restrict__ win)
{
    __shared__ float buf[2][2][SG_PL];
    __shared__ float mt[SG_PL + 2 * SG_MAXG];
    const int lane = threadIdx.x, fyi = blockIdx.x, row = blockIdx.y;
    const int nn = n_fft >> 1, K = nn + 1;
    const int64_t f = fy0 + fyi;
    const float *mrow = Mk + ((int64_t)row * Wm + (f - fm0)) * ldk;
    const float *xrow = X + ((int64_t)row * Wf + (f - fa0)) * ldk * 2;
    const bool smooth = nf > 0;
    if (smooth) {
        const float dt = (float)(nt + 1);
        for (int i = lane; i < K + 2 * nf; i += 64) {
            const int k = i - nf;
            float acc = 0.f;
            if (k >= 0 && k < K)
                for (int b = -nt; b <= nt; ++b) acc += ((float)(nt + 1 - (b < 0 ? -b : b)) / dt) * mrow[b * ldk + k];
            mt[i] = acc;
        }
        __syncthreads();
    }
    const float df = (float)(nf + 1), norm = (float)((nf + 1) * (nt + 1));
    for (int k = lane; k < K; k += 64) {
        float mm;
        if (smooth) {
            float acc = 0.f;
            for (int a = -nf; a <= nf; ++a) acc += ((float)(nf + 1 - (a < 0 ? -a : a)) / df) * mt[k + nf + a];
            mm = acc / norm;
        } else {
            mm = mrow[k];
        }
        const float2 xv = *(const float2 *)(xrow + 2 * k);
        buf[1][0][sg_pad(k)] = xv.x * mm;
        buf[1][1][sg_pad(k)] = xv.y * mm;
    }
    __syncthreads();
    // the inverse of the split: Z'[k] = E'[k] + i O'[k], 2 E' = Y[k] + conj Y[nn - k], 2 O' = (Y[k] - conj Y[nn - k]) conj W^k
    for (int k = lane; k < nn; k += 64) {
        const float yr = buf[1][0][sg_pad(k)], yi = buf[1][1][sg_pad(k)];
        const float cr = buf[1][0][sg_pad(nn - k)], ci = -buf[1][1][sg_pad(nn - k)];
        const float er = yr + cr, ei = yi + ci, dr = yr - cr, di = yi - ci;
        const float2 w = tw[k];
        const float pr = dr * w.x + di * w.y, pi = di * w.x - dr * w.y;
        buf[0][0][sg_pad(k)] = er - pi;
        buf[0][1][sg_pad(k)] = ei + pr;
    }
    const int cur = sg_fft(buf, nn, n_fft, tw, -1.f, lane);
    const float *zr = buf[cur][0], *zi = buf[cur][1];
    const float scale = 1.f / (float)n_fft;                                  // 1 / nn of the inverse and the two halves above
    float *yrow = Yf + ((int64_t)row * Wy + fyi) * n_fft;
    for (int q = lane; q < (n_fft >> 2); q += 64) {
        const float4 w = *(const float4 *)(win + 4 * q);
        *(float4 *)(yrow + 4 * q) = make_float4(zr[sg_pad(2 * q)] * scale * w.x, zi[sg_pad(2 * q)] * scale * w.y,
                                                zr[sg_pad(2 * q + 1)] * scale * w.z, zi[sg_pad(2 * q + 1)] * scale * w.w);
    }
}

__device__ __forceinline__ float sg_nan_to_num(float v)
{
    if (v != v) return 0.f;
    if (v > FLT_MAX) return FLT_MAX;
    if (v < -FLT_MAX) return -FLT_MAX;
    return v;
}

// grid (ceil((s_end - s_begin) / 4 / 256), rows): output samples [s_begin, s_end), s_begin a multiple of the hop
__global__ __launch_bounds__(256) void sg_ola_kernel(const float *__restrict__ Yf, const float *__restrict__ win, float *__restrict__ out,
                                                     int64_t out_stride, int64_t s_begin, int64_t s_end, int64_t fy0, int64_t F,
                                                     int n_fft, int Wy)
{
    const int row = blockIdx.y, hop = n_fft >> 2;
    const int64_t s = s_begin + ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (s >= s_end) return;
    const int64_t h = s / hop;
    const int t = (int)(s - h * hop);                                        // the 4 samples lie in one hop (hop is a multiple of 4)
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f), env = acc;
#pragma unroll
    for (int d = -1; d <= 2; ++d) {
        const int64_t f = h + d;
        if (f < 0 || f >= F) continue;
        const int idx = t + (2 - d) * hop;
        const float4 v = *(const float4 *)(Yf + ((int64_t)row * Wy + (f - fy0)) * n_fft + idx);
        const float4 w = *(const float4 *)(win + idx);
        acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
        env.x += w.x * w.x; env.y += w.y * w.y; env.z += w.z * w.z; env.w += w.w * w.w;
    }
    const float o[4] = {sg_nan_to_num(acc.x / env.x), sg_nan_to_num(acc.y / env.y), sg_nan_to_num(acc.z / env.z),
                        sg_nan_to_num(acc.w / env.w)};
    float *dst = out + (int64_t)row * out_stride + s;
    if (s + 4 <= s_end && (((uintptr_t)dst) & 15u) == 0) {
        *(float4 *)dst = make_float4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (s + e < s_end) dst[e] = o[e];
    }
}

struct SgLayout {
    int ldk, Wf, Wm, Wy, block;
    size_t off_tw, off_win, off_x, off_a, off_m, off_y, total;
};

bool sg_cfg_ok(const swx_gate_cfg *c)
{
    if (!c) return false;
    if (c->n_fft != 256 && c->n_fft != 512 && c->n_fft != 1024) return false;
    if (c->n_mean < 1 || c->n_mean > SG_MAX_MEAN) return false;
    if (!(c->thresh == c->thresh) || !(c->slope == c->slope) || !(c->prop_decrease == c->prop_decrease)) return false;
    if (c->n_grad_freq == 0 && c->n_grad_time == 0) return true;
    return c->n_grad_freq >= 1 && c->n_grad_freq <= SG_MAXG && c->n_grad_time >= 1 && c->n_grad_time <= SG_MAXG;
}

size_t sg_align(size_t v) { return (v + 255) & ~(size_t)255; }

SgLayout sg_layout(int rows, const swx_gate_cfg *c)
{
    SgLayout l;
    l.block = g_block > 0 ? g_block : SG_DEFAULT_BLOCK;
    l.ldk = (c->n_fft / 2 + 1 + 3) & ~3;
    l.Wy = l.block + 3;
    l.Wm = l.Wy + 2 * c->n_grad_time;
    l.Wf = l.Wm + c->n_mean - 1;
    size_t o = 0;
    l.off_tw = o;  o += sg_align((size_t)(c->n_fft / 2) * sizeof(float2));
    l.off_win = o; o += sg_align((size_t)c->n_fft * sizeof(float));
    l.off_x = o;   o += sg_align((size_t)rows * l.Wf * l.ldk * 2 * sizeof(float));
    l.off_a = o;   o += sg_align((size_t)rows * l.Wf * l.ldk * sizeof(float));
    l.off_m = o;   o += sg_align((size_t)rows * l.Wm * l.ldk * sizeof(float));
    l.off_y = o;   o += sg_align((size_t)rows * l.Wy * c->n_fft * sizeof(float));
    l.total = o;
    return l;
}

}  // namespace

extern "C" int swx_test_spectral_gate_block(int frames_per_block)
{
    if (frames_per_block < 0 || frames_per_block > (1 << 20)) return -1;
    g_block = frames_per_block;
    return 0;
}

extern "C" size_t swx_spectral_gate_scratch_bytes(int rows, const swx_gate_cfg *cfg)
{
    if (rows <= 0 || rows > 65535 || !sg_cfg_ok(cfg)) return 0;
    return sg_layout(rows, cfg).total;
}

extern "C" int swx_spectral_gate(const float *d_pcm, int64_t pcm_stride, int rows, int64_t n, const swx_gate_cfg *cfg, float *d_out,
                                 int64_t out_stride, void *d_scratch, size_t scratch_bytes, void *stream)
{
    if (!d_pcm || !d_out || !d_scratch || rows <= 0 || rows > 65535 || n < 1 || !sg_cfg_ok(cfg)) return -1;
    if (pcm_stride < n || out_stride < n || n > ((int64_t)1 << 40) || (((uintptr_t)d_scratch) & 15u) != 0) return -1;
    {   // the two buffers must not overlap
        const uintptr_t a0 = (uintptr_t)d_pcm, a1 = a0 + (size_t)(((int64_t)(rows - 1) * pcm_stride + n) * 4);
        const uintptr_t b0 = (uintptr_t)d_out, b1 = b0 + (size_t)(((int64_t)(rows - 1) * out_stride + n) * 4);
        if (a0 < b1 && b0 < a1) return -1;
    }
    const SgLayout l = sg_layout(rows, cfg);
    if (scratch_bytes < l.total) return -1;
    hipStream_t s = (hipStream_t)stream;
    char *base = (char *)d_scratch;
    float2 *tw = (float2 *)(base + l.off_tw);
    float *win = (float *)(base + l.off_win), *X = (float *)(base + l.off_x), *A = (float *)(base + l.off_a);
    float *Mk = (float *)(base + l.off_m), *Yf = (float *)(base + l.off_y);
    const int n_fft = cfg->n_fft, hop = n_fft / 4, M = cfg->n_mean, L = (M - 1) / 2, nf = cfg->n_grad_freq, nt = cfg->n_grad_time;
    const int64_t hops = (n + hop - 1) / hop, F = hops + 1;

    hipLaunchKernelGGL(sg_tables_kernel, dim3(cdiv(n_fft, 256)), dim3(256), 0, s, tw, win, n_fft);
    for (int64_t h0 = 0; h0 < hops; h0 += l.block) {
        const int64_t h1 = h0 + l.block < hops ? h0 + l.block : hops;
        const int64_t fy0 = h0 - 1 > 0 ? h0 - 1 : 0, fy1 = h1 + 2 < F ? h1 + 2 : F;       // frames that cover the block's samples
        const int64_t fm0 = fy0 - nt, fm1 = fy1 + nt;                                     // mask frames (zeros outside the grid)
        const int64_t fa0 = fm0 - L > 0 ? fm0 - L : 0;                                     // frames whose |X| the means read
        const int64_t fa1 = fm1 - 1 - L + M < F ? fm1 - 1 - L + M : F;
        const int na = (int)(fa1 - fa0), nm = (int)(fm1 - fm0), ny = (int)(fy1 - fy0);
        if (na > l.Wf || nm > l.Wm || ny > l.Wy) return -2;
        const int64_t s_end = h1 * hop < n ? h1 * hop : n;
        hipLaunchKernelGGL(sg_stft_kernel, dim3(na, rows), dim3(64), 0, s, d_pcm, pcm_stride, n, fa0, n_fft, tw, win, X, A, l.Wf, l.ldk);
        hipLaunchKernelGGL(sg_mask_kernel, dim3(cdiv((int64_t)nm * (l.ldk / 4), 256), rows), dim3(256), 0, s, A, Mk, F, fa0, fm0, nm,
                           l.ldk, l.Wf, l.Wm, M, L, cfg->thresh, cfg->slope, cfg->prop_decrease);
        hipLaunchKernelGGL(sg_synth_kernel, dim3(ny, rows), dim3(64), 0, s, X, Mk, Yf, fy0, fa0, fm0, n_fft, l.ldk, l.Wf, l.Wm, l.Wy, nf,
                           nt, tw, win);
        hipLaunchKernelGGL(sg_ola_kernel, dim3(cdiv((s_end - h0 * hop + 3) / 4, 256), rows), dim3(256), 0, s, Yf, win, d_out, out_stride,
                           h0 * hop, s_end, fy0, F, n_fft, l.Wy);
    }
    SWX_CHECK_LAUNCH();
    return 0;
}
