"""The spectral gate of denoiser="noisereduce" (DESIGN.md section 8), restated on the CPU with torch.stft, conv1d, conv2d and
torch.istft: the yardstick of tests/test_gpu_spectral_gate.py (f64, and f32 for the rounding floor) and the subject of
tests/test_spectral_gate_ref_cpu.py.  Not a test module; nothing here touches the device."""
import math
import warnings

import numpy as np
import torch
import torch.nn.functional as F

SR = 16000
DEFAULTS = dict(n_fft=512, prop_decrease=1.0, time_constant_s=2.0, thresh_n_mult_nonstationary=2.0,
                sigmoid_slope_nonstationary=10.0, freq_mask_smooth_hz=500, time_mask_smooth_ms=50)


def triangle(n: int, dtype=torch.float64) -> torch.Tensor:
    """v_n[a] = 1 - |a| / (n + 1) for |a| <= n"""
    a = torch.arange(-n, n + 1, dtype=dtype)
    return 1 - a.abs() / (n + 1)


def widths(sr=SR, **options):
    """(M, n_f or None, n_t or None) of the statement; None = that smoothing option was None"""
    o = {**DEFAULTS, **options}
    n_fft = o["n_fft"]
    hop = n_fft // 4
    M = int(o["time_constant_s"] / hop * sr)
    n_f = None if o["freq_mask_smooth_hz"] is None else int(o["freq_mask_smooth_hz"] / (sr / (n_fft / 2)))
    n_t = None if o["time_mask_smooth_ms"] is None else int(o["time_mask_smooth_ms"] / (hop / sr * 1000))
    for v in (n_f, n_t):
        if v is not None and v < 1:
            raise ValueError("smoothing width below one bin")
    return M, n_f, n_t


def smoothing_filter(n_f, n_t, dtype=torch.float64):
    """the 2-D filter of step 4, or None when both options are None"""
    if n_f is None and n_t is None:
        return None
    k = torch.outer(triangle(1 if n_f is None else n_f, dtype), triangle(1 if n_t is None else n_t, dtype))
    return k / k.sum()


def n_frames(n: int, n_fft: int = 512) -> int:
    hop = n_fft // 4
    return -(-n // hop) + 1


def gate(x, dtype=torch.float64, sr=SR, **options) -> torch.Tensor:
    """steps 1-5 on one row [n] (or rows [C][n], each on its own)"""
    o = {**DEFAULTS, **options}
    n_fft = o["n_fft"]
    hop = n_fft // 4
    M, n_f, n_t = widths(sr, **options)
    x = torch.as_tensor(x).to(dtype)
    if x.dim() == 2:
        return torch.stack([gate(r, dtype, sr, **options) for r in x])
    n = x.shape[-1]
    n_pad = -(-n // hop) * hop
    w = torch.hann_window(n_fft, dtype=dtype)
    X = torch.stft(F.pad(x, (0, n_pad - n)), n_fft, hop, n_fft, window=w, center=True, pad_mode="constant", return_complex=True)
    A = X.abs()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)              # "even kernel lengths ... may require a zero-padded copy"
        S = F.conv1d(A[:, None, :], torch.ones(1, 1, M, dtype=dtype), padding="same")[:, 0, :] / M
    m = torch.sigmoid(((A - S) / (S + 1e-6) - o["thresh_n_mult_nonstationary"]) * o["sigmoid_slope_nonstationary"])
    m = o["prop_decrease"] * (m - 1.0) + 1.0
    k = smoothing_filter(n_f, n_t, dtype)
    if k is not None:
        m = F.conv2d(m[None, None], k[None, None], padding="same")[0, 0]
    y = torch.istft(X * m, n_fft, hop, n_fft, window=w, center=True, length=n_pad)
    return torch.nan_to_num(y[:n])


def gate_literal(x: np.ndarray, sr=SR, **options) -> np.ndarray:
    """steps 1-5 as written, in f64 numpy with an O(n_fft^2) DFT and explicit loops over the filter taps: for short rows only"""
    o = {**DEFAULTS, **options}
    n_fft = o["n_fft"]
    hop, K = n_fft // 4, n_fft // 2 + 1
    M, n_f, n_t = widths(sr, **options)
    x = np.asarray(x, np.float64)
    n = len(x)
    n_pad = -(-n // hop) * hop
    Fr = n_pad // hop + 1
    i = np.arange(n_fft)
    w = 0.5 - 0.5 * np.cos(2 * np.pi * i / n_fft)
    dft = np.exp(-2j * np.pi * np.outer(np.arange(K), i) / n_fft)
    X = np.zeros((K, Fr), np.complex128)
    for f in range(Fr):
        s = f * hop - n_fft // 2 + i
        frame = np.where((s >= 0) & (s < n), x[np.clip(s, 0, n - 1)], 0.0)
        X[:, f] = dft @ (w * frame)
    A = np.abs(X)
    L = (M - 1) // 2
    S = np.zeros_like(A)
    for f in range(Fr):
        lo, hi = max(f - L, 0), min(f - L + M, Fr)
        S[:, f] = A[:, lo:hi].sum(axis=1) / M
    m = 1.0 / (1.0 + np.exp(-((A - S) / (S + 1e-6) - o["thresh_n_mult_nonstationary"]) * o["sigmoid_slope_nonstationary"]))
    m = o["prop_decrease"] * (m - 1.0) + 1.0
    if n_f is not None or n_t is not None:
        n_f, n_t = n_f or 1, n_t or 1
        vf = 1 - np.abs(np.arange(-n_f, n_f + 1)) / (n_f + 1)
        vt = 1 - np.abs(np.arange(-n_t, n_t + 1)) / (n_t + 1)
        padded = np.zeros((K + 2 * n_f, Fr + 2 * n_t))
        padded[n_f:n_f + K, n_t:n_t + Fr] = m
        sm = np.zeros_like(m)
        for a in range(2 * n_f + 1):
            for b in range(2 * n_t + 1):
                sm += vf[a] * vt[b] * padded[a:a + K, b:b + Fr]
        m = sm / (vf.sum() * vt.sum())
    Y = X * m
    full = np.concatenate([Y, np.conj(Y[-2:0:-1])], axis=0)                   # Hermitian extension, bins 0 .. n_fft - 1
    full[0], full[K - 1] = full[0].real, full[K - 1].real
    idft = np.exp(2j * np.pi * np.outer(i, np.arange(n_fft)) / n_fft) / n_fft
    acc = np.zeros(n_pad + n_fft)
    env = np.zeros(n_pad + n_fft)
    for f in range(Fr):
        acc[f * hop:f * hop + n_fft] += w * (idft @ full[:, f]).real
        env[f * hop:f * hop + n_fft] += w * w
    y = acc[n_fft // 2:n_fft // 2 + n] / env[n_fft // 2:n_fft // 2 + n]
    return np.nan_to_num(y, nan=0.0, posinf=np.finfo(np.float32).max, neginf=-np.finfo(np.float32).max)


def bursts_plus_noise(seconds: int = 10, seed: int = 0):
    """0.6 s of 220 Hz + 880 Hz tones at amplitude 0.3 every 2 s plus 0.02 randn noise -> (row f32, noise-only index mask that
    leaves out the first and the last second, the noise alone)"""
    g = torch.Generator().manual_seed(seed)
    n = SR * seconds
    t = torch.arange(n) / SR
    env = ((t % 2.0) < 0.6).float()
    sig = 0.3 * env * (torch.sin(2 * math.pi * 220 * t) + 0.5 * torch.sin(2 * math.pi * 880 * t))
    noise = 0.02 * torch.randn(n, generator=g)
    q = env == 0
    q[:SR] = False
    q[-SR:] = False
    return (sig + noise).float(), q, noise


def attenuation_db(y, q, noise) -> float:
    """level of the gated noise-only stretches over the level of the noise that went in"""
    out = float((torch.as_tensor(y).double()[q] ** 2).mean().sqrt())
    inn = float((noise.double()[q] ** 2).mean().sqrt())
    return 20 * math.log10(out / inn)
