"""denoiser="noisereduce": non-stationary spectral gating of the audio on the device.

The reference's wrapper (``stable_whisper/audio/noisereduce.py``) hands the audio to the ``noisereduce`` package with
``n_fft=512, stationary=False, use_torch=True, sr=16000``.  That is a published, model-free algorithm -- STFT, one mask value
per time-frequency bin, inverse STFT -- and it runs here as HIP kernels behind ``swx_spectral_gate`` (``csrc/swx_denoise.hip``).
The statement that is implemented, what of it could not be checked against the package, and the measured numbers are in
DESIGN.md section 8; ``tests/spectral_gate_ref.py`` restates it on the CPU.

``demucs`` and ``dfnet`` need model files and stay refused (``audio_io.reject_denoiser``).
"""
import ctypes
from typing import Callable, Optional, Union

import numpy as np
import torch

from .audio import SAMPLE_RATE

GATE_DEFAULTS = dict(n_fft=512, prop_decrease=1.0, time_constant_s=2.0, thresh_n_mult_nonstationary=2.0,
                     sigmoid_slope_nonstationary=10.0, freq_mask_smooth_hz=500, time_mask_smooth_ms=50)
# options of noisereduce.reduce_noise that only steer how the package schedules its own work
_IGNORED = ("progress", "use_tqdm", "n_jobs", "chunk_size", "padding", "use_torch", "tmp_folder", "device")
_MAX_GRAD = 128           # csrc/swx_denoise.hip SG_MAXG


def gate_config(options: Optional[dict], sr: int = SAMPLE_RATE) -> dict:
    """``reduce_noise`` options -> the fields of ``swx_gate_cfg`` (n_fft, n_mean, thresh, slope, prop_decrease, n_grad_freq,
    n_grad_time).  A pure host function: the derived widths of DESIGN.md section 8, the refusals, no device."""
    o = dict(GATE_DEFAULTS)
    options = dict(options or {})
    for k in _IGNORED:
        options.pop(k, None)
    if options.pop("sr", sr) != sr:
        raise ValueError("Specified conflicting ``input_sr`` and ``sr``.")
    if options.pop("stationary", False):
        raise NotImplementedError("stationary=True (a noise profile over the whole clip) is not implemented: "
                                  "the non-stationary gate is what the reference's wrapper runs")
    if options.pop("y_noise", None) is not None:
        raise NotImplementedError("y_noise (a separate noise clip) belongs to the stationary gate, which is not implemented")
    win_length, hop_length = options.pop("win_length", None), options.pop("hop_length", None)
    unknown = [k for k in options if k not in o]
    if unknown:
        raise TypeError(f"unknown noisereduce option(s): {', '.join(sorted(unknown))}")
    o.update(options)
    n_fft = int(o["n_fft"])
    if n_fft not in (256, 512, 1024):
        raise NotImplementedError(f"n_fft={n_fft}: the device gate has 256, 512 and 1024")
    hop = n_fft // 4
    if win_length not in (None, n_fft) or hop_length not in (None, hop):
        raise NotImplementedError("win_length / hop_length other than n_fft and n_fft // 4 are not implemented")
    n_mean = int(o["time_constant_s"] / hop * sr)
    if n_mean < 1:
        raise ValueError("time_constant_s is shorter than one frame")
    hz, ms = o["freq_mask_smooth_hz"], o["time_mask_smooth_ms"]
    if hz is None and ms is None:
        n_f = n_t = 0
    else:
        n_f = 1 if hz is None else int(hz / (sr / (n_fft / 2)))
        n_t = 1 if ms is None else int(ms / (hop / sr * 1000))
        if n_f < 1:
            raise ValueError(f"freq_mask_smooth_hz needs to be at least {int(sr / (n_fft / 2))} Hz")
        if n_t < 1:
            raise ValueError(f"time_mask_smooth_ms needs to be at least {int(hop / sr * 1000)} ms")
        if n_f > _MAX_GRAD or n_t > _MAX_GRAD:
            raise NotImplementedError(f"mask smoothing over more than {_MAX_GRAD} bins is not implemented")
    return dict(n_fft=n_fft, n_mean=n_mean, thresh=float(o["thresh_n_mult_nonstationary"]),
                slope=float(o["sigmoid_slope_nonstationary"]), prop_decrease=float(o["prop_decrease"]),
                n_grad_freq=n_f, n_grad_time=n_t)


def spectral_gate(pcm: torch.Tensor, cfg: dict) -> torch.Tensor:
    """f32 device tensor [n] or [rows][n] -> the gated rows (a new tensor of the same shape), on the current stream."""
    from . import _lib
    lib = _lib.load()
    if not pcm.is_cuda:
        raise _lib.SwxError("spectral_gate needs a device tensor")
    x = pcm.to(torch.float32)
    x = (x[None] if x.dim() == 1 else x).contiguous()
    rows, n = x.shape
    if n == 0:
        return torch.empty_like(pcm, dtype=torch.float32)
    c = _lib.swx_gate_cfg(**cfg)
    out = torch.empty_like(x)
    with torch.cuda.device(x.device):
        nbytes = lib.swx_spectral_gate_scratch_bytes(rows, ctypes.byref(c))
        scratch = torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=x.device)
        _lib.check(lib.swx_spectral_gate(ctypes.c_void_p(x.data_ptr()), x.stride(0), rows, n, ctypes.byref(c),
                                         ctypes.c_void_p(out.data_ptr()), out.stride(0), ctypes.c_void_p(scratch.data_ptr()),
                                         scratch.numel(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
                   "swx_spectral_gate")
        scratch.record_stream(torch.cuda.current_stream())
    return out[0] if pcm.dim() == 1 else out


class NRWrapper:
    """what the reference's ``load_noisereduce_model`` returns: the rate the gate runs at, and the gate as a callable"""
    samplerate = SAMPLE_RATE

    def __call__(self, audio: torch.Tensor, **options) -> torch.Tensor:
        return spectral_gate(audio, gate_config(options, self.samplerate))


def load_noisereduce_model(cache: bool = True, **kwargs) -> NRWrapper:
    return NRWrapper()


def is_noisereduce_available():
    """the gate is part of libswx.so: nothing to install"""


def noisereduce_audio(audio: Union[torch.Tensor, np.ndarray, str, bytes], input_sr: Optional[int] = None,
                      output_sr: Optional[int] = None, model=None, device=None, verbose: Optional[bool] = True,
                      save_path: Optional[Union[str, Callable]] = None, **noisereduce_options) -> torch.Tensor:
    """Remove noise from ``audio`` by spectral gating (audio/noisereduce.py:38-87).  The result lives where the input lived:
    a file, an array or a CPU tensor gives a CPU tensor, a device tensor stays on its device."""
    from . import _lib
    from .audio_io import load_audio, resample, write_wav
    if model is None:
        model = load_noisereduce_model()
    if noisereduce_options.get("sr", input_sr) != input_sr:
        raise ValueError("Specified conflicting ``input_sr`` and ``sr``.")
    if isinstance(audio, (str, bytes)):
        audio = torch.from_numpy(load_audio(audio, model.samplerate))
        input_sr = model.samplerate
    else:
        if isinstance(audio, np.ndarray):
            audio = torch.from_numpy(audio)
        if input_sr != model.samplerate:
            if input_sr is None:
                raise ValueError("No ``input_sr`` specified for audio tensor.")
            audio = resample(audio, input_sr, model.samplerate)
    assert audio.dim() <= 2
    noisereduce_options = {k: v for k, v in noisereduce_options.items() if k != "sr"}
    cfg = gate_config(noisereduce_options, model.samplerate)           # refusals come before any device work
    _lib.require_gpu()
    home = audio.device
    if audio.is_cuda:
        dev = audio.device
    else:
        dev = torch.device("cuda", torch.cuda.current_device()) if device in (None, "cuda") else torch.device(device)
    rows = audio.to(device=dev, dtype=torch.float32)
    gated = spectral_gate(rows, cfg)
    denoised = gated.mean(dim=0) if gated.dim() == 2 else gated
    denoised = denoised.to(home)

    if output_sr is not None and input_sr != output_sr:
        denoised = resample(denoised, input_sr, output_sr)
    if save_path is not None:
        if isinstance(save_path, str):
            write_wav(save_path, denoised, output_sr or input_sr)
            if verbose:
                print(f"Saved: {save_path}")
        else:
            save_path(denoised, output_sr)
    return denoised


SUPPORTED_DENOISERS = {
    "noisereduce": {"run": noisereduce_audio, "load": load_noisereduce_model, "access": is_noisereduce_available},
}
# named by the reference, refused here: they need model files (audio_io.reject_denoiser)
REFERENCE_DENOISERS = ("demucs", "dfnet", "noisereduce")


def get_denoiser_func(denoiser: Optional[str], key: str):
    """audio/__init__.py:26-33"""
    if denoiser is None:
        return None
    if denoiser not in REFERENCE_DENOISERS:
        raise NotImplementedError(f'"{denoiser}" is not one of the supported denoisers: {REFERENCE_DENOISERS}.')
    if denoiser not in SUPPORTED_DENOISERS:
        from .audio_io import reject_denoiser
        reject_denoiser(denoiser)
    assert key in ("run", "load", "access")
    return SUPPORTED_DENOISERS[denoiser][key]
