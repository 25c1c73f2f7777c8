"""The statement of the spectral gate (tests/spectral_gate_ref.py) checked against a literal evaluation and
against the facts recorded with it, the host half of ``denoiser="noisereduce"`` (``denoise.gate_config``) and the wiring that
needs no device.  The device half: tests/test_gpu_spectral_gate.py."""
import warnings

import numpy as np
import pytest
import torch

import spectral_gate_ref as sg


def _randn(n, seed=0):
    return 0.1 * torch.randn(n, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


@pytest.mark.parametrize("options", [
    dict(n_fft=256),
    dict(n_fft=256, time_constant_s=0.05),                       # M = 12 < F: an even window with 5 frames before, 6 after
    dict(n_fft=256, time_constant_s=0.052, prop_decrease=0.5),    # M = 13
    dict(n_fft=256, freq_mask_smooth_hz=None),
    dict(n_fft=256, time_mask_smooth_ms=None),
    dict(n_fft=256, freq_mask_smooth_hz=None, time_mask_smooth_ms=None),
])
def test_literal_dft_evaluation_equals_the_statement(options):
    for n in (300, 1500):
        x = _randn(n, n)
        lit = sg.gate_literal(x.numpy(), **options)
        got = sg.gate(x, **options).numpy()
        assert sg.n_frames(n, 256) == -(-n // 64) + 1
        assert np.abs(lit - got).max() <= 1e-10, (options, n)


def test_default_filter_is_17_by_13_symmetric_and_sums_to_one():
    M, n_f, n_t = sg.widths()
    assert (M, n_f, n_t) == (250, 8, 6)
    k = sg.smoothing_filter(n_f, n_t)
    assert tuple(k.shape) == (17, 13)
    assert torch.equal(k, k.flip(0)) and torch.equal(k, k.flip(1))
    assert abs(float(k.sum()) - 1.0) <= 1e-15
    assert float(k[8, 6]) == float(k.max())
    assert tuple(sg.smoothing_filter(None, n_t).shape) == (3, 13) and tuple(sg.smoothing_filter(n_f, None).shape) == (17, 3)
    assert sg.smoothing_filter(None, None) is None
    assert torch.equal(sg.triangle(1), torch.tensor([0.5, 1.0, 0.5], dtype=torch.float64))


@pytest.mark.parametrize("n", (1, 127, 128, 129, 511, 513, 4000, 32001))
def test_identity_without_smoothing_and_decrease(n):
    x = _randn(n, n)
    y = sg.gate(x, freq_mask_smooth_hz=None, time_mask_smooth_ms=None, prop_decrease=0.0)
    assert float((y - x).abs().max()) <= 1e-12


def test_frame_counts_and_f32_floor():
    lengths = (1, 127, 128, 129, 511, 513, 32000, 32001, 160000)
    assert [sg.n_frames(n) for n in lengths] == [2, 2, 2, 3, 5, 6, 251, 252, 1251]
    for n in lengths[:8]:
        x = _randn(n, n)
        y64, y32 = sg.gate(x), sg.gate(x.float(), torch.float32)
        assert y64.shape == (n,) and y32.dtype == torch.float32
        assert float((y32.double() - sg.gate(x.float())).abs().max()) <= 1e-6


def test_bursts_plus_noise_is_attenuated_and_nan_blanks_a_known_range():
    x, q, noise = sg.bursts_plus_noise(10)
    y = sg.gate(x)
    db = sg.attenuation_db(y, q, noise)
    assert db <= -25.0, db
    bad = x.clone()
    bad[80000] = float("nan")
    yn = sg.gate(bad)
    zero = (yn == 0).nonzero().flatten()
    assert (int(zero.min()), int(zero.max()), len(zero)) == (62848, 97151, 34304)
    assert bool(torch.isfinite(yn).all())
    assert float(sg.gate(torch.zeros(4000)).abs().max()) == 0.0


def test_gate_config_widths_and_refusals():
    from stable_ts_amd.denoise import gate_config
    c = gate_config({}, 16000)
    assert (c["n_fft"], c["n_mean"], c["n_grad_freq"], c["n_grad_time"]) == (512, 250, 8, 6)
    assert (c["thresh"], c["slope"], c["prop_decrease"]) == (2.0, 10.0, 1.0)
    c = gate_config(dict(n_fft=1024), 16000)
    assert (c["n_mean"], c["n_grad_freq"], c["n_grad_time"]) == (125, 16, 3)
    c = gate_config(dict(freq_mask_smooth_hz=None), 16000)
    assert (c["n_grad_freq"], c["n_grad_time"]) == (1, 6)
    c = gate_config(dict(freq_mask_smooth_hz=None, time_mask_smooth_ms=None, prop_decrease=0.25), 16000)
    assert (c["n_grad_freq"], c["n_grad_time"], c["prop_decrease"]) == (0, 0, 0.25)
    for o in ({}, dict(n_fft=256), dict(n_fft=1024, time_constant_s=0.5)):                       # the statement's own widths
        c, (M, n_f, n_t) = gate_config(o, 16000), sg.widths(**o)
        assert (c["n_mean"], c["n_grad_freq"], c["n_grad_time"]) == (M, n_f, n_t)
    ignored = dict(progress=True, use_tqdm=True, n_jobs=4, chunk_size=600000, padding=30000, use_torch=True, tmp_folder=None,
                   device="cuda", sr=16000, stationary=False, win_length=512, hop_length=128, y_noise=None)
    assert gate_config(ignored, 16000) == gate_config({}, 16000)
    for bad in (dict(stationary=True), dict(y_noise=np.zeros(4)), dict(win_length=400), dict(hop_length=64), dict(n_fft=2048)):
        with pytest.raises(NotImplementedError):
            gate_config(bad, 16000)
    with pytest.raises(TypeError, match="clip_noise_stationary"):
        gate_config(dict(clip_noise_stationary=True), 16000)
    for bad in (dict(freq_mask_smooth_hz=10), dict(time_mask_smooth_ms=4), dict(time_constant_s=0.001), dict(sr=8000)):
        with pytest.raises(ValueError):
            gate_config(bad, 16000)


def test_wiring_that_needs_no_device(tmp_path):
    from stable_ts_amd.audio_io import AudioLoader, prep_audio
    from stable_ts_amd.denoise import SUPPORTED_DENOISERS, get_denoiser_func, load_noisereduce_model, noisereduce_audio
    from stable_ts_amd.transcribe import pop_audio_options
    x = torch.zeros(1600)
    with pytest.raises(NotImplementedError, match="model files"):
        prep_audio(x, denoiser="dfnet")
    with pytest.raises(NotImplementedError, match="model files"):
        prep_audio(x, demucs=True)
    sentence = "\"spleeter\" is not one of the supported denoisers: ('demucs', 'dfnet', 'noisereduce')."
    for call in (lambda: prep_audio(x, denoiser="spleeter"), lambda: get_denoiser_func("spleeter", "run"),
                 lambda: pop_audio_options(dict(denoiser="spleeter")), lambda: AudioLoader(x, denoiser="spleeter")):
        with pytest.raises(NotImplementedError) as e:
            call()
        assert str(e.value) == sentence
    assert get_denoiser_func(None, "run") is None
    assert get_denoiser_func("noisereduce", "run") is noisereduce_audio and "noisereduce" in SUPPORTED_DENOISERS
    assert load_noisereduce_model().samplerate == 16000

    opts = dict(denoiser="noisereduce", denoiser_options=dict(prop_decrease=0.5), only_voice_freq=True, stream=True, beam_size=5)
    assert pop_audio_options(opts) == dict(only_voice_freq=True, denoiser="noisereduce", denoiser_options=dict(prop_decrease=0.5))
    assert opts == dict(beam_size=5)
    assert pop_audio_options(dict(denoiser_options=dict(prop_decrease=0.5))) == dict(only_voice_freq=False)
    with pytest.raises(NotImplementedError, match="model files"):
        pop_audio_options(dict(denoiser="demucs"))

    loader = AudioLoader(x)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        got = loader.validate_external_args(denoiser="noisereduce", denoiser_options=dict(prop_decrease=0.5))
    said = [str(w.message) for w in caught]
    assert any("``denoiser`` will have no effect unless specified at AudioLoader initialization." in m for m in said)
    assert any("``denoiser_options`` does not match" in m for m in said)
    assert got == (False, None, {}, False)

    # refusals of the options and of the arguments come before any device work
    with pytest.raises(NotImplementedError):
        noisereduce_audio(x, input_sr=16000, stationary=True)
    with pytest.raises(ValueError, match="conflicting"):
        noisereduce_audio(x, input_sr=16000, sr=8000)
    with pytest.raises(ValueError, match="No ``input_sr``"):
        noisereduce_audio(x)
    if not torch.cuda.is_available():                                    # no CPU path, as everywhere in this package
        from stable_ts_amd._lib import SwxError
        with pytest.raises(SwxError):
            prep_audio(x, denoiser="noisereduce")
