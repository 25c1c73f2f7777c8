"""``swx_spectral_gate`` (csrc/swx_denoise.hip) and ``denoiser="noisereduce"`` on hardware.

The kernels are compared with the f64 evaluation of the statement in tests/spectral_gate_ref.py.  The tolerance is measured, not
chosen: for every input the f32 CPU evaluation of the same statement gives ``floor = max|y_f32cpu - y_f64|`` and the device may
be ``max(8 floor, 2^-20 max|y_f64|)`` away -- a factor 8 for another transform factorisation and summation order (both f32
rounding), and a lower limit because at two frames the CPU lands within half an ulp by luck, which is no yardstick.  Each test
prints its figures before it asserts.  Beyond accuracy: the output is the same bits for every block size of the walk over the
recording, for a row alone and among others, and from run to run; the scratch does not grow with the length; a NaN blanks exactly
the samples it blanks in the statement.  Then the Python layer: ``noisereduce_audio``, ``prep_audio``, ``AudioLoader`` and the
entry points that take ``denoiser=`` (tiny.en, seeded random weights, f32).
"""
import ctypes
import os
import warnings

import numpy as np
import pytest
import torch

import spectral_gate_ref as sg

pytestmark = pytest.mark.gpu

_REF = {}
_ROWS = {}
_CACHE = {}


def _lib():
    from stable_ts_amd import _lib
    return _lib.load()


def _row(kind, n):
    """seeded input rows, made once: 'randn' = 0.1 randn, 'bursts' = the bursts-plus-noise row (n = 160 000)"""
    if (kind, n) not in _ROWS:
        if kind == "randn":
            _ROWS[(kind, n)] = (0.1 * torch.randn(n, generator=torch.Generator().manual_seed(1000 + n))).float()
        elif kind == "zeros":
            _ROWS[(kind, n)] = torch.zeros(n)
        else:
            row = sg.bursts_plus_noise(n // sg.SR)[0]
            if kind == "bursts_nan":
                row = row.clone()
                row[80000] = float("nan")
            _ROWS[(kind, n)] = row
    return _ROWS[(kind, n)]


def _ref(kind, n, options):
    """(y_f64, floor, tolerance) of a row under the statement, computed once and left unchanged"""
    key = (kind, n, tuple(sorted(options.items())))
    if key not in _REF:
        x = _row(kind, n)
        y64 = sg.gate(x, torch.float64, **options)
        y32 = sg.gate(x, torch.float32, **options)
        floor = float((y32.double() - y64).abs().max())
        _REF[key] = (y64, floor, max(8 * floor, 2.0 ** -20 * float(y64.abs().max())))
    return _REF[key]


def _gate_raw(rows, options, block=0, in_pad=0, out_pad=0, scratch_cut=0):
    """the C entry on f32 rows [R][n] (CPU tensor) with row strides n + pad -> (return code, output [R][n] CPU tensor)"""
    from stable_ts_amd import _lib as L
    from stable_ts_amd.denoise import gate_config
    lib = _lib()
    rows = rows[None] if rows.dim() == 1 else rows
    R, n = rows.shape
    cfg = L.swx_gate_cfg(**gate_config(options, sg.SR))
    assert lib.swx_test_spectral_gate_block(block) == 0
    try:
        x = torch.full((R, n + in_pad), float("nan"), device="cuda")
        x[:, :n] = rows.cuda()
        out = torch.full((R, n + out_pad), 7.0, device="cuda")
        nbytes = lib.swx_spectral_gate_scratch_bytes(R, ctypes.byref(cfg))
        assert nbytes > 0
        scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        rc = lib.swx_spectral_gate(ctypes.c_void_p(x.data_ptr()), n + in_pad, R, n, ctypes.byref(cfg), ctypes.c_void_p(out.data_ptr()),
                                   n + out_pad, ctypes.c_void_p(scratch.data_ptr()), nbytes - scratch_cut,
                                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        if rc == 0 and out_pad:
            assert bool((out[:, n:] == 7.0).all()), "wrote past the row"
        return rc, out[:, :n].cpu()
    finally:
        lib.swx_test_spectral_gate_block(0)


def _check(kind, n, options, label):
    y64, floor, tol = _ref(kind, n, options)
    rc, y = _gate_raw(_row(kind, n), options)
    assert rc == 0
    err = float((y[0].double() - y64).abs().max())
    print(f"ACCURACY {label} kind={kind} n={n} frames={sg.n_frames(n, options.get('n_fft', 512))} floor={floor:.3e} "
          f"tol={tol:.3e} gpu_err={err:.3e} max_abs={float(y64.abs().max()):.3e}")
    assert bool(torch.isfinite(y).all())
    assert err <= tol, (label, kind, n, err, tol, floor)
    return err


LENGTHS = (1, 127, 128, 129, 511, 512, 513, 32000, 32001, 160000, 480000)


@pytest.mark.parametrize("n", LENGTHS)
def test_kernel_matches_statement_n_fft_512(n):
    _check("randn", n, {}, "default")


def test_kernel_matches_statement_on_bursts_plus_noise():
    _check("bursts", 160000, {}, "default")


@pytest.mark.parametrize("n_fft", (256, 1024))
@pytest.mark.parametrize("n", (129, 32001, 160000))
def test_kernel_matches_statement_other_n_fft(n_fft, n):
    _check("randn", n, dict(n_fft=n_fft), f"n_fft={n_fft}")


@pytest.mark.parametrize("name,options", [
    ("prop_half", dict(prop_decrease=0.5)),
    ("freq_none", dict(freq_mask_smooth_hz=None)),
    ("time_none", dict(time_mask_smooth_ms=None)),
    ("both_none", dict(freq_mask_smooth_hz=None, time_mask_smooth_ms=None)),
])
def test_kernel_matches_statement_options(name, options):
    _check("randn", 32001, options, name)
    _check("bursts", 160000, options, name)


@pytest.mark.parametrize("n", (1, 127, 129, 513, 32001, 160000))
def test_identity_without_smoothing_and_decrease(n):
    options = dict(freq_mask_smooth_hz=None, time_mask_smooth_ms=None, prop_decrease=0.0)
    _, floor, tol = _ref("randn", n, options)
    x = _row("randn", n)
    rc, y = _gate_raw(x, options)
    assert rc == 0
    err = float((y[0].double() - x.double()).abs().max())
    print(f"IDENTITY n={n} floor={floor:.3e} tol={tol:.3e} gpu_err={err:.3e}")
    assert err <= tol


@pytest.mark.parametrize("n", (7936, 8064, 8191, 8192, 8193, 16384, 160000))
def test_block_size_does_not_change_a_bit(n):
    """F = 63, 64, 65, 65, 66, 129 and 1251 frames, walked 16, 64 and 4096 hops at a time"""
    x = _row("randn", n)
    outs = []
    for block in (16, 64, 0):
        rc, y = _gate_raw(x, {}, block=block)
        assert rc == 0
        outs.append(y.numpy())
    assert np.array_equal(outs[0], outs[2]) and np.array_equal(outs[1], outs[2])
    y64, _, tol = _ref("randn", n, {})
    assert float((torch.from_numpy(outs[2][0]).double() - y64).abs().max()) <= tol


def test_blocks_with_other_options_and_runs_repeat():
    x = _row("bursts", 160000)
    for options in (dict(n_fft=1024), dict(n_fft=256, time_mask_smooth_ms=None), dict(time_constant_s=0.1)):
        a = _gate_raw(x, options, block=16)[1].numpy()
        b = _gate_raw(x, options, block=0)[1].numpy()
        c = _gate_raw(x, options, block=0)[1].numpy()
        assert np.array_equal(a, b) and np.array_equal(b, c), options


def test_rows_are_independent_with_padded_strides():
    n = 8193
    rows = torch.stack([_row("randn", n), _row("bursts", 160000)[40000:40000 + n], _row("zeros", n)])
    rc, together = _gate_raw(rows, {}, in_pad=37, out_pad=5)
    assert rc == 0
    for r in range(3):
        rc, alone = _gate_raw(rows[r], {})
        assert rc == 0
        assert np.array_equal(together[r].numpy(), alone[0].numpy()), r
    rc, odd = _gate_raw(rows, {}, in_pad=1, out_pad=3, block=16)            # rows off the 16-byte grid
    assert rc == 0 and np.array_equal(odd.numpy(), together.numpy())


def test_scratch_is_bounded_and_checked():
    from stable_ts_amd import _lib as L
    from stable_ts_amd.denoise import gate_config
    lib = _lib()
    cfg = L.swx_gate_cfg(**gate_config({}, sg.SR))
    one, two = lib.swx_spectral_gate_scratch_bytes(1, ctypes.byref(cfg)), lib.swx_spectral_gate_scratch_bytes(2, ctypes.byref(cfg))
    assert 0 < one < two < 256 << 20                 # per row, and no function of the length (the call takes none)
    assert lib.swx_test_spectral_gate_block(16) == 0
    small = lib.swx_spectral_gate_scratch_bytes(1, ctypes.byref(cfg))
    assert lib.swx_test_spectral_gate_block(0) == 0
    assert 0 < small < one
    x = _row("randn", 32000)
    rc, _ = _gate_raw(x, {}, scratch_cut=1)
    assert rc < 0 and lib.swx_strerror(rc) == b"invalid argument"
    rc, y = _gate_raw(x, {})
    assert rc == 0


def test_bad_arguments_are_refused_before_any_launch():
    from stable_ts_amd import _lib as L
    from stable_ts_amd.denoise import gate_config
    lib = _lib()
    good = gate_config({}, sg.SR)
    x = torch.zeros(4096, device="cuda")
    out = torch.full((4096,), 7.0, device="cuda")
    scratch = torch.empty(lib.swx_spectral_gate_scratch_bytes(1, ctypes.byref(L.swx_gate_cfg(**good))), dtype=torch.uint8, device="cuda")

    def call(cfg, src=x, dst=out, n=4096, rows=1):
        c = L.swx_gate_cfg(**cfg)
        return lib.swx_spectral_gate(ctypes.c_void_p(src.data_ptr()), 4096, rows, n, ctypes.byref(c), ctypes.c_void_p(dst.data_ptr()),
                                     4096, ctypes.c_void_p(scratch.data_ptr()), scratch.numel(), None)

    for bad in (dict(good, n_fft=300), dict(good, n_mean=0), dict(good, n_grad_freq=0), dict(good, n_grad_time=129),
                dict(good, thresh=float("nan"))):
        assert lib.swx_strerror(call(bad)) == b"invalid argument", bad
        assert lib.swx_spectral_gate_scratch_bytes(1, ctypes.byref(L.swx_gate_cfg(**bad))) == 0
    assert lib.swx_strerror(call(good, dst=x)) == b"invalid argument"       # in place
    assert lib.swx_strerror(call(good, n=0)) == b"invalid argument"
    assert lib.swx_strerror(call(good, rows=0)) == b"invalid argument"
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert call(good) == 0
    torch.cuda.synchronize()
    assert bool((out == 0.0).all())


def test_nan_blanks_what_it_blanks_in_the_statement():
    y64, floor, tol = _ref("bursts_nan", 160000, {})
    rc, y = _gate_raw(_row("bursts_nan", 160000), {})
    assert rc == 0
    want = (y64 == 0).nonzero().flatten()
    got = (y[0] == 0).nonzero().flatten()
    assert int(want.min()) == 62848 and int(want.max()) == 97151 and len(want) == 34304
    assert torch.equal(got, want)
    assert bool(torch.isfinite(y).all())
    err = float((y[0].double() - y64).abs().max())
    print(f"NAN floor={floor:.3e} tol={tol:.3e} gpu_err={err:.3e}")
    assert err <= tol


def test_zeros_in_zeros_out():
    rc, y = _gate_raw(_row("zeros", 4000), {})
    assert rc == 0 and bool((y == 0).all())


def test_noise_only_attenuation_matches_the_statement():
    x, q, noise = sg.bursts_plus_noise(10)
    y64 = _ref("bursts", 160000, {})[0]
    rc, y = _gate_raw(x, {})
    assert rc == 0
    want, got = sg.attenuation_db(y64, q, noise), sg.attenuation_db(y[0], q, noise)
    print(f"EFFECT statement={want:.3f} dB gpu={got:.3f} dB")
    assert want <= -25.0
    assert abs(got - want) <= 0.05


# ------------------------------------------------------------------------------------------------------- the Python layer
HERE = os.path.dirname(os.path.abspath(__file__))
TEXT = " the quick brown fox jumps over the lazy dog"


def _synth_audio(seconds, seed):
    if "synth" not in _CACHE:
        import importlib.util
        spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "golden", "make_golden.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        _CACHE["synth"] = mod.synth_audio
    return torch.as_tensor(_CACHE["synth"](seconds, seed), dtype=torch.float32)


def _noisy(seconds, seed):
    if ("noisy", seconds, seed) not in _CACHE:
        a = _synth_audio(seconds, seed)
        _CACHE[("noisy", seconds, seed)] = a + 0.02 * torch.randn(a.shape, generator=torch.Generator().manual_seed(seed))
    return _CACHE[("noisy", seconds, seed)]


def _model():
    import stable_ts_amd as sw
    if "model" not in _CACHE:
        dims = sw.dims_for("tiny.en")
        m = sw.Whisper(dims, dtype="f32", max_windows=1, max_rows=5)
        m.load_state_dict(sw.random_state_dict(dims, seed=1234, std=0.02, embed_gain=2.0, ts_gain=0.5))
        _CACHE["model"] = m
    return _CACHE["model"]


def test_prep_audio_is_noisereduce_audio_and_keeps_the_residence():
    from stable_ts_amd.audio_io import prep_audio
    from stable_ts_amd.denoise import noisereduce_audio
    x = _noisy(6.0, 71)
    want = noisereduce_audio(x, input_sr=16000)
    got = prep_audio(x, denoiser="noisereduce")
    assert not want.is_cuda and not got.is_cuda and got.dtype == torch.float32 and got.shape == x.shape
    assert torch.equal(got, want)
    assert torch.equal(prep_audio(x.numpy(), denoiser="noisereduce"), want)
    on_device = prep_audio(x.cuda(), denoiser="noisereduce")
    assert on_device.is_cuda and torch.equal(on_device.cpu(), want)
    y64 = sg.gate(x)
    floor = float((sg.gate(x, torch.float32).double() - y64).abs().max())
    assert float((want.double() - y64).abs().max()) <= max(8 * floor, 2.0 ** -20 * float(y64.abs().max()))
    # the voice-band filter runs after the gate (audio/__init__.py:146-147)
    from stable_ts_amd.audio_io import voice_freq_filter
    assert torch.equal(prep_audio(x, denoiser="noisereduce", only_voice_freq=True), voice_freq_filter(want, 16000))


def test_two_rows_are_gated_apiece_and_averaged():
    from stable_ts_amd.denoise import noisereduce_audio
    a, b = _noisy(6.0, 71), _noisy(6.0, 72)
    both = noisereduce_audio(torch.stack([a, b]), input_sr=16000)
    ya, yb = noisereduce_audio(a.cuda(), input_sr=16000), noisereduce_audio(b.cuda(), input_sr=16000)
    assert both.shape == a.shape and not both.is_cuda
    assert torch.equal(both, torch.stack([ya, yb]).mean(dim=0).cpu())


def test_denoiser_options_reach_the_kernel():
    from stable_ts_amd.audio_io import prep_audio
    x = _noisy(6.0, 71)
    off = dict(prop_decrease=0.0, freq_mask_smooth_hz=None, time_mask_smooth_ms=None)
    y64 = sg.gate(x, **off)
    floor = float((sg.gate(x, torch.float32, **off).double() - y64).abs().max())
    got = prep_audio(x, denoiser="noisereduce", denoiser_options=off)
    assert float((got.double() - x.double()).abs().max()) <= max(8 * floor, 2.0 ** -20 * float(y64.abs().max()))
    half = prep_audio(x, denoiser="noisereduce", denoiser_options=dict(prop_decrease=0.5))
    assert not torch.equal(half, prep_audio(x, denoiser="noisereduce"))
    with pytest.raises(TypeError):
        prep_audio(x, denoiser="noisereduce", denoiser_options=dict(no_such_option=1))


def test_entry_points_take_the_denoiser():
    from stable_ts_amd.audio_io import prep_audio
    from stable_ts_amd.result import WhisperResult
    model = _model()
    x, x2 = _noisy(6.0, 71).cuda(), _noisy(5.0, 73)
    clean, clean2 = prep_audio(x, denoiser="noisereduce"), prep_audio(x2, denoiser="noisereduce")
    assert not torch.equal(clean, x)
    # greedy and no fallback ladder: random weights fail every threshold and the sampled retries would draw from torch's generator
    kw = dict(language="en", verbose=None, temperature=0.0, logprob_threshold=None, compression_ratio_threshold=None,
              no_speech_threshold=None)
    want = model.transcribe(clean, **kw).to_dict()
    assert want["segments"]
    assert model.transcribe(x, denoiser="noisereduce", **kw).to_dict() == want
    many = model.transcribe_many([x, x2], denoiser="noisereduce", max_tracks=2, **kw)
    assert [r.to_dict() for r in many] == [r.to_dict() for r in model.transcribe_many([clean, clean2], max_tracks=2, **kw)]
    assert many[0].to_dict() == want

    aligned = model.align(clean, TEXT, language="en")
    assert model.align(x, TEXT, language="en", denoiser="noisereduce").to_dict() == aligned.to_dict()
    opts = dict(prop_decrease=0.5)
    half = prep_audio(x, denoiser="noisereduce", denoiser_options=opts)
    assert (model.align(x, TEXT, language="en", denoiser="noisereduce", denoiser_options=opts).to_dict()
            == model.align(half, TEXT, language="en").to_dict())

    refined = model.refine(clean, WhisperResult(aligned.to_dict()), verbose=None)
    assert model.refine(x, WhisperResult(aligned.to_dict()), verbose=None, denoiser="noisereduce").to_dict() == refined.to_dict()

    def flat(matches):
        return [m.to_dict() if hasattr(m, "to_dict") else m for m in matches]

    tokens = [t for w in aligned.all_words()[:2] for t in w.tokens]
    found = flat(model.locate(clean, tokens, "en", probability_threshold=0.0, verbose=None))
    assert flat(model.locate(x, tokens, "en", probability_threshold=0.0, verbose=None, denoiser="noisereduce")) == found


def test_stream_loader_denoises_every_block(tmp_path):
    from stable_ts_amd.audio_io import AudioLoader, load_audio, write_wav
    from stable_ts_amd.denoise import noisereduce_audio
    path = str(tmp_path / "noisy.wav")
    write_wav(path, _noisy(6.0, 74)[:56000], 16000)
    x = torch.from_numpy(load_audio(path))
    assert x.shape[-1] == 56000
    whole = noisereduce_audio(x, input_sr=16000)
    with AudioLoader(path, stream=True, denoiser="noisereduce", buffer_size=16000, new_chunk_divisor=None) as loader:
        assert loader.validate_external_args(denoiser="noisereduce")[1] == "noisereduce"
        for seek in range(0, 56000, 16000):
            chunk = loader.next_chunk(seek)
            want = noisereduce_audio(x[seek:seek + 16000], input_sr=16000)
            assert not chunk.is_cuda and torch.equal(chunk, want), seek
            assert not torch.equal(chunk, whole[seek:seek + 16000]), seek
        assert loader.next_chunk(56000) is None
    with AudioLoader(path, stream=False, denoiser="noisereduce") as loader:        # held whole: gated once
        assert torch.equal(loader.next_chunk(16000, 16000), whole[16000:32000])


def test_save_path_writes_the_denoised_audio(tmp_path):
    from stable_ts_amd.audio_io import AudioLoader, read_wav
    from stable_ts_amd.denoise import noisereduce_audio
    x = _noisy(6.0, 71)
    path = str(tmp_path / "denoised.wav")
    y = noisereduce_audio(x, input_sr=16000, save_path=path, verbose=None)
    back, sr = read_wav(path)
    assert sr == 16000 and back.shape == (x.shape[-1], 1)
    assert float((torch.from_numpy(back[:, 0]) - y).abs().max()) <= 1.0 / 32768
    seen = []
    noisereduce_audio(x, input_sr=16000, save_path=lambda audio, sr: seen.append((audio, sr)))
    assert len(seen) == 1 and torch.equal(seen[0][0], y)
    path2 = str(tmp_path / "from_loader.wav")
    with AudioLoader(x, denoiser="noisereduce", denoiser_options=dict(save_path=path2)) as loader:
        assert torch.equal(loader.next_chunk(0, 16000), y[:16000])
    back2, _ = read_wav(path2)
    assert float((torch.from_numpy(back2[:, 0]) - y).abs().max()) <= 1.0 / 32768
