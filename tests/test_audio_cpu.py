"""Audio front-end (stable_ts_amd/audio_io.py): WAVE decoding, resampling, voice-band filter and AudioLoader.

* AudioLoader is driven with the same randomly generated call sequences as the reference's own class
  (stable_whisper/audio/__init__.py:152-638) -- in-memory sources directly, streamed sources through a stand-in for the
  ffmpeg child process on the reference side and the PCM stream hook on this side -- and every returned chunk, seek and
  estimate must be equal.  (The reference's results are recorded in tests/golden/audioloader_cases.json.gz; the comparison
  also runs live where the reference checkout is importable.)
* decoding / resampling / filtering have no runnable reference here (ffmpeg and torchaudio are absent): they are checked
  against independent implementations (stdlib ``wave``, ``scipy.signal.resample_poly``, a direct-form recurrence).
"""
import io
import math
import os
import struct
import sys
import wave

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

from stable_ts_amd import audio_io as AIO  # noqa: E402
from stable_ts_amd.audio_io import AudioLoader, load_audio, read_wav, resample, resample_blocks, voice_freq_filter  # noqa: E402

HAVE_REF = os.path.isdir("/root/reference/stable_whisper")


# ------------------------------------------------------------------------------------------------------------ WAVE
def _wav_bytes(fmt_tag, bits, channels, sr, payload, extensible=False, extra_chunk=True):
    block = channels * bits // 8
    if extensible:
        guid = struct.pack("<H", fmt_tag) + bytes.fromhex("000000001000800000aa00389b71")
        fmt = struct.pack("<HHIIHH", 0xFFFE, channels, sr, sr * block, block, bits) + struct.pack("<HHI", 22, bits, 3) + guid
    else:
        fmt = struct.pack("<HHIIHH", fmt_tag, channels, sr, sr * block, block, bits)
    chunks = b"fmt " + struct.pack("<I", len(fmt)) + fmt
    if extra_chunk:
        chunks += b"LIST" + struct.pack("<I", 5) + b"hello" + b"\0"            # odd-sized chunk + pad byte
    chunks += b"data" + struct.pack("<I", len(payload)) + payload
    return b"RIFF" + struct.pack("<I", 4 + len(chunks)) + b"WAVE" + chunks


def test_read_wav_formats():
    g = np.random.default_rng(0)
    ints = g.integers(-32768, 32768, size=(1000, 2)).astype("<i2")
    data, sr = read_wav(_wav_bytes(1, 16, 2, 22050, ints.tobytes()))
    assert sr == 22050 and data.shape == (1000, 2) and np.array_equal(data, ints.astype(np.float32) / 32768.0)
    # the same file through the stdlib reader
    with wave.open(io.BytesIO(_wav_bytes(1, 16, 2, 22050, ints.tobytes())), "rb") as w:
        assert np.array_equal(np.frombuffer(w.readframes(1000), "<i2").reshape(-1, 2), ints)
    u8 = g.integers(0, 256, size=(500, 1)).astype(np.uint8)
    data, _ = read_wav(_wav_bytes(1, 8, 1, 8000, u8.tobytes()))
    assert np.array_equal(data, (u8.astype(np.float32) - 128) / 128)
    i24 = g.integers(-(1 << 23), 1 << 23, size=(300, 2))
    raw = b"".join(int(v).to_bytes(3, "little", signed=True) for v in i24.reshape(-1))
    data, _ = read_wav(_wav_bytes(1, 24, 2, 48000, raw, extensible=True))
    assert np.array_equal(data, (i24 / 8388608.0).astype(np.float32))
    i32 = g.integers(-(1 << 31), 1 << 31, size=(100, 1)).astype("<i4")
    data, _ = read_wav(_wav_bytes(1, 32, 1, 16000, i32.tobytes()))
    assert np.allclose(data, i32 / 2147483648.0, atol=1e-7)
    f32 = g.standard_normal((200, 2)).astype("<f4")
    data, _ = read_wav(_wav_bytes(3, 32, 2, 16000, f32.tobytes(), extensible=True))
    assert np.array_equal(data, f32)
    f64 = g.standard_normal((50, 1)).astype("<f8")
    data, _ = read_wav(_wav_bytes(3, 64, 1, 16000, f64.tobytes()))
    assert np.array_equal(data, f64.astype(np.float32))
    # open-ended data chunk (size field 0xFFFFFFFF as streaming writers leave it) and a truncated one
    b = bytearray(_wav_bytes(1, 16, 1, 16000, ints[:, 0].tobytes(), extra_chunk=False))
    b[40:44] = b"\xff\xff\xff\xff"
    assert read_wav(bytes(b))[0].shape == (1000, 1)
    assert read_wav(bytes(b[:-501]))[0].shape == (749, 1)
    for bad in (b"", b"RIFF1234WAVE", b"OggS" + bytes(100), _wav_bytes(2, 4, 1, 16000, bytes(64))):
        with pytest.raises(RuntimeError):
            read_wav(bad)


def test_load_audio_wav_paths(tmp_path):
    g = np.random.default_rng(1)
    mono16 = (g.standard_normal(16000) * 3000).astype("<i2")
    p = str(tmp_path / "a.wav")
    with wave.open(p, "wb") as w:
        w.setnchannels(1), w.setsampwidth(2), w.setframerate(16000)
        w.writeframes(mono16.tobytes())
    # 16 kHz mono s16: exactly what ``ffmpeg -f s16le -ac 1 -ar 16000`` hands the reference (audio/utils.py:120-123)
    want = mono16.astype(np.float32) / 32768.0
    assert np.array_equal(load_audio(p), want)
    assert np.array_equal(load_audio(open(p, "rb").read()), want)
    assert AIO.get_metadata(p) == dict(sr=16000, duration=1.0)
    # stereo 44.1 kHz: down-mix, resample, s16 grid; stereo output keeps both channels
    t = np.arange(44100) / 44100.0
    st = np.stack([0.4 * np.sin(2 * np.pi * 300 * t), 0.2 * np.sin(2 * np.pi * 1200 * t)], 1)
    raw = AIO.to_s16(st.reshape(-1)).tobytes()
    blob = _wav_bytes(1, 16, 2, 44100, raw)
    y = load_audio(blob)
    assert y.shape == (16000,) and y.dtype == np.float32 and np.array_equal(y * 32768, np.rint(y * 32768))
    t16 = np.arange(16000) / 16000.0
    want = 0.2 * np.sin(2 * np.pi * 300 * t16) + 0.1 * np.sin(2 * np.pi * 1200 * t16)
    assert np.abs(y[200:-200] - want[200:-200]).max() < 2e-3
    y2 = load_audio(blob, mono=False)
    assert y2.shape == (2, 16000) and np.abs(y2[0, 200:-200] - 0.4 * np.sin(2 * np.pi * 300 * t16)[200:-200]).max() < 2e-3
    with pytest.raises(NotImplementedError):
        load_audio("https://example.com/a.mp3")
    if AIO.shutil.which("ffmpeg") is None:
        with pytest.raises(RuntimeError):
            load_audio(b"ID3" + bytes(64))


@pytest.mark.skipif(not os.path.isfile("/root/reference/examples/demo.wav"), reason="reference checkout not present")
def test_demo_wav_config0_front_end():
    # BASELINE.json configs[0]: examples/demo.wav (stereo 44.1 kHz s16) -> 16 kHz mono; independent polyphase resampler
    from scipy.signal import resample_poly
    p = "/root/reference/examples/demo.wav"
    with wave.open(p, "rb") as w:
        sr, ch, n = w.getframerate(), w.getnchannels(), w.getnframes()
        x = np.frombuffer(w.readframes(n), "<i2").astype(np.float64).reshape(-1, ch).mean(1) / 32768.0
    y = load_audio(p)
    assert y.shape == (math.ceil(n * 16000 / sr),)
    ref = resample_poly(x, 160, 441)[: len(y)]
    a, b = y[500:-500], ref[500:-500]
    # the two filters differ in their transition band just below 8 kHz; the bar is on the energy of the difference
    rel = float(np.sqrt(np.mean((a - b) ** 2) / np.mean(b ** 2)))
    assert rel < 0.02 and np.corrcoef(a, b)[0, 1] > 0.9995, rel


# ------------------------------------------------------------------------------------------------------- resampling
@pytest.mark.parametrize("a,b,n", [(44100, 16000, 100003), (48000, 16000, 50000), (8000, 16000, 12345),
                                   (22050, 16000, 441 * 7), (16000, 16000, 1000), (44100, 16000, 5), (11025, 16000, 0)])
def test_resample_lengths_and_streaming(a, b, n):
    g = np.random.default_rng(n)
    x = g.standard_normal(n).astype(np.float32)
    y = resample(torch.from_numpy(x), a, b).numpy()
    assert len(y) == math.ceil(n * b / a)
    cuts = np.sort(g.integers(0, n + 1, size=7)) if n else []
    parts = list(resample_blocks(iter(np.split(x, cuts) if n else [x]), a, b, block_periods=16))
    z = np.concatenate(parts) if parts else np.zeros(0, np.float32)
    assert len(z) == len(y) and (len(y) == 0 or np.abs(y - z).max() < 2e-6)


def test_resample_response_and_batch():
    t = np.arange(44100) / 44100.0
    amp = {}
    for f in (1000, 5000, 15000):
        y = resample(torch.from_numpy(np.sin(2 * np.pi * f * t).astype(np.float32)), 44100, 16000).numpy()
        amp[f] = float(np.sqrt(2 * np.mean(y[2000:14000] ** 2)))
    assert abs(amp[1000] - 1) < 5e-3 and abs(amp[5000] - 1) < 1e-2 and amp[15000] < 1e-3      # alias of 15 kHz removed
    x = torch.randn(3, 2, 4410)
    y = resample(x, 44100, 16000)
    assert y.shape == (3, 2, 1600) and torch.allclose(y[1, 0], resample(x[1, 0], 44100, 16000), atol=2e-6)
    assert resample(np.arange(10), 16000, 16000).dtype == torch.float32


# ------------------------------------------------------------------------------------------------- voice-band filter
def _direct_form(x, b, a):
    y = np.zeros(len(x))
    for n in range(len(x)):
        acc = b[0] * x[n]
        if n >= 1:
            acc += b[1] * x[n - 1] - a[1] * y[n - 1]
        if n >= 2:
            acc += b[2] * x[n - 2] - a[2] * y[n - 2]
        y[n] = acc
    return y


def test_voice_freq_filter():
    sr = 16000
    g = np.random.default_rng(2)
    x = (0.1 * g.standard_normal(400)).astype(np.float32)
    got = voice_freq_filter(x, sr).numpy()

    def coeffs(kind, fc):
        w0 = 2 * math.pi * fc / sr
        al, c = math.sin(w0) / 2 / 0.707, math.cos(w0)
        b = ((1 - c) / 2, 1 - c, (1 - c) / 2) if kind == "lp" else ((1 + c) / 2, -1 - c, (1 + c) / 2)
        a0 = 1 + al
        return [v / a0 for v in b], [1.0, -2 * c / a0, (1 - al) / a0]

    want = _direct_form(_direct_form(x.astype(np.float64), *coeffs("lp", 5000)), *coeffs("hp", 200))
    assert np.abs(got - want).max() < 1e-6
    # pass band / stop bands
    t = np.arange(sr) / sr
    rms = lambda f: float(np.sqrt(2 * np.mean(voice_freq_filter((0.5 * np.sin(2 * np.pi * f * t)).astype(np.float32), sr).numpy()[4000:] ** 2)))
    assert abs(rms(1000) - 0.5) < 0.02 and rms(40) < 0.03 and rms(7800) < 0.05
    assert voice_freq_filter(torch.full((1000,), 5.0), sr).abs().max() <= 1.0           # clamp like lfilter(clamp=True)
    with pytest.raises(AssertionError):
        voice_freq_filter(x, sr, upper_freq=100, lower_freq=200)
    assert AIO.prep_audio(x, only_voice_freq=True).shape == (400,)
    same = torch.randn(10)
    assert AIO.prep_audio(same) is same
    with pytest.raises(NotImplementedError):
        AIO.prep_audio(same, denoiser="demucs")


# ------------------------------------------------------------------------------------------------------ AudioLoader
def test_audioloader_literal_cases():
    x = torch.arange(100000, dtype=torch.float32)
    L = AudioLoader(x, buffer_size=16000)
    assert not L.stream and L.sr == 16000 and L.get_duration(2) == 6.25 and L.get_total_samples() == 100000
    assert torch.equal(L.next_chunk(0), x[:16000])
    assert torch.equal(L.next_chunk(90000, 30000), x[90000:]) and L.prev_seek == 90000
    assert L.next_chunk(100000) is None
    with pytest.raises(AssertionError):
        L.next_chunk(5)
    L = AudioLoader(x, buffer_size="0.5s", load_sections=[(1.0, 2.0), (3.0, None)])
    assert L.buffer_size == 8000
    c, s = L.next_valid_chunk(0, 480000)
    assert s == 16000 and torch.equal(c, x[16000:32000]) and L.curr_load_section_index == 0
    c, s = L.next_valid_chunk(31999, 480000)                    # seek + 1 reaches the section end: next section
    assert s == 48000 and torch.equal(c, x[48000:]) and L.curr_load_section_seeks == (48000, None)
    assert L.next_valid_chunk(100000, 1)[0] is None
    assert AudioLoader.negate_ts_sections([(1.0, 2.0), (2.0, 3.0), (5.0, 6.0)]) == [(0.0, 1.0), (3.0, 5.0), (6.0, None)]
    assert AudioLoader.negate_ts_sections([(0.0, 2.0)]) == [(2.0, None)]
    with pytest.raises(ValueError):
        AudioLoader(x, buffer_size="30")
    with pytest.raises(ValueError):
        AudioLoader(x, buffer_size=-1)
    with pytest.raises(NotImplementedError):
        AudioLoader(x, stream=True)
    with pytest.raises(RuntimeError):
        AudioLoader(torch.zeros(0))
    with pytest.raises(ValueError):
        AudioLoader(x).validate_external_args(sr=8000)
    with pytest.warns(UserWarning):
        AudioLoader(x).validate_external_args(sr=16000, stream=True, only_voice_freq=True)
    with pytest.raises(NotImplementedError):
        AIO.audioloader_not_supported(AudioLoader(x))
    seen = []
    L = AudioLoader(x, post_prep_callback=None)
    L.update_post_prep_callback(lambda s: seen.append(len(s)))
    assert seen == [100000]


class _FakePopen:
    """stand-in for the reference's ffmpeg child: s16le bytes on stdout, poll() turns 0 once they are consumed"""

    def __init__(self, data: bytes):
        self.stdout = io.BytesIO(data)
        self._n = len(data)

    def poll(self):
        return 0 if self.stdout.tell() >= self._n else None

    def terminate(self):
        pass


def _drive(loader, ops):
    out, floor = [], 0
    for kind, seek, size in ops:
        seek = max(seek, floor)                                 # a section jump moved the loader past the planned seek
        if kind == "chunk":
            c = loader.next_chunk(seek, size)
            out.append(("chunk", None if c is None else c.clone()))
        else:
            c, s = loader.next_valid_chunk(seek, size)
            out.append(("valid", None if c is None else c.clone(), s, loader.curr_load_section_index, loader.curr_load_section_seeks))
        floor = loader.prev_seek if loader.prev_seek is not None else floor
        out.append(("state", loader.prev_seek, loader.get_duration(3), loader.get_total_samples()))
    return out


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x[0] == y[0]
        for u, v in zip(x[1:], y[1:]):
            if torch.is_tensor(u) or torch.is_tensor(v):
                assert torch.is_tensor(u) and torch.is_tensor(v) and torch.equal(u, v), (x[0], None if u is None else u.shape, None if v is None else v.shape)
            else:
                assert u == v, (x, y)


GOLDEN_LOADER = os.path.join(HERE, "golden", "audioloader_cases.json.gz")


def _loader_case(seed, monkeypatch, RA=None):
    """seeded AudioLoader case: constructor arguments, a call sequence, and (streamed sources) the stand-ins for ffmpeg --
    patched into the reference's module ``RA`` too when it is given"""
    g = np.random.default_rng(seed)
    n = int(g.integers(1, 200000))
    pcm = g.integers(-20000, 20000, size=n).astype("<i2")
    wave_f32 = torch.from_numpy(pcm.astype(np.float32) / 32768.0)
    stream = bool(seed % 2)
    kw = dict(buffer_size=[None, 16000, "1.5s", 7, 0][int(g.integers(0, 5))], new_chunk_divisor=[512, None, 1000][int(g.integers(0, 3))])
    sections = None
    if g.random() < 0.6:
        cuts = np.sort(g.uniform(0, n / 16000 * 1.2, size=int(g.integers(1, 4)) * 2)).round(2).tolist()
        sections = [tuple(cuts[i:i + 2]) for i in range(0, len(cuts), 2)]
        if g.random() < 0.3:
            sections[-1] = (sections[-1][0], None)
        kw.update(load_sections=sections, negate_load=bool(g.random() < 0.3))
    est = n / 16000 * float(g.choice([1.0, 0.5, 1.7]))                      # ffmpeg's banner duration is an estimate
    if stream:
        if RA is not None:
            monkeypatch.setattr(RA, "get_metadata", lambda src: dict(sr=44100, duration=est))
            monkeypatch.setattr(RA.AudioLoader, "_audio_loading_process", lambda self: _FakePopen(pcm.tobytes()))
        monkeypatch.setattr(AIO, "get_metadata", lambda src: dict(sr=44100, duration=est))
        step = int(g.integers(1, 70000))
        monkeypatch.setattr(AIO, "open_pcm_stream", lambda src, sr: AIO.PcmStream(
            iter([pcm.tobytes()[i:i + 2 * step] for i in range(0, 2 * n, 2 * step)])))
        src_ref = src_mine = "fake.mp3"
    else:
        src_ref, src_mine = wave_f32.clone(), wave_f32.clone()
    # monotone seeks with occasional repeats / jumps past the end, sizes around the window size
    ops, seek = [], 0
    for _ in range(int(g.integers(3, 14))):
        seek += int(g.choice([0, 1, 160, 4800, 16000, 33333, 80000])) if g.random() < 0.8 else int(g.integers(0, n + 50000))
        size = [None, 480000, 16000, 1, 100000][int(g.integers(0, 5))]
        ops.append(("valid" if sections and g.random() < 0.8 else "chunk", seek, size))
    return kw, ops, stream, src_ref, src_mine


def _run_loader(cls, src, stream, kw, ops):
    try:
        loader = cls(src, stream=True if stream else None, **kw)
    except RuntimeError as e:                                   # empty first chunk (e.g. buffer_size=0)
        return ("error", type(e).__name__)
    out = _drive(loader, ops)
    loader.terminate()
    return out


def _canon(x):
    """JSON form of a _run_loader result: tensors as (dtype, shape, sha256 of the bytes) -- equal iff torch.equal"""
    import hashlib
    if torch.is_tensor(x):
        t = x.contiguous().cpu()
        return ["tensor", str(t.dtype), list(t.shape), hashlib.sha256(t.numpy().tobytes()).hexdigest()]
    if isinstance(x, (list, tuple)):
        return [_canon(v) for v in x]
    return x


@pytest.mark.parametrize("seed", range(60))
def test_audioloader_matches_reference(seed, monkeypatch):
    """against the reference's AudioLoader as recorded in tests/golden/audioloader_cases.json.gz
    (tests/golden/make_audioloader_golden.py), and live as well where the reference checkout is importable"""
    RA = None
    if HAVE_REF:
        import make_golden as G
        G.import_reference()
        import stable_whisper.audio as RA
    kw, ops, stream, src_ref, src_mine = _loader_case(seed, monkeypatch, RA)
    mine = _run_loader(AudioLoader, src_mine, stream, kw, ops)
    import gzip
    import json
    with gzip.open(GOLDEN_LOADER, "rt") as f:
        assert _canon(mine) == json.load(f)[str(seed)]
    if RA is not None:
        ref = _run_loader(RA.AudioLoader, src_ref, stream, kw, ops)
        if isinstance(ref, tuple) or isinstance(mine, tuple):
            assert ref == mine
        else:
            _same(ref, mine)


def test_audioloader_wav_stream_equals_memory(tmp_path):
    g = np.random.default_rng(5)
    pcm = (g.standard_normal(3 * 16000 + 77) * 4000).astype("<i2")
    p16 = str(tmp_path / "m16.wav")
    with wave.open(p16, "wb") as w:
        w.setnchannels(1), w.setsampwidth(2), w.setframerate(16000)
        w.writeframes(pcm.tobytes())
    want = torch.from_numpy(pcm.astype(np.float32) / 32768.0)
    for stream in (True, False, None):
        with AudioLoader(p16, stream=stream, buffer_size=16000) as L:
            assert L.stream == (stream is not False) and L.source_sr == 16000
            got, seek = [], 0
            while (c := L.next_chunk(seek)) is not None:
                got.append(c)
                seek += len(c)
            assert torch.equal(torch.cat(got), want) and L.get_total_samples() == len(want)
    # 44.1 kHz stereo file: streamed decoding + block-wise resampling against the one-shot path (<= 1 LSB of s16)
    t = np.arange(int(2.3 * 44100)) / 44100.0
    st = np.stack([0.3 * np.sin(2 * np.pi * 220 * t), 0.3 * np.sin(2 * np.pi * 3000 * t + 1)], 1)
    p44 = str(tmp_path / "s44.wav")
    with wave.open(p44, "wb") as w:
        w.setnchannels(2), w.setsampwidth(2), w.setframerate(44100)
        w.writeframes(AIO.to_s16(st.reshape(-1)).tobytes())
    whole = torch.from_numpy(load_audio(p44))
    save = str(tmp_path / "final.wav")
    with AudioLoader(p44, stream=True, buffer_size=5000, save_path=save) as L:
        got, seek = [], 0
        while (c := L.next_chunk(seek)) is not None:
            got.append(c)
            seek += len(c)
    got = torch.cat(got)
    assert got.shape == whole.shape and (got - whole).abs().max() <= 1.0 / 32768 + 1e-9
    assert (got != whole).float().mean() < 0.01
    saved, sr = read_wav(save)                                          # save_path: the prepared audio as 16-bit WAVE
    assert sr == 16000 and np.array_equal(saved[:, 0], got.numpy())


def test_as_waveform_whole_file_callers(tmp_path):
    # align / align_words / refine / locate take the whole recording (the reference's prep_audio callers)
    from stable_ts_amd.transcribe import as_waveform
    pcm = (np.random.default_rng(3).standard_normal(5000) * 2000).astype("<i2")
    p = str(tmp_path / "w.wav")
    with wave.open(p, "wb") as w:
        w.setnchannels(1), w.setsampwidth(2), w.setframerate(16000)
        w.writeframes(pcm.tobytes())
    want = torch.from_numpy(pcm.astype(np.float32) / 32768.0)
    assert torch.equal(as_waveform(p), want) and torch.equal(as_waveform(want.numpy()), want)
    assert torch.equal(as_waveform(torch.stack([want, -want])), torch.zeros_like(want))       # channels first, down-mixed
    assert as_waveform(want.double()).dtype == torch.float32
    assert as_waveform(want, only_voice_freq=True).shape == want.shape
    with pytest.raises(NotImplementedError):
        as_waveform(AudioLoader(want))
