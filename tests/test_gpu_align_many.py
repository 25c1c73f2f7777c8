"""``model.align_many`` on hardware: seven recordings advance their forced-alignment state machines in lockstep
(stable_ts_amd/many.py) and every result equals ``model.align`` of that recording alone -- exactly: the project's batch
invariance (tests/test_gpu_batch_invariance.py) makes window k of a pass the window alone, and the driver gives every recording
its own sequence of windows.

Multilingual ``tiny``, seeded random weights (the recipe of tests/test_gpu_transcribe_many.py), strict f32 and f16.  The rounds
are the ragged passes ``transcribe(batch_size=)`` never produced: a 25-frame window with one text token next to full 1500-frame
windows with 100, windows trimmed by the non-speech skip, three different sot sequences (en / de / ja) in one scoring pass.
Recordings: 0.5 s with one token, 4 s (de), 33 s, 65 s (ja), 35 s of exact zeros + 20 s of signal, 8 s of exact zeros (never
reaches the device), 4 s with 150 tokens (far more than fit).  All device-resident except the 33-s one, which stays on the host.
"""
import os
import random
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
N_TOKENS = (1, 9, 70, 260, 40, 6, 150)
LANGS = ["en", "de", "en", "ja", "en", "en", "en"]
_CACHE = {}


def _synth_audio(seconds, seed):
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "golden", "make_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return torch.as_tensor(mod.synth_audio(seconds, seed), dtype=torch.float32)


def _model(dtype):
    import stable_ts_amd as sw
    if ("m", dtype) not in _CACHE:
        dims = sw.dims_for("tiny")
        m = sw.Whisper(dims, dtype=dtype, max_windows=1, max_rows=5)
        m.load_state_dict(sw.random_state_dict(dims, seed=1234, std=0.02, embed_gain=2.0, ts_gain=0.5))
        _CACHE[("m", dtype)] = m
    return _CACHE[("m", dtype)]


def _inputs():
    if "in" not in _CACHE:
        clips = [_synth_audio(4.0, 31)[:8000], _synth_audio(4.0, 32), _synth_audio(33.0, 33), _synth_audio(65.0, 34),
                 torch.cat([torch.zeros(35 * 16000), _synth_audio(20.0, 35)]), torch.zeros(8 * 16000), _synth_audio(4.0, 36)]
        clips = [a if i == 2 else a.cuda() for i, a in enumerate(clips)]
        rng = random.Random(9)
        _CACHE["in"] = (clips, [[rng.randrange(300, 20000) for _ in range(n)] for n in N_TOKENS])
    return _CACHE["in"]


def _recorded(fn):
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        out = fn()
    return out, sorted(m for m in (str(w.message) for w in caught) if "lign" in m or "max timestamp" in m)


def _expected(dtype):
    """model.align per recording (the parent commit's code path), once per dtype: results, warnings, windows per recording"""
    if ("want", dtype) not in _CACHE:
        model, (clips, texts) = _model(dtype), _inputs()
        res, warned, windows = [], [], []
        for a, t, l in zip(clips, texts, LANGS):
            c0, w0 = model.engine.encode_calls, model.engine.encode_windows
            r, w = _recorded(lambda: model.align(a, t, language=l))
            assert model.engine.encode_windows - w0 == model.engine.encode_calls - c0      # one window per device pass
            res.append(r)
            warned += w
            windows.append(model.engine.encode_calls - c0)
        _CACHE[("want", dtype)] = (res, sorted(warned), windows)
    return _CACHE[("want", dtype)]


def _assert_same(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        gw, ww = g.all_words(), w.all_words()
        assert [x.word for x in gw] == [x.word for x in ww], i
        assert [(x.start, x.end) for x in gw] == [(x.start, x.end) for x in ww], i
        assert [float(x.probability) for x in gw] == [float(x.probability) for x in ww], i
        assert [list(x.tokens) for x in gw] == [list(x.tokens) for x in ww], i
        assert g.nonspeech_sections == w.nonspeech_sections, i
        assert g.language == w.language == LANGS[i], i
        assert g.to_dict() == w.to_dict(), i


@pytest.mark.parametrize("max_tracks", [2, 7])
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_align_many_equals_align_per_recording(dtype, max_tracks):
    model, (clips, texts) = _model(dtype), _inputs()
    want, want_warned, windows = _expected(dtype)
    assert windows[5] == 0 and windows[0] == 1 and max(windows) >= 2 and sum(windows) > max(windows)
    c0, w0, bound0 = model.engine.encode_calls, model.engine.encode_windows, model.engine.max_windows
    got, warned = _recorded(lambda: model.align_many(clips, texts, LANGS, max_tracks=max_tracks))
    rounds, in_rounds = model.engine.encode_calls - c0, model.engine.encode_windows - w0
    print(f"[align_many {dtype} max_tracks={max_tracks}] windows per recording {windows}, {rounds} rounds for {in_rounds} windows")
    _assert_same(got, want)
    assert warned == want_warned
    # the all-zero recording never reaches the device: every word at the end of the file with probability 0
    zero = got[5].all_words()
    assert len(zero) > 0 and all((w.start, w.end, w.probability) == (8.0, 8.0, 0.0) for w in zero)
    # the recording that opens with 35 s of zeros starts where the signal does
    assert got[4].all_words()[0].start >= 30.0
    # the same windows in fewer device passes
    assert in_rounds == sum(windows)
    if max_tracks == 7:
        assert rounds == max(windows) < sum(windows)
    else:
        assert sum(windows) / 2 <= rounds < sum(windows)
    assert model.engine.max_windows <= max(bound0, max_tracks)             # the workspace grows to max_tracks windows, no further


def test_align_many_options_and_errors():
    """string texts with ``original_split``, a ``WhisperResult`` as text (it brings its language), one tokenizer for all"""
    import copy
    from stable_ts_amd.tokenizer import get_tokenizer
    model, (clips, texts) = _model("f16"), _inputs()
    tok = get_tokenizer(True, num_languages=model.num_languages, language="en", task="transcribe")
    lines = "\n".join(tok.decode(texts[2][a:a + 7]) for a in range(0, 28, 7))
    as_text = copy.deepcopy(_expected("f16")[0][1])
    assert as_text.language == "de"
    audios, given, langs = [clips[2], clips[1], clips[6]], [lines, as_text, texts[6]], ["en", None, "en"]
    opts = dict(original_split=True, fast_mode=True)
    want, want_warned = _recorded(lambda: [model.align(a, t, language=l, **opts) for a, t, l in zip(audios, given, langs)])
    got, warned = _recorded(lambda: model.align_many(audios, given, langs, max_tracks=3, **opts))
    assert [g.to_dict() for g in got] == [w.to_dict() for w in want] and warned == want_warned
    assert [g.language for g in got] == ["en", "de", "en"] and len(got[0].segments) == 4
    want = [model.align(a, t, tokenizer=tok) for a, t in zip(clips[:2], texts[:2])]
    got = model.align_many(clips[:2], texts[:2], tokenizer=tok)
    assert [g.to_dict() for g in got] == [w.to_dict() for w in want]
    assert model.align_many([], []) == []
    with pytest.raises(TypeError, match="expected argument for language"):
        model.align_many(clips[:2], texts[:2], ["en", None])
    with pytest.raises(ValueError):
        model.align_many(clips[:2], texts[:1], "en")
    with pytest.raises(TypeError):
        model.align_many(clips[1], texts[:1], "en")
