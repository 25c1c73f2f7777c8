"""``model.transcribe_many`` on hardware: five recordings advance in lockstep (stable_ts_amd/many.py), each with its own language
state, and every result equals ``model.transcribe`` of that recording alone -- exactly: the project's batch invariance
(tests/test_gpu_batch_invariance.py) makes window k of a batch the window alone, and the driver gives every recording the
reference's own sequence of windows and prompts.

Multilingual ``tiny``, seeded random weights (the recipe of tests/test_gpu_golden.py), f32 and f16.  Recordings: 4 s, 31 s, 65 s,
35 s of exact zeros followed by 20 s of signal (its first window is skipped as silent: the language comes from the second), and
8 s of exact zeros (never decoded: ``language is None``, no segments).  ``max_tracks=2`` refills slots while other recordings are
still running, ``max_tracks=5`` holds all of them at once.  Decoding is deterministic (temperature 0, no fallback thresholds).
"""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
BASE = dict(temperature=0.0, logprob_threshold=None, compression_ratio_threshold=None, no_speech_threshold=None, sample_len=24)
LANGS = {"detect": None, "en": "en", "list": ["en", None, "de", None, "ja"]}
_CACHE = {}


def _snap(res):
    out = []
    for s in res.segments:
        ws = None if not s.has_words else [(w.word, round(w.start, 3), round(w.end, 3), round(float(w.probability), 9), list(w.tokens))
                                           for w in s.words]
        out.append((round(s.start, 3), round(s.end, 3), s.text, list(s.tokens), ws))
    return out


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


def _clips():
    if "clips" not in _CACHE:
        _CACHE["clips"] = [a.cuda() for a in (
            _synth_audio(4.0, 21), _synth_audio(31.0, 22), _synth_audio(65.0, 23),
            torch.cat([torch.zeros(35 * 16000), _synth_audio(20.0, 24)]), torch.zeros(8 * 16000))]
    return _CACHE["clips"]


def _per_language(language, n):
    return [language] * n if language is None or isinstance(language, str) else list(language)


def _expected(dtype, lang_key, opt_key="base", **opts):
    """model.transcribe per recording (the parent commit's code path), once per (dtype, languages, options)"""
    key = ("want", dtype, lang_key, opt_key)
    if key not in _CACHE:
        model, clips = _model(dtype), _clips()
        _CACHE[key] = [model.transcribe(a, language=l, **BASE, **opts) for a, l in zip(clips, _per_language(LANGS[lang_key], len(clips)))]
    return _CACHE[key]


def _assert_same(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.language == w.language, i
        assert _snap(g) == _snap(w), i
        assert g.text == w.text, i
        assert g.nonspeech_sections == w.nonspeech_sections, i
    assert got[4].language is None and len(got[4].segments) == 0            # all zeros: never decoded
    assert got[3].language is not None and len(got[3].segments) > 0 and got[3].segments[0].start >= 30.0
    assert sum(len(g.segments) for g in got) >= 6


@pytest.mark.parametrize("max_tracks", [2, 5])
@pytest.mark.parametrize("lang_key", list(LANGS))
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_many_equals_transcribe_per_recording(dtype, lang_key, max_tracks, monkeypatch):
    import stable_ts_amd.transcribe as T
    model, clips = _model(dtype), _clips()
    want = _expected(dtype, lang_key)
    if lang_key == "list":
        assert [w.language for w in want[:3:2]] == ["en", "de"] and want[4].language is None
    rounds = {"n": 0}
    real = T._process_batch

    def counted(*a, **kw):
        rounds["n"] += 1
        return real(*a, **kw)

    monkeypatch.setattr(T, "_process_batch", counted)
    calls0, bound0 = model.engine.encode_calls, model.engine.max_windows
    got = model.transcribe_many(clips, language=LANGS[lang_key], max_tracks=max_tracks, **BASE)
    _assert_same(got, want)
    # the language step reads the features the round encodes anyway: one encoder pass per round, not one more per recording
    # (the loop pays 2 for the first decoded window of every recording whose language is unknown)
    assert rounds["n"] >= 3
    assert model.engine.encode_calls - calls0 == rounds["n"]
    assert model.engine.max_windows <= max(bound0, max_tracks)             # the workspace grows to max_tracks windows, no further


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_many_beam_with_initial_prompt(dtype):
    """beam 2 + an initial prompt: the prompt is encoded with each recording's own tokenizer once its language is known, and
    rides in every later window's prompt (ragged initial tokens in one job)"""
    model, clips = _model(dtype), _clips()
    opts = dict(beam_size=2, initial_prompt=" aaat aaau")
    want = _expected(dtype, "detect", "beam_prompt", **opts)
    got = model.transcribe_many(clips, max_tracks=2, **BASE, **opts)
    _assert_same(got, want)


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_many_segment_level(dtype):
    model, clips = _model(dtype), _clips()
    opts = dict(word_timestamps=False)
    want = _expected(dtype, "list", "segments", **opts)
    got = model.transcribe_many(clips, language=LANGS["list"], max_tracks=2, **BASE, **opts)
    _assert_same(got, want)
    assert not any(s.has_words for g in got for s in g.segments)


def test_many_empty_list_and_errors():
    model, clips = _model("f16"), _clips()
    assert model.transcribe_many([]) == []
    with pytest.raises(NotImplementedError):
        model.transcribe_many(clips[:2], batch_size=2, **BASE)
    with pytest.raises(ValueError):
        model.transcribe_many(clips[:2], language=["en"], **BASE)
    with pytest.raises(RuntimeError, match=r"audios\[1\]"):
        model.transcribe_many([clips[0], torch.zeros(0)], language="en", **BASE)
