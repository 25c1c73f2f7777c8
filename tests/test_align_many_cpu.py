"""``align_many`` (stable_ts_amd/many.py) on the CPU oracle stand-in: the window state machines of several recordings
(``Aligner.steps``) advance in lockstep, one ``make_alignment_func(...).batch`` call answers the current window of every live
recording, a finished recording hands its slot to the next one.

Oracle: ``stable_ts_amd.alignment.align`` per recording, which tests/test_aligner_cpu.py pins against the reference's own
``Aligner`` and ``model.align``.  Exact by construction: every recording sees its own sequence of windows; only the number of
windows per inference call differs.

Recordings (multilingual ``tiny``, seed 77): 0.5 s with one token, 4 s (de), 33 s, 65 s (ja: words are not split at spaces),
35 s of exact zeros followed by 20 s of signal (its first window is skipped, the second is trimmed), 8 s of exact zeros (never
reaches the inference function), and 4 s with 150 tokens (far more than fit: the leftover words land at the end of the file).
"""
import contextlib
import copy
import os
import random
import sys
import warnings

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)

import stable_ts_amd.alignment as A  # noqa: E402
from stable_ts_amd.aligner import Aligner  # noqa: E402
from stable_ts_amd.many import align_many  # noqa: E402
from stable_ts_amd.result import WhisperResult  # noqa: E402

N_TOKENS = (1, 9, 70, 260, 40, 6, 150)
LANGS = ["en", "de", "en", "ja", "en", "en", "en"]
SHORT = (1, 2, 6)                   # the recordings of the option cases: 4 s, 33 s, 4 s with the overlong text


@contextlib.contextmanager
def _counting():
    """every device job of ``make_alignment_func`` appends its number of windows to the list this yields"""
    real, log = A.make_alignment_func, []

    def factory(model, tokenizer, **variant):
        f = real(model, tokenizer, **variant)

        def one(segment, words):
            log.append(1)
            return f(segment, words)

        def batch(chunks, words, **kw):
            log.append(len(chunks))
            return f.batch(chunks, words, **kw)

        one.batch = batch
        return one

    A.make_alignment_func = factory
    try:
        yield log
    finally:
        A.make_alignment_func = real


def _recorded(fn):
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        out = fn()
    # the Aligner's own warnings (torch's warn-once notices depend on what ran earlier in the process)
    return out, sorted(m for m in (str(w.message) for w in caught) if "lign" in m or "max timestamp" in m)


@pytest.fixture(scope="module")
def world():
    import make_golden as G
    from oracle.whisper.model import build_model
    from oracle_engine import CpuWhisper
    mine = CpuWhisper(build_model("tiny", seed=77, std=0.02, embed_gain=2.0, ts_gain=0.5))
    mine.manual_attention_encoder = True

    def synth(seconds, seed):
        return torch.as_tensor(G.synth_audio(seconds, seed=seed), dtype=torch.float32)

    audios = [synth(4.0, 31)[:8000], synth(4.0, 32), synth(33.0, 33), synth(65.0, 34),
              torch.cat([torch.zeros(35 * 16000), synth(20.0, 35)]), torch.zeros(8 * 16000), synth(4.0, 36)]
    rng = random.Random(9)
    texts = [[rng.randrange(300, 20000) for _ in range(n)] for n in N_TOKENS]
    return dict(model=mine, audios=audios, texts=texts, want={})


def _pick(world, indices):
    return [world["audios"][i] for i in indices], [world["texts"][i] for i in indices], [LANGS[i] for i in indices]


def _expected(world, key, audios, texts, languages, **opts):
    """``align`` per recording, once per case: (results, warnings, windows per recording)"""
    if key not in world["want"]:
        res, warned, windows = [], [], []
        with _counting() as log:
            for audio, text, language in zip(audios, texts, languages):
                n0 = len(log)
                r, w = _recorded(lambda: A.align(world["model"], audio, text, language=language, **opts))
                res.append(r)
                warned += w
                windows.append(len(log) - n0)
        world["want"][key] = (res, sorted(warned), windows)
    return world["want"][key]


def _same(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        if w is None:
            assert g is None, i
            continue
        gw, ww = g.all_words(), w.all_words()
        assert [x.word for x in gw] == [x.word for x in ww], i
        assert [(x.start, x.end) for x in gw] == [(x.start, x.end) for x in ww], i
        assert [float(x.probability) for x in gw] == [float(x.probability) for x in ww], i
        assert [list(x.tokens) for x in gw] == [list(x.tokens) for x in ww], i
        assert g.nonspeech_sections == w.nonspeech_sections, i
        assert g.language == w.language and w.language is not None, i
        assert g.to_dict() == w.to_dict(), i


@pytest.mark.parametrize("max_tracks", [1, 2, 7])
def test_align_many_equals_align_per_recording(world, monkeypatch, max_tracks):
    from oracle_engine import install
    install(monkeypatch)
    want, want_warned, windows = _expected(world, "seven", world["audios"], world["texts"], LANGS)
    assert windows[5] == 0 and windows[0] == 1 and max(windows) >= 5 and sum(windows) > 2 * max(windows)
    with _counting() as log:
        got, warned = _recorded(lambda: align_many(world["model"], world["audios"], world["texts"], LANGS, max_tracks=max_tracks))
    _same(got, want)
    assert [g.language for g in got] == LANGS
    assert warned == want_warned                                  # the same warnings, whichever recording finished first
    # the all-zero recording: every word at the end of the file with probability 0, without a window
    assert [(w.start, w.end, w.probability) for w in got[5].all_words()] == [(8.0, 8.0, 0.0)] * len(got[5].all_words())
    assert len(got[5].all_words()) > 0
    # the overlong text: what did not fit lands at the end of the file, with align()'s warning
    left = [w for w in got[6].all_words() if w.start == w.end == 4.0 and w.probability == 0.0]
    assert len(left) > 10 and any(f"Failed to align the last {len(left)}/" in m for m in warned)
    # sharing: the same windows in fewer device jobs
    assert sum(log) == sum(windows) and max(log) <= max_tracks
    if max_tracks == 7:
        assert len(log) == max(windows) < sum(windows)            # as many rounds as the longest recording has windows
    elif max_tracks == 2:
        assert sum(windows) / 2 <= len(log) < sum(windows)
    else:
        assert log == [1] * sum(windows)


def test_steps_is_the_state_machine_align_drives():
    """``Aligner.steps`` yields exactly the calls ``align`` makes, and a recording of silence returns without yielding"""
    import make_aligner_golden as mg
    from stable_ts_amd.tokenizer import get_tokenizer
    tok = get_tokenizer(False, num_languages=99)
    audio, ids, opts = mg.synth_case(3)
    f = mg.make_inference(3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = Aligner(f, tok.decode, tok.encode, **opts).align(audio, ids)
        steps, n = Aligner(None, tok.decode, tok.encode, **opts).steps(audio, ids), 0
        try:
            request = next(steps)
            while True:
                n += 1
                assert len(request) == 2 and torch.is_tensor(request[0])
                request = steps.send(f(*request))
        except StopIteration as end:
            got = end.value
    assert n > 1 and got.to_dict() == want.to_dict()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(StopIteration) as end:
            next(Aligner(None, tok.decode, tok.encode).steps(torch.zeros(16000 * 7), ids[:5]))
    words = end.value.value.all_words()
    assert len(words) > 0 and all((w.start, w.end, w.probability) == (7.0, 7.0, 0.0) for w in words)


CASES = {
    "defaults": dict(),
    "plain": dict(regroup=False, suppress_silence=False),
    "fast_mode": dict(fast_mode=True),
    "failure_threshold": dict(failure_threshold=0.3),
    "dynamic_heads": dict(dynamic_heads="4,2"),
    "token_step": dict(token_step=30, nonspeech_skip=None),
}


@pytest.mark.parametrize("name", list(CASES))
def test_align_many_options(world, monkeypatch, name):
    from oracle_engine import install
    install(monkeypatch)
    opts = CASES[name]
    audios, texts, languages = _pick(world, SHORT)
    want, want_warned, windows = _expected(world, name, audios, texts, languages, **opts)
    if name == "failure_threshold":                                # some recordings give up early while others go on
        assert 0 < sum("Alignment aborted" in m for m in want_warned) < len(SHORT)
    with _counting() as log:
        got, warned = _recorded(lambda: align_many(world["model"], audios, texts, languages, max_tracks=3, **opts))
    _same(got, want)
    assert warned == want_warned
    assert len(log) == max(windows) and sum(log) == sum(windows)


def test_align_many_strings_with_original_split(world, monkeypatch):
    from oracle_engine import install
    from stable_ts_amd.tokenizer import get_tokenizer
    install(monkeypatch)
    tok = get_tokenizer(True, num_languages=world["model"].num_languages, language="en", task="transcribe")
    ids = world["texts"][2]
    texts = ["\n".join(tok.decode(ids[a:a + 7]) for a in range(0, 28, 7)), tok.decode(ids[30:42]) + "\n\n" + tok.decode(ids[42:50])]
    audios = [world["audios"][2], world["audios"][1]]
    want, want_warned, _ = _expected(world, "strings", audios, texts, ["en", "en"], original_split=True)
    assert len(want[0].segments) == 4 and len(want[1].segments) == 2           # one segment per line
    got, warned = _recorded(lambda: align_many(world["model"], audios, texts, "en", original_split=True))
    _same(got, want)
    assert warned == want_warned


def test_align_many_result_as_text_brings_its_language(world, monkeypatch):
    from oracle_engine import install
    install(monkeypatch)
    first, _, _ = _expected(world, "defaults", *_pick(world, SHORT))
    as_text = copy.deepcopy(first[0])                                          # the 4-s recording, language "de"
    assert isinstance(as_text, WhisperResult) and as_text.language == "de"
    audios, texts = [world["audios"][1], world["audios"][2]], [as_text, world["texts"][2]]
    want, want_warned, _ = _expected(world, "result_text", audios, texts, [None, "en"])
    seen = []
    got, warned = _recorded(lambda: align_many(world["model"], audios, texts, [None, "en"], max_tracks=2,
                                               progress_callback=lambda a, b: seen.append((a, b))))
    _same(got, want)
    assert [g.language for g in got] == ["de", "en"] and warned == want_warned
    total = (audios[0].shape[-1] + audios[1].shape[-1]) / 16000
    assert seen and all(b == total for _, b in seen) and [a for a, _ in seen] == sorted(a for a, _ in seen)
    assert abs(seen[-1][0] - total) < 1e-9 and 0 < seen[0][0] < total


def test_align_many_validation(world, monkeypatch):
    from oracle_engine import install
    install(monkeypatch)
    model, audios, texts = world["model"], world["audios"], world["texts"]
    with _counting() as log:
        _validation_errors(model, audios, texts)
    assert log == []                                               # all of it refused before the first device job


def _validation_errors(model, audios, texts):
    assert align_many(model, [], []) == []
    with pytest.raises(TypeError, match="list of recordings"):
        align_many(model, audios[1], [texts[1]], "en")
    with pytest.raises(TypeError, match="list of recordings"):
        align_many(model, "clip.wav", [texts[1]], "en")
    with pytest.raises(ValueError, match="texts has 1 entries for 2 recordings"):
        align_many(model, audios[:2], texts[:1], "en")
    with pytest.raises(ValueError, match="3 entries for 2 recordings"):
        align_many(model, audios[:2], texts[:2], ["en", "de", "en"])
    for bad in (0, -1, None):
        with pytest.raises(ValueError, match="max_tracks"):
            align_many(model, audios[:2], texts[:2], "en", max_tracks=bad)
    with pytest.raises(ValueError, match="token_step"):
        align_many(model, audios[:2], texts[:2], "en", token_step=10 ** 6)
    with pytest.raises(TypeError, match="no_such_option"):
        align_many(model, audios[:2], texts[:2], "en", no_such_option=1)
    with pytest.raises(ValueError, match="failure_threshold"):
        align_many(model, audios[:2], texts[:2], "en", failure_threshold=1.5)
    # a multilingual model and a recording whose language nothing tells: refused before the first recording runs
    for language in (None, ["en", None]):
        with pytest.raises(TypeError, match="expected argument for language"):
            align_many(model, audios[1:3], texts[1:3], language)


def test_align_many_error_of_one_recording_propagates(world, monkeypatch):
    """an inference answer that breaks the contract for ONE window (a word short) is that recording's RuntimeError"""
    from oracle_engine import install
    install(monkeypatch)
    real = A.make_alignment_func

    def factory(model, tokenizer, **variant):
        f = real(model, tokenizer, **variant)
        whole = f.batch

        def batch(chunks, words, **kw):
            outs = whole(chunks, words, **kw)
            return outs[:-1] + [outs[-1][:-1]]

        f.batch = batch
        return f

    monkeypatch.setattr(A, "make_alignment_func", factory)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(RuntimeError, match="expected output word count"):
            align_many(world["model"], world["audios"][1:3], world["texts"][1:3], ["de", "en"])
