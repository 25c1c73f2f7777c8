"""``locate_many`` (stable_ts_amd/many.py) on the CPU oracle stand-in: the chunk state machines of several recordings
(``locator.LocateJob.steps``) advance in lockstep; a round answers their requests phase by phase with one call each, and a
finished recording hands its slot to the next one.

Oracle: ``stable_ts_amd.locator.locate`` per recording, which tests/test_locate_cpu.py pins against the reference's own
``locate``.  Exact by construction: every recording sees its own sequence of chunks and greedy steps; only the number of
windows per call differs.  The stand-in has no ``device_next_token``, so every greedy step takes the host arithmetic.

Recordings (``tiny.en``, the weights of tests/test_locate_cpu.py): 0.5 s, 4 s, 20 s, 33 s, 75 s, 12 s of exact zeros, 47 s.
"""
import contextlib
import io
import os
import sys
import warnings

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)

import stable_ts_amd.locator as L  # noqa: E402
from stable_ts_amd.many import locate_many  # noqa: E402

TEXTS = [" aaat", " aaat aabc", [25, 31], " aaat", " aaat aabc", " aabc", [25, 31, 40]]

CASES = {
    "mode2": dict(mode=2, count=0),
    "mode2_window": dict(mode=2, count=3, start=2.0, end=70.0),
    "mode1": dict(mode=1, count=2, probability_threshold=0.0),
    "mode1_budget": dict(mode=1, count=0, probability_threshold=0.0, eots=2, max_token_per_seg=6, duration_window=(2.0, 4.0)),
    "mode0": dict(mode=0, count=2, probability_threshold=0.0),
    "mode0_exact_prompt": dict(mode=0, count=1, probability_threshold=0.0, exact_token=True, initial_prompt="aabf aabi"),
    "mode1_case_prompt": dict(mode=1, count=1, probability_threshold=0.0, case_sensitive=True, initial_prompt="aabf",
                              suppress_tokens="1,2"),
    "mode1_unconfirmed": dict(mode=1, count=0, probability_threshold=0.9, max_token_per_seg=3, end=40.0),
}


def _norm(matches):
    from test_locate_cpu import _norm as norm
    return norm(matches)


@contextlib.contextmanager
def _counting(model):
    """every device call (encoder pass, scoring pass, logits pass) appends its number of windows to the list this yields"""
    eng, log = model.engine, []
    real = dict(encoder=model.encoder, score=eng.score, forward_logits=eng.forward_logits)
    model.encoder = lambda mel: (log.append(1 if mel.ndim == 2 else int(mel.shape[0])), real["encoder"](mel))[1]
    eng.score = lambda xkv, tokens, *a, **kw: (log.append(len(tokens)), real["score"](xkv, tokens, *a, **kw))[1]
    eng.forward_logits = lambda xkv, tokens, *a, **kw: (log.append(len(tokens)), real["forward_logits"](xkv, tokens, *a, **kw))[1]
    try:
        yield log
    finally:
        del model.encoder, eng.score, eng.forward_logits


def _quiet(fn):
    with warnings.catch_warnings(), contextlib.redirect_stdout(io.StringIO()):
        warnings.simplefilter("ignore")
        return fn()


@pytest.fixture(scope="module")
def world():
    import make_golden as G
    from oracle.whisper.model import build_model
    from oracle_engine import CpuWhisper
    mine = CpuWhisper(build_model("tiny.en", seed=1234, std=0.02, embed_gain=2.0, ts_gain=0.5))

    def synth(seconds, seed):
        return torch.as_tensor(G.synth_audio(seconds, seed=seed), dtype=torch.float32)

    audios = [synth(4.0, 41)[:8000], synth(4.0, 42), synth(20.0, 43), synth(33.0, 44), synth(75.0, 45), torch.zeros(12 * 16000),
              synth(47.0, 46)]
    return dict(model=mine, audios=audios, want={})


@pytest.fixture(autouse=True)
def _stand_in(monkeypatch):
    from oracle_engine import install
    install(monkeypatch)


def _expected(world, name):
    """``locate`` per recording, once per case: (normalised results, device calls per recording)"""
    if name not in world["want"]:
        res, calls = [], []
        with _counting(world["model"]) as log:
            for audio, text in zip(world["audios"], TEXTS):
                n0 = len(log)
                res.append(_norm(_quiet(lambda: L.locate(world["model"], audio, text, "en", verbose=None, **CASES[name]))))
                calls.append(len(log) - n0)
            assert set(log) == {1}
        world["want"][name] = (res, calls)
    return world["want"][name]


@pytest.mark.parametrize("max_tracks", [1, 3, len(TEXTS)])
@pytest.mark.parametrize("name", list(CASES))
def test_locate_many_equals_the_loop(world, name, max_tracks):
    want, calls = _expected(world, name)
    with _counting(world["model"]) as log:
        got = _quiet(lambda: locate_many(world["model"], world["audios"], TEXTS, "en", max_tracks=max_tracks, verbose=None,
                                         **CASES[name]))
    assert [_norm(g) for g in got] == want                  # in input order
    assert any(want) or name == "mode1_unconfirmed", "the case locates nothing anywhere"
    assert max(log) <= max_tracks
    if max_tracks == 1:
        assert len(log) == sum(calls)
    if max_tracks >= len(TEXTS):
        assert len(log) < sum(calls)


def test_recordings_of_one_shape_cost_the_calls_of_one(world):
    """three times the same recording and text: every phase of every round holds all three, so the job makes the calls one
    recording makes alone; the same tensor object is passed three times"""
    opts = dict(mode=0, count=2, probability_threshold=0.0)
    audio = world["audios"][3]
    with _counting(world["model"]) as alone:
        want = _norm(_quiet(lambda: L.locate(world["model"], audio, " aaat", "en", verbose=None, **opts)))
    with _counting(world["model"]) as log:
        got = _quiet(lambda: locate_many(world["model"], [audio] * 3, [" aaat"] * 3, ["en"] * 3, verbose=None, **opts))
    assert [_norm(g) for g in got] == [want] * 3 and want
    assert len(log) <= len(alone) and max(log) == 3


def test_one_recording_many_phrases(world):
    audio = world["audios"][4]
    texts = [" aaat", " aabc aaat", [25, 31]]
    opts = dict(mode=1, count=2, probability_threshold=0.0)
    want = [_norm(_quiet(lambda: L.locate(world["model"], audio, t, "en", verbose=None, **opts))) for t in texts]
    got = _quiet(lambda: locate_many(world["model"], [audio] * 3, texts, "en", max_tracks=2, verbose=None, **opts))
    assert [_norm(g) for g in got] == want


@pytest.mark.parametrize("kwargs, error", [
    (dict(texts=[" aaat"]), ValueError),                                 # one text for two recordings
    (dict(texts=" aaat"), TypeError),                                    # a single text, not a list
    (dict(language=["en"]), ValueError),
    (dict(max_tracks=0), ValueError),
    (dict(max_tracks=1.5), ValueError),
    (dict(no_such_option=1), TypeError),
    (dict(device_probe=True), RuntimeError),                             # the stand-in has no native call
    (dict(duration_window=300000.0), AssertionError),                    # what locate() refuses before it touches the audio
])
def test_argument_errors_come_before_any_device_call(world, kwargs, error):
    args = dict(texts=[" aaat", " aabc"], language="en")
    args.update(kwargs)
    texts, language = args.pop("texts"), args.pop("language")
    with _counting(world["model"]) as log:
        with pytest.raises(error):
            locate_many(world["model"], world["audios"][:2], texts, language, **args)
    assert log == []


def test_audios_must_be_a_list(world):
    with pytest.raises(TypeError):
        locate_many(world["model"], world["audios"][1], [" aaat"], "en")


def test_what_locate_raises_locate_many_raises(world):
    """a token id outside the vocabulary fails inside the scoring pass of its recording, for both"""
    with pytest.raises(Exception) as alone:
        _quiet(lambda: L.locate(world["model"], world["audios"][1], [10 ** 6], "en", mode=2, verbose=None))
    with pytest.raises(type(alone.value)):
        _quiet(lambda: locate_many(world["model"], world["audios"][:2], [" aaat", [10 ** 6]], "en", mode=2, verbose=None))


def test_empty_job(world):
    assert locate_many(world["model"], [], [], "en") == []
