"""``transcribe_many`` (stable_ts_amd/many.py) on the CPU oracle stand-in: several recordings advance in lockstep, each with
its own loader, silence predictor and language state; a finished recording hands its slot to the next one.

Oracle: the reference's own ``transcribe()`` per recording where its checkout is importable (exact by construction, as for
the span mode: every recording runs the reference's sequential algorithm and only the batching differs), else this
package's ``model.transcribe`` per recording.  The stand-in has no ``device_language_id``: the language comes from
``model.detect_language`` per recording here (the device path is tests/test_gpu_transcribe_many.py).
"""
import os
import sys
import warnings

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)

from stable_ts_amd.many import transcribe_many  # noqa: E402
from test_spans_cpu import BASE, CASES, _snap  # noqa: E402

HAVE_REF = os.path.isdir("/root/reference/stable_whisper")
# seconds, seed: one shorter than a window, one of two windows, one that is the shortest of all and comes LAST but one (it
# finishes first: order check), one a little over a window
CLIPS = ((33.0, 3), (47.0, 4), (6.0, 5), (19.0, 6))


@pytest.fixture(scope="module")
def models():
    import make_golden as G
    from oracle.whisper.model import build_model
    from oracle_engine import CpuWhisper
    m = build_model("tiny", seed=77, std=0.02, embed_gain=2.0, ts_gain=0.5)
    if HAVE_REF:
        G.import_reference().modify_model(m)
    mine = CpuWhisper(m)
    audios = [torch.as_tensor(G.synth_audio(s, seed=k)) for s, k in CLIPS]
    return G, (m if HAVE_REF else None), mine, audios


_WANT = {}


def _expected(models, name, languages):
    """per recording: the reference's transcribe() (or, without its checkout, this package's), computed once per case"""
    _, ref_model, mine, audios = models
    key = (name, tuple(languages))
    if key not in _WANT:
        opts = dict(BASE, **CASES[name])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            if ref_model is not None:
                _WANT[key] = [ref_model.transcribe(a, language=l, verbose=None, ignore_compatibility=True, **opts)
                              for a, l in zip(audios, languages)]
            else:
                _WANT[key] = [mine.transcribe(a, language=l, **opts) for a, l in zip(audios, languages)]
    return _WANT[key]


def _same(got, want, opts):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.language == w.language and w.language is not None
        assert _snap(g) == _snap(w)
        assert g.text == w.text
        assert g.to_dict() == w.to_dict()
        if opts.get("suppress_silence", True):
            assert g.nonspeech_sections == w.nonspeech_sections


@pytest.mark.parametrize("max_tracks", [1, 2, 4])
@pytest.mark.parametrize("name", list(CASES))
def test_many_equals_transcribe_per_recording(models, monkeypatch, name, max_tracks):
    """language=None: every recording settles its own language on its first decoded window (the random multilingual model
    does not give all four clips the same one: asserted), max_tracks 1 / 2 / 4: one slot reused four times, slots refilled
    while others are still running, all four at once"""
    _, _, mine, audios = models
    from oracle_engine import install
    install(monkeypatch)
    opts = dict(BASE, **CASES[name])
    want = _expected(models, name, [None] * len(audios))
    if name != "ts_tokens_skip":       # (nonspeech_skip trims the first windows to a fraction of a second: mostly padding, one language)
        assert len({w.language for w in want}) > 1, "the clips should not all detect the same language"
    assert sum(len(w.segments) for w in want) > 4
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = transcribe_many(mine, audios, max_tracks=max_tracks, **opts)
    _same(got, want, opts)


def test_many_language_list_and_single_code(models, monkeypatch):
    _, _, mine, audios = models
    from oracle_engine import install
    install(monkeypatch)
    langs = ["en", None, "de", "ja"]
    want = _expected(models, "defaults", langs)
    assert [w.language for w in want][0::2] == ["en", "de"] and want[3].language == "ja"
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = transcribe_many(mine, audios, language=langs, max_tracks=3, **BASE)
        _same(got, want, BASE)
        got = transcribe_many(mine, audios[:2], language="en", max_tracks=2, **BASE)
    _same(got, _expected(models, "defaults", ["en"] * 4)[:2], BASE)


def test_many_results_come_back_in_input_order(models, monkeypatch):
    """the 6-s clip finishes in the first round, the 47-s clip in the third: results are indexed by input position, whichever
    finished first; a silent recording yields language None and no segments without holding the others up; progress counts all
    recordings and ends at the total"""
    _, _, mine, audios = models
    from oracle_engine import install
    install(monkeypatch)
    order = [2, 1, 3, 0]
    clips = [audios[i] for i in order] + [torch.zeros(16000 * 8)]
    want = [_expected(models, "defaults", [None] * 4)[i] for i in order]
    seen = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = transcribe_many(mine, clips, max_tracks=2, progress_callback=lambda a, b: seen.append((a, b)), **BASE)
    _same(got[:4], want, BASE)
    assert got[4].language is None and len(got[4].segments) == 0
    total = sum(c.shape[-1] for c in clips) / 16000
    assert seen and all(b == total for _, b in seen) and [a for a, _ in seen] == sorted(a for a, _ in seen)
    assert seen[-1][0] <= total and seen[-1][0] >= total - 8.0 - 1e-6      # (the silent clip ends without a decoded round)


def test_many_option_errors_and_empty_list(models, monkeypatch):
    _, _, mine, audios = models
    from oracle_engine import install
    install(monkeypatch)
    assert transcribe_many(mine, [], **BASE) == []
    for bad in (dict(batch_size=2), dict(clip_timestamps=[0.0, 5.0]), dict(streams=2)):
        with pytest.raises(NotImplementedError):
            transcribe_many(mine, audios[:2], **BASE, **bad)
    with pytest.raises(ValueError, match="3 entries for 2 recordings"):
        transcribe_many(mine, audios[:2], language=["en", None, "de"], **BASE)
    with pytest.raises(ValueError):
        transcribe_many(mine, audios[:2], max_tracks=0, **BASE)
    with pytest.raises(TypeError):
        transcribe_many(mine, "clip.wav", **BASE)
    with pytest.raises(TypeError):
        transcribe_many(mine, audios[:1], no_such_option=1, **BASE)
    with pytest.raises(RuntimeError, match=r"audios\[1\]"):               # what transcribe() raises, with the index
        transcribe_many(mine, [audios[2], torch.zeros(0)], language="en", **BASE)


def test_many_keyboard_interrupt_marks_every_result(models, monkeypatch):
    """Ctrl-C in the second round: finished recordings are complete (-1), live ones carry their own seek, recordings that were
    never opened start at 0"""
    _, _, mine, audios = models
    from oracle_engine import install
    import stable_ts_amd.transcribe as T
    install(monkeypatch)
    real, calls = T._process_batch, {"n": 0}

    def flaky(*a, **kw):
        calls["n"] += 1
        if calls["n"] == 2:
            raise KeyboardInterrupt
        return real(*a, **kw)

    monkeypatch.setattr(T, "_process_batch", flaky)
    clips = [audios[2], audios[1], audios[3]]            # 6 s, 47 s, 19 s; two slots
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = transcribe_many(mine, clips, language="en", max_tracks=2, **BASE)
    assert len(got) == 3
    assert got[0].unfinished_start in (-1, -1.0) and len(got[0].segments) > 0          # done in round 1
    assert 0 < got[1].unfinished_start <= 30.0 and len(got[1].segments) > 0            # one window of it is in
    assert got[2].unfinished_start == 0.0 and len(got[2].segments) == 0                # took a slot in round 2: nothing decoded
