"""The result writers at the end of the device path: what ``model.transcribe`` / ``model.transcribe_many`` return is
written as SRT, VTT, ASS, TSV, TXT and JSON and read back.

Multilingual ``tiny``, seeded random weights (the recipe of tests/test_gpu_transcribe_many.py), strict f32, the
synthetic audio of the other GPU tests.  The writers themselves are host code and are pinned byte for byte by
tests/test_text_output_cpu.py; here the point is that results as the device produces them go through every format, and
that a batch of recordings yields the subtitle files the recordings yield one by one.
"""
import os
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
BASE = dict(temperature=0.0, logprob_threshold=None, compression_ratio_threshold=None, no_speech_threshold=None, sample_len=24)
_CACHE = {}

SRT_TIMES = re.compile(r"^\d+\n(\d+):(\d\d):(\d\d),(\d\d\d) --> (\d+):(\d\d):(\d\d),(\d\d\d)$", re.M)
TSV_ROW = re.compile(r"^(\d+)\t(\d+)\t", re.M)


def _synth_audio(seconds, seed):
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "golden", "make_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return torch.as_tensor(mod.synth_audio(seconds, seed), dtype=torch.float32)


def _model():
    import stable_ts_amd as sw
    if "m" not in _CACHE:
        dims = sw.dims_for("tiny")
        m = sw.Whisper(dims, dtype="f32", max_windows=1, max_rows=5)
        m.load_state_dict(sw.random_state_dict(dims, seed=1234, std=0.02, embed_gain=2.0, ts_gain=0.5))
        _CACHE["m"] = m
    return _CACHE["m"]


def _ms(h, m, s, ms):
    return ((int(h) * 60 + int(m)) * 60 + int(s)) * 1000 + int(ms)


def test_transcribe_result_through_every_format(tmp_path, capsys):
    import stable_ts_amd as sw
    result = _model().transcribe(_synth_audio(35.0, 22).cuda(), language="en", **BASE)
    clean = result.apply_min_dur(0.02, inplace=False)
    assert len(clean.segments) >= 1 and clean.has_words        # there is something to write
    before = result.to_dict()
    capsys.readouterr()

    paths = {ext: str(tmp_path / f"clip.{ext}") for ext in ("srt", "vtt", "ass", "tsv", "txt")}
    result.to_srt_vtt(paths["srt"], word_level=False)
    result.to_srt_vtt(paths["vtt"])
    result.to_ass(paths["ass"])
    result.to_tsv(paths["tsv"], word_level=True)
    result.to_txt(paths["txt"])
    printed = capsys.readouterr().out.splitlines()
    assert printed == [f"Saved: {os.path.abspath(p)}" for p in paths.values()]
    text = {}
    for ext, p in paths.items():
        with open(p, "r", encoding="utf-8", newline="") as f:
            text[ext] = f.read()
    assert text["vtt"].startswith("WEBVTT\n\n") and text["ass"].startswith("[Script Info]\n")
    assert text["ass"].count("\nDialogue: ") == len(clean.segments)
    assert text["txt"] == "\n".join(s.text.strip() for s in clean.segments)

    cues = SRT_TIMES.findall(text["srt"])                          # segment level: one cue per segment, at its times
    assert len(cues) == len(clean.segments)
    for c, s in zip(cues, clean.segments):
        assert (_ms(*c[:4]), _ms(*c[4:])) == (round(s.start * 1000), round(s.end * 1000))

    rows = TSV_ROW.findall(text["tsv"])                            # word level: one row per word
    words = clean.all_words()
    assert len(rows) == len(words) >= len(clean.segments)
    assert [(int(a), int(b)) for a, b in rows] == [(round(w.start * 1000), round(w.end * 1000)) for w in words]

    sw.save_as_json(result, str(tmp_path / "clip"))                # the module-level function appends .json
    again = sw.WhisperResult(sw.load_result(str(tmp_path / "clip.json")))
    assert again.to_srt_vtt() == result.to_srt_vtt()
    assert again.to_srt_vtt(vtt=True) == text["vtt"]
    assert result.to_dict() == before                              # writing changed nothing in the result


def test_transcribe_many_gives_the_same_subtitles(tmp_path):
    model = _model()
    clips = [_synth_audio(sec, seed).cuda() for sec, seed in ((4.0, 21), (12.0, 25), (20.0, 24))]
    many = model.transcribe_many(clips, language="en", max_tracks=3, **BASE)
    assert len(many) == 3 and sum(len(r.segments) for r in many) >= 1
    for i, (clip, got) in enumerate(zip(clips, many)):
        alone = model.transcribe(clip, language="en", **BASE)
        assert got.to_srt_vtt() == alone.to_srt_vtt(), i
        assert got.to_ass() == alone.to_ass(), i
    many[-1].to_srt_vtt(str(tmp_path / "last"))                    # no extension given: SRT
    with open(tmp_path / "last.srt", "r", encoding="utf-8", newline="") as f:
        assert f.read() == many[-1].to_srt_vtt()
