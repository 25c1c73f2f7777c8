"""Result writers (stable_ts_amd/text_output.py and their WhisperResult methods) against the reference's own writers.

* golden: tests/golden/text_output_cases.json.gz holds what /root/reference's writers returned, wrote, printed, warned
  and raised for seeded synthetic results, the stored JFK result and hand-made edge results over a grid of options
  (tests/golden/make_text_output_golden.py).  These are strings built from the same numbers: equality, no tolerance.
* live: where /root/reference is importable (this container) a few hundred random option sets run against it as well.
"""
import gzip
import json
import os
import random
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

from make_text_output_golden import GRID, NOT_A_RESULT, all_inputs, random_case, run_case  # noqa: E402

import stable_ts_amd  # noqa: E402
from stable_ts_amd import text_output  # noqa: E402
from stable_ts_amd.result import WhisperResult  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    with gzip.open(os.path.join(HERE, "golden", "text_output_cases.json.gz"), "rb") as f:
        return json.loads(f.read().decode("utf-8"))


def test_public_surface():
    for name in ("to_srt_vtt", "to_ass", "to_tsv", "to_txt"):
        assert callable(getattr(WhisperResult, name)), name
    for name in ("result_to_srt_vtt", "result_to_ass", "result_to_tsv", "result_to_txt", "save_as_json", "load_result"):
        assert getattr(stable_ts_amd, name) is getattr(text_output, name), name
        assert name in text_output.__all__
    assert text_output.SUPPORTED_FORMATS == ("srt", "vtt", "ass", "tsv", "txt")
    assert WhisperResult.to_srt_vtt is text_output.result_to_srt_vtt       # bound as the reference binds them
    assert WhisperResult.to_ass is text_output.result_to_ass
    assert WhisperResult.to_tsv is text_output.result_to_tsv
    assert WhisperResult.to_txt is text_output.result_to_txt
    assert callable(text_output.result_to_any)


def test_fixture_covers_the_grid(golden):
    inputs = golden["inputs"]
    assert json.loads(json.dumps(all_inputs())) == inputs          # the generator's inputs are deterministic
    assert sum(1 for n in inputs if n.startswith("synth")) >= 12 and "jfk" in inputs
    seen = {(c["fn"], c["kwargs"], c["file"]) for c in golden["cases"]}
    assert seen == {(fn, repr(kw), file) for fn, kw, file in GRID}
    for name in inputs:
        forms = {"dict", "list"} if name in NOT_A_RESULT else {"obj", "dict", "list"}
        assert {c["form"] for c in golden["cases"] if c["input"] == name} == forms, name
    calls = [r for c in golden["cases"] for r in c["calls"]]
    assert any(r.get("error") == "NotImplementedError" for r in calls)
    assert any(r.get("error") == "AssertionError" for r in calls)
    assert any(r.get("error") == "TypeError" for r in calls)
    assert any(r.get("files") for r in calls) and any(r.get("warnings") for r in calls)
    assert any(r.get("words_after") for r in calls)


def _compare(case, got, want):
    key = (case["input"], case["form"], case["fn"], case["kwargs"], case["file"])
    assert len(got) == len(want), key
    for n, (g, w) in enumerate(zip(got, want)):
        where = key + (f"call {n}",)
        assert "setup_error" not in g and "setup_error" not in w, where        # every input can be built
        assert g["error"] == w["error"], where + (g["error"], w["error"])
        assert g.get("message") == w.get("message"), where
        assert g["ret"] == w["ret"], where
        assert sorted(g["files"]) == sorted(w["files"]), where                  # the names the reference chose
        assert g["files"] == w["files"], where
        assert g["stdout"] == w["stdout"], where
        if w["files"]:
            assert g["stdout"] == f"Saved: {os.path.join('<TMP>', next(iter(w['files'])))}\n", where
        assert [c for c, _ in g["warnings"]] == [c for c, _ in w["warnings"]], where + (g["warnings"], w["warnings"])
        assert g["warnings"] == w["warnings"], where
        assert g.get("loaded_equals_saved") == w.get("loaded_equals_saved"), where
        assert g.get("words_after") == w.get("words_after"), where              # the same edits to a caller's dict
        if case["form"] == "obj":
            # the caller's result is left alone (the reference's own copy shares the text of word-less segments with
            # the caller's, so its record can say False there; what it writes is the same either way)
            assert g["unchanged"] is True, where


def test_writers_match_reference_golden(golden, tmp_path):
    tmp = os.path.realpath(str(tmp_path))
    assert len(golden["cases"]) >= 2000
    for case in golden["cases"]:
        got = json.loads(json.dumps(run_case(stable_ts_amd, case, golden["inputs"], tmp)))
        _compare(case, got, case["calls"])


def test_segment_to_dict_default_is_unchanged(golden):
    """``reverse_text`` is new on ``Segment.to_dict`` / ``segments_to_dicts``; without it nothing may change."""
    for name, inp in golden["inputs"].items():
        try:
            res = WhisperResult(json.loads(json.dumps(inp)))
        except Exception:
            continue
        plain = res.segments_to_dicts()
        assert plain == res.segments_to_dicts(reverse_text=False) == [s.to_dict() for s in res.segments]
        assert all("reversed_text" not in d for d in plain)
        assert res.to_dict()["segments"] == plain


@pytest.mark.skipif(not os.path.isdir("/root/reference/stable_whisper"), reason="reference checkout not present")
def test_writers_match_reference_live(golden, tmp_path):
    from make_golden import import_reference
    sw = import_reference()
    rng = random.Random(20240607)
    inputs = golden["inputs"]
    tmp = os.path.realpath(str(tmp_path))
    raised = 0
    for _ in range(400):
        case = random_case(rng, inputs)
        want = json.loads(json.dumps(run_case(sw, case, inputs, tmp)))
        got = json.loads(json.dumps(run_case(stable_ts_amd, case, inputs, tmp)))
        _compare(case, got, want)
        raised += any(r.get("error") or r.get("setup_error") for r in want)
    assert raised < 300                                 # most random option sets are valid calls
