"""``refine(batch_size=N)`` on hardware: the native probe (``swx_forward_token_ranks``: a probability and a rank per token leave the
device, no distribution) and the lockstep word groups.

* tests/hw_checks/refine_lockstep_check.py first, in a child process: the new entry points through the C ABI (ranks exact against
  the device's own logits, probabilities against float64 within twice ``swx_score``'s own deviation, batch invariance W = 6 vs
  W = 2 bit for bit, the grouped log-mel clamp floor).  Its report is profiles/refine_lockstep_report.json.
* end to end on the four option sets of tests/golden/reference_refine_e2e.json: ``batch_size`` 1 and 4 meet the bar of
  tests/test_gpu_golden.py::test_refine_end_to_end_matches_reference (every word within 20 ms of the reference's refine(), the
  same number of words moved).
* end to end on a recording with several word groups: 126 s of synthetic audio, the golden case's sharp tiny.en weights, a
  starting result made by this package's ``align()`` (one call per 21-s passage -- on random weights a single ``align()`` over two
  minutes collapses most words into the last seconds, which leaves two groups -- joined into one result of 6 segments, >= 4
  groups).  f32: ``refine(batch_size=4)``, ``refine(batch_size=1)`` and ``refine()`` give EQUAL word times; f16: every word within
  20 ms.  ``prob_threshold=0`` because random weights give word probabilities of ~1e-5 (as in the golden's option sets),
  ``precision=0.02`` so that a 0.2-s word takes three bisection rounds; that at least half of the (step, group) pairs run >= 2
  rounds and that words move is asserted on the default path's own run.
"""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHUNK_S, N_CHUNKS = 21.0, 6
KW = dict(prob_threshold=0.0, precision=0.02)


def _synth_audio(seconds, seed):
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "golden", "make_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.synth_audio(seconds, seed)


def _model(case, dtype="f32", max_windows=1):
    import stable_ts_amd as sw
    dims = sw.dims_for(case["model"])
    m = sw.Whisper(dims, dtype=dtype, max_windows=max_windows, max_rows=5)
    m.load_state_dict(sw.random_state_dict(dims, seed=1234, std=0.02, embed_gain=case["gain"], ts_gain=case["ts_gain"]))
    return m


def test_device_paths_in_a_child_process(tmp_path):
    from conftest import subprocess_env
    report = tmp_path / "refine_lockstep_report.json"
    r = subprocess.run([sys.executable, os.path.join(HERE, "hw_checks", "refine_lockstep_check.py"), "--report", str(report)],
                       capture_output=True, text=True, timeout=900, env=subprocess_env())
    print(r.stdout[-4000:])
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-4000:])
    rep = json.loads(report.read_text())
    assert sorted(rep) == ["base.en/f16", "base.en/f32", "tiny.en/f16", "tiny.en/f32"]
    for key, v in rep.items():
        assert v["rank_mismatches"] == 0 and v["prob_max_rel_err_vs_f64"] <= v["prob_allowed"] and all(v["window_of_w6_equals_w2"]), (key, v)


@pytest.mark.parametrize("batch_size", [1, 4])
@pytest.mark.parametrize("name", ["default_thresholds", "both_ends", "coarse_rel", "starts_only"])
def test_refine_end_to_end_matches_reference(name, batch_size):
    from stable_ts_amd.result import WhisperResult
    with open(os.path.join(HERE, "golden", "reference_refine_e2e.json")) as f:
        g = json.load(f)
    case, want = g["case"], g["refined"][name]
    model = _model(case)
    audio = _synth_audio(case["seconds"], case["seed"])
    words = [dict(w) for w in g["before"]]
    res = WhisperResult(dict(segments=[dict(start=words[0]["start"], end=words[-1]["end"], text="".join(w["word"] for w in words),
                                            words=words)], language="en"))
    out = model.refine(audio, res, verbose=None, batch_size=batch_size, **want["kw"])
    got = out.all_words()
    assert [w.word for w in got] == [w["word"] for w in want["words"]]
    dev = [max(abs(a.start - b["start"]), abs(a.end - b["end"])) for a, b in zip(got, want["words"])]
    close = sum(d <= 0.02 + 1e-9 for d in dev)
    moved_ref = sum(abs(a["start"] - b["start"]) > 1e-9 or abs(a["end"] - b["end"]) > 1e-9 for a, b in zip(g["before"], want["words"]))
    moved_got = sum(abs(a["start"] - b.start) > 1e-9 or abs(a["end"] - b.end) > 1e-9 for a, b in zip(g["before"], got))
    print(name, batch_size, dict(words=len(dev), within_20ms=close, max_dev=max(dev), moved_ref=moved_ref, moved_got=moved_got))
    assert close == len(dev) and max(dev) <= 0.02 + 1e-9, (close, len(dev), max(dev), moved_ref, moved_got)
    assert moved_got == moved_ref, (moved_got, moved_ref)


def test_refine_batch_size_is_a_new_keyword():
    """``refine(batch_size=4)`` raised TypeError before this feature (the keyword fell through to ``Refiner``'s unknown options)"""
    from stable_ts_amd.result import WhisperResult
    with open(os.path.join(HERE, "golden", "reference_refine_e2e.json")) as f:
        g = json.load(f)
    model = _model(g["case"])
    words = [dict(w) for w in g["before"]]
    res = WhisperResult(dict(segments=[dict(start=words[0]["start"], end=words[-1]["end"], text="".join(w["word"] for w in words),
                                            words=words)], language="en"))
    out = model.refine(_synth_audio(g["case"]["seconds"], g["case"]["seed"]), res, batch_size=4, single_batch=True, steps="s")
    assert len(out.all_words()) == len(words)
    with pytest.raises(ValueError):
        model.refine(torch.zeros(16000), res, batch_size=0)


def _start(model, text):
    """this package's align() per 21-s passage, joined: (audio [126 s], result dict of 6 segments)"""
    chunks = [_synth_audio(CHUNK_S, 4 + k) for k in range(N_CHUNKS)]
    segs = []
    for k, c in enumerate(chunks):
        r = model.align(c, text, language="en")
        ws = [dict(word=w.word, start=round(w.start + CHUNK_S * k, 3), end=round(w.end + CHUNK_S * k, 3),
                   probability=w.probability, tokens=list(w.tokens)) for w in r.all_words()]
        segs.append(dict(start=ws[0]["start"], end=ws[-1]["end"], text=text, words=ws))
    return torch.cat(chunks), dict(segments=segs, language="en")


def _times(res):
    return [(w.word, w.start, w.end) for w in res.all_words()]


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_refine_lockstep_equals_sequential_on_many_groups(dtype):
    from stable_ts_amd.result import WhisperResult
    with open(os.path.join(HERE, "golden", "reference_glue.json")) as f:
        g = json.load(f)["align_tiny_en"]
    model = _model(g["case"], dtype)
    audio, rd = _start(model, g["text"])
    before = _times(WhisperResult(rd))

    # the default path, with the probes of every group of every step counted where they are issued: one generator = one group
    from stable_ts_amd.refiner import Refiner
    calls = []
    real = Refiner._group_rounds

    def counted(self, *a):
        mine = [a[-1], 0]                                   # [at_end, probes]
        calls.append(mine)
        gen = real(self, *a)
        answer = None
        while True:
            try:
                request = gen.send(answer)
            except StopIteration:
                return
            mine[1] += 1
            answer = yield request
    Refiner._group_rounds = counted
    try:
        today = model.refine(audio, WhisperResult(rd), **KW)
    finally:
        Refiner._group_rounds = real
    groups = len([c for c in calls if not c[0]])
    busy = sum(1 for c in calls if c[1] - 1 >= 2)                # first probe = the reference probe
    moved = sum(a != b for a, b in zip(before, _times(today)))
    print(dtype, dict(groups=groups, group_steps=len(calls), with_2_rounds=busy, moved=moved, words=len(before)))
    assert groups >= 4 and 2 * busy >= len(calls) and moved >= 1

    one = model.refine(audio, WhisperResult(rd), batch_size=1, **KW)
    four = model.refine(audio, WhisperResult(rd), batch_size=4, **KW)
    if dtype == "f32":
        assert _times(one) == _times(four)               # batch invariance: a window's numbers do not depend on the batch
        assert _times(four) == _times(today)
    else:
        for got in (one, four):
            dev = [max(abs(a[1] - b[1]), abs(a[2] - b[2])) for a, b in zip(_times(got), _times(today))]
            print(dtype, "max deviation from the default path", max(dev))
            assert max(dev) <= 0.02 + 1e-9, max(dev)
        dev = [max(abs(a[1] - b[1]), abs(a[2] - b[2])) for a, b in zip(_times(one), _times(four))]
        assert max(dev) <= 0.02 + 1e-9
