"""The head-selection variants of the word-timestamp stage (``dynamic_heads``, ``aligner='new'``, ``extra_models``) for all
windows of a batch in one pass: ``Engine.score_q_batch`` / ``heads_dynamic_batch`` / ``heads_new_batch`` (csrc/swx_headsel.hip
over a window axis) and the lockstep driver ``timing._find_alignment_variants``.

Oracle everywhere: the single-window calls / the per-window loop (``timing.HEADSEL_BATCH = False``), which
tests/test_gpu_golden.py and tests/hw_checks/score_qk_check.py tie to the reference.  Everything is compared bit for bit: the
arithmetic per (window, row, head) is the same code, and the project's batch invariance (tests/test_gpu_batch_invariance.py)
makes a window of a scoring pass the window alone.

Multilingual ``tiny`` (4 layers x 6 heads), seeded random weights, strict f32 and f16.  Three windows with 1, 9 and 40 text
tokens and 25, 987 and 1500 frames: the 25-frame window exercises the median filter's reflection at both ends.
"""
import ctypes
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
N_TEXT = (1, 9, 40)
N_FRAMES = (25, 987, 1500)
NAN_BITS = 0x7FC0BEEF            # a quiet NaN with a payload: "never written"
_CACHE = {}


def _synth_audio(seconds, seed):
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "golden", "make_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return torch.as_tensor(mod.synth_audio(seconds, seed), dtype=torch.float32)


def _model(dtype, seed=1234):
    import stable_ts_amd as sw
    if ("m", dtype, seed) not in _CACHE:
        dims = sw.dims_for("tiny")
        m = sw.Whisper(dims, dtype=dtype, max_windows=1, max_rows=5)
        m.load_state_dict(sw.random_state_dict(dims, seed=seed, std=0.02, embed_gain=2.0, ts_gain=0.5))
        _CACHE[("m", dtype, seed)] = m
    return _CACHE[("m", dtype, seed)]


def _world(dtype):
    """model, tokenizer, the three windows' mel and cross-K/V, their jobs"""
    if ("w", dtype) not in _CACHE:
        from stable_ts_amd.timing import AlignmentJob
        from stable_ts_amd.tokenizer import get_tokenizer
        model = _model(dtype)
        tok = get_tokenizer(True, num_languages=model.num_languages, language="en", task="transcribe")
        if "audio" not in _CACHE:
            _CACHE["audio"] = [_synth_audio(30.0, 41 + k)[:480000] for k in range(3)]
        mel = model.log_mel_batch(_CACHE["audio"])
        xkv = model.cross_kv(model.encoder(mel))
        rng = random.Random(5)
        texts = [[rng.randrange(300, 20000) for _ in range(n)] for n in N_TEXT]
        mk = lambda: [AlignmentJob(tok, t, F * 320) for t, F in zip(texts, N_FRAMES)]      # noqa: E731
        assert [j.n_frames for j in mk()] == list(N_FRAMES)
        _CACHE[("w", dtype)] = dict(model=model, tok=tok, mel=mel, xkv=xkv, jobs=mk)
    return _CACHE[("w", dtype)]


def _singles(dtype):
    """the single-window ``score_q`` state of every window (the oracle of parts 1 and 2), once per dtype"""
    if ("s", dtype) not in _CACHE:
        from stable_ts_amd.transcribe import _xkv_select
        w = _world(dtype)
        eng, tok = w["model"].engine, w["tok"]
        _CACHE[("s", dtype)] = [eng.score_q(_xkv_select(w["model"], w["xkv"], [k]), j.tokens, n_sot=len(tok.sot_sequence), eot=tok.eot)
                                for k, j in enumerate(w["jobs"]())]
    return _CACHE[("s", dtype)]


def _q_view(eng, st):
    """the captured queries of a batch state as [L, W, max_n, d]"""
    return st["q"].view(eng.tdtype).view(eng.dims.n_text_layer, st["W"], st["max_n"], eng.dims.n_text_state)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _batch_state_from_singles(dtype):
    """a batch state whose queries are the single-window passes' own, the padding rows NaN"""
    w = _world(dtype)
    eng, tok, jobs = w["model"].engine, w["tok"], w["jobs"]()
    st = eng.score_q_batch(w["xkv"], [j.tokens for j in jobs], n_sot=len(tok.sot_sequence), eot=tok.eot)
    qb = _q_view(eng, st)
    qb.fill_(float("nan"))
    for k, s in enumerate(_singles(dtype)):
        qb[:, k, :s["n"]] = s["q"].view(eng.tdtype).view(eng.dims.n_text_layer, s["n"], -1)
    return st


def _check_blocks(out, singles, rows, what):
    """every window's block equals the single-window matrix bit for bit; nothing else was written"""
    untouched = torch.full_like(_bits(out), NAN_BITS)
    for k, (single, n, F) in enumerate(zip(singles, rows, N_FRAMES)):
        assert single.shape[0] == n
        assert torch.equal(_bits(out[k, :n, :F]), _bits(single[:, :F])), (what, k)
        assert not torch.isnan(out[k, :n, :F]).any(), (what, k)
        untouched[k, :n, :F] = _bits(out[k, :n, :F])
    assert torch.equal(_bits(out), untouched), what


def _prefilled(eng, st):
    out = torch.empty(st["W"], st["max_n"] - st["n_sot"] - 1, eng.dims.n_audio_ctx, dtype=torch.float32, device=eng.device)
    out.view(torch.int32).fill_(NAN_BITS)
    return out


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_kernels_over_the_window_axis_equal_the_single_window_kernels(dtype):
    eng = _world(dtype)["model"].engine
    singles = _singles(dtype)
    st = _batch_state_from_singles(dtype)
    rows = [s["n"] - s["n_sot"] - 1 for s in singles]
    assert rows == [n + 1 for n in N_TEXT]
    # jump indices for the "midpoints" case: the DTW path of each window's own count=4 matrix
    first = [eng.heads_dynamic(s, F, count=4) for s, F in zip(singles, N_FRAMES)]
    jumps = []
    for neg, n, F in zip(first, rows, N_FRAMES):
        (ti, tj), = eng.dtw(neg[None, :, :F].contiguous(), [n], [F])
        jumps.append(tj[np.pad(np.diff(ti), (1, 0), constant_values=1).astype(bool)].clip(min=0))
    for opts, jj in ((dict(count=4), None), (dict(count=3), jumps), (dict(count=5, qk_scale=2.0), None)):
        want = first if opts == dict(count=4) else [eng.heads_dynamic(s, F, jump_indices=None if jj is None else jj[k], **opts)
                                                    for k, (s, F) in enumerate(zip(singles, N_FRAMES))]
        out = eng.heads_dynamic_batch(st, list(N_FRAMES), jump_indices_list=jj, out=_prefilled(eng, st), **opts)
        _check_blocks(out, want, rows, ("dynamic", opts, jj is not None))
    for opts in (dict(), dict(topk=7, w_coverage=0.5, medfilt_width=5)):
        want = [eng.heads_new(s, F, **opts) for s, F in zip(singles, N_FRAMES)]
        out = eng.heads_new_batch(st, list(N_FRAMES), out=_prefilled(eng, st), **opts)
        _check_blocks(out, want, rows, ("new", opts))


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_score_q_batch_equals_score_q(dtype):
    w = _world(dtype)
    eng, tok, jobs = w["model"].engine, w["tok"], w["jobs"]()
    singles = _singles(dtype)
    c0, w0 = eng.score_q_calls, eng.score_q_windows
    st = eng.score_q_batch(w["xkv"], [j.tokens for j in jobs], n_sot=len(tok.sot_sequence), eot=tok.eot)
    assert (eng.score_q_calls - c0, eng.score_q_windows - w0) == (1, 3)
    qb = _q_view(eng, st)
    for k, s in enumerate(singles):
        q1 = s["q"].view(eng.tdtype).view(eng.dims.n_text_layer, s["n"], -1)
        diff = (qb[:, k, :s["n"]].float() - q1.float()).abs().max().item()
        print(f"[score_q_batch {dtype}] window {k}: n_tok {s['n']}, max |q_batch - q_single| = {diff:.3e}")
        assert torch.equal(qb[:, k, :s["n"]], q1), k
        assert st["probs"][k] == s["probs"], k
    # a sub-batch is an offset into the buffer: windows 1..2 alone
    sub = eng.score_q_batch(w["xkv"], [j.tokens for j in jobs[1:]], n_sot=len(tok.sot_sequence), eot=tok.eot, window0=1)
    qs = _q_view(eng, sub)
    for k in (1, 2):
        assert torch.equal(qs[:, k - 1, :singles[k]["n"]], qb[:, k, :singles[k]["n"]]) and sub["probs"][k - 1] == singles[k]["probs"]


def test_batch_entries_refuse_bad_arguments():
    from stable_ts_amd._lib import SwxError
    w = _world("f16")
    eng, tok, jobs = w["model"].engine, w["tok"], w["jobs"]()
    n_sot = len(tok.sot_sequence)
    with pytest.raises(SwxError):                                  # a window with no text row at all
        eng.score_q_batch(w["xkv"], [jobs[0].tokens, jobs[0].tokens[:n_sot + 1]], n_sot=n_sot, eot=tok.eot)
    st = eng.score_q_batch(w["xkv"], [j.tokens for j in jobs], n_sot=n_sot, eot=tok.eot)
    st["scratch"] = torch.empty(1 << 20, dtype=torch.uint8, device=eng.device)
    need = eng.lib.swx_heads_batch_scratch_bytes(eng.h, 3, st["max_n"], 4)
    assert need > st["scratch"].numel()
    neg = torch.zeros(3, st["max_n"] - n_sot - 1, 1500, dtype=torch.float32, device=eng.device)
    frames = (ctypes.c_int32 * 3)(*N_FRAMES)
    n_tok = (ctypes.c_int32 * 3)(*st["n_tok"])
    call = lambda scratch_bytes, count: eng.lib.swx_heads_dynamic_batch(                                  # noqa: E731
        eng.h, ctypes.c_void_p(st["q"].data_ptr()), 3, st["max_n"], n_sot, n_tok, frames, st["xkv_ptr"], 3, 1.0, 7, count, None,
        ctypes.c_void_p(neg.data_ptr()), 1500, ctypes.c_void_p(st["scratch"].data_ptr()), scratch_bytes, eng.stream)
    assert call(st["scratch"].numel(), 4) == -8                    # short scratch
    assert call(st["scratch"].numel(), 0) == -1                    # no heads asked for
    torch.cuda.synchronize()
    assert not neg.any()


# ---------------------------------------------------------------------------------------------------------------- driver
def _align(dtype, opts, batch, budget=None):
    """``find_alignment_batch`` on the three jobs: (word timings, debug, score_q calls, score_q windows)"""
    import stable_ts_amd.timing as T
    w = _world(dtype)
    model, jobs = w["model"], w["jobs"]()
    kw = dict(opts)
    engines = [model.engine]
    if kw.pop("extra", False):
        kw["extra_models"] = [_model(dtype, seed=4321)]
        engines.append(kw["extra_models"][0].engine)
    before = [(e.score_q_calls, e.score_q_windows) for e in engines]
    old = T.HEADSEL_BATCH, T.HEADSEL_BATCH_BYTES
    T.HEADSEL_BATCH = batch
    if budget is not None:
        count = 0 if kw.get("aligner", "legacy") != "legacy" else (T.parse_dynamic_heads(kw.get("dynamic_heads"))[0] or 0)
        T.HEADSEL_BATCH_BYTES = budget(model.engine.headsel_window_bytes(max(len(j.tokens) for j in jobs), count) * len(engines))
    try:
        out = T.find_alignment_batch(model, jobs, w["xkv"], mel=w["mel"], return_debug=True, **kw)
    finally:
        T.HEADSEL_BATCH, T.HEADSEL_BATCH_BYTES = old
    calls = [e.score_q_calls - b[0] for e, b in zip(engines, before)]
    windows = [e.score_q_windows - b[1] for e, b in zip(engines, before)]
    return out, [j.debug for j in jobs], calls, windows


def _same_alignment(got, want):
    (gw, gd), (ww, wd) = got, want
    assert len(gw) == len(ww) == 3
    for a, b in zip(gw, ww):
        assert [(x.word, x.tokens, x.start, x.end) for x in a] == [(x.word, x.tokens, x.start, x.end) for x in b]
        np.testing.assert_array_equal(np.asarray([x.probability for x in a]), np.asarray([x.probability for x in b]))
    for a, b in zip(gd, wd):
        assert np.array_equal(a["path"][0], b["path"][0]) and np.array_equal(a["path"][1], b["path"][1])
        assert np.array_equal(a["jump_idx"], b["jump_idx"]) and a["token_probs"] == b["token_probs"]


DRIVER_CASES = {
    # name: (options, passes that keep the queries per model, refinement rounds)
    "dynamic": (dict(dynamic_heads=4), 1, 1),
    "dynamic_iterations": (dict(dynamic_heads="3,2"), 1, 2),
    "new": (dict(aligner="new"), 1, 1),
    "extra_models": (dict(extra=True), 0, 1),
    "extra_models_dynamic": (dict(extra=True, dynamic_heads=3), 1, 1),
}


@pytest.mark.parametrize("name", list(DRIVER_CASES))
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_driver_in_lockstep_equals_the_per_window_loop(dtype, name):
    opts, passes, rounds = DRIVER_CASES[name]
    want_w, want_d, loop_calls, loop_windows = _align(dtype, opts, batch=False)
    got_w, got_d, calls, windows = _align(dtype, opts, batch=True)
    _same_alignment((got_w, got_d), (want_w, want_d))
    # one pass per model, whatever the number of windows and rounds; the loop makes one per window and model
    assert calls == [passes] * len(calls) and windows == [3 * passes] * len(calls), (calls, windows)
    assert loop_calls == [3 * passes] * len(calls) and loop_windows == loop_calls
    # a budget that holds two windows (of every model's buffers) and not three: sub-batches of 2 + 1, the same results
    two = lambda per_window: 2 * per_window + 1024       # noqa: E731
    sub_w, sub_d, sub_calls, sub_windows = _align(dtype, opts, batch=True, budget=two)
    _same_alignment((sub_w, sub_d), (want_w, want_d))
    assert sub_calls == [2 * passes] * len(calls) and sub_windows == [3 * passes] * len(calls), (sub_calls, sub_windows)


# ---------------------------------------------------------------------------------------------------------------- end to end
def _with_switch(batch, fn):
    import stable_ts_amd.timing as T
    old = T.HEADSEL_BATCH
    T.HEADSEL_BATCH = batch
    try:
        return fn()
    finally:
        T.HEADSEL_BATCH = old


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_transcribe_and_align_many_reach_the_batched_stage(dtype):
    model = _model(dtype)
    eng = model.engine
    if "audio70" not in _CACHE:
        _CACHE["audio70"] = _synth_audio(70.0, 7)
        _CACHE["clips"] = [_synth_audio(4.0, 32).cuda(), _synth_audio(33.0, 33), _synth_audio(12.0, 37).cuda()]
    audio = _CACHE["audio70"]

    def counted(fn):
        c0, w0, e0 = eng.score_q_calls, eng.score_q_windows, eng.encode_calls
        res = fn()
        return res, eng.score_q_calls - c0, eng.score_q_windows - w0, eng.encode_calls - e0

    run = lambda: model.transcribe(audio, batch_size=3, dynamic_heads="3,2", language="en", temperature=0.0)      # noqa: E731
    want, loop_calls, loop_windows, _ = counted(lambda: _with_switch(False, run))
    got, calls, windows, passes = counted(lambda: _with_switch(True, run))
    print(f"[transcribe {dtype}] {passes} device passes, score_q calls {calls} (loop {loop_calls}) for {windows} windows")
    assert got.to_dict() == want.to_dict()
    assert len(got.all_words()) > 0 and windows == loop_windows == loop_calls > 0
    assert 0 < calls <= passes and calls < loop_calls

    rng = random.Random(11)
    texts = [[rng.randrange(300, 20000) for _ in range(n)] for n in (9, 70, 25)]
    langs = ["de", "en", "ja"]
    run = lambda: model.align_many(_CACHE["clips"], texts, langs, max_tracks=3, aligner="new")                      # noqa: E731
    want, loop_calls, loop_windows, _ = counted(lambda: _with_switch(False, run))
    got, calls, windows, passes = counted(lambda: _with_switch(True, run))
    print(f"[align_many {dtype}] {passes} device passes, score_q calls {calls} (loop {loop_calls}) for {windows} windows")
    assert [g.to_dict() for g in got] == [w.to_dict() for w in want]
    assert windows == loop_windows == loop_calls >= 3
    assert 0 < calls <= passes and calls < loop_calls
