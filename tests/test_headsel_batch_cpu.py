"""The lockstep driver of the head-selection variants (``timing._find_alignment_variants``) on the CPU oracle stand-in.

The stand-in (tests/oracle_engine.py) has no batch calls, so ``find_alignment_batch`` takes the per-window loop on it.  Here it
is wrapped in an engine that OFFERS the three batch calls -- as loops over the stand-in's single-window ones, so the arithmetic
is the same by construction -- and records every call.  What is checked is the control flow of the batched driver:

* it returns exactly what the per-window loop returns (words, times, probabilities, DTW paths);
* it makes one scoring pass per model, one matrix call per model and refinement round, one ``dtw`` call per round;
* it never gathers a single window out of the cross-K/V buffer (``_xkv_select``).
"""
import os
import random
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)

import stable_ts_amd.timing as T  # noqa: E402
import stable_ts_amd.transcribe as TR  # noqa: E402
from stable_ts_amd.tokenizer import get_tokenizer  # noqa: E402

N_TEXT = (1, 9, 40)                          # text tokens per window
N_SAMPLES = (25 * 320, 987 * 320, 480000)    # 25, 987 and 1500 frames


class BatchingEngine:
    """the stand-in's engine plus the three batch calls, each a loop over the single-window call; every call is logged"""

    def __init__(self, inner, log, name):
        self._inner, self._log, self._name = inner, log, name

    def __getattr__(self, item):
        return getattr(self._inner, item)

    def score(self, *a, **kw):
        self._log.append((self._name, "score", len(a[1])))
        return self._inner.score(*a, **kw)

    def score_q(self, *a, **kw):
        self._log.append((self._name, "score_q", 1))
        return self._inner.score_q(*a, **kw)

    def dtw(self, neg, N, M):
        self._log.append((self._name, "dtw", len(N)))
        return self._inner.dtw(neg, N, M)

    def pool_matrices(self, negs, n_heads):
        self._log.append((self._name, "pool", int(negs[0].shape[0])))
        return self._inner.pool_matrices(negs, n_heads)

    def score_q_batch(self, xkv, tokens_list, *, n_sot, eot, window0=0):
        self._log.append((self._name, "score_q_batch", len(tokens_list)))
        states = [self._inner.score_q(xkv.select([window0 + k]), t, n_sot=n_sot, eot=eot) for k, t in enumerate(tokens_list)]
        return dict(states=states, n_sot=n_sot, max_n=max(len(t) for t in tokens_list), probs=[s["probs"] for s in states])

    def _stack(self, st, mats):
        out = torch.zeros(len(mats), st["max_n"] - st["n_sot"] - 1, self._inner.dims.n_audio_ctx)
        for w, m in enumerate(mats):
            out[w, :m.shape[0]] = m
        return out

    def heads_dynamic_batch(self, st, n_frames_list, *, count, qk_scale=1.0, medfilt_width=7, jump_indices_list=None):
        self._log.append((self._name, "heads_dynamic_batch", len(n_frames_list)))
        jumps = jump_indices_list or [None] * len(n_frames_list)
        return self._stack(st, [self._inner.heads_dynamic(s, F, count=count, qk_scale=qk_scale, medfilt_width=medfilt_width,
                                                          jump_indices=j) for s, F, j in zip(st["states"], n_frames_list, jumps)])

    def heads_new_batch(self, st, n_frames_list, **options):
        self._log.append((self._name, "heads_new_batch", len(n_frames_list)))
        return self._stack(st, [self._inner.heads_new(s, F, **options) for s, F in zip(st["states"], n_frames_list)])


@pytest.fixture(scope="module")
def world():
    import make_golden as G
    from oracle.whisper.model import build_model
    from oracle_engine import CpuWhisper
    main = CpuWhisper(build_model("tiny", seed=77, std=0.02, embed_gain=2.0, ts_gain=0.5))
    other = CpuWhisper(build_model("tiny", seed=78, std=0.02, embed_gain=2.0, ts_gain=0.5))
    main.manual_attention_encoder = other.manual_attention_encoder = True
    tok = get_tokenizer(True, num_languages=main.num_languages, language="en", task="transcribe")
    rng = random.Random(5)
    texts = [[rng.randrange(300, 20000) for _ in range(n)] for n in N_TEXT]
    audios = [torch.as_tensor(G.synth_audio(30.0, seed=41 + k), dtype=torch.float32)[:480000] for k in range(3)]
    mel = main.log_mel_batch([torch.nn.functional.pad(a, (0, 480000 - a.shape[-1])) for a in audios])
    xkv = main.cross_kv(main.encoder(mel))
    return dict(main=main, other=other, tok=tok, texts=texts, mel=mel, xkv=xkv)


def _jobs(world):
    return [T.AlignmentJob(world["tok"], t, n) for t, n in zip(world["texts"], N_SAMPLES)]


def _run(world, opts, monkeypatch, wrap):
    """(word timings per window, debug per window, call log) of ``find_alignment_batch`` with the engines wrapped or not"""
    from oracle_engine import install
    install(monkeypatch)
    log, selects = [], []
    real_select = TR._xkv_select
    monkeypatch.setattr(TR, "_xkv_select", lambda model, xkv, idx: (selects.append(list(idx)), real_select(model, xkv, idx))[1])
    main, other = world["main"], world["other"]
    if wrap:
        monkeypatch.setattr(main, "engine", BatchingEngine(main.engine, log, "main"))
        monkeypatch.setattr(other, "engine", BatchingEngine(other.engine, log, "other"))
    kw = dict(opts)
    if kw.pop("extra", False):
        kw["extra_models"] = [other]
    jobs = _jobs(world)
    out = T.find_alignment_batch(main, jobs, world["xkv"], mel=world["mel"], return_debug=True, **kw)
    return out, [j.debug for j in jobs], log, selects


def _same(got, want):
    (gw, gd), (ww, wd) = got, want
    assert len(gw) == len(ww) == 3
    for a, b in zip(gw, ww):
        assert [(x.word, x.tokens, x.start, x.end) for x in a] == [(x.word, x.tokens, x.start, x.end) for x in b]
        np.testing.assert_array_equal(np.asarray([x.probability for x in a]), np.asarray([x.probability for x in b]))
    for a, b in zip(gd, wd):
        assert np.array_equal(a["path"][0], b["path"][0]) and np.array_equal(a["path"][1], b["path"][1])
        assert np.array_equal(a["jump_idx"], b["jump_idx"]) and a["token_probs"] == b["token_probs"]


CASES = {
    # name: (options, models, refinement rounds, name of the batch matrix call)
    "dynamic_iterations": (dict(dynamic_heads="3,2"), 1, 2, "heads_dynamic_batch"),
    "new": (dict(aligner="new"), 1, 1, "heads_new_batch"),
    "extra_models": (dict(extra=True), 2, 1, "score"),
    "extra_models_dynamic": (dict(extra=True, dynamic_heads="3,2"), 2, 2, "heads_dynamic_batch"),
}


@pytest.mark.parametrize("name", list(CASES))
def test_batched_driver_equals_per_window_loop(world, monkeypatch, name):
    opts, n_models, rounds, matrix_call = CASES[name]
    with monkeypatch.context() as mp:
        want_words, want_debug, _, want_selects = _run(world, opts, mp, wrap=False)
    assert any(len(s) == 1 for s in want_selects)            # the per-window loop gathers single windows: the spy sees them
    got_words, got_debug, log, selects = _run(world, opts, monkeypatch, wrap=True)
    _same((got_words, got_debug), (want_words, want_debug))
    calls = lambda what: [c for c in log if c[1] == what]                                     # noqa: E731
    assert not calls("score_q"), log                          # no single-window pass
    assert all(n == 3 for _, _, n in log), log                # every call carries all three windows
    assert len(calls(matrix_call)) == n_models * rounds, log
    assert len(calls("dtw")) == rounds, log
    if matrix_call != "score":
        assert sorted(c[0] for c in calls("score_q_batch")) == ["main", "other"][:n_models], log      # one pass per model
    assert len(calls("pool")) == (rounds if n_models > 1 else 0), log
    assert not [s for s in selects if len(s) == 1], selects   # no window is gathered out of the batch buffer


def test_switch_selects_the_per_window_loop(world, monkeypatch):
    """``HEADSEL_BATCH = False`` takes the loop on an engine that has the batch calls"""
    monkeypatch.setattr(T, "HEADSEL_BATCH", False)
    _, _, log, selects = _run(world, dict(dynamic_heads=3), monkeypatch, wrap=True)
    assert [c[1] for c in log].count("score_q") == 3 and not [c for c in log if c[1].endswith("_batch")]
    assert sorted(s[0] for s in selects if len(s) == 1) == [0, 1, 2]
