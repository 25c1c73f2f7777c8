"""``refine_many``: the driver that bisects the word groups of many recordings in lockstep (``stable_ts_amd.refiner.refine_tracks``)
against ``Refiner.refine`` per recording, and the recorded probe edits (``OpsProbe``) against the host tensor (``HostProbe``),
all on the seeded synthetic inference function of tests/golden/make_refiner_golden.py (one function per recording, by its seed).

Seven recordings: five seeded cases (``steps="se"``, groups of at most 12 tokens), one result without any word and one with a
single word.  Every group must see the same probes round for round -- a hash of the two audio copies of every call, keyed by
(recording, step, group) -- and every timestamp must be equal, for ``max_tracks`` 1, 3 and 64 in the three output forms.
That the comparison is not vacuous is asserted on the sequential driver's own run.
"""
import copy
import hashlib
import os
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import make_refiner_golden as mg  # noqa: E402

from stable_ts_amd.refiner import HostProbe, OpsProbe, Refiner, refine_tracks, token_rank  # noqa: E402
from stable_ts_amd.result import WhisperResult  # noqa: E402

SEEDS = (602, 606, 610, 612, 613, 618)
MAX_TRACKS = (1, 3, 64)
FORMS = ("2d", "3d", "rank")


def apply_ops(clean, probe, ops):
    """the oracle: ordered writes, so for every sample the last op of its row that covers it wins; kind 0 = +0.0, 1 = clean"""
    for row, a, b, kind in ops:
        probe[row, a:b] = clean[row >> 1, a:b] if kind else 0.0
    return probe


def _bits(t):
    return np.ascontiguousarray(np.asarray(t, dtype=np.float32)).view(np.int32)


class Both:
    """a probe buffer that is the host tensor AND the recorder: every write goes to both"""

    def __init__(self, clean):
        self.host, self.rec, self.clean = HostProbe(clean), OpsProbe(clean), clean
        self.audio = self.host.audio

    def mute(self, row, a, b):
        self.host.mute(row, a, b)
        self.rec.mute(row, a, b)

    def restore(self, row, a, b):
        self.host.restore(row, a, b)
        self.rec.restore(row, a, b)


class Logged(Refiner):
    """logs a hash of every probe under (recording, step, group) and, with ``Both`` buffers, replays the recorded ops of every
    round on a copy of the clean segment and compares with the host tensor bit for bit"""
    rec, log, replays = None, None, None

    def probe_buffer(self, clean):
        self._made = Both(clean)
        return self._made

    def _group_rounds(self, words, g_lo, g_hi, edge, at_end):
        gen = super()._group_rounds(words, g_lo, g_hi, edge, at_end)
        key = (self.rec, int(at_end), round(float(g_lo[0]), 6), tuple(t for w in words for t in w.tokens))
        ops, buf, answer = [], None, None
        while True:
            try:
                request = gen.send(answer)
            except StopIteration:
                return
            if buf is None:
                buf = self._made                                      # made by the generator's first step, just now
            self.log.setdefault(key, []).append(hashlib.sha1(request[0].contiguous().numpy().tobytes()).hexdigest())
            ops += buf.rec.take()
            want = apply_ops(buf.clean.numpy(), buf.clean.numpy().repeat(2, 0), ops)
            assert np.array_equal(_bits(want), _bits(request[0].numpy())), key
            self.replays[0] += 1
            answer = yield request


def _ranked(dist_fn):
    def infer(audio, tokens):
        dist = dist_fn(audio, tokens)
        ids = [int(t) for t in tokens]
        pos = torch.arange(len(ids))
        rank = torch.tensor([[token_rank(dist[r, j].numpy(), ids[j]) for j in range(len(ids))] for r in range(2)])
        return dist[:, pos, ids], rank
    return infer


def _cases():
    """[(seed of the inference function, audio, result dict, options)]: five seeded cases, an empty result, a single word"""
    out = []
    for seed in SEEDS[:5]:
        audio, rd, opts, _ = mg.synth_case(seed)
        for s in rd["segments"]:
            for w in s["words"]:
                w["tokens"] = [int(t) % mg.VOCAB for t in w["tokens"]]
        out.append((seed, audio, rd, dict(opts, steps="se", max_inference_tokens=12)))
    seed = SEEDS[5]
    audio, rd, opts, _ = mg.synth_case(seed)
    opts = dict(opts, steps="se", max_inference_tokens=12)
    out.append((seed, audio, dict(language="en", segments=[]), opts))
    word = next(dict(w, tokens=[int(t) % mg.VOCAB for t in w["tokens"]], probability=0.9) for s in rd["segments"] for w in s["words"]
                if w["end"] - w["start"] >= 0.5)
    out.append((seed, audio, dict(language="en", segments=[dict(start=word["start"], end=word["end"], text=word["word"],
                                                                words=[word])]), opts))
    return out


def _refiners(form, log, replays):
    made = []
    for rec, (seed, audio, rd, opts) in enumerate(_cases()):
        fn = mg.make_inference(seed, form != "2d")
        if form == "rank":
            fn = _ranked(fn)
            fn.batch = lambda items, fn=fn: [fn(a, t) for a, t in items]
        r = Logged(fn, **opts)
        r.rec, r.log, r.replays = rec, log, replays
        made.append((r, audio, WhisperResult(copy.deepcopy(rd))))
    return made


@pytest.fixture(scope="module")
def sequential():
    """form -> (snapshots, log, snapshots before) of ``Refiner.refine`` per recording (the empty result is left out of the loop:
    ``Refiner.refine`` raises IndexError on a result without words, ``refine_tracks`` hands it back as it is)"""
    cache = {}

    def run(form):
        if form not in cache:
            log, replays = {}, [0]
            snaps, before = [], []
            for r, audio, res in _refiners(form, log, replays):
                before.append(mg.snapshot(res))
                snaps.append(mg.snapshot(r.refine(audio, res) if res.all_words() else res))
            assert replays[0] == sum(len(v) for v in log.values()) > 0
            cache[form] = (snaps, log, before)
        return cache[form]
    return run


def test_refine_alone_raises_on_a_result_without_words():
    seed, audio, rd, opts = _cases()[5]
    with pytest.raises(IndexError):
        Refiner(mg.make_inference(seed, False), **opts).refine(audio, WhisperResult(copy.deepcopy(rd)))


@pytest.mark.parametrize("form", FORMS)
def test_sequential_run_is_not_vacuous(sequential, form):
    snaps, log, before = sequential("3d" if form == "rank" else form)
    assert len([k for k in log if k[1] == 0]) >= 4
    assert {k[1] for k in log} == {0, 1}
    busy = sum(1 for v in log.values() if len(v) - 1 >= 2)               # the first call is the reference probe
    assert 2 * busy >= len(log), (busy, len(log))
    nonempty = [i for i, b in enumerate(before) if b]
    moved = sum(snaps[i] != before[i] for i in nonempty)
    assert len(nonempty) == 6 and moved >= 0.8 * len(nonempty), (moved, len(nonempty))


@pytest.mark.parametrize("form", FORMS)
def test_many_equals_the_loop(sequential, form):
    """the same probes round for round (which also replays every round's recorded ops against the host tensor) and equal times"""
    want, want_log, _ = sequential("3d" if form == "rank" else form)
    for max_tracks in MAX_TRACKS:
        log, replays = {}, [0]
        made = _refiners(form, log, replays)
        refiners = [r for r, _, _ in made]
        work = [r._prepare(audio, res) for r, audio, res in made]
        done = []
        out = refine_tracks(refiners, work, max_tracks, progress_callback=lambda a, b: done.append((a, b)))
        assert [mg.snapshot(r) for r in out] == want, (form, max_tracks)
        assert log == want_log, (form, max_tracks)
        assert replays[0] == sum(len(v) for v in log.values())
        total = sum(a.shape[-1] for _, a, _ in made) / 16000
        assert done and abs(done[-1][1] - total) <= 0.011 and [d[0] for d in done] == sorted(d[0] for d in done)
        assert abs(done[-1][0] - done[-1][1]) <= 0.011                   # every step of every recording is done at the end
        for res in out:
            assert [s.id for s in res.segments] == list(range(len(res.segments)))


def test_rounds_hold_at_most_max_tracks_groups_and_slots_are_refilled():
    """``answer`` sees min(max_tracks, groups not yet finished) requests; a slot keeps its group until the group is done, a finished
    group's slot goes to a waiting group in the same round, and with nothing waiting only the LAST slot ever moves"""
    made = _refiners("rank", {}, [0])
    refiners = [r for r, _, _ in made]
    work = [r._prepare(audio, res) for r, audio, res in made]
    rounds, keep = [], []

    def answer(flying):
        keep.extend(request[0] for _, request in flying)                  # alive to the end, so that an id is one probe
        rounds.append([id(request[0]) for _, request in flying])
        return [refiners[i].inference_func(request[0], request[1]) for i, request in flying]

    refine_tracks(refiners, work, 3, answer)
    assert max(len(r) for r in rounds) == 3 and sum(len(r) == 3 for r in rounds) > len(rounds) // 2
    for prev, cur in zip(rounds, rounds[1:]):
        for k, p in enumerate(cur):
            if p in prev and prev.index(p) != k:                          # a move: the last slot of the round before, into a hole
                assert prev.index(p) == len(prev) - 1 or prev.index(p) >= len(cur), (prev, cur)


def test_random_op_sequences_recorder_equals_tensor():
    """200 random sequences of 1-40 writes, with negative, reversed, empty and overshooting slices, a mute followed by an overlapping
    restore in the same row, and the two rows of a pair edited differently: the host tensor against the replay of the recording"""
    rng = np.random.default_rng(11)
    cleans = {n: torch.from_numpy(rng.standard_normal((1, n)).astype(np.float32) + 3.0) for n in (1, 7, 4096, 480000)}
    seen = dict(negative=0, reversed=0, empty=0, overshoot=0, mute_then_restore=0, rows_differ=0)
    for trial in range(200):
        n = (1, 7, 4096, 480000)[trial % 4]
        clean = cleans[n]
        host, rec = HostProbe(clean), OpsProbe(clean)
        last_mute = None
        for k in range(int(rng.integers(1, 41))):
            row = int(rng.integers(0, 2))
            a, b = (int(v) for v in rng.integers(-n - 3, 2 * n + 4, 2))
            if rng.random() < 0.7 and a > b:
                a, b = b, a
            kind = int(rng.integers(0, 2))
            if last_mute is not None and rng.random() < 0.3:              # a restore that overlaps the last mute of that row
                row, (a0, b0), kind = last_mute[0], last_mute[1], 1
                a, b = a0 + (b0 - a0) // 3, b0 + 2
                seen["mute_then_restore"] += 1
            seen["negative"] += a < 0 or b < 0
            seen["overshoot"] += b > n
            sa, sb, _ = slice(a, b).indices(n)
            seen["reversed"] += a > b
            seen["empty"] += sa >= sb
            for buf in (host, rec):
                (buf.restore if kind else buf.mute)(row, a, b)
            last_mute = (row, (sa, sb)) if kind == 0 and sa < sb else last_mute
        ops = rec.take()
        assert rec.take() == [] and all(0 <= a < b <= n and r in (0, 1) and k in (0, 1) for r, a, b, k in ops)
        want = apply_ops(clean.numpy(), clean.numpy().repeat(2, 0), ops)
        assert np.array_equal(_bits(want), _bits(host.audio.numpy())), trial
        seen["rows_differ"] += not np.array_equal(_bits(host.audio[0].numpy()), _bits(host.audio[1].numpy()))
    assert all(v >= 10 for v in seen.values()), seen


def test_recorder_clips_to_the_samples_a_probe_keeps():
    clean = torch.arange(1, 21, dtype=torch.float32).unsqueeze(0)
    rec = OpsProbe(clean, limit=12)
    assert (rec.n, rec.n_kept) == (20, 12) and rec.audio is rec
    rec.mute(0, 5, 20)
    rec.restore(1, 12, 20)                                                # wholly past the limit: dropped
    rec.mute(1, -10, None)
    assert rec.take() == [(0, 5, 12, 0), (1, 10, 12, 0)]
    with pytest.raises(IndexError):
        rec.mute(2, 0, 1)


class _NoDevice:
    """a model whose device side must not be reached: any attribute past the three refine_many reads before work raises"""
    is_multilingual, num_languages, computes_on_host = False, 99, True
    dims = types.SimpleNamespace(n_text_ctx=448)

    def __getattr__(self, name):
        raise AssertionError(f"model.{name} was reached before the refusal")


def test_refusals_happen_before_any_inference_call():
    from stable_ts_amd.many import refine_many
    seed, audio, rd, _ = _cases()[0]
    model = _NoDevice()
    good = lambda: WhisperResult(copy.deepcopy(rd))  # noqa: E731
    no_words = copy.deepcopy(rd)
    no_words["language"] = None
    for s in no_words["segments"]:
        s.pop("words")
    with pytest.raises(NotImplementedError):
        refine_many(model, [audio], [good()], batch_size=4)
    with pytest.raises(RuntimeError, match="missing language"):
        refine_many(model, [audio, audio], [good(), WhisperResult(no_words)])
    with pytest.raises(ValueError):
        refine_many(model, [audio, audio], [good()])
    for bad in (0, -1, 1.5, None, True):
        with pytest.raises(ValueError):
            refine_many(model, [audio], [good()], max_tracks=bad)
    with pytest.raises(TypeError):
        refine_many(model, audio, [good()])
    with pytest.raises(TypeError):
        refine_many(model, [audio], good())
    with pytest.raises(ValueError):
        refine_many(model, [audio], [good()], steps="x")
    # refine() routes a result without word timestamps to align_words when it has a language, so through refine_many only the one
    # without a language can be refused up front (above); the "word-timestamps" refusal itself is the driver's prologue, as in
    # Refiner.refine, and it too comes before any inference call
    with pytest.raises(RuntimeError, match="word-timestamps"):
        Refiner(None)._prepare(audio, WhisperResult(no_words))
    assert refine_many(model, [], []) == []


def test_pcm_edit_plan_sorts_stably_and_offsets_rows():
    from stable_ts_amd.engine import pcm_edit_plan
    ops = [(3, 0, 5, 0), (0, 1, 2, 1), (3, 2, 9, 1), (7, 0, 1, 0), (0, 4, 6, 0), (-1, 0, 1, 0), (2, 0, 0, 0)]
    sorted_ops, row_start = pcm_edit_plan(ops, 4)
    assert sorted_ops.dtype == np.int32 and row_start.dtype == np.int32
    assert sorted_ops.tolist() == [[-1, 0, 1, 0], [0, 1, 2, 1], [0, 4, 6, 0], [2, 0, 0, 0], [3, 0, 5, 0], [3, 2, 9, 1], [7, 0, 1, 0]]
    assert row_start.tolist() == [1, 3, 3, 4, 6]                          # rows -1 and 7 lie outside every row's range
