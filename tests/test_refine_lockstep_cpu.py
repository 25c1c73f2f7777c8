"""``refine(batch_size=N)``: the lockstep driver of ``stable_ts_amd.refiner.Refiner`` against the reference's ``Refiner``
(stable_whisper/non_whisper/refinement.py) and against this package's sequential driver, all on the same seeded synthetic
inference function (tests/golden/make_refiner_golden.py), in the three output forms ``_pick`` takes: probabilities
``[2, T]``, distributions ``[2, T, vocab]``, and the native probe's pair ``(p [2, T], rank [2, T])``.

Every group must see the same probes round for round (a hash of the two audio copies of every call, keyed by step and
group) and every timestamp must be equal, for ``batch_size`` 1, 2, 3 and 64.  The cases are chosen so that the comparison
is not vacuous, and that is asserted on the yardstick's own run (the REFERENCE's; the sequential driver's in the second test):
>= 4 groups, at least half of the (step, group) pairs run >= 2 bisection rounds, >= 80 % of the cases move a timestamp.
"""
import contextlib
import copy
import hashlib
import io
import os
import sys
import warnings

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import make_refiner_golden as mg  # noqa: E402

from stable_ts_amd.refiner import Refiner, token_rank  # noqa: E402
from stable_ts_amd.result import WhisperResult  # noqa: E402

SEEDS = (602, 606, 610, 612, 613, 618)
BATCH_SIZES = (1, 2, 3, 64)
FORMS = ("2d", "3d", "rank")


HAVE_REFERENCE = os.path.isdir("/root/reference/stable_whisper")      # decided like tests/test_refiner_cpu.py, before any work


def _case(seed):
    """make_refiner_golden's seeded audio / result / options with every token id inside the synthetic vocabulary (the 3-D
    form indexes it), steps "se" and groups of at most 12 tokens, so that a result has many groups."""
    audio, rd, opts, _ = mg.synth_case(seed)
    for s in rd["segments"]:
        for w in s["words"]:
            w["tokens"] = [int(t) % mg.VOCAB for t in w["tokens"]]
    opts = dict(opts, steps="se", max_inference_tokens=12)
    return audio, rd, opts


def _ranked(dist_fn):
    """the native probe's form from the 3-D synthetic function: the token's probability and its (value, index) rank"""
    def infer(audio, tokens):
        dist = dist_fn(audio, tokens)
        ids = [int(t) for t in tokens]
        pos = torch.arange(len(ids))
        p = dist[:, pos, ids]
        rank = torch.tensor([[token_rank(dist[r, j].numpy(), ids[j]) for j in range(len(ids))] for r in range(2)])
        return p, rank
    return infer


class Recorder:
    """wraps an inference function: logs a hash of every probe under (step, segment length, tokens) = one group of one step"""

    def __init__(self, fn, with_batch):
        self.fn, self.step, self.log = fn, 0, {}
        if with_batch:
            self.batch = lambda items: [self(a, t) for a, t in items]

    def __call__(self, audio, tokens):
        key = (self.step, int(audio.shape[-1]), tuple(int(t) for t in tokens))
        self.log.setdefault(key, []).append(hashlib.sha1(audio.contiguous().numpy().tobytes()).hexdigest())
        return self.fn(audio, tokens)

    def stepping(self, refiner_cls):
        """``refiner_cls`` with the steps counted as they end (both classes run a step in ``_refine(result, step)``)"""
        rec = self

        class Stepping(refiner_cls):
            def _refine(self, result, step):
                super()._refine(result, step)
                rec.step += 1
        return Stepping


def _run(refiner_cls, result_cls, seed, form, batch_size=None, extra=None):
    audio, rd, opts = _case(seed)
    fn = mg.make_inference(seed, form != "2d")
    rec = Recorder(_ranked(fn) if form == "rank" else fn, with_batch=form == "rank")
    kw = dict(opts, **(extra or {}))
    if batch_size is not None:
        kw["batch_size"] = batch_size
    res = result_cls(copy.deepcopy(rd))
    with warnings.catch_warnings(), contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        warnings.simplefilter("ignore")
        out = rec.stepping(refiner_cls)(rec, **kw).refine(audio, res)
    before = mg.snapshot(result_cls(copy.deepcopy(rd)))
    return mg.snapshot(out), rec.log, before


def _baseline():
    """runner of the yardstick: the reference's Refiner (an import that fails with the checkout present is a failure)"""
    from make_golden import import_reference
    sw = import_reference()
    from stable_whisper.non_whisper.refinement import Refiner as RefRefiner
    return lambda seed, form: _run(RefRefiner, sw.WhisperResult, seed, form, extra=dict(verbose=None))


def _check_forms(forms):
    base = _baseline()
    moved = total = 0
    for seed in SEEDS:
        for form in forms:
            # the reference knows the 2-D and 3-D forms; the pair form carries the same distribution's numbers
            want, want_log, before = base(seed, "3d" if form == "rank" else form)
            steps = {k[0] for k in want_log}
            assert steps == {0, 1}, (seed, steps)
            groups = [k for k in want_log if k[0] == 0]
            assert len(groups) >= 4, (seed, len(groups))
            busy = sum(1 for v in want_log.values() if len(v) - 1 >= 2)         # first call = the reference probe
            assert 2 * busy >= len(want_log), (seed, form, busy, len(want_log))
            total += 1
            moved += want != before
            for n in BATCH_SIZES:
                got, log, _ = _run(Refiner, WhisperResult, seed, form, batch_size=n)
                assert log == want_log, (seed, form, n)
                assert got == want, (seed, form, n)
    assert moved >= 0.8 * total, (moved, total)


@pytest.mark.skipif(not HAVE_REFERENCE, reason="reference checkout not present")
@pytest.mark.parametrize("form", FORMS)
def test_lockstep_matches_reference_live(form):
    _check_forms((form,))


@pytest.mark.parametrize("form", FORMS)
def test_lockstep_matches_sequential_driver(form):
    """the same comparison without the reference checkout: the sequential driver is pinned to the reference by
    tests/test_refiner_cpu.py's golden file"""
    moved = total = 0
    for seed in SEEDS:
        want, want_log, before = _run(Refiner, WhisperResult, seed, "3d" if form == "rank" else form)
        assert len([k for k in want_log if k[0] == 0]) >= 4
        assert 2 * sum(1 for v in want_log.values() if len(v) - 1 >= 2) >= len(want_log), seed
        total += 1
        moved += want != before
        for n in BATCH_SIZES:
            got, log, _ = _run(Refiner, WhisperResult, seed, form, batch_size=n)
            assert log == want_log and got == want, (seed, form, n)
    assert moved >= 0.8 * total


def test_lockstep_batches_hold_at_most_batch_size_groups_and_refill():
    """a group leaves the batch when it is done and a waiting group takes its place: every call of ``.batch`` holds
    min(batch_size, groups not yet finished) requests"""
    seed = SEEDS[0]
    audio, rd, opts = _case(seed)
    fn = _ranked(mg.make_inference(seed, True))
    sizes = []

    def infer(a, t):
        return fn(a, t)

    def batch(items):
        sizes.append(len(items))
        return [fn(a, t) for a, t in items]

    infer.batch = batch
    Refiner(infer, **dict(opts, batch_size=3)).refine(audio, WhisperResult(copy.deepcopy(rd)))
    assert max(sizes) == 3 and min(sizes) >= 1
    assert sizes.count(3) > len(sizes) // 2          # the batch only shrinks when no group is waiting any more


def test_batch_size_is_validated():
    f = mg.make_inference(0, False)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError):
            Refiner(f, batch_size=bad)
    assert Refiner(f, batch_size=None).batch_size is None and Refiner(f, batch_size=4).batch_size == 4


def test_pair_form_shape_errors():
    seed = SEEDS[0]
    audio, rd, opts = _case(seed)
    bad = lambda a, t: (torch.zeros(2, len(t)), torch.zeros(2, len(t) + 1, dtype=torch.int64))  # noqa: E731
    with pytest.raises(RuntimeError):
        Refiner(bad, **dict(opts, batch_size=2)).refine(audio, WhisperResult(copy.deepcopy(rd)))


def test_rank_definition_is_the_stable_sort_position():
    """``token_rank`` (the host statement of what swx_forward_token_ranks counts) against ``torch.sort(stable=True)`` on random
    rows with planted exact ties, the target among the tied entries included"""
    g = torch.Generator().manual_seed(7)
    for trial in range(200):
        n = int(torch.randint(2, 400, (1,), generator=g))
        row = torch.randn(n, generator=g)
        k = int(torch.randint(0, n, (1,), generator=g))            # plant ties: copies of some values, -inf, and a constant run
        src = torch.randint(0, n, (k,), generator=g)
        dst = torch.randint(0, n, (k,), generator=g)
        row[dst] = row[src]
        if trial % 3 == 0:
            row[torch.randint(0, n, (max(1, n // 5),), generator=g)] = float("-inf")
        if trial % 5 == 0:
            row[: n // 2] = row[0]
        order = torch.sort(row, stable=True).indices
        pos = torch.empty(n, dtype=torch.int64)
        pos[order] = torch.arange(n)
        for t in torch.randint(0, n, (min(n, 16),), generator=g).tolist() + dst[:1].tolist():
            assert token_rank(row.numpy(), t) == int(pos[t]), (trial, t)


def test_native_batch_callable_on_the_cpu_standin():
    """``make_refinement_func(...).batch`` (the glue ``refine(batch_size=N)`` drives: pairs of audio copies, token rows, the slices
    handed back per group) on the oracle-backed stand-in, with the two device calls it adds restated on the host: every group's
    ``(p, rank)`` must be what the single-group distribution form says about the same probe."""
    from oracle.whisper.model import build_model
    from oracle_engine import CpuWhisper
    from stable_ts_amd.alignment import make_refinement_func
    from stable_ts_amd.tokenizer import get_tokenizer
    model = CpuWhisper(build_model("tiny.en", seed=1234, std=0.02, embed_gain=2.0, ts_gain=0.5))
    model.manual_attention_encoder = True
    plain = model.log_mel_segments

    def log_mel_segments(audios, padding=0, batch_max=False, group=None):
        if group is None:
            return plain(audios, padding, batch_max)
        assert len(audios) % group == 0
        return torch.cat([plain(audios[i: i + group], padding, True) for i in range(0, len(audios), group)])

    def forward_token_ranks(xkv, tokens, n_vocab_used=None, pad_token=0):
        logits = model.engine.forward_logits(xkv, tokens)[..., :n_vocab_used]
        prob, rank = torch.zeros(logits.shape[:2]), torch.full(logits.shape[:2], -1, dtype=torch.int32)
        for w, t in enumerate(tokens):
            for j in range(len(t) - 1):
                if 0 <= t[j + 1] < logits.shape[-1]:
                    prob[w, j] = logits[w, j].softmax(-1)[t[j + 1]]
                    rank[w, j] = token_rank(logits[w, j].numpy(), t[j + 1])
        return prob, rank

    model.log_mel_segments = log_mel_segments
    model.engine.forward_token_ranks = forward_token_ranks
    tok = get_tokenizer(False, num_languages=model.num_languages)
    func = make_refinement_func(model, tok)
    g = torch.Generator().manual_seed(3)
    items = []
    for n, ids in ((16000 * 3, [1234, 77, 40000]), (16000 * 2 + 123, [9, 50000, 31, 2222, 5])):
        audio = 0.1 * torch.randn(2, n, generator=g)
        audio[1, n // 2:] = 0                                            # the two copies differ, as a probe's do
        items.append((audio, ids))
    outs = func.batch(items)
    assert len(outs) == 2
    for (audio, ids), (p, rank) in zip(items, outs):
        dist = func(audio, ids)                                          # [2, T, eot]
        assert tuple(p.shape) == tuple(rank.shape) == (2, len(ids))
        for r in range(2):
            for j, t in enumerate(ids):
                assert abs(float(p[r, j]) - float(dist[r, j, t])) <= 1e-6 * float(dist[r, j, t]) + 1e-12
                lo, hi = int((dist[r, j] < dist[r, j, t]).sum()), int((dist[r, j] <= dist[r, j, t]).sum()) - 1
                assert lo <= int(rank[r, j]) <= hi, (r, j, lo, int(rank[r, j]), hi)
