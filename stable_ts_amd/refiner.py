"""``refine()``: tighten existing word timestamps by muting audio and watching the token probabilities (SURVEY.md 8f
row 3).

Behavioural contract = ``stable_whisper/non_whisper/refinement.py::Refiner`` (:13-487).  For every word the start is
moved as late (and the end as early) as possible while the probability of the word's first (last) token, computed by a
teacher-forced pass over the partly muted audio, stays acceptable.  Per group of words (<= ``max_inference_tokens``
tokens, <= 30 s) this is a bisection on the mute boundary of every word at once; two copies of the audio (even / odd
words) are evaluated per inference call so that neighbouring words do not mute each other (:359-475).

Generic over ``inference_func(audio[2, n], tokens) -> probabilities [2, len(tokens)] or [2, len(tokens), vocab]`` (seam
B3): the GPU path plugs in ``stable_ts_amd.alignment.make_refinement_func`` (mel -> encoder -> one teacher-forced decoder
pass for both copies -> softmax over the text vocabulary on the device), the CPU test plugs the same synthetic function
into this class and into the reference's ``Refiner`` and requires identical timestamps.

The bisection state lives in int32 sample arrays exactly like the reference's (`lo`, `hi`, `mid` per word), including
its quirks, which are part of the observable behaviour: the "original" probability a word is compared with is
overwritten by the latest probe (``new_probs`` aliases ``orig_probs``, :405, 472), and the audio copy a word mutes is
looked up in the per-TOKEN row table with the WORD index (:424).

One group's bisection is a generator (``_group_rounds``) that yields "probe this" and receives the picked ``(p, rank)``.
Within one step the groups are independent (every bound is computed up front, a group reads and writes only its own
words), so two drivers run the SAME generator: the sequential one (``batch_size=None``, the reference's order of calls)
and the lockstep one (``batch_size=N``), which keeps up to N unfinished groups in flight and hands all their probes of a
round to ``inference_func.batch`` in one call (``stable_ts_amd.alignment.make_refinement_func``: one mel / encoder /
decoder pass over 2 N windows, answered by ``swx_forward_token_ranks`` with a probability and a rank per token instead of a
distribution).  A group leaves the batch when all its words are done and a waiting group takes its place.  A third driver,
``refine_tracks`` (``refine_many``), pools the groups of many recordings, each with its own ``Refiner``, in the same way.

The generator writes its two audio copies through a probe buffer with two methods, mute and restore: ``HostProbe`` is the
tensor every path above probes with, ``OpsProbe`` records the writes for copies that live on the device.
"""
import copy
from typing import Callable, Iterator, List, Optional, Tuple

import numpy as np
import torch

from .result import WhisperResult, WordTiming


def token_rank(row, target: int) -> int:
    """The rank the native probe reports (``swx_forward_token_ranks``): the position of ``target`` in an ascending sort of
    ``row`` on (value, index) -- ``#{v : row[v] < row[target] or (row[v] == row[target] and v < target)}``.  A total order, so
    it is what a STABLE ascending sort gives; an unstable sort (the reference's ``dist.sort()``) may differ from it only where
    another entry ties with the target itself."""
    row = np.asarray(row)
    x = row[target]
    return int(np.count_nonzero(row < x) + np.count_nonzero(row[:target] == x))


class HostProbe:
    """The two audio copies of one word group as a host tensor ``audio[2, n]``: what every probe of ``refine()`` is made of.
    ``mute`` / ``restore`` are the only two writes the bisection makes; bounds follow the tensor's slice rules."""

    def __init__(self, clean: torch.Tensor):
        self.clean = clean
        self.audio = clean.clone().repeat_interleave(2, 0)               # copy 0: even words, copy 1: odd words

    def mute(self, row: int, a: int, b: int):
        self.audio[row, a:b] = 0

    def restore(self, row: int, a: int, b: int):
        self.audio[row, a:b] = self.clean[0, a:b]


class OpsProbe:
    """The same two copies kept somewhere else (on the device, ``refine_many``): the writes are recorded as ``(row, a, b, kind)``
    in issue order, kind 0 = mute, 1 = restore, and ``take()`` hands over what was recorded since the last call.  They are
    ORDERED writes, not a set of muted intervals: the bisection looks a word's copy up in the per-token row table with the word
    index, so two words can write to one row and a restore can overwrite another word's mute -- for every sample the last op of
    its row that covers it decides.  ``a, b`` are normalised as the tensor would (``slice(a, b).indices(n)``) and clipped to the
    ``limit`` samples a probe keeps on its way to the model; empty writes are dropped."""
    MUTE, RESTORE = 0, 1

    def __init__(self, clean: torch.Tensor, limit: Optional[int] = None):
        self.clean = clean
        self.n = int(clean.shape[-1])
        self.n_kept = self.n if limit is None else min(self.n, int(limit))
        self.ops: List[Tuple[int, int, int, int]] = []

    @property
    def audio(self):
        return self

    def _write(self, row: int, a, b, kind: int):
        row = int(row)
        if not 0 <= row < 2:
            raise IndexError(f"a probe has two copies, got row {row}")
        a, b, _ = slice(None if a is None else int(a), None if b is None else int(b)).indices(self.n)
        b = min(b, self.n_kept)
        if a < b:
            self.ops.append((row, a, b, kind))

    def mute(self, row: int, a, b):
        self._write(row, a, b, self.MUTE)

    def restore(self, row: int, a, b):
        self._write(row, a, b, self.RESTORE)

    def take(self) -> List[Tuple[int, int, int, int]]:
        ops, self.ops = self.ops, []
        return ops


class Refiner:
    probe_buffer = HostProbe                    # what ``_group_rounds`` keeps a group's two audio copies in

    def __init__(self, inference_func: Callable, sample_rate: int = 16000, max_segment_length="30s",
                 max_inference_tokens: int = 100, *, steps: str = "se", rel_prob_decrease: float = .03,
                 abs_prob_decrease: float = .05, rel_rel_prob_decrease: Optional[float] = None,
                 prob_threshold: float = .5, rel_dur_change: Optional[float] = .5,
                 abs_dur_change: Optional[float] = None, word_level: bool = True, precision: Optional[float] = None,
                 progress_callback: Optional[Callable] = None, batch_size: Optional[int] = None, **unsupported):
        steps = steps or "se"
        if batch_size is not None and (isinstance(batch_size, bool) or int(batch_size) != batch_size or batch_size < 1):
            raise ValueError(f"batch_size must be None or an integer >= 1, got {batch_size!r}")
        self.batch_size = None if batch_size is None else int(batch_size)
        bad = steps.replace("s", "").replace("e", "")
        if bad:
            raise ValueError(f'Invalid step(s): {", ".join(bad)}')
        if isinstance(max_segment_length, str):
            if not max_segment_length.endswith("s"):
                raise ValueError(f'expect string ``max_segment_length`` to end with "s" but got "{max_segment_length}"')
            self.max_segment_seconds = float(max_segment_length[:-1])
        else:
            self.max_segment_seconds = max_segment_length / sample_rate
        for k in ("only_voice_freq",):
            if unsupported.pop(k, None):
                raise NotImplementedError(f"{k} is outside this package's scope (DESIGN.md section 7)")
        for k in ("verbose", "denoiser", "denoiser_options", "all_options", "only_ffmpeg"):   # the audio arrives prepared
            unsupported.pop(k, None)
        if unsupported:
            raise TypeError(f"unexpected keyword argument(s): {', '.join(unsupported)}")
        self.inference_func = inference_func
        self.sample_rate = sample_rate
        self.max_inference_tokens = max_inference_tokens
        self.steps = steps
        self.precision = 0.1 if precision is None else precision
        self.sample_precision = max(round(self.precision * self.sample_rate), 2)
        self.rel_prob_decrease, self.abs_prob_decrease = rel_prob_decrease, abs_prob_decrease
        self.rel_rel_prob_decrease, self.prob_threshold = rel_rel_prob_decrease, prob_threshold
        self.rel_dur_change, self.abs_dur_change = rel_dur_change, abs_dur_change
        self.word_level = word_level
        self.progress_callback = progress_callback
        self._audio = torch.tensor([])

    # ----------------------------------------------------------------------------------------------- driver
    def refine(self, audio: torch.Tensor, result: WhisperResult, inplace: bool = True,
               encode: Optional[Callable] = None) -> WhisperResult:
        result = self._prepare(audio, result, inplace, encode)
        for n, step in enumerate(self.steps, 1):
            self._refine(result, step)
            if self.progress_callback is not None:
                total = round(self._audio.size(-1) / self.sample_rate, 2)
                self.progress_callback(round(total * n / len(self.steps), 2), total)
        result.reassign_ids()
        return result

    def _prepare(self, audio: torch.Tensor, result: WhisperResult, inplace: bool = True,
                 encode: Optional[Callable] = None) -> WhisperResult:
        """the result ``refine`` works on (tokens filled in, copied unless ``inplace``), with this recording's audio taken"""
        if result:
            if not result.has_words:
                raise RuntimeError("cannot refine result with missing word-timestamps")
            if not all(w.tokens for w in result.all_words()):
                if encode is None:
                    raise RuntimeError("result must have tokens or provide tokenization function to ``encode``")
                for w in result.all_words():
                    w.tokens = encode(w.word)
        if not inplace:
            result = copy.deepcopy(result)
        self._audio = torch.as_tensor(audio, dtype=torch.float32).detach().cpu()
        return result

    # ------------------------------------------------------------------------------------------- grouping
    def _groups(self, result: WhisperResult, total_duration: float) -> Iterator[Tuple[List[WordTiming], list, list, np.ndarray]]:
        """Consecutive words sharing one inference call, with the earliest start / latest end each word may move to
        (:220-271): bounded by ``rel_dur_change`` x its duration, ``abs_dur_change``, the neighbouring words, and 14.5 s."""
        words = result.all_words()
        edge = np.array([1 if i == 0 else (2 if i == len(s.words) - 1 else 0) for s in result.segments
                         for i in range(len(s.words))])
        lo = [max(0 if self.abs_dur_change is None else (w.start - self.abs_dur_change),
                  0 if self.rel_dur_change is None else (w.start - w.duration * self.rel_dur_change),
                  0 if i == 0 else max(words[i - 1].end, w.end - 14.5, 0))
              for i, w in enumerate(words)]
        hi = [min(total_duration if self.abs_dur_change is None else (w.end + self.abs_dur_change),
                  total_duration if self.rel_dur_change is None else (w.end + w.duration * self.rel_dur_change),
                  total_duration if i == len(words) else min(words[i].start, w.start + 14.5, total_duration))
              for i, w in enumerate(words, 1)]
        t0 = lo[0]
        first = 0
        g_words, g_lo, g_hi, n_tok = [], [], [], 0
        for i, w in enumerate(words, 1):
            if (hi[0] - t0 > self.max_segment_seconds) or (n_tok + len(w.tokens) > self.max_inference_tokens):
                if g_words:
                    yield g_words, g_lo, g_hi, edge[first:first + len(g_words)]
                    g_words, g_lo, g_hi = [], [], []
                t0 = lo[0]
                first = i - 1
                n_tok = 0
            g_words.append(w)
            g_lo.append(lo.pop(0))
            g_hi.append(hi.pop(0))
            n_tok += len(w.tokens)
            if i == len(words):
                yield g_words, g_lo, g_hi, edge[first:first + len(g_words)]

    def _samples(self, seconds, offset: float) -> np.ndarray:
        return ((np.asarray(seconds) - offset) * self.sample_rate).round().astype(np.int32)

    # ----------------------------------------------------------------------------------------------- probing
    def _probe(self, audio2: torch.Tensor, text_tokens: List[int], word_tokens: List[List[int]], rows: List[int],
               at_end: bool):
        """One inference call -> per word the probability of its first (last, for end refinement) token in the audio
        copy that word owns, and that token's rank among the vocabulary when the function returns a distribution."""
        return self._pick(self.inference_func(audio2, text_tokens), text_tokens, word_tokens, rows, at_end)

    def _pick(self, p, text_tokens: List[int], word_tokens: List[List[int]], rows: List[int], at_end: bool):
        """What one probe's output says about every word.  Three forms: probabilities ``[2, T]`` (no ranks), distributions
        ``[2, T, vocab]`` (ranks from a sort, as the reference), or a pair ``(p [2, T], rank [2, T])`` whose ranks were
        computed where the distribution lived (position of the token in an ascending order of its row)."""
        rank_t = None
        if isinstance(p, (tuple, list)):
            p, rank_t = p
            if p.ndim != 2 or tuple(rank_t.shape) != tuple(p.shape):
                raise RuntimeError(f"expected probabilities and ranks of one 2-D shape but got {tuple(p.shape)} and "
                                   f"{tuple(rank_t.shape)}")
        if p.size(0) != 2:
            raise RuntimeError(f"expected dim 0 to be length of 2 but got {p.size(0)}")
        if p.size(1) != len(text_tokens):
            raise RuntimeError(f"expected dim 1 to be length of {len(text_tokens)} but got {p.size(1)}")
        if p.ndim not in (2, 3):
            raise RuntimeError(f"expected inference_func output to have 2 or 3 dimensions but got {p.ndim}")
        pos = torch.arange(len(text_tokens))
        bounds = np.pad(np.cumsum([len(t) for t in word_tokens]), (1, 0))
        pick = [(j - 1 if at_end else i) for i, j in zip(bounds[:-1], bounds[1:])]
        if rank_t is not None:
            tok_p = p[rows, pos].tolist()
            where = rank_t[rows, pos].tolist()
            ranks = [int(where[k]) for k in pick]
        elif p.ndim == 2:
            tok_p = p[rows, pos].tolist()
            ranks = [0] * len(word_tokens)
        else:
            tok_p = p[:, pos, text_tokens][rows, pos].tolist()
            dist = p[:, pos][rows, pos]                                 # [n_tokens, vocab] of each token's own row
            ids = torch.tensor(text_tokens, device=p.device)
            where = (dist.sort().indices == ids.unsqueeze(1)).nonzero()[:, -1].tolist()
            ranks = [where[k] for k in pick]
        return np.array([tok_p[k] for k in pick]), ranks

    def _commit(self, idx: int, done: np.ndarray, track: np.ndarray, at_end: bool, offset: float, words: List[WordTiming]):
        """:329-357 -- write the last boundary that kept the best token into the word; a boundary found only through
        failed probes may not move the timestamp outwards."""
        if not done[idx] or track[idx, -1] == -1:
            return
        ts = round(offset + (float(track[idx, -1]) / self.sample_rate), 3)
        if track[idx, 0] and not track[idx, 1]:
            if at_end:
                if ts <= words[idx].end:
                    return
            elif ts >= words[idx].start:
                return
        if at_end:
            words[idx].end = ts
        else:
            words[idx].start = ts

    # ---------------------------------------------------------------------------------------------- one step
    def _refine(self, result: WhisperResult, step: str):
        total_duration = round(self._audio.shape[-1] / self.sample_rate, 3)
        at_end = step == "e"
        if self.batch_size is not None:
            return self._refine_lockstep(result, total_duration, at_end)
        for group in self._groups(result, total_duration):
            rounds = self._group_rounds(*group, at_end)
            request = next(rounds)
            while True:
                try:
                    request = rounds.send(self._probe(*request, at_end))
                except StopIteration:
                    break

    def _infer_batch(self, requests: list) -> list:
        """The probes of one lockstep round, one per group in flight: through ``inference_func.batch`` where the function
        has one (one device pass for all of them), else call by call."""
        batch = getattr(self.inference_func, "batch", None)
        if batch is None:
            return [self.inference_func(r[0], r[1]) for r in requests]
        outs = batch([(r[0], r[1]) for r in requests])
        if len(outs) != len(requests):
            raise RuntimeError(f"expected {len(requests)} outputs from inference_func.batch but got {len(outs)}")
        return outs

    def _refine_lockstep(self, result: WhisperResult, total_duration: float, at_end: bool):
        """Up to ``batch_size`` unfinished groups advance one bisection round per inference call.  Every group runs the
        generator the sequential driver runs and sees its own probes in its own order, so the timestamps are the
        sequential ones whenever a probe's answer does not depend on the batch it was computed in."""
        waiting = iter(list(self._groups(result, total_duration)))
        flying: list = []                                                # [generator, its pending request]
        while True:
            while len(flying) < self.batch_size:
                group = next(waiting, None)
                if group is None:
                    break
                rounds = self._group_rounds(*group, at_end)
                flying.append([rounds, next(rounds)])
            if not flying:
                return
            outs = self._infer_batch([request for _, request in flying])
            still = []
            for (rounds, request), out in zip(flying, outs):
                try:
                    still.append([rounds, rounds.send(self._pick(out, *request[1:], at_end))])
                except StopIteration:
                    pass
            flying = still

    def _group_rounds(self, words: List[WordTiming], g_lo: list, g_hi: list, edge: np.ndarray, at_end: bool):
        """One group's bisection (:359-475) as a generator: yields ``(audio[2, n], text_tokens, word_tokens, rows)`` -- the
        arguments of ``_probe`` -- and receives what ``_probe`` returns for it.  The yielded audio is the group's live probe
        buffer: the driver must be done with it before it sends the answer."""
        offset = g_lo[0]
        a, b = round(offset * self.sample_rate), round(g_hi[-1] * self.sample_rate)
        clean = self._audio[a:b + 1].unsqueeze(0)
        max_start = self._samples([w.end for w in words], offset)
        min_end = self._samples([w.start for w in words], offset)
        min_start = self._samples(g_lo, offset)
        max_end = self._samples(g_hi, offset)
        mid_start = min_start + ((max_start - min_start) / 2).round().astype(np.int32)
        mid_end = min_end + ((max_end - min_end) / 2).round().astype(np.int32)
        text_tokens = [t for w in words for t in w.tokens]
        word_tokens = [list(w.tokens) for w in words]
        buf = self.probe_buffer(clean)                              # copy 0: even words, copy 1: odd words
        n = clean.size(-1)
        done = np.less([w.probability for w in words], self.prob_threshold)
        done = np.logical_or(done, [w.duration == 0 for w in words])
        if not self.word_level:
            done[edge != (2 if at_end else 1)] = True
        rows: List[int] = []
        for idx, cut in enumerate(max_start if at_end else min_end):
            row = idx % 2
            rows.extend([row] * len(words[idx].tokens))
            if done[idx]:
                continue
            if at_end:                                               # mute from the word's end to the next word
                stop = n if idx == len(words) - 1 else mid_end[idx + 1]
                buf.mute(row, cut, stop)
            else:                                                    # mute from the previous word up to the start
                stop = 0 if idx == 0 else mid_start[idx - 1]
                buf.mute(row, stop, cut)
        ref_p, ref_rank = yield buf.audio, text_tokens, word_tokens, rows
        track = np.zeros((ref_p.shape[-1], 3), dtype=np.int32)       # [failed once, passed once, last good boundary]
        track[:, -1] = -1
        first_cut = (mid_end, max_start) if at_end else (min_end, mid_start)
        for idx, (s, e) in enumerate(zip(*first_cut)):
            if not done[idx]:
                buf.mute(idx % 2, s, e)
        prev_p = ref_p
        while not np.all(done):
            p, rank = yield buf.audio, text_tokens, word_tokens, rows
            abs_drop = ref_p - p
            rel_drop = abs_drop / ref_p
            step_drop = (prev_p - p) / prev_p
            prev_p = p
            for idx in range(len(words)):
                if done[idx]:
                    continue
                if at_end:
                    lo, hi, mid = min_end[idx], max_end[idx], mid_end[idx]
                else:
                    lo, hi, mid = min_start[idx], max_start[idx], mid_start[idx]
                row = rows[idx]
                lost_rank = ref_rank[idx] > rank[idx]
                failed = (abs_drop[idx] > self.abs_prob_decrease or rel_drop[idx] > self.rel_prob_decrease or
                          (self.rel_rel_prob_decrease is not None and step_drop[idx] > self.rel_rel_prob_decrease) or
                          p[idx] < self.prob_threshold or lost_rank)
                if failed:
                    track[idx][0] = 1
                    if at_end:
                        lo = mid
                    else:
                        hi = mid
                else:
                    track[idx][1] = 1
                    if at_end:
                        hi = mid
                    else:
                        lo = mid
                half = round((hi - lo) / 2)
                if half < self.sample_precision:
                    done[idx] = True
                    self._commit(idx, done, track, at_end, offset, words)
                    continue
                new_mid = lo + half
                if failed:                                           # give audio back
                    if at_end:
                        buf.restore(row, lo, new_mid)
                    else:
                        buf.restore(row, new_mid, hi)
                elif at_end:                                         # mute more
                    buf.mute(row, new_mid, hi)
                else:
                    buf.mute(row, lo, new_mid)
                if at_end:
                    min_end[idx], max_end[idx], mid_end[idx] = lo, hi, new_mid
                else:
                    min_start[idx], max_start[idx], mid_start[idx] = lo, hi, new_mid
                if not lost_rank:
                    track[idx][-1] = new_mid
                ref_p[idx] = p[idx]


def refine_tracks(refiners: List[Refiner], results: List[WhisperResult], max_tracks: int, answer: Optional[Callable] = None,
                  progress_callback: Optional[Callable] = None) -> List[WhisperResult]:
    """The word groups of many recordings bisected in lockstep (``refine_many``).  ``refiners[i]`` has taken its recording
    (``Refiner._prepare``) and ``results[i]`` is what that call returned.  A recording runs its steps in order; within a step its
    groups are independent and across recordings everything is, so up to ``max_tracks`` groups of any recordings are in flight,
    every one the ``_group_rounds`` generator ``Refiner.refine`` runs, and a round's requests are answered by ONE call of
    ``answer(flying)`` -- ``flying[k] = (recording index, request)``, one output per entry.  The place in that list is the
    group's slot: a group that finishes hands its slot to a waiting group in the same round (a recording's next step starts
    waiting the moment the last group of its current step finishes); when nothing waits the LAST slot moves into the hole, so the
    live slots stay dense and only the tail of a run ever moves.  Without ``answer`` every recording's own inference function
    answers its requests (``Refiner._infer_batch``).

    A result without words comes back as it is (``Refiner.refine`` alone raises IndexError there).
    ``progress_callback(seconds_done, seconds_total)`` counts every recording, a step at a time."""
    max_tracks = int(max_tracks)
    if max_tracks < 1:
        raise ValueError(f"max_tracks must be at least 1, got {max_tracks}")
    if len(refiners) != len(results):
        raise ValueError(f"{len(refiners)} refiners for {len(results)} results")
    if answer is None:
        def answer(flying):
            outs: list = [None] * len(flying)
            for i in sorted({i for i, _ in flying}):
                mine = [k for k, (j, _) in enumerate(flying) if j == i]
                for k, out in zip(mine, refiners[i]._infer_batch([flying[k][1] for k in mine])):
                    outs[k] = out
            return outs

    seconds = [r._audio.size(-1) / r.sample_rate for r in refiners]
    steps_done = [0] * len(refiners)
    open_groups = [0] * len(refiners)
    waiting: list = []                                               # (recording, group, at_end), handed out from the front

    def report():
        if progress_callback is not None:
            total = round(sum(seconds), 2)
            done = sum(s * n / len(r.steps) for s, n, r in zip(seconds, steps_done, refiners))
            progress_callback(min(round(done, 2), total), total)

    def next_step(i: int):
        """queue the groups of recording i's next step that has any; past the last step the recording is finished"""
        r = refiners[i]
        while steps_done[i] < len(r.steps):
            at_end = r.steps[steps_done[i]] == "e"
            groups = list(r._groups(results[i], round(r._audio.shape[-1] / r.sample_rate, 3))) if results[i].all_words() else []
            if groups:
                open_groups[i] = len(groups)
                waiting.extend((i, g, at_end) for g in groups)
                return
            steps_done[i] += 1
        results[i].reassign_ids()

    def take():
        """the next waiting group as a slot entry ``[recording, generator, at_end, request]``"""
        i, group, at_end = waiting.pop(0)
        rounds = refiners[i]._group_rounds(*group, at_end)
        return [i, rounds, at_end, next(rounds)]

    for i in range(len(refiners)):
        next_step(i)
    flying: list = []
    try:
        while waiting or flying:
            while waiting and len(flying) < max_tracks:
                flying.append(take())
            outs = answer([(e[0], e[3]) for e in flying])
            if len(outs) != len(flying):
                raise RuntimeError(f"expected {len(flying)} outputs for the round but got {len(outs)}")
            stepped = False
            for k, out in enumerate(outs):
                i, rounds, at_end, request = flying[k]
                try:
                    flying[k][3] = rounds.send(refiners[i]._pick(out, *request[1:], at_end))
                    continue
                except StopIteration:
                    pass
                open_groups[i] -= 1
                if open_groups[i] == 0:
                    steps_done[i] += 1
                    stepped = True
                    next_step(i)
                flying[k] = None
            for k in range(len(flying)):                             # a finished group's slot goes to a waiting group
                if flying[k] is None and waiting:
                    flying[k] = take()
            k = 0
            while k < len(flying):                                   # nothing waits any more: the last slot moves into a hole
                if flying[k] is None:
                    last = flying.pop()
                    if k < len(flying):
                        flying[k] = last
                    continue
                k += 1
            if stepped:
                report()
    finally:
        for e in flying:
            if e is not None:
                e[1].close()
    return results
