"""Many recordings at once: ``model.transcribe`` (or ``model.align``) per recording, all of them advanced together on this device.

The common way to label a folder of short clips is a loop of ``model.transcribe(path)``.  A clip shorter than 30 s is one
window per device pass there -- the launch-bound end of the decoder -- and with ``language=None`` every clip pays a second
encoder pass for its language.  ``transcribe_many`` runs the same sequential algorithm per recording (seek from the last
timestamp token, prompt carried over, silent windows skipped, language from the first window that is actually decoded), but
every device batch holds the current window of up to ``max_tracks`` recordings: it is the lockstep driver of
``transcribe_spans`` (spans.py) with tracks that come from different recordings, carry their own language state, and hand
their slot to the next pending recording when they run out of audio.

The oracle is exact by construction, as in spans.py: ``result[i]`` equals ``model.transcribe(audios[i], language=language_i,
**options)`` for deterministic decoding (greedy / beam at temperature 0 with thresholds that do not trigger the sampling
fallback; sampled fallbacks draw random numbers keyed on the window here and from torch's generator there).

Language per recording (``language=None``): on an engine with ``device_language_id`` the round's encoder pass is started
once, ``Engine.detect_language`` (``swx_detect_language``: one decoder step + the ~100 language rows of the embedding) reads
the rows of the recordings that start in this round, and the decode uses the same features: no second encoder pass, no
vocabulary-wide projection, no ``[W, n_vocab]`` copy.  Any other engine takes ``model.detect_language`` per recording.

``align_many`` is the same idea for forced alignment.  Inside one recording ``align`` cannot be batched: where a window starts
depends on the DTW result of the window before it.  Between recordings nothing depends on anything, so the window state
machine of every recording (``Aligner.steps``, the generator ``Aligner.align`` itself drives) is advanced to its next
inference request and the requests of a round -- ragged in audio length, token count and language -- are answered by one
``make_alignment_func(...).batch`` call: one mel / encoder / cross-K/V / scoring / DTW job for up to ``max_tracks`` windows.

``locate_many`` does it for ``locate``: the chunk state machine of every recording (``locator.LocateJob.steps``, the generator
``locate`` itself drives) is advanced phase by phase, and the greedy steps of a round's duration windows are answered by one
``Engine.forward_next_token`` call (``swx_forward_next_token``) instead of a vocabulary-wide logits tensor per window and step.

``refine_many`` does it for ``refine``.  ``refine(batch_size=N)`` bisects the word groups of ONE recording in lockstep, and a clip
of a few seconds is one or two groups, so its rounds hold 2-4 windows whatever N is.  Here the groups of all recordings share
the rounds (``stable_ts_amd.refiner.refine_tracks``: every group is the generator ``refine`` runs, a recording's steps stay in
order), answered by one ``make_refinement_func(...).batch`` call of 2 x (groups in flight) windows.  With ``device_probes=True`` the
two audio copies of every group live on the device (``DeviceProbes``): the clean segment is uploaded once when the group takes
a slot, and a round sends only the bisection's edits -- at most one interval per unfinished word -- as an ordered op list that
one launch of ``swx_pcm_edit`` applies; the log-mel reads the probe rows in place.
"""
from typing import Any, List, Optional, Sequence, Union

import torch

from .result import WhisperResult
from .stabilization import host_single_thread


@host_single_thread
def transcribe_many(model, audios: Sequence, *, language: Union[None, str, Sequence[Optional[str]]] = None, max_tracks: int = 20,
                    **transcribe_options) -> List[WhisperResult]:
    """``[model.transcribe(a, language=l, **transcribe_options) for a, l in zip(audios, languages)]`` with up to ``max_tracks``
    recordings per device batch.  ``audios``: whatever ``transcribe`` takes per item (tensor, array, path, bytes, ``AudioLoader``).
    ``language``: None (detected per recording), one code for all, or a list with a code or None per recording.  Options are
    those of ``transcribe`` except ``batch_size``, ``clip_timestamps`` and ``streams > 1``.  ``progress_callback(seconds_done,
    seconds_total)`` counts all recordings; after Ctrl-C every result carries its own ``unfinished_start``.  The device
    workspace grows to ``max_tracks`` windows and no further."""
    from .transcribe import transcribe_stable
    for k in ("batch_size", "clip_timestamps"):
        if transcribe_options.get(k):
            raise NotImplementedError(f"{k} does not combine with transcribe_many")
    if (transcribe_options.get("streams") or 1) > 1:
        raise NotImplementedError("streams > 1 does not combine with transcribe_many")
    for k in ("batch_size", "clip_timestamps", "streams"):
        transcribe_options.pop(k, None)
    if isinstance(audios, (str, bytes)) or not hasattr(audios, "__len__"):
        raise TypeError("audios must be a list of recordings (transcribe() takes a single one)")
    audios = list(audios)
    if max_tracks is None or int(max_tracks) < 1:
        raise ValueError(f"max_tracks must be at least 1, got {max_tracks}")
    if language is None or isinstance(language, str):
        languages = [language] * len(audios)
    else:
        languages = list(language)
        if len(languages) != len(audios):
            raise ValueError(f"language has {len(languages)} entries for {len(audios)} recordings")
    if not audios:
        return []
    return transcribe_stable(model, None, _many=dict(audios=audios, languages=languages, max_tracks=int(max_tracks)),
                             **transcribe_options)


@host_single_thread
def align_many(model, audios: Sequence, texts: Sequence[Union[str, List[int], WhisperResult]],
               language: Union[None, str, Sequence[Optional[str]]] = None, *, max_tracks: int = 20, tokenizer=None,
               **align_options) -> List[Optional[WhisperResult]]:
    """``[model.align(a, t, language=l, **align_options) for a, t, l in zip(audios, texts, languages)]`` with the current window
    of up to ``max_tracks`` recordings per device pass; every result equals the one of ``align`` alone, in input order.
    ``audios``: whatever ``align`` takes per item (tensor, array, path, bytes); a recording stays where the caller put it.
    ``texts``: a ``str``, token ids or a ``WhisperResult`` per recording.  ``language``: one code for all, or a list with a code or
    None per recording; None takes the language of a ``WhisperResult`` text, and a multilingual model refuses a recording whose
    language is still unknown before anything runs (no language detection here).  Options are those of ``align``.
    ``progress_callback(seconds_done, seconds_total)`` counts all recordings.  The device workspace grows to ``max_tracks``
    windows and no further."""
    from . import alignment as A
    from .audio import SAMPLE_RATE
    from .transcribe import _source_samples, _with_index, as_waveform, pop_audio_options
    if isinstance(audios, (str, bytes)) or not hasattr(audios, "__len__") or hasattr(audios, "shape"):
        raise TypeError("audios must be a list of recordings (align() takes a single one)")
    audios = list(audios)
    if isinstance(texts, (str, WhisperResult)) or not hasattr(texts, "__len__"):
        raise TypeError("texts must be a list with one text per recording")
    texts = list(texts)
    if len(texts) != len(audios):
        raise ValueError(f"texts has {len(texts)} entries for {len(audios)} recordings")
    if max_tracks is None or int(max_tracks) < 1:
        raise ValueError(f"max_tracks must be at least 1, got {max_tracks}")
    if language is None or isinstance(language, str):
        languages = [language] * len(audios)
    else:
        languages = list(language)
        if len(languages) != len(audios):
            raise ValueError(f"language has {len(languages)} entries for {len(audios)} recordings")
    options = dict(align_options)
    audio_options = pop_audio_options(options)
    for k in ("ignore_compatibility", "batch_size"):               # named arguments of align() without effect
        options.pop(k, None)
    options["token_step"] = A._checked_token_step(model, options.pop("token_step", 100))
    variant = {k: options.pop(k) for k in ("extra_models", "dynamic_heads", "aligner") if k in options}
    progress_callback = options.pop("progress_callback", None)
    if not audios:
        return []

    # ---- everything that can be refused is refused here, before any recording is decoded or any device work is queued
    by_language: dict = {}
    seconds = [0.0] * len(audios)

    def report(i: int):
        def cb(done: float, total: float):
            seconds[i] = done
        return cb if progress_callback is not None else None

    aligners = []
    for i, (text, lang) in enumerate(zip(texts, languages)):
        key = lang or getattr(text, "language", None)
        tok = by_language.get(key)
        if tok is None:
            tok = by_language[key] = A._alignment_tokenizer(model, text, lang, tokenizer)
        aligners.append(A._new_aligner(None, tok, progress_callback=report(i), **options))
    tokenizers = [by_language[lang or getattr(text, "language", None)] for text, lang in zip(texts, languages)]
    total = sum(_source_samples(a) for a in audios) / SAMPLE_RATE if progress_callback is not None else 0.0

    funcs: dict = {}

    def answer(live: list) -> List[Any]:
        """one device job for the round's requests; ``tokenizers=`` only where the round really mixes languages"""
        toks = [tokenizers[i] for i, _, _ in live]
        func = funcs.get(id(toks[0]))
        if func is None:
            func = funcs[id(toks[0])] = A.make_alignment_func(model, toks[0], **variant)
        chunks, words = [req[0] for _, _, req in live], [req[1] for _, _, req in live]
        if all(t is toks[0] for t in toks):
            return func.batch(chunks, words)
        return func.batch(chunks, words, tokenizers=toks)

    results: List[Optional[WhisperResult]] = [None] * len(audios)
    pending = list(range(len(audios)))
    pending.reverse()                                   # pop() hands them out in input order
    live: list = []                                     # (index, generator, its open request)
    done_seconds = 0.0

    def finish(i: int, result: Optional[WhisperResult]):
        nonlocal done_seconds
        if result is not None:
            result.language = A._result_language(model, tokenizers[i], languages[i])
        results[i] = result
        done_seconds += aligners[i].audio.get_duration()
        seconds[i] = 0.0

    def advance(i: int, steps, got=None):
        """the recording's next request, or None when its state machine has returned (possibly without ever asking)"""
        try:
            return next(steps) if got is None else steps.send(got)
        except StopIteration as end:
            finish(i, end.value)
            return None

    try:
        while live or pending:
            while pending and len(live) < int(max_tracks):
                i = pending.pop()
                try:
                    wave = as_waveform(audios[i], **audio_options).detach().float()
                except Exception as e:                  # what align() raises for this recording, with its place in the list
                    raise _with_index(e, i) from e
                steps = aligners[i].steps(wave, texts[i])
                request = advance(i, steps)
                if request is not None:
                    live.append((i, steps, request))
            if live:
                outs = answer(live)
                nxt = []
                for (i, steps, _), got in zip(live, outs):
                    request = advance(i, steps, got)
                    if request is not None:
                        nxt.append((i, steps, request))
                live = nxt
            if progress_callback is not None:
                progress_callback(min(done_seconds + sum(seconds), total), total)
    finally:
        for _, steps, _ in live:
            steps.close()
    return results


class DeviceProbes:
    """The probe audio of the groups in flight, resident on the device: ``clean`` f32 [max_tracks][480000] (a group's clean
    segment, uploaded once when it takes a slot) and ``probe`` f32 [2 * max_tracks][480000] (probe row r belongs to clean row
    r >> 1).  A round's list position is the slot; ``refine_tracks`` keeps the live slots dense, so rows ``[0, 2 * live)`` are what
    the log-mel reads, in place.  ``sync(probes)`` brings the device up to date with the round's ``OpsProbe`` objects: a probe
    that is new takes its slot (upload + a restore over ``[0, n)`` of both rows), one that sits in another slot is moved (a
    device-to-device copy; only the highest live slot ever moves, into a hole at the tail of a run), and the edits every probe
    recorded since the last round go out as ONE op list and ONE launch, rows offset by the slot."""

    def __init__(self, max_tracks: int, device):
        from .audio import N_SAMPLES
        self.n_samples = N_SAMPLES
        # uninitialised: a slot is filled over [0, n) when a group takes it and the log-mel never reads past a row's n_valid
        self.clean = torch.empty(max_tracks, N_SAMPLES, dtype=torch.float32, device=device)
        self.probe = torch.empty(2 * max_tracks, N_SAMPLES, dtype=torch.float32, device=device)
        self.slots: list = [None] * max_tracks

    def sync(self, probes: Sequence) -> tuple:
        """-> ``(probe rows [2 * len(probes), 480000] (a view), n_valid per row)``"""
        from .engine import pcm_edit
        if len(probes) > len(self.slots):
            raise ValueError(f"{len(probes)} probes for {len(self.slots)} slots")
        ops: list = []
        where = {id(p): k for k, p in enumerate(self.slots) if p is not None}
        for k, p in enumerate(probes):
            if self.slots[k] is p:
                continue
            j = where.get(id(p))
            if j is None:                                           # a new group: its clean segment goes up once
                self.clean[k, :p.n_kept] = p.clean[0, :p.n_kept].to(self.clean.device)
                ops += [(2 * k, 0, p.n_kept, 1), (2 * k + 1, 0, p.n_kept, 1)]
            else:                                                   # the highest live slot moves into a hole
                self.clean[k].copy_(self.clean[j])
                self.probe[2 * k: 2 * k + 2].copy_(self.probe[2 * j: 2 * j + 2])
        self.slots = list(probes) + [None] * (len(self.slots) - len(probes))
        for k, p in enumerate(probes):
            ops += [(2 * k + row, a, b, kind) for row, a, b, kind in p.take()]
        if ops:
            pcm_edit(self.clean, self.probe, ops, n_rows=2 * len(probes))
        return self.probe[: 2 * len(probes)], [p.n_kept for p in probes for _ in range(2)]


@host_single_thread
def refine_many(model, audios: Sequence, results: Sequence[WhisperResult], *, max_tracks: int = 16, device_probes: bool = False,
                **refine_options) -> List[WhisperResult]:
    """``[model.refine(a, r, **refine_options) for a, r in zip(audios, results)]`` with the word groups of all recordings bisected
    in lockstep: up to ``max_tracks`` groups of any recordings per device pass (2 windows each), every result equal to the one of
    ``refine`` alone, in input order.  ``audios``: whatever ``refine`` takes per item.  ``results``: a ``WhisperResult`` per
    recording; one without words or probabilities goes through ``align_words`` first, as in ``refine`` (a result without any
    words comes back as it is; ``refine`` alone raises IndexError there).  Options are those of ``refine`` except ``batch_size``;
    ``inplace`` applies per result; ``progress_callback(seconds_done, seconds_total)`` counts all recordings.
    ``device_probes=True``: the probe audio stays on the device and a round uploads only the bisection's edits (``swx_pcm_edit``)
    instead of rebuilding the probes on the host and uploading them every round; the same PCM bits reach the model either way.
    Off by default: measured, it is not faster beyond the spread of the repeats.  The device workspace
    grows to ``2 * max_tracks`` windows and no further (with device probes plus 3 x 1.92 MB x ``max_tracks`` of probe audio)."""
    from . import alignment as A
    from .audio import N_SAMPLES, SAMPLE_RATE
    from .refiner import OpsProbe, Refiner, refine_tracks
    from .tokenizer import get_tokenizer
    from .transcribe import _with_index, as_waveform, pop_audio_options
    if refine_options.get("batch_size") is not None:
        raise NotImplementedError("batch_size does not combine with refine_many")
    if isinstance(audios, (str, bytes)) or not hasattr(audios, "__len__") or hasattr(audios, "shape"):
        raise TypeError("audios must be a list of recordings (refine() takes a single one)")
    audios = list(audios)
    if isinstance(results, WhisperResult) or not hasattr(results, "__len__"):
        raise TypeError("results must be a list with one WhisperResult per recording")
    results = list(results)
    if len(results) != len(audios):
        raise ValueError(f"results has {len(results)} entries for {len(audios)} recordings")
    if max_tracks is None or isinstance(max_tracks, bool) or int(max_tracks) != max_tracks or int(max_tracks) < 1:
        raise ValueError(f"max_tracks must be an integer of at least 1, got {max_tracks}")
    max_tracks = int(max_tracks)
    options = dict(refine_options)
    audio_options = pop_audio_options(options)
    for k in ("batch_size", "single_batch"):                       # named arguments of refine() without effect here
        options.pop(k, None)
    inplace = options.pop("inplace", True)
    progress_callback = options.pop("progress_callback", None)
    if not audios:
        return []

    # ---- everything that can be refused is refused here, before any recording is decoded or any device work is queued
    by_language: dict = {}
    refiners, to_align = [], []
    for i, result in enumerate(results):
        if not isinstance(result, WhisperResult):
            raise TypeError(f"results[{i}] is not a WhisperResult")
        needs_words = bool(result) and (not result.has_words or any(w.probability is None for w in result.all_words()))
        if needs_words and not result.language:
            raise _with_index(RuntimeError("cannot align words with result missing language"), i)
        to_align.append(needs_words)
        key = result.language or "en"
        if key not in by_language:
            by_language[key] = get_tokenizer(model.is_multilingual, num_languages=model.num_languages, language=key,
                                             task="transcribe")
        refiners.append(Refiner(None, sample_rate=SAMPLE_RATE, max_inference_tokens=model.dims.n_text_ctx - 6, **options))
    tokenizers = [by_language[r.language or "en"] for r in results]
    func = A.make_refinement_func(model, tokenizers[0])

    work: List[WhisperResult] = []
    for i, (audio, result) in enumerate(zip(audios, results)):
        try:
            if to_align[i]:
                result = A.align_words(model, audio, result)
            wave = as_waveform(audio, **audio_options)
        except Exception as e:                                     # what refine() raises for this recording, with its place
            raise _with_index(e, i) from e
        if device_probes:
            refiners[i].probe_buffer = lambda clean: OpsProbe(clean, limit=N_SAMPLES)
        work.append(refiners[i]._prepare(wave, result, inplace, tokenizers[i].encode))

    resident = DeviceProbes(max_tracks, model.device) if device_probes else None

    def answer(flying: list) -> List[Any]:
        """one device pass for the round's probes; ``tokenizers=`` only where the round really mixes languages"""
        toks = [tokenizers[i] for i, _ in flying]
        kw = {} if all(t is toks[0] for t in toks) and toks[0] is tokenizers[0] else dict(tokenizers=toks)
        if resident is None:
            return func.batch([(request[0], request[1]) for _, request in flying], **kw)
        rows = resident.sync([request[0] for _, request in flying])
        return func.batch([(None, request[1]) for _, request in flying], resident=rows, **kw)

    return refine_tracks(refiners, work, max_tracks, answer, progress_callback)


@host_single_thread
def locate_many(model, audios: Sequence, texts: Sequence[Union[str, List[int]]], language: Union[str, Sequence[str]], *,
                max_tracks: int = 16, device_probe: Optional[bool] = None, **locate_options) -> List[list]:
    """``[model.locate(a, t, language=l, **locate_options) for a, t, l in zip(audios, texts, languages)]`` with the current chunk of
    up to ``max_tracks`` recordings per device pass, in input order.  ``audios``: whatever ``locate`` takes per item; the same object
    may appear several times (many phrases in one recording).  ``texts``: a ``str`` or token ids per recording.  ``language``: one
    code for all, or a list with a code per recording.  Options are those of ``locate``.

    Every recording runs the state machine ``locate`` runs (``locator.LocateJob.steps``); a round answers the requests of the live
    recordings phase by phase, one device call each: (A) log-mel, encoder, cross-K/V and the scoring pass of the round's chunks,
    (B) encoder and cross-K/V of the duration windows (modes 0 and 1), (C) the greedy steps of all these windows, ragged in
    length, until every window has stopped -- a stopped window stays in the batch as a one-token dummy, the cross-K/V is never
    copied between steps -- and (D) one word-timestamp job for the windows of mode 0 that confirmed their text.  A recording that
    runs out of audio or reaches ``count`` hands its slot to the next pending one at the round boundary.

    ``device_probe``: how a greedy step is answered.  True = ``Engine.forward_next_token`` (``swx_forward_next_token``: the last row
    of every window projected on the vocabulary, two ids and three probabilities per window copied back); False = one batched
    ``forward_logits`` call and the host arithmetic of ``locate``; None = the native call where the engine has it.  With False
    the results are those of the loop exactly, except that a greedy step whose context was cleared to ONE token takes another
    cross-attention kernel next to longer windows than alone (rounding-level); the native call differs from the host arithmetic
    by rounding (probabilities within 5e-5 in log), breaks an exact tie of two logits towards the higher id and never selects a
    NaN logit (the host sort ranks it highest).  The device
    workspace grows to ``max_tracks`` windows and no further; the cross-K/V of a round's chunks and of its duration windows are
    alive together (2 x ``max_tracks`` windows)."""
    from .locator import LocateJob, _pad_frames, end_row_tokens, next_token_on_host
    from .audio import N_FFT
    from .timing import add_word_timestamps_batch
    if isinstance(audios, (str, bytes)) or not hasattr(audios, "__len__") or hasattr(audios, "shape"):
        raise TypeError("audios must be a list of recordings (locate() takes a single one)")
    audios = list(audios)
    if isinstance(texts, str) or not hasattr(texts, "__len__"):
        raise TypeError("texts must be a list with one text per recording")
    texts = list(texts)
    if len(texts) != len(audios):
        raise ValueError(f"texts has {len(texts)} entries for {len(audios)} recordings")
    if max_tracks is None or isinstance(max_tracks, bool) or int(max_tracks) != max_tracks or int(max_tracks) < 1:
        raise ValueError(f"max_tracks must be an integer of at least 1, got {max_tracks}")
    max_tracks = int(max_tracks)
    if language is None or isinstance(language, str):
        languages = [language] * len(audios)
    else:
        languages = list(language)
        if len(languages) != len(audios):
            raise ValueError(f"language has {len(languages)} entries for {len(audios)} recordings")
    eng = model.engine
    native = bool(getattr(eng, "device_next_token", False))
    if device_probe and not native:
        raise RuntimeError("device_probe=True needs an engine with forward_next_token")
    if device_probe is not None:
        native = bool(device_probe)
    # ---- everything that can be refused is refused here, before any recording is decoded or any device work is queued
    jobs = [LocateJob(model, text, lang, **locate_options) for text, lang in zip(texts, languages)]
    if not audios:
        return []
    n_ctx = model.dims.n_audio_ctx
    alive: List[dict] = []                              # the device buffers of the current round

    def answer(kind: str, batch: list) -> List[Any]:
        """one device call for the requests of one phase; ``batch`` = [(recording, request)]"""
        if kind == "chunk":
            # the generators still hold last round's handles: empty the buffers behind them before the new ones are made, so
            # that two cross-K/V buffers are alive at a time (this round's chunks and its duration windows), not three
            for buffers in alive:
                buffers.clear()
            del alive[:]
            mel = model.log_mel_segments([req[1] for _, req in batch], padding=N_FFT // 2 + 1)
            whole = dict(mel=mel, xkv=model.cross_kv(model.encoder(mel)), n=len(batch))
            alive.append(whole)
            return [(whole, k) for k in range(len(batch))]
        if kind == "section":
            mel = torch.stack([_pad_frames(req[1][0]["mel"][req[1][1]][..., req[2]: req[3]]) for _, req in batch])
            part = dict(xkv=model.cross_kv(model.encoder(mel)), n=len(batch))
            alive.append(part)
            return [(part, k) for k in range(len(batch))]
        held = batch[0][1][1][0]                           # the phase's windows live in one buffer: [L][B][...] cannot be sliced
        assert all(req[1][0] is held for _, req in batch), "requests of one phase come from one batch"
        eot = jobs[batch[0][0]].tok.eot
        if kind == "end_row":
            assert [req[1][1] for _, req in batch] == list(range(held["n"]))
            rows = [end_row_tokens(jobs[i], req[2]) for i, req in batch]
            _, neg, _ = eng.score(held["xkv"], rows, [n_ctx] * len(rows), n_sot=0, eot=eot)
            return [(-neg[k, len(r) - 2, :n_ctx]).float().cpu() for k, r in enumerate(rows)]
        if kind == "next":
            out: List[Any] = [None] * len(batch)
            lists: dict = {}
            for b, (i, _) in enumerate(batch):
                lists.setdefault(tuple(jobs[i].suppressed), []).append(b)
            # a target id outside [0, eot) is an IndexError in locate(); the kernel would answer probability 0: such a step takes
            # the host arithmetic and raises what locate() raises
            on_device = native and all(req[3] == -1 or 0 <= req[3] < eot for _, req in batch)
            for suppressed, members in lists.items() if on_device else [(None, list(range(len(batch))))]:
                tokens, targets = [[0]] * held["n"], [-1] * held["n"]          # a window that has stopped: a one-token dummy
                for b in members:
                    req = batch[b][1]
                    tokens[req[1][1]], targets[req[1][1]] = req[2], req[3]
                if on_device:
                    top, prob = eng.forward_next_token(held["xkv"], tokens, eot, suppressed, targets)
                    for b in members:
                        k = batch[b][1][1][1]
                        out[b] = (int(top[k, 0]), int(top[k, 1]), float(prob[k, 0]), float(prob[k, 1]), float(prob[k, 2]))
                else:
                    logits = eng.forward_logits(held["xkv"], tokens)
                    ks = [batch[b][1][1][1] for b in members]
                    last = torch.stack([logits[k, len(tokens[k]) - 1, : eot + 1] for k in ks]).float().cpu()
                    for b, row in zip(members, last):
                        i, req = batch[b]
                        out[b] = next_token_on_host(row.clone(), eot, jobs[i].suppressed, req[3])
            return out
        from . import transcribe as T
        toks = [jobs[i].tok for i, _ in batch]
        segs = [dict(seek=0, tokens=req[2]) for _, req in batch]
        add_word_timestamps_batch(model=model, tokenizer=toks[0] if all(t is toks[0] for t in toks) else toks,
                                  xkv=T._xkv_select(model, held["xkv"], [req[1][1] for _, req in batch]), gap_padding=None,
                                  windows=[dict(segments=[seg], num_samples=req[3]) for seg, (_, req) in zip(segs, batch)])
        return [seg["words"] for seg in segs]

    results: List[Optional[list]] = [None] * len(audios)
    pending = list(range(len(audios)))
    pending.reverse()                                   # pop() hands them out in input order
    live: list = []                                     # [recording, generator, its open request]

    def advance(i: int, steps, got=None):
        try:
            return steps.send(got)
        except StopIteration as end:
            results[i] = end.value
            return None

    try:
        while live or pending:
            if all(request[0] == "chunk" for _, _, request in live):       # the round boundary: free slots go to pending recordings
                while pending and len(live) < max_tracks:
                    i = pending.pop()
                    steps = jobs[i].steps(jobs[i].waveform(audios[i]))
                    request = advance(i, steps)
                    if request is not None:
                        live.append([i, steps, request])
                if not live:
                    continue
            # everybody leaves "chunk" together, and a recording waits at its next "chunk" until nobody is in a phase of the
            # current round any more: the phases of a round are answered in their order, "chunk" last
            kind = next(k for k in ("end_row", "section", "next", "words", "chunk") if any(r[0] == k for _, _, r in live))
            members = [entry for entry in live if entry[2][0] == kind]
            for entry, got in zip(members, answer(kind, [(i, request) for i, _, request in members])):
                entry[2] = advance(entry[0], entry[1], got)
            live = [entry for entry in live if entry[2] is not None]
    finally:
        for _, steps, _ in live:
            steps.close()
    return results
