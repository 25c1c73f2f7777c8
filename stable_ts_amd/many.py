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
"""
from typing import Any, List, Optional, Sequence, Union

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
