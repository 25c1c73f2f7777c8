"""model.align() / model.align_words(): forced alignment of given text (stable_whisper/alignment.py:27-368).

Per window the device work is mel -> encoder -> one teacher-forced decoder pass with the alignment heads' qk captured
-> softmax / z-norm / median / head-mean -> DTW; no autoregressive decoding.  The boundary the
reference defines for this is ``compute_timestamps(audio_segment, word_tokens)`` (alignment.py:405-429, seam B2):
`make_alignment_func` returns exactly that callable, and `align` drives it with `stable_ts_amd.aligner.Aligner`, the
restatement of the reference's window state machine (non_whisper/alignment.py:58-1033: token batching by
``token_step``, gap padding, non-speech skipping, the re-alignment policy of ``_fallback``), which is tested against
the reference's own class on CPU (tests/test_aligner_cpu.py).
"""
from typing import List, Optional, Sequence, Tuple, Union

import torch

from .stabilization import host_single_thread
from .audio import N_SAMPLES, SAMPLE_RATE
from .result import WhisperResult
from .timing import add_word_timestamps_batch
from .tokenizer import get_tokenizer


from .aligner import WordToken  # noqa: E402,F401  (re-exported: the seam-B2 callable takes these)


def make_alignment_func(model, tokenizer, extra_models: Optional[list] = None, dynamic_heads=None,
                        aligner: Union[str, dict] = "legacy"):
    """alignment.py:396-429: inference_func(audio_segment f32[n<=480000], word_tokens) -> list of word dicts with times
    relative to the segment start.  ``extra_models`` / ``dynamic_heads`` / ``aligner`` select the head-selection variants
    of the attention stage (timing.py)."""

    def compute_timestamps(audio_segment: torch.Tensor, word_tokens: List[WordToken]) -> List[dict]:
        return compute_timestamps_batch([audio_segment], [word_tokens])[0]

    def compute_timestamps_batch(audio_segments: Sequence[torch.Tensor], word_tokens_list: Sequence[List[WordToken]],
                                 tokenizers: Optional[Sequence] = None):
        """``tokenizers``: one per window where the windows belong to recordings in different languages (``align_many``);
        every window then carries its own sot sequence and splits its words by its own language, in the same device job."""
        from . import transcribe as _tr                     # diagnostic stage timer (bench.py --phase-times), off by default
        import time
        t_ph = time.perf_counter() if _tr.PHASE_TIMES is not None else 0.0
        n = [int(a.shape[-1]) for a in audio_segments]
        mel = model.log_mel_batch(list(audio_segments), [max(N_SAMPLES - k, 0) for k in n])
        t_ph = _tr._phase("align: audio upload + mel", t_ph)
        xa = model.encoder(mel)
        t_ph = _tr._phase("align: encoder", t_ph)
        xkv = model.cross_kv(xa)
        t_ph = _tr._phase("align: cross K/V", t_ph)
        windows = []
        for k, wts in zip(n, word_tokens_list):
            seg = dict(seek=0, tokens=([w.word for w in wts], [list(w.tokens) for w in wts]))
            windows.append(dict(segments=[seg], num_samples=k))
        add_word_timestamps_batch(model=model, tokenizer=tokenizer if tokenizers is None else list(tokenizers),
                                  windows=windows, xkv=xkv, split_callback=lambda x, _: x, gap_padding=None,
                                  prepend_punctuations="", append_punctuations="", extra_models=extra_models,
                                  dynamic_heads=dynamic_heads, aligner=aligner, mel=mel if extra_models else None)
        _tr._phase("align: word timestamps (scoring pass + a7 + DTW + host)", t_ph)
        return [w["segments"][0]["words"] for w in windows]

    compute_timestamps.batch = compute_timestamps_batch
    return compute_timestamps


def make_refinement_func(model, tokenizer):
    """alignment.py:636-672 (seam B3): ``inference_func(audio_segment f32[2, n], tokens) -> probabilities
    [2, len(tokens), eot]`` over the text vocabulary, a device tensor.  Both audio copies go through mel -> encoder ->
    cross-KV and ONE teacher-forced decoder pass of ``sot_sequence + [no_timestamps] + tokens + [eot]``.
    ``inference_func.batch`` is the native form ``refine(batch_size=N)`` drives: the probes of several word groups in one pass,
    answered with ``(probability, rank)`` per token instead of a distribution.
    Like the reference the log-mel is computed on the un-padded segment and the remaining frames are filled with 0.0
    (``pad_or_trim`` of the mel, not of the audio).  Host-side bisection: stable_ts_amd/refiner.py (CPU-tested against
    the reference's Refiner); the callable is CPU-tested against the reference's on the engine stand-in
    (tests/test_locate_cpu.py) and has a hardware check (tests/hw_checks/b3_check.py; status in DESIGN.md section 7)."""
    sot = list(tokenizer.sot_sequence)

    def inference_func(audio_segment: torch.Tensor, tokens: List[int]) -> torch.Tensor:
        audio_segment = audio_segment[..., :N_SAMPLES]      # the Refiner's probes are word-local, far below 30 s
        mel = model.log_mel_segments([audio_segment[0], audio_segment[1]], batch_max=True)
        xkv = model.cross_kv(model.encoder(mel))
        ids = [*sot, tokenizer.no_timestamps, *[int(t) for t in tokens], tokenizer.eot]
        logits = model.engine.forward_logits(xkv, [ids, ids])
        return logits[:, len(sot): len(sot) + len(tokens), : tokenizer.eot].softmax(dim=-1)

    def inference_batch(items: Sequence[Tuple[torch.Tensor, List[int]]], tokenizers: Optional[Sequence] = None,
                        resident: Optional[Tuple[torch.Tensor, Sequence[int]]] = None) -> List[Tuple[torch.Tensor, torch.Tensor]]:
        """[(audio[2, n_g], tokens_g)] -> [(p[2, T_g], rank[2, T_g])] (host tensors): ONE mel / encoder / cross-KV / decoder
        pass over all 2 G windows, ragged in audio length and token count.  Each pair of copies keeps its own log-mel clamp
        floor (``swx_log_mel_ragged_grouped``), and of every row of the pass only the target token's probability and its rank
        in the row leave the device (``swx_forward_token_ranks``) -- the two numbers per token the bisection reads.
        ``tokenizers``: one per item where the groups belong to recordings in different languages (``refine_many``); every pair
        of windows then carries its own sot sequence.  ``resident = (pcm f32 [2 G, 480000] on the device, n_valid [2 G])``: the
        probes already lie there in the items' order (``refine_many``'s probe rows, read in place); the items' audio is not looked
        at and nothing is staged or uploaded."""
        if not items:
            return []
        toks = [tokenizer] * len(items) if tokenizers is None else list(tokenizers)
        if len(toks) != len(items):
            raise ValueError(f"{len(toks)} tokenizers for {len(items)} items")
        segs, ids, lead = [], [], []
        for (audio_segment, tokens), tok in zip(items, toks):
            if resident is None:
                audio_segment = audio_segment[..., :N_SAMPLES]
                segs += [audio_segment[0], audio_segment[1]]
            head = list(tok.sot_sequence)
            lead.append(len(head))
            ids += [[*head, tok.no_timestamps, *[int(t) for t in tokens], tok.eot]] * 2
        if resident is None:
            mel = model.log_mel_segments(segs, group=2)
        else:
            pcm, n_valid = resident
            if pcm.shape[0] != 2 * len(items) or len(n_valid) != 2 * len(items):
                raise ValueError(f"{pcm.shape[0]} resident rows and {len(n_valid)} lengths for {len(items)} items")
            n_valid = [int(n) for n in n_valid]
            mel = model.engine.log_mel_ragged(pcm, n_valid, n_valid, per_item_max=False, group=2)
        xkv = model.cross_kv(model.encoder(mel))
        prob, rank = model.engine.forward_token_ranks(xkv, ids, n_vocab_used=tokenizer.eot)
        prob, rank = prob.cpu(), rank.cpu()
        return [(prob[2 * g: 2 * g + 2, k: k + len(tokens)], rank[2 * g: 2 * g + 2, k: k + len(tokens)])
                for g, ((_, tokens), k) in enumerate(zip(items, lead))]

    inference_func.batch = inference_batch
    return inference_func


def _checked_token_step(model, token_step: int) -> int:
    max_step = model.dims.n_text_ctx - 6                       # alignment.py:181-185
    if token_step < 1:
        return max_step
    if token_step > max_step:
        raise ValueError(f"The max value for [token_step] is {max_step} but got {token_step}.")
    return token_step


def _alignment_tokenizer(model, text, language, tokenizer=None):
    """the tokenizer ``align`` works with: the caller's, or the one of ``language`` (a WhisperResult text brings its own)"""
    if tokenizer is not None:
        return tokenizer
    if not language and model.is_multilingual and (language := getattr(text, "language", None)) is None:
        raise TypeError("expected argument for language")                                  # alignment.py:375-383
    return get_tokenizer(model.is_multilingual, num_languages=model.num_languages, language=language or "en", task="transcribe")


def _language_code(tokenizer) -> Optional[str]:
    return getattr(tokenizer, "language_code", None) or getattr(tokenizer, "language", None)


def _result_language(model, tokenizer, language) -> Optional[str]:
    return _language_code(tokenizer) or language or (None if model.is_multilingual else "en")    # alignment.py:388-393


def _new_aligner(inference_func, tokenizer, **options):
    """``Aligner`` over this package's audio constants with the word splitting of the tokenizer's language"""
    from .aligner import Aligner
    return Aligner(inference_func=inference_func, decode=tokenizer.decode, encode=tokenizer.encode,
                   split_words_by_space=_language_code(tokenizer) not in {"zh", "ja", "th", "lo", "my"}, sample_rate=SAMPLE_RATE,
                   max_segment_length=N_SAMPLES, **options)


@host_single_thread
def align(model, audio, text: Union[str, List[int], WhisperResult], language: str = None, *, tokenizer=None,
          ignore_compatibility: bool = False, remove_instant_words: bool = False, token_step: int = 100,
          original_split: bool = False, word_dur_factor: Optional[float] = 2.0, max_word_dur: Optional[float] = 3.0,
          nonspeech_skip: Optional[float] = 5.0, fast_mode: bool = False, failure_threshold: Optional[float] = None,
          batch_size: int = 1, **options) -> Optional[WhisperResult]:
    """Forced alignment of ``text`` (plain text, token ids, or a WhisperResult whose text is re-aligned) with ``audio``
    (alignment.py:27-216).  The window state machine -- token batching, gap padding, non-speech skipping, the
    re-alignment policy -- is :class:`stable_ts_amd.aligner.Aligner`, a restatement of the reference's ``Aligner`` that is
    checked against it window for window on CPU; each window's timestamps come from the device through
    ``make_alignment_func`` (seam B2).  Returns None when nothing could be aligned."""
    from .transcribe import as_waveform, pop_audio_options
    audio_options = pop_audio_options(options)
    token_step = _checked_token_step(model, token_step)
    tokenizer = _alignment_tokenizer(model, text, language, tokenizer)
    variant = {k: options.pop(k) for k in ("extra_models", "dynamic_heads", "aligner") if k in options}
    aligner = _new_aligner(make_alignment_func(model, tokenizer, **variant), tokenizer, remove_instant_words=remove_instant_words,
                           token_step=token_step, original_split=original_split, word_dur_factor=word_dur_factor,
                           max_word_dur=max_word_dur, nonspeech_skip=nonspeech_skip, fast_mode=fast_mode,
                           failure_threshold=failure_threshold, **options)
    # the waveform stays where it is: windows of a recording that is resident on the GPU are analysed there (device probe of
    # the silence analysis) and are not uploaded again
    result = aligner.align(as_waveform(audio, **audio_options).detach().float(), text)
    if result is not None:
        result.language = _result_language(model, tokenizer, language)
    return result


@host_single_thread
def align_words(model, audio, result: Union[WhisperResult, List[dict]], language: str = None, *,
                ignore_compatibility: bool = False, tokenizer=None, normalize_text: bool = True, inplace: bool = True,
                batch_size: int = 8, **options) -> WhisperResult:
    """alignment.py:219-368 / non_whisper/alignment.py:396-474: (re-)time the words of every segment inside the
    segment's own start/end.  Segments are independent, so ``batch_size`` of them share one encoder / scoring pass on
    the device (the reference runs them one by one); the host logic is ``Aligner.align_words``, compared with the
    reference's on CPU, batched and unbatched."""
    from .aligner import Aligner
    from .transcribe import as_waveform, pop_audio_options
    # the fallback machinery of align() does not exist here: its options are refused like any unknown keyword
    # (options.py:16-18 via AllOptions at alignment.py:350)
    extras = [k for k in options if k in ("remove_instant_words", "token_step", "original_split", "word_dur_factor",
                                          "max_word_dur", "nonspeech_skip", "fast_mode", "failure_threshold")]
    if extras:
        raise TypeError(f"got unexpected keyword argument(s): {', '.join(extras)}")
    audio_options = pop_audio_options(options)
    if tokenizer is None:
        language = language or getattr(result, "language", None)
        if not language and model.is_multilingual:
            raise TypeError("expected argument for language")
        tokenizer = get_tokenizer(model.is_multilingual, num_languages=model.num_languages, language=language or "en",
                                  task="transcribe")
    lang_code = getattr(tokenizer, "language_code", None) or getattr(tokenizer, "language", None)
    variant = {k: options.pop(k) for k in ("extra_models", "dynamic_heads", "aligner") if k in options}
    func = make_alignment_func(model, tokenizer, **variant)

    def clipped(fn):        # a segment longer than one window is aligned against its first 30 s (the reference trims the mel)
        return lambda chunks, words: fn([c[..., :N_SAMPLES] for c in chunks], words)

    aligner = Aligner(inference_func=lambda seg, words: clipped(func.batch)([seg], [words])[0], decode=tokenizer.decode,
                      encode=tokenizer.encode, split_words_by_space=lang_code not in {"zh", "ja", "th", "lo", "my"},
                      sample_rate=SAMPLE_RATE, max_segment_length=N_SAMPLES, token_step=model.dims.n_text_ctx, **options)
    out = aligner.align_words(as_waveform(audio, **audio_options).detach().float(), result, normalize_text, inplace,
                              batch_inference=clipped(func.batch), batch_size=batch_size)
    out.language = lang_code or language or (None if model.is_multilingual else "en")
    return out

@host_single_thread
def refine(model, audio, result: WhisperResult, *, steps: str = None, rel_prob_decrease: float = .03,
           abs_prob_decrease: float = .05, rel_rel_prob_decrease: Optional[float] = None, prob_threshold: float = .5,
           rel_dur_change: Optional[float] = .5, abs_dur_change: Optional[float] = None, word_level: bool = True,
           precision: float = None, single_batch: bool = False, inplace: bool = True, batch_size: Optional[int] = None,
           **options) -> WhisperResult:
    """alignment.py:512-635: move word starts later / ends earlier as far as the token probabilities allow.  The
    bisection is :class:`stable_ts_amd.refiner.Refiner`; ``single_batch`` is accepted for signature compatibility (the
    two audio copies always share one batched pass here).

    ``batch_size``: None = one word group after the other, each probe a full-vocabulary distribution handed to the host
    logic (the reference's order of calls).  N >= 1 = the native probe (``swx_forward_token_ranks``: a probability and a rank
    per token leave the device) with up to N word groups of a step bisected in lockstep, 2 N windows per device pass; 1 is
    the native probe group by group.  The workspace grows to the 2 * min(N, groups) windows a round really holds
    (DESIGN.md section 8 lists the memory per N)."""
    from .refiner import Refiner
    from .transcribe import as_waveform, pop_audio_options
    audio_options = pop_audio_options(options)
    if result and (not result.has_words or any(w.probability is None for w in result.all_words())):
        if not result.language:
            raise RuntimeError("cannot align words with result missing language")
        result = align_words(model, audio, result)
    tokenizer = get_tokenizer(model.is_multilingual, num_languages=model.num_languages, language=result.language or "en",
                              task="transcribe")
    if result and not all(w.tokens for w in result.all_words()):
        for w in result.all_words():
            w.tokens = tokenizer.encode(w.word)
    refiner = Refiner(make_refinement_func(model, tokenizer), sample_rate=SAMPLE_RATE, steps=steps,
                      rel_prob_decrease=rel_prob_decrease, abs_prob_decrease=abs_prob_decrease,
                      rel_rel_prob_decrease=rel_rel_prob_decrease, prob_threshold=prob_threshold,
                      rel_dur_change=rel_dur_change, abs_dur_change=abs_dur_change, word_level=word_level,
                      precision=precision, max_inference_tokens=model.dims.n_text_ctx - 6, batch_size=batch_size, **options)
    return refiner.refine(as_waveform(audio, **audio_options), result, inplace)
