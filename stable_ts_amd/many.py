"""Many recordings at once: ``model.transcribe`` per recording, all of them advanced together on this device.

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
"""
from typing import List, Optional, Sequence, Union

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
