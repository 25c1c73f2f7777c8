"""Result writers: SRT, VTT, ASS, TSV, TXT and JSON output of a transcription result.

The public functions carry the names, signatures and defaults of stable-ts's ``text_output`` module and produce the
same bytes for the same input (pinned case by case by tests/golden/text_output_cases.json.gz, which is recorded from
the reference's own writers).  ``result`` is a :class:`~stable_ts_amd.result.WhisperResult`, a result ``dict`` or a
list of segment dicts.

Shape: every format goes through :func:`result_to_any`, which turns the input into a flat list of cues --
``dict(text=, start=, end=)`` -- by one of four cue builders (per segment, per word, per word with the whole segment
shown and the active word tagged, per segment with inline word timing), and hands the cues to one small renderer per
format.

Host-only by design: formatting a result is microseconds of string work after a device pass of hundreds of
milliseconds; there is nothing here for the GPU to do.
"""
import json
import os
import warnings
from typing import Callable, List, Optional, Tuple, Union

__all__ = ["result_to_srt_vtt", "result_to_ass", "result_to_tsv", "result_to_txt", "save_as_json", "load_result"]

SUPPORTED_FORMATS = ("srt", "vtt", "ass", "tsv", "txt")

_SRT_TAG = ('<font color="#00ff00">', "</font>")
_UNDERLINE_TAG = ("<u>", "</u>")

# the V4+ style line of an ASS file: the fields the format prescribes, with the values an unstyled export carries
_ASS_STYLE = (
    ("Name", "Default"), ("Fontname", "Arial"), ("Fontsize", "48"),
    ("PrimaryColour", "&Hffffff"), ("SecondaryColour", "&Hffffff"), ("OutlineColour", "&H0"), ("BackColour", "&H0"),
    ("Bold", "0"), ("Italic", "0"), ("Underline", "0"), ("StrikeOut", "0"),
    ("ScaleX", "100"), ("ScaleY", "100"), ("Spacing", "0"), ("Angle", "0"),
    ("BorderStyle", "1"), ("Outline", "1"), ("Shadow", "0"), ("Alignment", "2"),
    ("MarginL", "10"), ("MarginR", "10"), ("MarginV", "10"), ("Encoding", "0"),
)
_ASS_SCRIPT_INFO = "[Script Info]\nScriptType: v4.00+\nPlayResX: 384\nPlayResY: 288\nScaledBorderAndShadow: yes\n\n"
_ASS_EVENTS = "[Events]\nFormat: Layer, Start, End, Style, Name, MarginL, MarginR, MarginV, Effect, Text\n\n"


# ---------------------------------------------------------------------------------------------------------------------
# time fields
#
# The hour and minute come from float ``divmod`` and every field is rounded on its own by the format spec, so a
# seconds field can read 60.000 (59.9996 s), hours grow past two digits, and the ASS seconds field -- whose width of 2
# is below its own length -- is never zero-padded.  These edges are part of the pinned output.

def _clock(seconds, sec_spec: str, hour_spec: str = "0>2.0f") -> str:
    minutes, sec = divmod(seconds, 60)
    hours, minutes = divmod(minutes, 60)
    return ":".join((format(hours, hour_spec), format(minutes, "0>2.0f"), format(sec, sec_spec)))


def sec2vtt(seconds) -> str:
    """``HH:MM:SS.mmm``"""
    return _clock(seconds, "0>6.3f")


def sec2srt(seconds) -> str:
    """``HH:MM:SS,mmm``"""
    return sec2vtt(seconds).replace(".", ",")


def sec2ass(seconds) -> str:
    """``H:MM:SS.cc``"""
    return _clock(seconds, "0>2.2f", "0>1.0f")


def sec2milliseconds(seconds) -> int:
    return round(seconds * 1000)


def sec2centiseconds(seconds) -> int:
    return round(seconds * 100)


def finalize_text(text: str, strip: bool = True) -> str:
    """The text of one cue: stripped, and without the space that follows a line break."""
    return text.strip().replace("\n ", "\n") if strip else text


# ---------------------------------------------------------------------------------------------------------------------
# input -> segment dicts

def _segments_of(result, min_dur: float, reverse_text) -> Optional[List[dict]]:
    """The segment dicts to write.  Only a result object is sanitised (on a copy, the caller's is left alone); a dict
    or a list is taken as it is, so whatever a cue builder edits in it the caller sees."""
    if isinstance(result, list):
        return result
    if isinstance(result, dict):
        if reverse_text:
            warnings.warn(f"``reverse_text=True`` only applies to WhisperResult but result is {type(result)}")
        return result.get("segments")
    if not callable(getattr(result, "segments_to_dicts", None)):
        return result
    sanitised = result.apply_min_dur(min_dur, inplace=False)
    return sanitised.segments_to_dicts(reverse_text=reverse_text)


def _all_have_words(segments: List[dict]) -> bool:
    for seg in segments:
        if not seg.get("words"):
            warnings.warn("Result is missing word timestamps. Word-level timing cannot be exported. "
                          "Use ``word_level=False`` to avoid this warning")
            return False
    return True


def _in_order(cues: List[dict]) -> bool:
    stamps = [t for c in cues for t in (c["start"], c["end"])]
    return not any(a > b for a, b in zip(stamps, stamps[1:]))


def _cue(text: str, start, end) -> dict:
    return dict(text=text, start=start, end=end)


# ---------------------------------------------------------------------------------------------------------------------
# cue builders: segment dicts -> flat list of cues

def to_word_level(segments: List[dict]) -> List[dict]:
    """One cue per word."""
    return [_cue(w["word"], w["start"], w["end"]) for seg in segments for w in seg["words"]]


def _tagged(word: str, tag: Tuple[str, str]) -> str:
    """``word`` wrapped in ``tag``; a leading space stays outside the tag and blank words are left alone."""
    if word in ("", " "):
        return word
    lead = " " if word.startswith(" ") else ""
    return f"{lead}{tag[0]}{word[len(lead):]}{tag[1]}"


def words2segments(words: List[dict], tag: Tuple[str, str], reverse_text: bool = False) -> List[dict]:
    """The cues of one segment shown whole while each word is active: one cue per word with that word tagged, and an
    untagged cue for every gap between consecutive words (times compared at millisecond resolution)."""
    slots = []                                          # (text, start, end): the words and the gaps between them
    for i, w in enumerate(words):
        end = round(w["end"], 3)
        slots.append((w["word"], round(w["start"], 3), end))
        if w != words[-1]:                              # by value: a word equal to the last one closes no gap
            following = round(words[i + 1]["start"], 3)
            if following - end != 0:
                slots.append(("", end, following))
    shown = range(len(slots))
    if reverse_text:
        shown = shown[::-1]
    return [_cue("".join(_tagged(slots[j][0], tag) if j == active else slots[j][0] for j in shown), start, end)
            for active, (_, start, end) in enumerate(slots)]


def to_word_level_segments(segments: List[dict], tag: Tuple[str, str]) -> List[dict]:
    """Segment and word level together, with a highlight tag."""
    cues = []
    for seg in segments:
        cues += words2segments(seg["words"], tag, reverse_text=seg.get("reversed_text"))
    return cues


def _vtt_inline_text(words: List[dict]) -> str:
    """The words of one cue with WebVTT's inline ``<timestamp>`` before every word but the first.  Where two words do
    not touch, the gap is written as ``<end> <start>`` and takes the place of the space between them: the space is
    dropped from the text so far or else from the word -- in the word's dict itself, which for dict / list input is
    the caller's."""
    text, prev_end = "", 0
    for i, w in enumerate(words):
        if i:
            if w["start"] == prev_end:
                text += f"<{sec2vtt(w['start'])}>"
            else:
                if text.endswith(" "):
                    text = text[:-1]
                elif w["word"].startswith(" "):
                    w["word"] = w["word"][1:]
                text += f"<{sec2vtt(prev_end)}> <{sec2vtt(w['start'])}>"
        text += w["word"]
        prev_end = w["end"]
    return text


def to_vtt_word_level_segments(segments: List[dict], tag: Tuple[str, str] = None) -> List[dict]:
    """Segment and word level together, as one cue per segment with inline word timestamps (``tag`` is unused)."""
    return [_cue(_vtt_inline_text(seg["words"]), seg["start"], seg["end"]) for seg in segments]


def _ass_karaoke_text(words: List[dict], fill: bool) -> str:
    parts = []
    for w in words:
        lead = " " if w["word"].startswith(" ") else ""
        parts.append(f"{lead}{{\\k{'f' if fill else ''}{sec2centiseconds(w['end'] - w['start'])}}}{w['word'][len(lead):]}")
    return "".join(parts)


def to_ass_word_level_segments(segments: List[dict], tag: Tuple[str, str], karaoke: bool = False) -> List[dict]:
    """Segment and word level together, as one cue per segment with a ``\\k`` (``\\kf`` for ``karaoke``) duration in
    centiseconds before every word (``tag`` is unused)."""
    return [_cue(_ass_karaoke_text(seg["words"], karaoke), seg["start"], seg["end"]) for seg in segments]


# ---------------------------------------------------------------------------------------------------------------------
# renderers: cues -> file content

def segment2srtblock(segment: dict, idx: int, strip: bool = True) -> str:
    return f"{idx}\n{sec2srt(segment['start'])} --> {sec2srt(segment['end'])}\n{finalize_text(segment['text'], strip)}"


def segment2vttblock(segment: dict, strip: bool = True) -> str:
    return f"{sec2vtt(segment['start'])} --> {sec2vtt(segment['end'])}\n{finalize_text(segment['text'], strip)}"


def segment2assblock(segment: dict, idx: int, strip: bool = True) -> str:
    return (f"Dialogue: {idx},{sec2ass(segment['start'])},{sec2ass(segment['end'])},Default,,0,0,0,,"
            f"{finalize_text(segment['text'], strip)}")


def segment2tsvblock(segment: dict, strip: bool = True) -> str:
    text = segment["text"].strip() if strip else segment["text"]
    return f"{sec2milliseconds(segment['start'])}\t{sec2milliseconds(segment['end'])}\t{text}"


def _render_srt(cues: List[dict], strip: bool) -> str:
    return "\n\n".join(segment2srtblock(c, n, strip=strip) for n, c in enumerate(cues, 1))


def _render_vtt(cues: List[dict], strip: bool) -> str:
    return "WEBVTT\n\n" + "\n\n".join(segment2vttblock(c, strip=strip) for c in cues)


def _render_tsv(cues: List[dict], strip: bool) -> str:
    return "\n\n".join(segment2tsvblock(c, strip=strip) for c in cues)


def _render_txt(cues: List[dict]) -> str:
    return "\n".join(c["text"].strip() for c in cues)             # plain text is stripped whatever ``strip`` says


def _ass_style(overrides: dict, primary: Optional[str], font: Optional[str], font_size) -> dict:
    """The style fields of an export: ``overrides`` by field name (unknown names are ignored; colour values gain the
    ``&H`` prefix, in ``overrides`` itself), then ``primary``, ``font`` and ``font_size`` where given."""
    for key, value in overrides.items():
        if "colour" in key.lower() and not str(value).startswith("&H"):
            overrides[key] = f"&H{value}"
    style = dict(_ASS_STYLE)
    style.update((k, v) for k, v in overrides.items() if k in style)
    if primary is not None and "PrimaryColour" not in overrides:
        style["PrimaryColour"] = primary if primary.startswith("&H") else f"&H{primary}"
    if font:
        style["Fontname"] = font
    if font_size:
        style["Fontsize"] = font_size
    return style


def _render_ass(cues: List[dict], strip: bool, style: dict) -> str:
    head = (f"{_ASS_SCRIPT_INFO}[V4+ Styles]\nFormat: {', '.join(map(str, style))}\n"
            f"Style: {','.join(map(str, style.values()))}\n\n{_ASS_EVENTS}")
    return head + "\n".join(segment2assblock(c, n, strip=strip) for n, c in enumerate(cues))


def _write(path: str, content: str):
    with open(path, "w", encoding="utf-8") as out:
        out.write(content)
    print("Saved:", os.path.abspath(path))


def _target(filepath: Optional[str], filetype: Optional[str]) -> Tuple[Optional[str], str]:
    """The path to write (``.<filetype>`` appended where it does not end so) and the file type, which comes from the
    path's extension when not given, else is 'srt'."""
    if filetype is None:
        filetype = os.path.splitext(filepath)[1][1:] or "srt"
    if filetype.lower() not in SUPPORTED_FORMATS:
        raise NotImplementedError(f"{filetype} not supported")
    suffix = "." + filetype
    if filepath and not filepath.lower().endswith(suffix):
        filepath += suffix
    return filepath, filetype


# ---------------------------------------------------------------------------------------------------------------------
# public entry points

def result_to_any(result: Union[dict, list], filepath: str = None, filetype: str = None,
                  segments2blocks: Callable = None, segment_level=True, word_level=True, min_dur: float = 0.02,
                  tag: Tuple[str, str] = None, default_tag: Tuple[str, str] = None, strip=True,
                  reverse_text: Union[bool, tuple] = False, to_word_level_string_callback: Callable = None):
    """
    Generate a file from ``result`` with segment-level and/or word-level timestamps.

    ``segments2blocks(cues) -> str`` renders the content (SRT when None).  With both levels on,
    ``to_word_level_string_callback(segments, tag) -> cues`` builds the cues (:func:`to_word_level_segments` when
    None) and ``tag`` falls back to ``default_tag``, then to the format's own.

    Returns the content as ``str`` if ``filepath`` is None.
    """
    assert segment_level or word_level, "`segment_level` or `word_level` must be True"
    cues = _segments_of(result, min_dur, reverse_text)
    if word_level:
        word_level = _all_have_words(cues)

    filepath, filetype = _target(filepath, filetype)

    if word_level and segment_level:
        if tag is None:
            tag = default_tag
        if tag is None:
            tag = _SRT_TAG if filetype == "srt" else _UNDERLINE_TAG
        cues = (to_word_level_string_callback or to_word_level_segments)(cues, tag)
    elif word_level:
        cues = to_word_level(cues)

    if not _in_order(cues):
        warnings.warn(message="Result contains out of order timestamp(s). Output file may not playback properly.")

    content = _render_srt(cues, strip) if segments2blocks is None else segments2blocks(cues)
    if not filepath:
        return content
    _write(filepath, content)


def result_to_srt_vtt(result: Union[dict, list], filepath: str = None, segment_level=True, word_level=True,
                      min_dur: float = 0.02, tag: Tuple[str, str] = None, vtt: bool = None, strip=True,
                      reverse_text: Union[bool, tuple] = False):
    """
    Generate SRT/VTT from ``result`` with segment-level and/or word-level timestamps.

    Parameters
    ----------
    result : dict or list or WhisperResult
    filepath : str, default None, meaning the content is returned as a ``str``
    segment_level, word_level : bool, default True
        With both, each word is shown in its whole segment and marked by ``tag`` while it is spoken.
    min_dur : float, default 0.02
        Words/segments shorter than this are merged with a neighbour first (result objects only).
    tag : tuple of (str, str), default None, meaning ``('<font color="#00ff00">', '</font>')`` for SRT and, for VTT,
        inline word timestamps instead of a tag.
    vtt : bool, default None, meaning by the extension of ``filepath``, else SRT
    strip : bool, default True
        Whether to strip each cue's text.
    reverse_text : bool or tuple, default False
        Deprecated: ``(prepend_punctuations, append_punctuations)`` to write each segment's words in reverse order.

    Examples
    --------
    >>> result = model.transcribe('audio.mp3')
    >>> result.to_srt_vtt('audio.srt')
    Saved: audio.srt
    """
    if vtt is None:
        vtt = filepath is not None and filepath.lower().endswith(".vtt")
    if not vtt:
        return result_to_any(result, filepath, "srt", None, segment_level, word_level, min_dur, tag, None, strip,
                             reverse_text, None)
    return result_to_any(result, filepath, "vtt", lambda cues: _render_vtt(cues, strip), segment_level, word_level,
                         min_dur, tag, None, strip, reverse_text, to_vtt_word_level_segments if tag is None else None)


def result_to_tsv(result: Union[dict, list], filepath: str = None, segment_level: bool = None, word_level: bool = None,
                  min_dur: float = 0.02, strip=True, reverse_text: Union[bool, tuple] = False):
    """
    Generate TSV (``start_ms<TAB>end_ms<TAB>text``) from ``result``, at segment level (the default) or word level.

    Same parameters as :func:`result_to_srt_vtt`, without ``tag`` / ``vtt``; exactly one level is to be chosen.

    Examples
    --------
    >>> result.to_tsv('audio.tsv')
    Saved: audio.tsv
    """
    if segment_level is None and word_level is None:
        segment_level = True
    assert word_level is not segment_level, ("[word_level] and [segment_level] cannot be the same "
                                             "since [tag] is not support for this format")
    return result_to_any(result, filepath, "tsv", lambda cues: _render_tsv(cues, strip), segment_level, word_level,
                         min_dur, strip=strip, reverse_text=reverse_text)


def result_to_ass(result: Union[dict, list], filepath: str = None, segment_level=True, word_level=True,
                  min_dur: float = 0.02, tag: Union[Tuple[str, str], int] = None, font: str = None,
                  font_size: int = 24, strip=True, highlight_color: str = None, karaoke=False,
                  reverse_text: Union[bool, tuple] = False, **kwargs):
    """
    Generate Advanced SubStation Alpha (ASS) from ``result`` with segment-level and/or word-level timestamps.

    Same parameters as :func:`result_to_srt_vtt`, and:

    tag : tuple of (str, str) or int, default None, meaning ``\\k`` word timing in the segment's line; -1 for one line
        per word with that word in ``highlight_color``.
    font : str, default 'Arial'
    font_size : int, default 24
    highlight_color : str, default '00ff00'
        '<bb><gg><rr>' of the default highlight.
    karaoke : bool, default False
        Progressive fill (``\\kf``); ``tag`` is ignored with it.
    kwargs :
        Style fields: Name, Fontname, Fontsize, PrimaryColour, SecondaryColour, OutlineColour, BackColour, Bold,
        Italic, Underline, StrikeOut, ScaleX, ScaleY, Spacing, Angle, BorderStyle, Outline, Shadow, Alignment,
        MarginL, MarginR, MarginV, Encoding.

    Examples
    --------
    >>> result.to_ass('audio.ass')
    Saved: audio.ass
    """
    tag = -1 if tag == ["-1"] else tag                  # as a command line hands it over
    highlight_color = "00ff00" if highlight_color is None else highlight_color
    if tag is not None and karaoke:
        warnings.warn("``tag`` is not support for ``karaoke=True``; ``tag`` will be ignored.")

    def render(cues):
        return _render_ass(cues, strip, _ass_style(kwargs, highlight_color if tag is None else None, font, font_size))

    timed_text = None
    if karaoke or (word_level and segment_level and tag is None):
        def timed_text(segments, _tag):
            return to_ass_word_level_segments(segments, _tag, karaoke=karaoke)

    return result_to_any(result, filepath, "ass", render, segment_level, word_level, min_dur,
                         None if tag == -1 else tag, (f"{{\\1c{highlight_color}&}}", "{\\r}"), strip, reverse_text,
                         timed_text)


def result_to_txt(result: Union[dict, list], filepath: str = None, min_dur: float = 0.02, strip=True,
                  reverse_text: Union[bool, tuple] = False):
    """
    Generate plain text without timestamps from ``result``: one stripped line per segment.

    Examples
    --------
    >>> result.to_txt('audio.txt')
    Saved: audio.txt
    """
    return result_to_any(result, filepath, "txt", _render_txt, True, False, min_dur, strip=strip,
                         reverse_text=reverse_text)


def save_as_json(result: dict, path: str, ensure_ascii: bool = False, **kwargs):
    """
    Save ``result`` (a dict, or an object with ``to_dict()``) as JSON to ``path``; ``.json`` is appended when missing
    and ``kwargs`` go to :func:`json.dumps`.

    This is the stable-ts function: the whole ``to_dict()`` including ``ori_dict``, and a ``Saved:`` line.  The
    method ``WhisperResult.save_as_json(path)`` of this package is an older, reduced form -- ``path`` as given, no
    ``ori_dict``, nothing printed -- and is kept as it is.

    Examples
    --------
    >>> stable_whisper.save_as_json(result, 'audio.json')
    Saved: audio.json
    """
    if not isinstance(result, dict):
        result = result.to_dict()
    if not path.lower().endswith(".json"):
        path += ".json"
    _write(path, json.dumps(result, allow_nan=True, ensure_ascii=ensure_ascii, **kwargs))


def load_result(json_path: str) -> dict:
    """The ``dict`` stored in ``json_path``."""
    with open(json_path, "r", encoding="utf-8") as f:
        return json.load(f)
