"""Golden fixtures for the result writers: run the REFERENCE's own writers (stable_whisper/text_output.py, bound on its
``WhisperResult``) over seeded synthetic results, the stored JFK result and hand-made edge results with a grid of
options, and store the inputs, the calls and what came back.

Only runs where /root/reference exists (this container); tests/golden/text_output_cases.json.gz is committed and is
what tests/test_text_output_cpu.py compares stable_ts_amd against on machines without the reference.

    python tests/golden/make_text_output_golden.py

A case is ``dict(input=<name>, form='obj'|'dict'|'list', fn=<writer>, kwargs=<repr of the keyword arguments>,
file=<file name or None>, calls=[...])``.  ``run_case`` below makes the calls -- it is shared with the test, so both
sides go through the same protocol -- and returns one record per call: the returned string, the files that appeared
(name and text), what was printed, every warning as [category, text], and the exception type where the call raised.
A dict or list input is written twice from the same object, and where a call changed that object (the VTT inline path
edits its word strings) the record holds the words it left.
"""
import ast
import contextlib
import copy
import io
import json
import os
import random
import sys
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_regroup_golden import synth_result  # noqa: E402

# seeds whose results stay small (the both-levels formats grow with the square of a segment's word count)
SYNTH_SEEDS = [7, 9, 22, 23, 26, 27, 30, 32, 35, 42, 46, 51]
FORMS = ("obj", "dict", "list")
NOT_A_RESULT = ("unordered", "twins")                   # out of order: WhisperResult() refuses them, dict / list only


def _w(word, start, end, **kw):
    return dict(word=word, start=start, end=end, probability=kw.get("p", 0.5), tokens=kw.get("tokens", [7]))


def _seg(words=None, **kw):
    d = dict(seek=0.0, tokens=[7], temperature=0.0, avg_logprob=-0.3, compression_ratio=1.2, no_speech_prob=0.05)
    if words:
        d.update(start=words[0]["start"], end=words[-1]["end"], text="".join(w["word"] for w in words), words=words)
    elif words is not None:
        d["words"] = words
    d.update(kw)
    return d


def edge_inputs() -> dict:
    e = {}
    e["cjk"] = dict(language="zh", segments=[
        _seg([_w("今天", 0.5, 0.9), _w("天气", 0.9, 1.3), _w("很好。", 1.5, 2.1)]),
        _seg([_w("我们", 2.4, 2.8), _w("，", 2.8, 2.8), _w("走吧", 2.8, 3.35), _w("！", 3.35, 3.5)])])
    e["blanks"] = dict(language="en", segments=[
        _seg([_w(" so", 0.0, 0.4), _w("", 0.4, 0.6), _w(" ", 0.6, 0.8), _w(" it", 0.9, 1.2), _w(" goes.", 1.2, 1.9)]),
        _seg([_w(" ", 2.0, 2.3), _w("End", 2.3, 2.9)])])
    e["touch"] = dict(language="en", segments=[
        _seg([_w(" one", 1.0, 1.5), _w(" two", 1.5, 2.0), _w(" three", 2.25, 2.75), _w("-four", 2.75, 3.0),
              _w("five ", 3.1, 3.4), _w(" six", 3.6, 4.0), _w("seven", 4.3, 4.4)]),
        _seg([_w(" a", 4.4004, 4.9), _w(" b", 4.9004, 5.2), _w(" c", 5.2006, 5.4)])])
    e["short"] = dict(language="en", segments=[
        _seg([_w(" I", 0.0, 0.0), _w(" was", 0.0, 0.3), _w(" er", 0.3, 0.31), _w(" there", 0.31, 0.9),
              _w(".", 0.9, 0.9)]),
        _seg([_w(" Hm", 1.2, 1.21)]),
        _seg([_w(" Well", 1.5, 2.0), _w(" then", 2.0, 2.015), _w(" ok", 2.015, 2.5)]),
        _seg([_w(" x", 3.0, 3.0), _w(" y", 3.0, 3.0)])])
    e["mixed"] = dict(language="en", segments=[
        _seg([_w(" With", 0.0, 0.5), _w(" words.", 0.6, 1.0)]),
        _seg(start=1.2, end=2.4, text=" Without any words."),
        _seg([_w(" Again", 2.5, 3.0), _w(" with.", 3.0, 3.6)])])
    e["nowords"] = dict(language="en", text=" First line. Second, line?", segments=[
        _seg(start=0.0, end=1.5, text=" First line."),
        _seg(start=1.5, end=1.51, text=" (tiny)"),
        _seg(start=2.0, end=3.25, text=' Second, "line"?')])
    e["emptywords"] = dict(language="en", segments=[
        _seg(start=0.0, end=1.5, text=" Has an empty list.", words=[]),
        _seg([_w(" Next", 2.0, 2.5)])])
    e["times"] = dict(language="en", segments=[
        _seg([_w(" zero", 0, 59.9996), _w(" minute", 59.9996, 61)]),
        _seg([_w(" hour", 3599.9996, 3600.004), _w(" more", 3600.005, 3661.555)]),
        _seg([_w(" century", 360000.5, 360001.25), _w(" plus", 360001.25, 360059.996)])])
    e["times_seg"] = dict(language="en", segments=[
        _seg(start=0, end=59.9996, text=" zero"), _seg(start=59.9996, end=3599.9996, text=" minute"),
        _seg(start=3599.9996, end=360000.5, text=" hour"), _seg(start=360000.5, end=360059.995, text=" century")])
    e["unordered"] = dict(language="en", segments=[
        _seg([_w(" late", 2.0, 2.5), _w(" early", 1.0, 1.5)]),
        _seg([_w(" after", 3.0, 3.5)])])
    e["multiline"] = dict(language="en", segments=[
        _seg([_w(" Line", 0.0, 0.4), _w(" one\n", 0.4, 0.9), _w(" line", 1.0, 1.4), _w(" two \n", 1.4, 2.0),
              _w(" three ", 2.0, 2.6)]),
        _seg(start=3.0, end=4.0, text="  padded\n text \n  here  ")])
    e["twins"] = dict(language="en", segments=[                       # words equal by value, bare word dicts
        _seg(words=[dict(word=" la", start=0.0, end=0.5), dict(word=" di", start=0.75, end=1.0),
                    dict(word=" la", start=0.0, end=0.5), dict(word=" la", start=1.25, end=1.5),
                    dict(word=" la", start=0.0, end=0.5)])])
    e["punct"] = dict(language="en", segments=[
        _seg([_w(' "Quoted', 0.0, 0.5), _w(' words,"', 0.5, 1.1), _w(" (and", 1.3, 1.6), _w(" brackets).", 1.6, 2.4),
              _w(' "', 2.4, 2.5), _w(" -dash", 2.6, 3.0), _w("...", 3.0, 3.2)]),
        _seg(start=3.5, end=4.5, text=' "No words," he (said).')])
    e["empty"] = dict(language="en", segments=[])
    return e


def jfk_input():
    with open(os.path.join(HERE, "reference_jfk.json"), "r", encoding="utf-8") as f:
        d = json.load(f)
    if not isinstance(d.get("segments"), list):
        return None
    return dict(language="en", text=d.get("text", ""), segments=d["segments"])


def all_inputs() -> dict:
    inputs = {f"synth{seed}": synth_result(seed) for seed in SYNTH_SEEDS}
    jfk = jfk_input()
    if jfk is not None:
        inputs["jfk"] = jfk
    inputs.update(edge_inputs())
    return inputs


# callables for result_to_any's hooks, named in the stored keyword arguments as '@name'
def _plain_blocks(cues):
    return " | ".join(f"{c['start']}>{c['end']}:{c['text']}" for c in cues)


def _upper_words(segments, tag):
    return [dict(text=tag[0] + s["text"].upper() + tag[1], start=s["start"], end=s["end"]) for s in segments]


HOOKS = {"@plain": _plain_blocks, "@upper": _upper_words}

B = ("<b>", "</b>")
GRID = [
    # -- SRT / VTT
    ("srt_vtt", {}, None),
    ("srt_vtt", dict(vtt=True), None),
    ("srt_vtt", dict(vtt=True, tag=B), None),
    ("srt_vtt", dict(tag=("<i>", "</i>")), None),
    ("srt_vtt", dict(segment_level=False), None),
    ("srt_vtt", dict(word_level=False), None),
    ("srt_vtt", dict(word_level=False, vtt=True, strip=False), None),
    ("srt_vtt", dict(strip=False), None),
    ("srt_vtt", dict(vtt=True, strip=False), None),
    ("srt_vtt", dict(min_dur=0.3), None),
    ("srt_vtt", dict(min_dur=0), None),
    ("srt_vtt", dict(segment_level=False, vtt=True, min_dur=0.12), None),
    ("srt_vtt", dict(reverse_text=(None, None)), None),
    ("srt_vtt", dict(reverse_text=(None, None), vtt=True, tag=B), None),
    ("srt_vtt", dict(reverse_text=True), None),
    ("srt_vtt", dict(reverse_text=('"(', ".,)"), word_level=False), None),
    ("srt_vtt", dict(reverse_text=("", "")), None),
    ("srt_vtt", dict(reverse_text=("", ".?"), segment_level=False), None),
    ("srt_vtt", dict(reverse_text=(None, None, None)), None),
    ("srt_vtt", dict(segment_level=False, word_level=False), None),
    ("srt_vtt", {}, "out.srt"),
    ("srt_vtt", {}, "out.vtt"),
    ("srt_vtt", {}, "out"),
    ("srt_vtt", dict(word_level=False), "OUT.VTT"),
    ("srt_vtt", dict(vtt=False), "out.vtt"),
    ("srt_vtt", dict(vtt=True, segment_level=False), "clip.srt"),
    ("srt_vtt", dict(word_level=False), "notes.txt"),
    # -- ASS
    ("ass", {}, None),
    ("ass", dict(tag=-1), None),
    ("ass", dict(tag=-1, highlight_color="0000ff"), None),
    ("ass", dict(tag=["-1"], highlight_color="&Hff0000"), None),
    ("ass", dict(tag=("{\\b1}", "{\\b0}")), None),
    ("ass", dict(karaoke=True), None),
    ("ass", dict(karaoke=True, tag=-1), None),
    ("ass", dict(karaoke=True, tag=B, word_level=False), None),
    ("ass", dict(karaoke=True, segment_level=False), None),
    ("ass", dict(segment_level=False), None),
    ("ass", dict(word_level=False), None),
    ("ass", dict(word_level=False, tag=-1, strip=False), None),
    ("ass", dict(font="Noto Sans", font_size=30), None),
    ("ass", dict(font_size=0, highlight_color="&H00ffff"), None),
    ("ass", dict(PrimaryColour="00ffff", OutlineColour="&H101010", BackColour=80, Bold=1, Bogus=3, MarginV=25,
                 bogusColour="12"), None),
    ("ass", dict(tag=-1, PrimaryColour="&H123456", Fontsize=12, Name="Top", Alignment=8), None),
    ("ass", dict(strip=False, min_dur=0.3), None),
    ("ass", dict(reverse_text=(None, None), tag=-1), None),
    ("ass", dict(segment_level=False, word_level=False), None),
    ("ass", {}, "out.ass"),
    ("ass", dict(tag=-1), "out"),
    ("ass", dict(word_level=False), "Subs.ASS"),
    # -- TSV
    ("tsv", {}, None),
    ("tsv", dict(word_level=True), None),
    ("tsv", dict(word_level=True, strip=False), None),
    ("tsv", dict(segment_level=True, strip=False, min_dur=0.3), None),
    ("tsv", dict(segment_level=True, word_level=False), None),
    ("tsv", dict(segment_level=False, word_level=True, min_dur=0), None),
    ("tsv", dict(segment_level=True, word_level=True), None),
    ("tsv", dict(segment_level=False, word_level=False), None),
    ("tsv", dict(segment_level=False), None),
    ("tsv", dict(segment_level=1, word_level=True), None),
    ("tsv", dict(word_level=True, reverse_text=(None, None)), None),
    ("tsv", {}, "out.tsv"),
    ("tsv", dict(word_level=True), "out"),
    # -- TXT
    ("txt", {}, None),
    ("txt", dict(strip=False), None),
    ("txt", dict(min_dur=0.3), None),
    ("txt", dict(reverse_text=(None, None)), None),
    ("txt", dict(reverse_text=True), None),
    ("txt", {}, "out.txt"),
    ("txt", {}, "out.text"),
    # -- the generic entry
    ("any", dict(filetype="vtt"), None),
    ("any", dict(filetype="SRT"), None),
    ("any", dict(filetype="xml"), None),
    ("any", {}, None),
    ("any", {}, "x.tsv"),
    ("any", {}, "x.mp4"),
    ("any", {}, "x"),
    ("any", dict(filetype="ass", default_tag=("[", "]")), None),
    ("any", dict(filetype="srt", default_tag=("[", "]"), tag=B), None),
    ("any", dict(filetype="txt", segments2blocks="@plain"), None),
    ("any", dict(filetype="txt", segments2blocks="@plain", word_level=False), "plain"),
    ("any", dict(filetype="vtt", to_word_level_string_callback="@upper"), None),
    ("any", dict(filetype="tsv", segments2blocks="@plain", segment_level=False, min_dur=0.5), None),
    # -- JSON
    ("json", {}, "r.json"),
    ("json", {}, "r"),
    ("json", dict(ensure_ascii=True, indent=1), "R.JSON"),
]
# what every synthetic result is written with in each form, beside a rotating slice of the grid
COMMON = [0, 1]


def build_cases(inputs: dict) -> list:
    cases = []
    k = 0
    for name in inputs:
        for form in FORMS:
            if form == "obj" and name in NOT_A_RESULT:
                continue
            if name.startswith("synth"):
                k += 1
                picks = COMMON + [(k * 7 + j * 11) % len(GRID) for j in range(7)]
            elif name == "jfk":
                picks = range(0, len(GRID), 1 if form == "obj" else 3)
            else:                                       # hand-made results: the whole grid as a result object,
                k += 1                                  # alternating halves of it as dict and as list
                picks = range(len(GRID)) if form == "obj" else [i for i in range(len(GRID)) if (i + k) % 2 == 0]
            for gi in dict.fromkeys(picks):
                fn, kwargs, file = GRID[gi]
                if fn == "json" and form == "list":
                    continue
                cases.append(dict(input=name, form=form, fn=fn, kwargs=repr(kwargs), file=file))
    return cases


def _snapshot_dir(tmp):
    out = {}
    for n in sorted(os.listdir(tmp)):
        with open(os.path.join(tmp, n), "r", encoding="utf-8", newline="") as f:
            out[n] = f.read()
    return out


def run_case(mod, case: dict, inputs: dict, tmp: str) -> list:
    """Make the calls of ``case`` with the package ``mod`` (the reference's or this one's) in the empty directory
    ``tmp`` and return their records.  The record of an 'obj' call also says whether ``to_dict()`` changed."""
    data = copy.deepcopy(inputs[case["input"]])
    kwargs = ast.literal_eval(case["kwargs"])
    for key, val in kwargs.items():
        if isinstance(val, str) and val in HOOKS:
            kwargs[key] = HOOKS[val]
    fn, form = case["fn"], case["form"]
    path = None if case["file"] is None else os.path.join(tmp, case["file"])
    records = []
    with warnings.catch_warnings(record=True), contextlib.redirect_stdout(io.StringIO()):
        warnings.simplefilter("always")
        try:
            target = dict(obj=lambda: mod.WhisperResult(data), dict=lambda: data, list=lambda: data["segments"])[form]()
        except Exception as e:
            return [dict(setup_error=type(e).__name__)]
    before = target.to_dict() if form == "obj" else None
    for _ in range(1 if form == "obj" else 2):
        for n in os.listdir(tmp):
            os.remove(os.path.join(tmp, n))
        rec = dict(ret=None, error=None)
        out = io.StringIO()
        with warnings.catch_warnings(record=True) as caught, contextlib.redirect_stdout(out):
            warnings.simplefilter("always")
            try:
                if fn == "json":
                    mod.save_as_json(target, path, **kwargs)
                elif fn == "any":
                    rec["ret"] = mod.text_output.result_to_any(target, path, **kwargs)
                elif form == "obj":
                    rec["ret"] = getattr(target, f"to_{fn}")(path, **kwargs)
                else:
                    rec["ret"] = getattr(mod, f"result_to_{fn}")(target, path, **kwargs)
            except Exception as e:
                rec["error"] = type(e).__name__
                if isinstance(e, (AssertionError, NotImplementedError)):
                    rec["message"] = str(e)
        rec["warnings"] = [[w.category.__name__, str(w.message)] for w in caught]
        rec["stdout"] = out.getvalue().replace(tmp, "<TMP>")
        rec["files"] = _snapshot_dir(tmp)
        if fn == "json" and rec["error"] is None:
            rec["loaded_equals_saved"] = all(
                mod.load_result(os.path.join(tmp, n)) == json.loads(text) for n, text in rec["files"].items())
        if form == "obj":
            rec["unchanged"] = target.to_dict() == before
        elif data != inputs[case["input"]]:             # a writer edited the caller's dict: keep what it left
            rec["words_after"] = [w["word"] for s in data["segments"] for w in s.get("words") or []]
        records.append(rec)
    return records


def random_case(rng: random.Random, inputs: dict) -> dict:
    """A random option set for the live differential test."""
    fn = rng.choice(["srt_vtt", "srt_vtt", "ass", "ass", "tsv", "txt"])
    kw = {}

    def maybe(key, values, p=0.4):
        if rng.random() < p:
            kw[key] = rng.choice(values)

    if fn != "txt":
        maybe("segment_level", [True, False, None])
        maybe("word_level", [True, False, None])
    maybe("min_dur", [0, 0.02, 0.05, 0.2, 0.5, 1.0])
    maybe("strip", [True, False])
    maybe("reverse_text", [False, (None, None), ("", ".,?!"), ('"\'(', None), True], 0.15)
    if fn == "srt_vtt":
        maybe("vtt", [True, False, None], 0.6)
        maybe("tag", [None, B, ("<c.hi>", "</c>")])
    if fn == "ass":
        maybe("tag", [None, -1, ("{\\i1}", "{\\i0}")], 0.5)
        maybe("karaoke", [True, False], 0.3)
        maybe("highlight_color", ["ff00ff", "&H00ff00", None])
        maybe("font", ["DejaVu Sans", None], 0.2)
        maybe("font_size", [0, 18, 48], 0.2)
        maybe("PrimaryColour", ["ffff00", "&Hffffff"], 0.2)
        maybe("Outline", [0, 2], 0.2)
    ext = dict(srt_vtt=rng.choice(["srt", "vtt"]), ass="ass", tsv="tsv", txt="txt")[fn]
    file = rng.choice([None, None, f"f.{ext}", "f"])
    name = rng.choice(list(inputs))
    form = rng.choice(FORMS[1:] if name in NOT_A_RESULT else FORMS)
    return dict(input=name, form=form, fn=fn, kwargs=repr(kw), file=file)


def main():
    import gzip
    import tempfile
    from make_golden import import_reference
    sw = import_reference()
    inputs = all_inputs()
    cases = build_cases(inputs)
    with tempfile.TemporaryDirectory() as tmp:
        tmp = os.path.realpath(tmp)
        for c in cases:
            c["calls"] = run_case(sw, c, inputs, tmp)
    out = os.path.join(HERE, "text_output_cases.json.gz")
    with gzip.GzipFile(out, "wb", mtime=0) as f:
        f.write(json.dumps(dict(inputs=inputs, cases=cases), ensure_ascii=False, separators=(",", ":")).encode("utf-8"))
    raising = sum(1 for c in cases for r in c["calls"] if r.get("error") or r.get("setup_error"))
    print(f"wrote {len(cases)} cases ({raising} raising calls) -> {out} ({os.path.getsize(out) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
