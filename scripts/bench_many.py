"""Time a folder of short clips: ``for a in clips: model.transcribe(a)`` (the parent commit's code path, one window per device
pass) against ``model.transcribe_many(clips)`` (the clips' current windows in one device batch, slots refilled), with
``language=None`` (detected per clip) and with ``language="en"``.

large-v3 fp16 with the bench's weight recipe (stable_ts_amd.BENCH_WEIGHTS) and bench.py's decode options (beam 5, 112 tokens per
window).  ``--clips`` clips are cut from ``bench.synth_audio`` at lengths drawn from a fixed seed between 3 and 45 s.  One process;
one warm-up of every variant, then the variants alternate ``--repeats`` times and the median per variant is reported with all
samples.  Both paths must return equal results (asserted).  Writes one JSON object (``--out``) and prints it.

    python scripts/bench_many.py --out profiles/transcribe_many_bench.json      (needs a GPU)
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def snap(res):
    return (res.language, res.text, [(d["start"], d["end"]) for d in res.nonspeech_sections],
            [(s.start, s.end, s.text, list(s.tokens),
              None if not s.has_words else [(w.word, w.start, w.end, float(w.probability), list(w.tokens)) for w in s.words])
             for s in res.segments])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="large-v3")
    ap.add_argument("--dtype", default="f16")
    ap.add_argument("--clips", type=int, default=40)
    ap.add_argument("--max-tracks", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import bench
    import stable_ts_amd as sw

    dims = sw.dims_for(args.model)
    heads = bench.LARGE_V3_HEADS if dims.n_text_layer == 32 and dims.n_text_head == 20 else None
    model = sw.Whisper(dims, device="cuda:0", dtype=args.dtype, alignment_heads=heads, max_windows=args.max_tracks,
                       max_rows=args.max_tracks * 5)
    model.load_state_dict(sw.random_state_dict(dims, seed=1234, std=0.02, **sw.BENCH_WEIGHTS))
    rng = np.random.RandomState(args.seed)
    lengths = [float(x) for x in np.round(rng.uniform(3.0, 45.0, size=args.clips), 2)]
    source = bench.synth_audio(sum(lengths) + 1.0, seed=args.seed)
    clips, at = [], 0
    for s in lengths:
        n = int(s * 16000)
        clips.append(source[at: at + n].clone().cuda())
        at += n
    kw = dict(temperature=0.0, logprob_threshold=None, compression_ratio_threshold=None, no_speech_threshold=None, beam_size=5,
              sample_len=112, min_tokens=112, word_timestamps=True, max_instant_words=1.0)       # bench.py's decode options

    def loop(language):
        return [model.transcribe(a, language=language, **kw) for a in clips]

    def many(language):
        return model.transcribe_many(clips, language=language, max_tracks=args.max_tracks, **kw)

    variants = [("loop", None), ("many", None), ("loop", "en"), ("many", "en")]
    times = {v: [] for v in variants}
    encodes, snaps = {}, {}
    for rep in range(args.repeats + 1):                          # round 0 = warm-up (workspace growth, first launches, graphs)
        for v in variants:
            torch.cuda.synchronize()
            c0, w0 = model.engine.encode_calls, model.engine.encode_windows
            t0 = time.perf_counter()
            out = (loop if v[0] == "loop" else many)(v[1])
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if rep:
                times[v].append(dt)
            encodes[v] = (model.engine.encode_calls - c0, model.engine.encode_windows - w0)
            snaps[v] = [snap(r) for r in out]
            print(f"[bench_many] round {rep} {v[0]} language={v[1]}: {dt:.3f} s", file=sys.stderr, flush=True)
    for lang in (None, "en"):
        assert snaps[("loop", lang)] == snaps[("many", lang)], f"loop and transcribe_many differ (language={lang})"
    audio_s = sum(lengths)
    rep = dict(model=args.model, dtype=args.dtype, clips=args.clips, clip_seconds_total=round(audio_s, 2),
               clip_seconds_min=min(lengths), clip_seconds_max=max(lengths), max_tracks=args.max_tracks, repeats=args.repeats,
               decode="beam 5, 112 tokens per window (bench.py's options)", results_equal=True,
               languages_detected=sorted({s[0] for s in snaps[("many", None)] if s[0]}), variants={})
    for v in variants:
        med = statistics.median(times[v])
        rep["variants"][f"{v[0]}/language={v[1]}"] = dict(
            seconds_median=round(med, 4), seconds_all=[round(t, 4) for t in times[v]], x_realtime=round(audio_s / med, 1),
            encoder_passes=encodes[v][0], encoder_windows=encodes[v][1])
    for lang in (None, "en"):
        a = rep["variants"][f"loop/language={lang}"]["seconds_median"]
        b = rep["variants"][f"many/language={lang}"]["seconds_median"]
        rep[f"speedup_language={lang}"] = round(a / b, 2)
    text = json.dumps(rep, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
