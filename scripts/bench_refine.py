"""Time ``refine()``: today's path (``batch_size=None``: group after group, a full-vocabulary distribution per probe handed to the
host logic) against the native probe with N word groups in lockstep (``batch_size`` 1, 4, 8, 16).

large-v3 with the bench's weight recipe (stable_ts_amd.BENCH_WEIGHTS), the words of one ``transcribe()`` pass over
``bench.synth_audio(600, 0)``.  One process; after one warm-up round over all variants the variants are run alternately, ``--repeats``
times, and the median per variant is reported with the spread.  Random weights give word probabilities far below the default
``prob_threshold`` of 0.5, which would end every search after its first probe; the bench passes ``prob_threshold=0`` (as the
end-to-end goldens do) so that the bisection runs.  Writes one JSON object (``--out``) and prints it.

Baseline = the parent commit's ``refine()``: export that commit into a directory, build it, run this script on it with
``--tree DIR --default-only`` next to the main run (same session, same box), and hand its output(s) to the main run's ``--parent-json``.

    python scripts/bench_refine.py --out profiles/refine_lockstep_bench.json      (needs a GPU)
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="large-v3")
    ap.add_argument("--dtype", default="f16")
    ap.add_argument("--seconds", type=float, default=600.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batch-sizes", default="1,4,8,16")
    ap.add_argument("--out", default=None)
    ap.add_argument("--tree", default=ROOT, help="the checkout whose package is timed (a parent commit's, for the baseline line)")
    ap.add_argument("--default-only", action="store_true", help="time refine() without batch_size only (a tree that has none)")
    ap.add_argument("--parent-json", default="", help="comma-separated outputs of --default-only runs on the parent commit's "
                                                      "tree, made in the same session: merged in as the baseline")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import bench
    import stable_ts_amd as sw
    from stable_ts_amd.result import WhisperResult

    dims = sw.dims_for(args.model)
    heads = bench.LARGE_V3_HEADS if dims.n_text_layer == 32 and dims.n_text_head == 20 else None
    model = sw.Whisper(dims, device="cuda:0", dtype=args.dtype, alignment_heads=heads, max_windows=20, max_rows=100)
    model.load_state_dict(sw.random_state_dict(dims, seed=1234, std=0.02, **sw.BENCH_WEIGHTS))
    audio = bench.synth_audio(args.seconds, seed=0)
    t0 = time.perf_counter()
    start = model.transcribe(audio.cuda(), language="en", temperature=0.0, logprob_threshold=None, compression_ratio_threshold=None,
                             no_speech_threshold=None, beam_size=5, sample_len=112, min_tokens=112, word_timestamps=True,
                             batch_size=20, max_instant_words=1.0)       # bench.py's transcribe call
    torch.cuda.synchronize()
    t_transcribe = time.perf_counter() - t0
    rd = start.to_dict()
    kw = dict(prob_threshold=0.0)
    variants = [None] + ([] if args.default_only else [int(b) for b in args.batch_sizes.split(",")])
    times = {v: [] for v in variants}
    probes = {}
    snaps = {}
    for rep in range(args.repeats + 1):                          # round 0 = warm-up (workspace growth, first launches)
        for v in variants:
            res = WhisperResult(rd)
            torch.cuda.synchronize()
            calls0 = model.engine.encode_calls
            t0 = time.perf_counter()
            out = model.refine(audio, res, **({} if v is None else dict(batch_size=v)), **kw)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if rep:
                times[v].append(dt)
            probes[v] = model.engine.encode_calls - calls0
            snaps[v] = [(w.start, w.end) for w in out.all_words()]
            print(f"round {rep} batch_size={v}: {dt:.3f} s, {probes[v]} device passes", file=sys.stderr, flush=True)
    before = [(w.start, w.end) for w in WhisperResult(rd).all_words()]
    base = statistics.median(times[None])
    lines = []
    for v in variants:
        med = statistics.median(times[v])
        lines.append(dict(batch_size=v, median_s=med, min_s=min(times[v]), max_s=max(times[v]), runs=times[v],
                          device_passes=probes[v], speedup_vs_default=base / med,
                          words_moved=sum(a != b for a, b in zip(before, snaps[v])),
                          words_equal_to_default=sum(a == b for a, b in zip(snaps[None], snaps[v]))))
    rep = dict(model=args.model, dtype=args.dtype, audio_seconds=args.seconds, words=len(before), refine_kw=kw,
               transcribe_s=t_transcribe, repeats=args.repeats, lines=lines, device=torch.cuda.get_device_name(0),
               word_times=[list(t) for t in snaps[None]] if args.default_only else None)
    if not args.default_only:
        best = max(lines[1:], key=lambda r: r["speedup_vs_default"])
        rep["headline"] = dict(default_s=base, best_batch_size=best["batch_size"], best_s=best["median_s"],
                               ratio=best["speedup_vs_default"])
        parents = [json.load(open(p)) for p in args.parent_json.split(",") if p]
        if parents:
            runs = [t for p in parents for t in p["lines"][0]["runs"]]
            med = statistics.median(runs)
            rep["parent_commit"] = dict(
                what="refine() of the parent commit's tree on the same input, its own process(es), same session and box",
                median_s=med, min_s=min(runs), max_s=max(runs), runs=runs,
                word_times_equal_to_default=all(p["word_times"] == [list(t) for t in snaps[None]] for p in parents))
            for ln in lines:
                ln["speedup_vs_parent"] = med / ln["median_s"]
        else:
            rep["baseline_note"] = ("no parent-commit line in this run: batch_size null (the group-by-group path of this tree, the "
                                    "same device work as the parent's refine()) stands in for it")
    text = json.dumps(rep, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
