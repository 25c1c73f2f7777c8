"""Time the word-timestamp stage's head-selection variants inside a batched transcription: the per-window loop
(``timing.HEADSEL_BATCH = False``: the parent commit's code path -- one batch-1 scoring pass, one head selection and one DTW per
window and refinement round) against the lockstep driver (all windows of the device pass in one call each).

large-v3 fp16 with the bench's weight recipe (stable_ts_amd.BENCH_WEIGHTS); ``--model base`` is the launch-bound end.  Workload:
``model.transcribe(bench.synth_audio(600, 0), batch_size=20, word_timestamps=True, ...)`` with bench.py's decode options (beam 5,
a fixed budget of ``--tokens`` = 112 tokens per window: random weights have no meaningful EOT, so every window brings ~112 text
tokens to the word stage) and ``dynamic_heads=True``, ``dynamic_heads="6,2"`` and ``aligner="new"``.  One process; one warm-up
of every (option set, switch) pair, then the switch alternates ``--repeats`` times per option set and the median is reported with the range and all samples, together with the
``score_q`` passes and the windows in them the engine counted.  Both paths must return equal results (asserted).
``--phase-times`` adds one more run of each pair with the stage timer of ``bench.py --phase-times`` on (it synchronises at every
stage boundary, so it is kept out of the timed runs) and reports the seconds of the word-timestamp stage alone.  The report of
this model is stored under its name in the JSON object at ``--out`` (other models' entries there are kept) and printed.

    python scripts/bench_headsel_batch.py --phase-times --out profiles/headsel_batch_bench.json      (needs a GPU)
"""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTION_SETS = {"dynamic_heads=True": dict(dynamic_heads=True), 'dynamic_heads="6,2"': dict(dynamic_heads="6,2"),
               'aligner="new"': dict(aligner="new")}
WORD_STAGE = "word timestamps (scoring pass + a7 + DTW + host word assembly)"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="large-v3")
    ap.add_argument("--dtype", default="f16")
    ap.add_argument("--seconds", type=float, default=600.0)
    ap.add_argument("--batch-size", type=int, default=20)
    ap.add_argument("--beam", type=int, default=5)
    ap.add_argument("--tokens", type=int, default=112, help="fixed decode budget per window (bench.py's)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--phase-times", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import bench
    import stable_ts_amd as sw
    import stable_ts_amd.timing as timing
    import stable_ts_amd.transcribe as T

    dims = sw.dims_for(args.model)
    heads = bench.LARGE_V3_HEADS if dims.n_text_layer == 32 and dims.n_text_head == 20 else None
    model = sw.Whisper(dims, device="cuda:0", dtype=args.dtype, alignment_heads=heads, max_windows=args.batch_size,
                       max_rows=args.batch_size)
    model.load_state_dict(sw.random_state_dict(dims, seed=1234, std=0.02, **sw.BENCH_WEIGHTS))
    audio = bench.synth_audio(args.seconds, 0)
    eng = model.engine
    warnings.simplefilter("ignore")
    kw = dict(language="en", temperature=0.0, logprob_threshold=None, compression_ratio_threshold=None, no_speech_threshold=None,
              beam_size=args.beam if args.beam > 1 else None, sample_len=args.tokens, min_tokens=args.tokens, word_timestamps=True,
              batch_size=args.batch_size, max_instant_words=1.0)  # bench.py's flagship options (no segment is dropped)

    def run(opts, batch):
        timing.HEADSEL_BATCH = batch
        torch.cuda.synchronize()
        c0, w0 = eng.score_q_calls, eng.score_q_windows
        t0 = time.perf_counter()
        res = model.transcribe(audio, **kw, **opts)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, res, eng.score_q_calls - c0, eng.score_q_windows - w0

    rep = dict(model=args.model, dtype=args.dtype, audio_seconds=args.seconds, batch_size=args.batch_size, beam=args.beam,
               tokens_per_window=args.tokens, repeats=args.repeats, budget_bytes=timing.HEADSEL_BATCH_BYTES, results_equal=True, option_sets={})
    switches = [("per_window_loop", False), ("lockstep", True)]
    for label, opts in OPTION_SETS.items():
        times = {name: [] for name, _ in switches}
        counts, snaps, words = {}, {}, 0
        for r in range(args.repeats + 1):                        # round 0 = warm-up (workspace growth, first launches)
            for name, batch in switches:
                dt, res, calls, windows = run(opts, batch)
                if r:
                    times[name].append(dt)
                counts[name] = (calls, windows)
                snaps[name] = res.to_dict()
                words = len(res.all_words())
                print(f"[bench_headsel_batch] {label} round {r} {name}: {dt:.3f} s", file=sys.stderr, flush=True)
        assert snaps["per_window_loop"] == snaps["lockstep"], f"{label}: the per-window loop and the lockstep driver differ"
        entry = dict(words=words, variants={})
        for name, _ in switches:
            med = statistics.median(times[name])
            entry["variants"][name] = dict(seconds_median=round(med, 4), seconds_min=round(min(times[name]), 4),
                                           seconds_max=round(max(times[name]), 4), seconds_all=[round(t, 4) for t in times[name]],
                                           x_realtime=round(args.seconds / med, 1), score_q_calls=counts[name][0],
                                           score_q_windows=counts[name][1])
        entry["speedup_whole_transcription"] = round(entry["variants"]["per_window_loop"]["seconds_median"] /
                                                     entry["variants"]["lockstep"]["seconds_median"], 2)
        if args.phase_times:
            stage, entry["phase_seconds"] = {}, {}
            for name, batch in switches:
                T.PHASE_TIMES = {}
                run(opts, batch)
                ph, T.PHASE_TIMES = T.PHASE_TIMES, None
                stage[name] = round(ph.get(WORD_STAGE, 0.0), 4)
                entry["phase_seconds"][name] = {k: round(v, 4) for k, v in ph.items()}
            entry["word_stage_seconds"] = stage
            entry["speedup_word_stage"] = round(stage["per_window_loop"] / stage["lockstep"], 2) if stage["lockstep"] > 0 else None
        rep["option_sets"][label] = entry
    timing.HEADSEL_BATCH = True
    report = {}
    if args.out and os.path.exists(args.out):
        with open(args.out) as f:
            report = json.load(f)
    report[args.model] = rep
    text = json.dumps(report, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({args.model: rep}, indent=1))


if __name__ == "__main__":
    main()
