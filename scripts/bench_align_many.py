"""Time forced alignment of a folder of short clips, each with its own transcript: ``[model.align(a, t) for a, t in ...]`` (the
parent commit's code path, one window per device pass) against ``model.align_many(clips, texts)`` (the clips' current windows
in one device pass, slots refilled).

large-v3 fp16 with the bench's weight recipe (stable_ts_amd.BENCH_WEIGHTS); ``--model base`` is the launch-bound end.  The same
``--clips`` clips as scripts/bench_many.py: cut from ``bench.synth_audio`` at lengths drawn from a fixed seed between 3 and 45 s,
device-resident, each trimmed by up to 10 ms to a whole number of 20-ms frames (a clip of an odd number of hundredths can leave
``align`` -- this package's and the reference's alike -- a last window of half a frame, which neither survives).  Texts are random token ids at bench.py's ``--align-tokens-per-min`` rate (150) per clip.  One process; one
warm-up of both variants, then they alternate ``--repeats`` times and the median per variant is reported with all samples, with
the encoder passes and windows the engine counted.  Both paths must return equal results (asserted).  ``--phase-times`` adds one
more run of each variant with the stage timer of ``bench.py --phase-times`` on (it synchronises at every stage boundary, so it is
kept out of the timed runs) and reports seconds per stage; "silence analysis + host state machines" is what is left of that run
outside the device job.  Writes one JSON object (``--out``) and prints it.

    python scripts/bench_align_many.py --out profiles/align_many_bench.json      (needs a GPU)
"""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def snap(res):
    return None if res is None else res.to_dict()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="large-v3")
    ap.add_argument("--dtype", default="f16")
    ap.add_argument("--clips", type=int, default=40)
    ap.add_argument("--max-tracks", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--tokens-per-min", type=int, default=150)
    ap.add_argument("--phase-times", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import bench
    import stable_ts_amd as sw
    import stable_ts_amd.transcribe as T

    dims = sw.dims_for(args.model)
    heads = bench.LARGE_V3_HEADS if dims.n_text_layer == 32 and dims.n_text_head == 20 else None
    model = sw.Whisper(dims, device="cuda:0", dtype=args.dtype, alignment_heads=heads, max_windows=args.max_tracks,
                       max_rows=args.max_tracks)
    model.load_state_dict(sw.random_state_dict(dims, seed=1234, std=0.02, **sw.BENCH_WEIGHTS))
    rng = np.random.RandomState(args.seed)
    lengths = [float(x) for x in np.round(rng.uniform(3.0, 45.0, size=args.clips), 2)]
    source = bench.synth_audio(sum(lengths) + 1.0, seed=args.seed)
    g = torch.Generator().manual_seed(args.seed)
    clips, texts, at = [], [], 0
    for s in lengths:
        n = int(s * 16000) // 320 * 320
        clips.append(source[at: at + n].clone().cuda())
        texts.append(torch.randint(18, 50000, (max(int(args.tokens_per_min * s / 60.0), 1),), generator=g).tolist())
        at += n
    kw = dict(language="en", token_step=100)                     # bench.py's align options

    def loop():
        return [model.align(a, list(t), **kw) for a, t in zip(clips, texts)]

    def many():
        return model.align_many(clips, [list(t) for t in texts], max_tracks=args.max_tracks, **kw)

    variants = [("loop", loop), ("many", many)]
    times = {name: [] for name, _ in variants}
    encodes, snaps, n_words = {}, {}, 0
    warnings.simplefilter("ignore")
    for rep in range(args.repeats + 1):                          # round 0 = warm-up (workspace growth, first launches)
        for name, fn in variants:
            torch.cuda.synchronize()
            c0, w0 = model.engine.encode_calls, model.engine.encode_windows
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if rep:
                times[name].append(dt)
            encodes[name] = (model.engine.encode_calls - c0, model.engine.encode_windows - w0)
            snaps[name] = [snap(r) for r in out]
            n_words = sum(len(r.all_words()) for r in out if r is not None)
            print(f"[bench_align_many] round {rep} {name}: {dt:.3f} s", file=sys.stderr, flush=True)
    assert snaps["loop"] == snaps["many"], "the loop of align() and align_many() differ"
    audio_s = sum(int(c.shape[-1]) for c in clips) / 16000.0
    rep = dict(model=args.model, dtype=args.dtype, clips=args.clips, clip_seconds_total=round(audio_s, 2),
               clip_seconds_min=min(lengths), clip_seconds_max=max(lengths), text_tokens_total=sum(len(t) for t in texts),
               tokens_per_min=args.tokens_per_min, max_tracks=args.max_tracks, repeats=args.repeats, results_equal=True,
               words=n_words, variants={})
    for name, _ in variants:
        med = statistics.median(times[name])
        rep["variants"][name] = dict(seconds_median=round(med, 4), seconds_all=[round(t, 4) for t in times[name]],
                                     x_realtime=round(audio_s / med, 1), encoder_passes=encodes[name][0],
                                     encoder_windows=encodes[name][1])
    rep["speedup"] = round(rep["variants"]["loop"]["seconds_median"] / rep["variants"]["many"]["seconds_median"], 2)
    if args.phase_times:
        rep["phase_seconds"] = {}
        for name, fn in variants:
            T.PHASE_TIMES = {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            ph, T.PHASE_TIMES = T.PHASE_TIMES, None
            inside = sum(v for k, v in ph.items() if k.startswith("align:"))
            ph["silence analysis + host state machines (outside the device job)"] = dt - inside
            ph["total (synchronised at every stage)"] = dt
            rep["phase_seconds"][name] = {k: round(v, 4) for k, v in ph.items()}
    text = json.dumps(rep, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
