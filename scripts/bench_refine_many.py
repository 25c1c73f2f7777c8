"""Time ``refine`` over a folder of short clips, four ways:

1. ``loop``            ``[model.refine(a, r) for a, r in zip(clips, results)]``
2. ``loop_bs16``       the same loop with ``batch_size=16`` -- the best the code before ``refine_many`` offers: the word groups of ONE
                       clip in lockstep, and a clip of 3-45 s is one or two groups
3. ``many_host``       ``model.refine_many(clips, results, device_probes=False)``: the groups of all clips in lockstep, the probe audio
                       rebuilt on the host and uploaded every round
4. ``many``            ``model.refine_many(clips, results, device_probes=True)``: the probe audio stays on the device, a round uploads its edits

large-v3 fp16 with the bench's weight recipe (stable_ts_amd.BENCH_WEIGHTS), the 40 clips of scripts/bench_many.py, starting results
from ``transcribe_many`` with bench.py's decode options, ``prob_threshold=0`` as in scripts/bench_refine.py (random weights give word
probabilities far below 0.5, which would end every search after its first probe).  One process; one warm-up of every variant, then the
variants alternate ``--repeats`` times; the median per variant is reported with all samples and the device passes (encoder calls).
Variants 3 and 4 send the same PCM bits through the same batches, so their results must be EQUAL (asserted); against the loops the
words that are equal and the largest deviation are reported (in fp16 the encoder's rounding follows the batch a window is computed
in: tests/test_gpu_refine_many.py holds the f32 equality and the fp16 bar).  Writes one JSON object (``--out``) and prints it.

    python scripts/bench_refine_many.py --out profiles/refine_many_bench.json      (needs a GPU)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="large-v3")
    ap.add_argument("--dtype", default="f16")
    ap.add_argument("--clips", type=int, default=40)
    ap.add_argument("--max-tracks", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import bench
    import stable_ts_amd as sw
    from stable_ts_amd.result import WhisperResult

    dims = sw.dims_for(args.model)
    heads = bench.LARGE_V3_HEADS if dims.n_text_layer == 32 and dims.n_text_head == 20 else None
    model = sw.Whisper(dims, device="cuda:0", dtype=args.dtype, alignment_heads=heads, max_windows=20, max_rows=100)
    model.load_state_dict(sw.random_state_dict(dims, seed=1234, std=0.02, **sw.BENCH_WEIGHTS))
    rng = np.random.RandomState(args.seed)                        # the clips of scripts/bench_many.py
    lengths = [float(x) for x in np.round(rng.uniform(3.0, 45.0, size=args.clips), 2)]
    source = bench.synth_audio(sum(lengths) + 1.0, seed=args.seed)
    clips, at = [], 0
    for s in lengths:
        n = int(s * 16000)
        clips.append(source[at: at + n].clone())
        at += n
    start = model.transcribe_many([c.cuda() for c in clips], language="en", max_tracks=20, temperature=0.0, logprob_threshold=None,
                                  compression_ratio_threshold=None, no_speech_threshold=None, beam_size=5, sample_len=112,
                                  min_tokens=112, word_timestamps=True, max_instant_words=1.0)       # bench.py's decode options
    keep = [i for i, r in enumerate(start) if r.all_words()]
    clips, rds = [clips[i] for i in keep], [start[i].to_dict() for i in keep]
    kw = dict(prob_threshold=0.0)

    def fresh():
        return [WhisperResult(rd) for rd in rds]

    variants = {
        "loop": lambda: [model.refine(a, r, **kw) for a, r in zip(clips, fresh())],
        "loop_bs16": lambda: [model.refine(a, r, batch_size=16, **kw) for a, r in zip(clips, fresh())],
        "many_host": lambda: model.refine_many(clips, fresh(), max_tracks=args.max_tracks, device_probes=False, **kw),
        "many": lambda: model.refine_many(clips, fresh(), max_tracks=args.max_tracks, device_probes=True, **kw),
    }
    times = {v: [] for v in variants}
    passes, windows, snaps = {}, {}, {}
    for rep in range(args.repeats + 1):                          # round 0 = warm-up (workspace growth, first launches)
        for v, run in variants.items():
            torch.cuda.synchronize()
            c0, w0 = model.engine.encode_calls, model.engine.encode_windows
            t0 = time.perf_counter()
            out = run()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if rep:
                times[v].append(dt)
            passes[v], windows[v] = model.engine.encode_calls - c0, model.engine.encode_windows - w0
            snaps[v] = [(w.start, w.end) for r in out for w in r.all_words()]
            print(f"[bench_refine_many] round {rep} {v}: {dt:.3f} s, {passes[v]} device passes", file=sys.stderr, flush=True)
    assert snaps["many"] == snaps["many_host"], "device probes and host probes differ"
    before = [(w.start, w.end) for r in fresh() for w in r.all_words()]
    audio_s = sum(c.shape[-1] for c in clips) / 16000
    rep = dict(model=args.model, dtype=args.dtype, clips=len(clips), clip_seconds_total=round(audio_s, 2),
               clip_seconds_min=min(lengths), clip_seconds_max=max(lengths), words=len(before), max_tracks=args.max_tracks,
               repeats=args.repeats, refine_kw=kw, device=torch.cuda.get_device_name(0), many_equals_many_host=True, variants={})
    for v in variants:
        med = statistics.median(times[v])
        dev = [max(abs(a[0] - b[0]), abs(a[1] - b[1])) for a, b in zip(snaps[v], snaps["loop"])]
        rep["variants"][v] = dict(seconds_median=round(med, 4), seconds_all=[round(t, 4) for t in times[v]],
                                  device_passes=passes[v], encoder_windows=windows[v],
                                  words_moved=sum(a != b for a, b in zip(before, snaps[v])),
                                  words_equal_to_loop=sum(a == b for a, b in zip(snaps[v], snaps["loop"])),
                                  max_deviation_from_loop_s=round(max(dev), 3))
    med = {v: rep["variants"][v]["seconds_median"] for v in variants}
    rep["refine_many_vs_loop_bs16"] = round(med["loop_bs16"] / med["many"], 2)
    rep["refine_many_vs_loop"] = round(med["loop"] / med["many"], 2)
    rep["device_probes_vs_host_probes"] = round(med["many_host"] / med["many"], 3)
    # beyond the spread of the repeats = the two variants' samples do not overlap
    rep["device_probes_faster_beyond_spread"] = bool(max(times["many"]) < min(times["many_host"]))
    text = json.dumps(rep, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
