"""Time ``locate`` over a folder of short clips, each searched for its own phrase: ``[model.locate(a, t, ...) for a, t in ...]`` (the
parent commit's code path: every device call at batch 1, a vocabulary-wide logits row copied to the host per greedy step) against
``model.locate_many(clips, texts, device_probe=False)`` (the clips' chunks in lockstep, the host arithmetic per step) and
``model.locate_many(clips, texts, device_probe=True)`` (the step answered by ``swx_forward_next_token``).

large-v3 fp16 with the bench's weight recipe (stable_ts_amd.BENCH_WEIGHTS) and the ``--clips`` clips of scripts/bench_many.py (cut
from ``bench.synth_audio`` at lengths drawn from a fixed seed between 3 and 45 s, device-resident); the phrase of a clip is
``--text-tokens`` random token ids.  ``probability_threshold=0.0``: random weights never reach 0.5, and with 0.0 the greedy loop
runs, forces the phrase in and confirms it.  Modes 0 (greedy steps + word timestamps) and 2 (the end-time pass only).  One
process; one warm-up of every variant, then they alternate ``--repeats`` times; the median per variant is reported with all
samples, next to the device passes the engine made (encoder, scoring, logits, next-token).  The variants must agree the way
tests/test_gpu_locate_many.py asks of f16: the same matches, words and tokens, times within 20 ms (asserted after the report
is written).

    python scripts/bench_locate_many.py --out profiles/locate_many_bench.json      (needs a GPU)
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
COUNTED = ("encode", "score", "forward_logits", "forward_next_token")


def flat(matches):
    out = []
    for x in matches:
        if isinstance(x, dict) and "target_end" in x:
            out.append(("end", [], [x["target_end"]]))
        elif isinstance(x, dict):
            ws = x["duration_window_word"]
            out.append(("window", [(w["word"], tuple(w["tokens"])) for w in ws] + [x["text"], x["duration_window_text"]], [x["end"]]))
        else:
            out.append(("segment", [(w.word, tuple(w.tokens)) for w in x.words], [x.seek] + [t for w in x.words for t in (w.start, w.end)]))
    return out


def agree(a, b, bar=0.02):
    """the same matches, words and tokens; times within ``bar``"""
    if len(a) != len(b):
        return False
    for ra, rb in zip(a, b):
        if [(m[0], m[1]) for m in ra] != [(m[0], m[1]) for m in rb]:
            return False
        if any(abs(s - t) > bar + 1e-9 for ma, mb in zip(ra, rb) for s, t in zip(ma[2], mb[2])):
            return False
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="large-v3")
    ap.add_argument("--dtype", default="f16")
    ap.add_argument("--clips", type=int, default=40)
    ap.add_argument("--max-tracks", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--text-tokens", type=int, default=4)
    ap.add_argument("--modes", default="0,2")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import bench
    import stable_ts_amd as sw

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
        texts.append(torch.randint(18, 50000, (args.text_tokens,), generator=g).tolist())
        at += n

    eng = model.engine
    passes = dict.fromkeys(COUNTED, 0)
    for name in COUNTED:
        def counted(*a, _real=getattr(eng, name), _name=name, **kw):
            passes[_name] += 1
            return _real(*a, **kw)
        setattr(eng, name, counted)

    audio_s = sum(int(c.shape[-1]) for c in clips) / 16000.0
    rep = dict(model=args.model, dtype=args.dtype, clips=args.clips, clip_seconds_total=round(audio_s, 2),
               clip_seconds_min=min(lengths), clip_seconds_max=max(lengths), text_tokens=args.text_tokens,
               max_tracks=args.max_tracks, repeats=args.repeats, probability_threshold=0.0, modes={})
    warnings.simplefilter("ignore")
    ok = True
    for mode in [int(m) for m in args.modes.split(",")]:
        kw = dict(mode=mode, probability_threshold=0.0, verbose=None)
        variants = [
            ("loop", lambda: [model.locate(a, list(t), "en", **kw) for a, t in zip(clips, texts)]),
            ("many_host_probe", lambda: model.locate_many(clips, [list(t) for t in texts], "en", max_tracks=args.max_tracks,
                                                          device_probe=False, **kw)),
            ("many_device_probe", lambda: model.locate_many(clips, [list(t) for t in texts], "en", max_tracks=args.max_tracks,
                                                            device_probe=True, **kw)),
        ]
        times = {name: [] for name, _ in variants}
        made, snaps = {}, {}
        for r in range(args.repeats + 1):                        # round 0 = warm-up (workspace growth, first launches)
            for name, fn in variants:
                for k in passes:
                    passes[k] = 0
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = fn()
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if r:
                    times[name].append(dt)
                made[name] = dict(passes)
                snaps[name] = [flat(m) for m in out]
                print(f"[bench_locate_many] mode {mode} round {r} {name}: {dt:.3f} s", file=sys.stderr, flush=True)
        entry = dict(matches=sum(len(m) for m in snaps["loop"]), variants={})
        for name, _ in variants:
            med = statistics.median(times[name])
            entry["variants"][name] = dict(seconds_median=round(med, 4), seconds_all=[round(t, 4) for t in times[name]],
                                           x_realtime=round(audio_s / med, 1), device_passes=made[name],
                                           device_passes_total=sum(made[name].values()),
                                           agrees_with_loop=agree(snaps[name], snaps["loop"]))
            ok = ok and entry["variants"][name]["agrees_with_loop"]
        loop_s = entry["variants"]["loop"]["seconds_median"]
        entry["speedup_host_probe"] = round(loop_s / entry["variants"]["many_host_probe"]["seconds_median"], 2)
        entry["speedup_device_probe"] = round(loop_s / entry["variants"]["many_device_probe"]["seconds_median"], 2)
        rep["modes"][str(mode)] = entry
    rep["xkv_gib_per_window"] = round(eng.lib.swx_cross_kv_bytes(eng.h, 1) / 2 ** 30, 3)
    rep["workspace_gib"] = round(eng.ws.numel() / 2 ** 30, 3)
    rep["peak_device_gib"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
    text = json.dumps(rep, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)
    assert ok, "the variants of locate disagree (matches, words, tokens, or a time by more than 20 ms)"


if __name__ == "__main__":
    main()
