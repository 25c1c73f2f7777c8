"""A/B of ragged decode jobs: `_decode_with_fallback` on W windows of large-v3 (BENCH_WEIGHTS, beam 5, a fixed step count) whose
prompts have W distinct lengths between 0 and 223 tokens -- what a lockstep round of transcribe_spans() looks like while the
spans' histories differ.  Switch off = one lockstep job per distinct initial length (W batch-1 jobs, the only way before ragged
jobs existed); on = one job.  Same process, same buffers, alternating, median of `--reps`.  Prints one JSON line.
    python scripts/ab_ragged_decode.py [--windows 20 --tokens 112 --reps 5]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=20)
    ap.add_argument("--tokens", type=int, default=112)
    ap.add_argument("--beam", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import bench
    import stable_ts_amd as sw
    import stable_ts_amd.decoding as D
    import stable_ts_amd.transcribe as T
    W = a.windows
    dims = sw.dims_for("large-v3")
    model = sw.Whisper(dims, device="cuda:0", dtype="f16", max_windows=W, max_rows=W * a.beam)
    model.load_state_dict(sw.random_state_dict(dims, seed=1234, std=0.02, **sw.BENCH_WEIGHTS))
    audio = bench.synth_audio(30.0 * W, seed=0).cuda()
    wins = [audio[i * 480000:(i + 1) * 480000].contiguous() for i in range(W)]
    xkv = model.cross_kv(model.encoder(model.log_mel_batch(wins, [0] * W)))
    rng = np.random.RandomState(0)
    lengths = [int(round(x)) for x in np.linspace(0, 223, W)]
    prompts = [[int(t) for t in rng.randint(300, 20000, size=n)] or None for n in lengths]
    base = dict(language="en", beam_size=a.beam, sample_len=a.tokens, min_tokens=a.tokens, max_initial_timestamp=None)

    def run(switch):
        D.RAGGED_DECODE = switch
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = T._decode_with_fallback(model, xkv, base, [0.0], prompts, None, None, None, None)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, res

    times = {False: [], True: []}
    outs = {}
    for switch in (False, True):          # warm-up: graph captures, allocator
        outs[switch] = run(switch)[1]
    same = all(x.tokens == y.tokens and x.avg_logprob == y.avg_logprob for x, y in zip(outs[False], outs[True]))
    for _ in range(a.reps):
        for switch in (False, True):
            times[switch].append(run(switch)[0])
    off, on = statistics.median(times[False]), statistics.median(times[True])
    print(json.dumps(dict(windows=W, beam=a.beam, tokens=a.tokens, prompt_lengths=lengths, reps=a.reps,
                          grouped_ms=round(off * 1e3, 2), ragged_ms=round(on * 1e3, 2), speedup=round(off / on, 2),
                          grouped_ms_all=[round(t * 1e3, 2) for t in times[False]],
                          ragged_ms_all=[round(t * 1e3, 2) for t in times[True]], results_identical=bool(same))))


if __name__ == "__main__":
    main()
