"""Time ``denoiser="noisereduce"``: ``prep_audio(bench.synth_audio(S, 0), denoiser="noisereduce")`` for S = 600 s and 3 600 s on the
device, and the f32 CPU evaluation of the same statement (tests/spectral_gate_ref.py, 16 threads) for 600 s on the same box.

Each case runs in a child process of its own: one warm-up, then ``--repeats`` timed calls; the median is reported with the range
and all samples.  A device case also times its three parts apart, each ending in a synchronise: the upload of the host tensor,
the gate on the resident tensor (``denoise.spectral_gate``), the copy back -- their medians give the shares.  ``prep_audio`` of a
host tensor is those three in a row.  The report goes to ``--out`` as JSON and is printed.

    python scripts/bench_denoise.py --out profiles/spectral_gate_bench.json                         (needs a GPU)
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/bench_denoise.py --case gpu600 --repeats 1    (per-kernel times)
    python scripts/bench_denoise.py --kernel-stats DIR --out profiles/spectral_gate_bench.json      (folds the trace's CSV in)
"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"gpu600": 600, "gpu3600": 3600, "cpu600": 600}
CPU_THREADS = 16


def _summary(samples):
    return dict(median_s=statistics.median(samples), min_s=min(samples), max_s=max(samples), samples_s=samples)


def run_case(case: str, repeats: int) -> dict:
    sys.path.insert(0, ROOT)
    import torch
    import bench
    seconds = CASES[case]
    audio = bench.synth_audio(seconds, 0)
    out = dict(case=case, audio_seconds=seconds, samples=int(audio.shape[-1]))
    if case.startswith("cpu"):
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import spectral_gate_ref as sg
        torch.set_num_threads(CPU_THREADS)
        out["threads"] = torch.get_num_threads()

        def call():
            t0 = time.perf_counter()
            sg.gate(audio, torch.float32)
            return time.perf_counter() - t0
        call()
        out["cpu_statement_f32"] = _summary([call() for _ in range(repeats)])
        return out

    from stable_ts_amd.audio_io import prep_audio
    from stable_ts_amd.denoise import gate_config, spectral_gate
    cfg = gate_config({}, 16000)

    def sync_timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, time.perf_counter() - t0

    def parts():
        d, up = sync_timed(lambda: audio.cuda())
        g, gate = sync_timed(lambda: spectral_gate(d, cfg))
        _, back = sync_timed(lambda: g.cpu())
        return up, gate, back

    sync_timed(lambda: prep_audio(audio, denoiser="noisereduce"))
    parts()
    whole, split = [], []
    for _ in range(repeats):
        whole.append(sync_timed(lambda: prep_audio(audio, denoiser="noisereduce"))[1])
        split.append(parts())
    out["prep_audio_host_tensor"] = _summary(whole)
    for i, name in enumerate(("upload", "gate_resident", "copy_back")):
        out[name] = _summary([s[i] for s in split])
    total = sum(out[k]["median_s"] for k in ("upload", "gate_resident", "copy_back"))
    out["shares"] = {k: out[k]["median_s"] / total for k in ("upload", "gate_resident", "copy_back")}
    out["times_real_time"] = seconds / out["prep_audio_host_tensor"]["median_s"]
    out["gate_resident_times_real_time"] = seconds / out["gate_resident"]["median_s"]
    out["device"] = torch.cuda.get_device_name(0)
    return out


def kernel_stats(directory: str) -> list:
    """one row per kernel name from a ``rocprofv3 --kernel-trace --stats`` output directory (its database, or its CSV)"""
    import sqlite3
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*.db"), recursive=True):
        c = sqlite3.connect(path)
        for name, calls, total, avg in c.execute("select name, count(*), sum(duration) / 1000.0, avg(duration) / 1000.0 from kernels "
                                                 "group by name"):
            rows.append(dict(name=name[:80], calls=calls, total_us=total, average_us=avg))
    if not rows:
        for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
            with open(path, newline="") as f:
                for r in csv.DictReader(f):
                    rows.append(dict(name=r["Name"][:80], calls=int(r["Calls"]), total_us=float(r["TotalDurationNs"]) / 1e3,
                                     average_us=float(r["AverageNs"]) / 1e3))
    busy = sum(r["total_us"] for r in rows) or 1.0
    for r in rows:
        r["percent"] = 100.0 * r["total_us"] / busy
    return sorted(rows, key=lambda r: -r["total_us"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(CASES), default=None, help="run one case in this process and print its JSON line")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--kernel-stats", default=None, metavar="DIR", help="fold a kernel trace's statistics into --out")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.case:
        print("RESULT " + json.dumps(run_case(args.case, args.repeats)), flush=True)
        return
    report = {}
    if args.out and os.path.exists(args.out):
        with open(args.out) as f:
            report = json.load(f)
    if args.kernel_stats:
        report["kernel_trace_gpu600_one_warmup_one_call"] = kernel_stats(args.kernel_stats)
    else:
        for case in ("gpu600", "gpu3600", "cpu600"):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", case, "--repeats", str(args.repeats)],
                               capture_output=True, text=True, timeout=900)
            lines = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
            if p.returncode != 0 or not lines:
                raise RuntimeError(f"case {case} failed ({p.returncode}):\n{p.stderr[-2000:]}")
            report[case] = json.loads(lines[-1][7:])
    text = json.dumps(report, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
