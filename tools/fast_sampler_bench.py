#!/usr/bin/env python3
"""Measure the counter-based device sampler against the project's
other two samplers on the rmat2m workload (B = 512, fanouts 25,10), in one
process, after warm-up, in alternating rounds:

  per batch   the fast sampler, the bit-exact device sampler (both event-timed
              over batches issued back to back on one stream) and one host
              sampler stream (wall clock of gs_sample_pack_run on one thread);
  sustained   roots/s of Runner(sampler="device-fast") with 2..4 device
              streams and of the host-sampler runner at the bench's stream
              count, host clock around gs_runner_run + a device synchronise.

    python tools/fast_sampler_bench.py --out profiles/fast_sampler_bench.json

--kernels-only runs the fast sampler alone, for a kernel trace in a run of its
own (tracing slows the host, so no end-to-end number is taken there):

    rocprofv3 --kernel-trace --stats -d OUT -o run --output-format csv -- \\
        python tools/fast_sampler_bench.py --kernels-only
    python tools/fast_sampler_bench.py --summarize OUT --out profiles/fast_sampler_kernels.txt

Needs the GPU: there is no CPU path.  This is a measurement tool, not bench.py;
it asserts nothing about speed."""
import argparse
import ctypes
import glob
import json
import os
import sys
import time
from importlib import import_module

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

gs = import_module("graphsage-pytorch_amd")
L = import_module("graphsage-pytorch_amd._lib")
S = import_module("graphsage-pytorch_amd.sampler")
train = import_module("graphsage-pytorch_amd.train")
ops = import_module("graphsage-pytorch_amd.hip_ops")

SCALE, PAIRS, FEAT, FAN, B, CLASSES, SEED = 21, 20_000_000, 256, [25, 10], 512, 16, 824
THREADS = 16


def workload(device):
    src, dst = gs.rmat_pairs(SCALE, PAIRS, seed=SEED, n_threads=THREADS)
    graph = gs.CSRGraph.from_pairs(src, dst, 1 << SCALE, n_threads=THREADS)
    cand = np.nonzero(graph.degrees() > 0)[0]
    return graph, cand


def root_batches(cand, n, seed):
    perm = np.resize(np.random.RandomState(seed).permutation(cand), n * B)  # wraps if the graph is small
    return [np.ascontiguousarray(perm[i * B:(i + 1) * B], dtype=np.int64) for i in range(n)]


class DeviceTimer:
    """ms per batch of `issue(i)` called n times back to back on the current stream."""

    def __init__(self):
        self.e0, self.e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def run(self, issue, n):
        torch.cuda.synchronize()
        self.e0.record()
        for i in range(n):
            issue(i)
        self.e1.record()
        torch.cuda.synchronize()
        return self.e0.elapsed_time(self.e1) / n


def sampler_issuers(graph, batches, device):
    """(issue functions, result checks) of the fast and the bit-exact device sampler."""
    lib = L.lib()
    st = L.stream_ptr(device)
    roots = [torch.from_numpy(b.astype(np.int32)).to(device) for b in batches]
    fast = S.FastDeviceSampler(graph, FAN, B, SEED, device=device)
    exact = S.DeviceSampler(graph, FAN, B, device=device)
    exact.set_rng(gs.RNG(SEED))
    pack_f = torch.zeros(fast.pack_bound(B), dtype=torch.int32, device=device)
    pack_e = torch.zeros(exact.pack_bound(B), dtype=torch.int32, device=device)

    def issue_fast(i):
        L.check(lib.gs_dsampler_run_at(fast._h, i, roots[i % len(roots)].data_ptr(), B, pack_f.data_ptr(),
                                       pack_f.numel(), st))

    def issue_exact(i):
        L.check(lib.gs_dsampler_run(exact._h, roots[i % len(roots)].data_ptr(), B, pack_e.data_ptr(), pack_e.numel(),
                                    st))

    def check(h):  # the last run's status (a capacity miss of the bit-exact sampler shows here)
        hs = np.zeros(4 * L.GS_MAX_HOPS, np.int64)
        off = np.zeros(L.GS_MAX_HOPS * L.GS_PK_NFIELDS, np.int64)
        used = ctypes.c_int64()
        L.check(lib.gs_dsampler_result(h, hs.ctypes.data, off.ctypes.data, ctypes.byref(used)))
        return hs.reshape(-1, 4)[:2].tolist()

    return (issue_fast, lambda: check(fast._h), fast), (issue_exact, lambda: check(exact._h), exact)


def host_stream_ms(graph, batches, n):
    lib = L.lib()
    fan = np.asarray(FAN, np.int32)
    bound = int(lib.gs_sample_pack_bound(graph.handle, B, fan.ctypes.data, 2)) + B
    buf = np.zeros(bound, np.int32)
    hs = np.zeros(4 * L.GS_MAX_HOPS, np.int64)
    off = np.zeros(L.GS_MAX_HOPS * L.GS_PK_NFIELDS, np.int64)
    used = ctypes.c_int64()
    rng = gs.RNG(SEED)
    t0 = time.perf_counter()
    for i in range(n):
        r = batches[i % len(batches)]
        L.check(lib.gs_sample_pack_run(graph.handle, rng._h, r.ctypes.data, B, fan.ctypes.data, 2, 0, buf.ctypes.data,
                                       bound, hs.ctypes.data, off.ctypes.data, ctypes.byref(used)))
    return 1e3 * (time.perf_counter() - t0) / n


def runner_rate(graph, X, labels, batches, warm, steps, sampler, streams):
    """Sustained roots/s of `steps` training steps after `warm` warm-up steps."""
    tr = train.NativeTrainer(graph, X, labels, CLASSES, fanouts=FAN, seed=SEED)
    rngs = streams if sampler == "device-fast" else [train.make_rng(SEED, 0, w) for w in range(streams)]
    r = train.Runner(tr, graph, batches[:warm + steps], rngs, FAN, depth=4, sampler=sampler, seed=SEED,
                     warm=sampler == "host")
    try:
        r.run(warm)
        torch.cuda.synchronize()
        r.stats(reset=True)
        t0 = time.perf_counter()
        r.run(steps)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        loss = float(tr.loss)
        st = r.stats()
    finally:
        r.close()
    # ms per step of the issuing thread (launches issued, waits for a sampled batch, for a ring entry) and the
    # runner's own sampling time per batch (device events around a device run, the sampler thread's clock on the host)
    host = {"issue": round(1e3 * st["issue_s"] / steps, 4), "wait_sample": round(1e3 * st["wait_sample_s"] / steps, 4),
            "wait_ring": round(1e3 * st["wait_ring_s"] / steps, 4),
            "sampler_ms_per_batch": round(1e3 * st["sample_s"] / steps, 4)}
    return steps * B / dt, loss, host


def summarize(trace_dir, out):
    files = sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True))
    if not files:
        raise SystemExit(f"no *kernel_stats.csv under {trace_dir}")
    import csv
    rows = [r for r in csv.DictReader(open(files[-1])) if "gs::fs::" in r["Name"]]
    if not rows:
        raise SystemExit(f"{files[-1]} holds no gs::fs:: kernel")
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    calls_per_batch = None
    lines = ["rocprofv3 --kernel-trace --stats, fast sampler alone (rmat2m, B = 512, fanouts 25,10)",
             f"{'kernel':58s} {'calls':>7s} {'avg us':>9s} {'min us':>9s} {'max us':>9s} {'share':>7s}"]
    for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"])):
        name = r["Name"].split("(")[0].replace("void ", "").replace("gs::fs::", "")
        lines.append(f"{name:58s} {int(r['Calls']):7d} {float(r['AverageNs']) / 1e3:9.2f} "
                     f"{float(r['MinNs']) / 1e3:9.2f} {float(r['MaxNs']) / 1e3:9.2f} "
                     f"{100 * float(r['TotalDurationNs']) / total:6.1f}%")
        if name.startswith("finish_kernel"):
            calls_per_batch = int(r["Calls"])
    if calls_per_batch:
        lines.append(f"kernel time per batch (sum over the sampler's kernels / {calls_per_batch} batches): "
                     f"{total / calls_per_batch / 1e3:.1f} us in {sum(int(r['Calls']) for r in rows) // calls_per_batch}"
                     " launches")
    text = "\n".join(lines) + "\n"
    if out:
        with open(out, "w") as f:
            f.write(text)
    print(text)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", type=int, default=200, help="batches per timed sampler window")
    ap.add_argument("--rounds", type=int, default=5, help="alternating rounds")
    ap.add_argument("--steps", type=int, default=1000, help="timed runner steps")
    ap.add_argument("--warmup", type=int, default=150, help="runner warm-up steps")
    ap.add_argument("--host-streams", type=int, default=12, help="sampler streams of the host runner (bench default)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--summarize", metavar="DIR", default=None)
    args = ap.parse_args()
    if args.summarize:
        return summarize(args.summarize, args.out)
    if not torch.cuda.is_available():
        raise SystemExit("fast_sampler_bench needs a HIP device")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    t0 = time.perf_counter()
    graph, cand = workload(device)
    batches = root_batches(cand, args.warmup + args.steps, SEED)
    print(f"graph: {time.perf_counter() - t0:.1f} s", file=sys.stderr)
    (issue_fast, check_fast, _f), (issue_exact, check_exact, _e) = sampler_issuers(graph, batches[:64], device)
    timer = DeviceTimer()
    timer.run(issue_fast, 20)  # warm-up: code objects, first-touch of every buffer
    if args.kernels_only:
        timer.run(issue_fast, 200)
        print("sizes", check_fast())
        return
    timer.run(issue_exact, 20)
    host_stream_ms(graph, batches, 20)
    res = {"workload": f"rmat2m (scale {SCALE}, {PAIRS} pairs), B = {B}, fanouts {FAN}",
           "per_batch_ms": {"fast": [], "bit_exact_device": [], "host_one_stream": []}, "runner_roots_per_s": {}}
    for _ in range(args.rounds):
        res["per_batch_ms"]["fast"].append(round(timer.run(issue_fast, args.batches), 4))
        res["per_batch_ms"]["bit_exact_device"].append(round(timer.run(issue_exact, args.batches), 4))
        res["per_batch_ms"]["host_one_stream"].append(round(host_stream_ms(graph, batches, args.batches), 4))
    res["hop_sizes_last_batch"] = {"fast": check_fast()}
    try:
        res["hop_sizes_last_batch"]["bit_exact_device"] = check_exact()
    except Exception as e:  # a capacity miss is a result of the measurement, not a failure of the tool
        res["hop_sizes_last_batch"]["bit_exact_device"] = f"{type(e).__name__}: {e}"
    X = torch.empty(1 << SCALE, FEAT, dtype=torch.float32, device=device)
    ops.fill_uniform(X, SEED)
    labels = torch.from_numpy((np.arange(1 << SCALE, dtype=np.int64) % CLASSES).astype(np.int32)).to(device)
    configs = [("device-fast", 2), ("device-fast", 3), ("device-fast", 4), ("host", args.host_streams)]
    for sampler, streams in configs:
        res["runner_roots_per_s"][f"{sampler} S={streams}"] = []
    res["runner_loss"] = {}
    runner_rate(graph, X, labels, batches, 20, 50, "device-fast", 2)  # warm-up of the step's code objects
    res["runner_host_ms_per_step"] = {}
    for _ in range(min(args.rounds, 3)):
        for sampler, streams in configs:
            rate, loss, host = runner_rate(graph, X, labels, batches, args.warmup, args.steps, sampler, streams)
            res["runner_host_ms_per_step"][f"{sampler} S={streams}"] = host
            res["runner_roots_per_s"][f"{sampler} S={streams}"].append(round(rate))
            res["runner_loss"][f"{sampler} S={streams}"] = loss
    med = lambda v: float(np.median(v))  # noqa: E731
    res["median"] = {"per_batch_ms": {k: med(v) for k, v in res["per_batch_ms"].items()},
                     "runner_roots_per_s": {k: med(v) for k, v in res["runner_roots_per_s"].items()}}
    text = json.dumps(res, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
