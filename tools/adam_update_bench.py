#!/usr/bin/env python3
"""Measure what the fused clip + Adam update costs next to clip + SGD (DESIGN
§4, "Adam / AdamW update"), in one process, after warm-up, in alternating
rounds:

  update      one update call on flat buffers with the trainer's two clip
              groups, at the rmat2m parameter count (F = 256, 16 classes:
              100368 floats, float4 kernels) and at the Pubmed one (F = 500,
              3 classes: 161155 floats, scalar kernels): gs_clip_adam and
              gs_clip_sgd, and gs_trainer_update_local under Adam and under
              SGD.  Calls issued back to back have no step between them, so
              each is the two-launch form (norm partials, then the update);
              the norm launch is the same kernel in all four, so Adam - SGD
              is the difference of the update kernels.  HIP events around 200
              calls after 20.
  runner      steps/s of 200 runner steps (after 20) on the tiny R-MAT of the
              tests (B = 48, F = 256, fanouts 25,10) under Adam, under SGD
              with the deferred update switched off (the like-for-like
              comparison: one update launch per step in both) and under the
              default SGD (deferred), host clock around gs_runner_run + a
              device synchronise.  200 steps of this size are about 10 ms, so
              --runner-steps takes a longer window, and --full-size adds the
              same three paths on the rmat2m workload (B = 512, 12 sampler
              streams, 1000 steps after 150), where the step is not a toy.

    python tools/adam_update_bench.py --full-size --out profiles/adam_update_bench.json

Needs the GPU: there is no CPU path.  A measurement tool, not bench.py; it
asserts nothing about speed."""
import argparse
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
train = import_module("graphsage-pytorch_amd.train")
ops = import_module("graphsage-pytorch_amd.hip_ops")

H, FAN, B, SEED = 128, [25, 10], 48, 824
SIZES = {"rmat2m": dict(feat=256, classes=16), "pubmed": dict(feat=500, classes=3)}
ADAM = dict(optimizer="adam", lr=0.01, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)


def tiny_rmat():
    g = np.load(os.path.join(ROOT, "tests", "golden", "graphs.npz"))
    n = int(g["rmat_n"][0])
    return gs.CSRGraph.from_pairs(g["rmat_src"], g["rmat_dst"], n), n


def us_per_call(issue, n, warm):
    for _ in range(warm):
        issue()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        issue()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / n


def update_issuers(graph, n, feat, classes, device):
    """The four update calls at this parameter count, each on its own state."""
    X = torch.empty(n, feat, dtype=torch.float32, device=device)
    ops.fill_uniform(X, SEED)
    labels = torch.from_numpy((np.arange(n) % classes).astype(np.int32)).to(device)
    lib = L.lib()
    st = L.stream_ptr(device)
    out = {}
    keep = []
    for name, kw in (("adam", ADAM), ("sgd", {})):
        tr = train.NativeTrainer(graph, X, labels, classes, hidden=H, fanouts=FAN, seed=SEED, **kw)
        tr.p.grads.normal_(0, 1e-3)
        keep.append(tr)
        out[f"trainer_update_local_{name}"] = lambda tr=tr: L.check(lib.gs_trainer_update_local(tr._h, st))
    tr = keep[0]
    total = tr.p.params.numel()
    goff = tr.p.group_off
    p, g = tr.p.params.clone(), torch.randn(total, device=device) * 1e-3
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    ws = torch.empty(130, dtype=torch.float32, device=device)
    step = [0]

    def clip_adam():
        step[0] += 1
        ops.clip_adam(goff, p, g, m, v, 1.0, 5.0, 0.01, (0.9, 0.999), 1e-8, 0.01, step[0], ws)

    p2, g2 = p.clone(), g.clone()
    out["clip_adam"] = clip_adam
    out["clip_sgd"] = lambda: ops.clip_sgd(goff, p2, g2, 1.0, 5.0, 0.7, ws)
    return out, total, keep


def runner_rate(graph, X, labels, batches, warm, steps, kw, defer, streams=4):
    tr = train.NativeTrainer(graph, X, labels, 16, hidden=H, fanouts=FAN, seed=SEED, **kw)
    if defer is not None:
        tr.set_option("defer_update", defer)
    r = train.Runner(tr, graph, batches[:warm + steps], [train.make_rng(SEED, 0, w) for w in range(streams)], FAN,
                     depth=4, warm=True)
    try:
        r.run(warm)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r.run(steps)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        loss = float(tr.loss)
    finally:
        r.close()
    return steps / dt, loss


def root_batches(cand, n, batch):
    perm = np.resize(np.random.RandomState(SEED).permutation(cand), n * batch)  # wraps if the graph is small
    return [np.ascontiguousarray(perm[i * batch:(i + 1) * batch], dtype=np.int64) for i in range(n)]


def runner_rounds(graph, n, batch, warm, steps, rounds, streams, device):
    """Steps/s of the three update paths, alternating, F = 256 and 16 classes."""
    X = torch.empty(n, 256, dtype=torch.float32, device=device)
    ops.fill_uniform(X, SEED)
    labels = torch.from_numpy((np.arange(n) % 16).astype(np.int32)).to(device)
    batches = root_batches(np.nonzero(graph.degrees() > 0)[0], warm + steps, batch)
    configs = {"adam": (ADAM, None), "sgd_defer_off": ({}, False), "sgd_deferred": ({}, True)}
    out = {"batch": batch, "steps": steps, "warmup": warm, "sampler_streams": streams,
           "steps_per_s": {k: [] for k in configs}, "loss": {}}
    runner_rate(graph, X, labels, batches, warm, 50, ADAM, None, streams)  # warm-up of the step's code objects
    for _ in range(rounds):
        for k, (kw, defer) in configs.items():
            rate, loss = runner_rate(graph, X, labels, batches, warm, steps, kw, defer, streams)
            out["steps_per_s"][k].append(round(rate, 1))
            out["loss"][k] = loss
    r = {k: float(np.median(v)) for k, v in out["steps_per_s"].items()}
    out["median"] = {"steps_per_s": r, "us_per_step": {k: round(1e6 / x, 2) for k, x in r.items()},
                     "roots_per_s": {k: round(x * batch) for k, x in r.items()},
                     "adam_vs_sgd_defer_off": round(r["adam"] / r["sgd_defer_off"], 4),
                     "not_deferring_costs": round(1.0 - r["sgd_defer_off"] / r["sgd_deferred"], 4),
                     "adam_vs_sgd_deferred": round(r["adam"] / r["sgd_deferred"], 4)}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--launches", type=int, default=200, help="timed update calls per round")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5, help="alternating rounds")
    ap.add_argument("--runner-steps", type=int, default=200, help="timed runner steps on the tiny R-MAT")
    ap.add_argument("--full-size", action="store_true",
                    help="also the three runner paths on the rmat2m workload (B = 512, 12 sampler streams, 1000 steps)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("adam_update_bench needs a HIP device")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    graph, n = tiny_rmat()
    res = {"launches": args.launches, "warmup": args.warmup, "rounds": args.rounds, "update_us_per_call": {},
           "bytes_per_update": {}}
    for size, cfg in SIZES.items():
        issuers, total, _keep = update_issuers(graph, n, cfg["feat"], cfg["classes"], device)
        times = {k: [] for k in issuers}
        for _ in range(args.rounds):
            for k, issue in issuers.items():
                times[k].append(round(us_per_call(issue, args.launches, args.warmup), 3))
        res["update_us_per_call"][size] = {"n_params": total, "float4": total % 4 == 0, **times}
        # read + write of p, g (SGD) and of p, g, m, v (Adam), plus the norm launch's read of g
        res["bytes_per_update"][size] = {"sgd": 20 * total, "adam": 36 * total}
    med = lambda v: float(np.median(v))  # noqa: E731
    res["median_update_us_per_call"] = {s: {k: med(v) for k, v in d.items() if isinstance(v, list)}
                                        for s, d in res["update_us_per_call"].items()}
    res["runner_tiny_rmat"] = runner_rounds(graph, n, B, args.warmup, args.runner_steps, args.rounds, 4, device)
    if args.full_size:
        src, dst = gs.rmat_pairs(21, 20_000_000, seed=SEED, n_threads=16)
        big = gs.CSRGraph.from_pairs(src, dst, 1 << 21, n_threads=16)
        res["runner_rmat2m"] = runner_rounds(big, 1 << 21, 512, 150, 1000, min(args.rounds, 3), 12, device)
    text = json.dumps(res, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
