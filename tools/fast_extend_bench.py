#!/usr/bin/env python3
"""Measure the counter-based extend_nodes (UnsupervisedLoss(extend="fast"),
DESIGN §5e) next to the bit-exact one, in one process, after warm-up, in
alternating rounds over the same batches of 512 training ids.

Two configurations, those of tools/full_unsup_bench.py:

  pubmed   the golden Pubmed graph, its training split
  rmat2m   scale 21, 20 M pairs, one edge for every node without one; the
           training set is the first 2^17 ids of a fixed permutation

Per configuration and num_neg (100 and 6):

  exact_ms / fast_ms   host clock around extend_nodes_array (both end in a
                       synchronise of the object's own stream): median, min,
                       max and every round; exact_over_fast per round
  fast_phases_ms       device events inside the fast call: walks, balls,
                       masks, negatives, unique, copy_back (medians)
  exact_prof_ms        the exact call's own GS_UNSUP_PROF split of the same
                       batches (medians of the lines it prints to stderr, which
                       this tool redirects to a file and parses)
  sizes                U, P, N of the last batch under either rule

and FullTrainer.unsup_step end to end ("normal" and "margin", learn_method
"unsup") with an exact and with a fast object, alternating.

    python tools/fast_extend_bench.py --out profiles/fast_extend_bench.json

Needs the GPU.  A measurement tool, not bench.py; it asserts nothing about
speed."""
import argparse
import json
import os
import random
import re
import sys
import tempfile
import time
from importlib import import_module

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["GS_UNSUP_PROF"] = "1"  # read once, at the library's first extend

import numpy as np  # noqa: E402
import torch  # noqa: E402

gs = import_module("graphsage-pytorch_amd")
train = import_module("graphsage-pytorch_amd.train")
unsup = import_module("graphsage-pytorch_amd.unsup")
fub = import_module("tools.full_unsup_bench")

SEED, B = fub.SEED, fub.B
PROF_DEV = re.compile(r"\[unsup dev\] balls ([\d.]+) far lists ([\d.]+) \((\d+) fresh sets, (\d+) ids\) draws ([\d.]+) "
                      r"requests ([\d.]+) select ([\d.]+) \((\d+) picks\) fresh-order wait ([\d.]+) compose ([\d.]+) ms")
PROF_ALL = re.compile(r"\[unsup\] walks ([\d.]+) negatives ([\d.]+) unique: sets ([\d.]+) union ([\d.]+) subset "
                      r"([\d.]+) ms")


def note(msg):
    print(f"[fast_extend_bench] {msg}", flush=True)


class StderrToFile:
    """The process's stderr (fd 2, where the native library prints its split) into a file while inside."""

    def __init__(self, path):
        self.path = path

    def __enter__(self):
        sys.stderr.flush()
        self.saved = os.dup(2)
        self.fd = os.open(self.path, os.O_WRONLY | os.O_CREAT | os.O_APPEND, 0o600)
        os.dup2(self.fd, 2)

    def __exit__(self, *exc):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        os.close(self.fd)


def stats(v):
    return {"median": round(float(np.median(v)), 3), "min": round(float(min(v)), 3), "max": round(float(max(v)), 3),
            "rounds": [round(float(x), 3) for x in v]}


def exact_split(path, skip, keep):
    """Medians of the last `keep` exact calls' printed split (the first `skip` are warm-up)."""
    with open(path) as f:
        text = f.read()
    dev = [[float(x) for x in m.groups()] for m in PROF_DEV.finditer(text)][skip:skip + keep]
    tot = [[float(x) for x in m.groups()] for m in PROF_ALL.finditer(text)][skip:skip + keep]
    out = {}
    if dev:
        names = ("balls", "far_lists", "fresh_sets", "fresh_ids", "draws", "requests", "select", "picks",
                 "fresh_order_wait", "compose")
        out.update({k: round(float(np.median([r[i] for r in dev])), 3) for i, k in enumerate(names)})
    if tot:
        names = ("walks", "negatives", "unique_sets", "unique_union", "subset")
        out.update({k: round(float(np.median([r[i] for r in tot])), 3) for i, k in enumerate(names)})
    out["calls_parsed"] = len(tot)
    return out


def measure(name, dev, rounds, log):
    graph, n, X, train_ids, labels, C, extra = {"pubmed": fub.pubmed, "rmat2m": fub.rmat2m}[name](dev)
    note(f"{name}: {n} nodes, {graph.n_entries} entries, {len(train_ids)} training ids")
    exact = unsup.UnsupervisedLoss(graph, train_ids, dev)
    fast = unsup.UnsupervisedLoss(graph, train_ids, dev, extend="fast", seed=7)
    assert exact.device_balls and fast.device_balls
    fast.fast_phases(True)
    order = np.random.RandomState(SEED + 1).permutation(train_ids)
    n_batches = len(order) // B
    cursor = [0]

    def next_batch():
        cursor[0] = (cursor[0] + 1) % n_batches
        return order[cursor[0] * B:(cursor[0] + 1) * B]

    random.seed(SEED)
    res = {"graph": dict(extra, n=n, entries=int(graph.n_entries), train_ids=int(len(train_ids))), "batch": B,
           "rounds": rounds, "extend": {}, "unsup_step": {}}
    warm = 2
    for num_neg in (100, 6):
        open(log, "w").close()
        t_exact, t_fast, phases = [], [], []
        sizes = {}
        for r in range(warm + rounds):
            ids = next_batch()
            with StderrToFile(log):
                te, ue = fub.host_ms(lambda: exact.extend_nodes_array(ids, num_neg=num_neg))
            tf, uf = fub.host_ms(lambda: fast.extend_nodes_array(ids, num_neg=num_neg))
            if r < warm:
                continue
            t_exact.append(te)
            t_fast.append(tf)
            phases.append(fast.fast_phases(True))
            sizes = {"exact": [len(ue), len(exact._last["pos"]), len(exact._last["neg"])],
                     "fast": [len(uf), len(fast._last["pos"]), len(fast._last["neg"])]}
        row = {"exact_ms": stats(t_exact), "fast_ms": stats(t_fast),
               "exact_over_fast": stats([a / b for a, b in zip(t_exact, t_fast)]),
               "fast_phases_ms": {k: round(float(np.median([p[k] for p in phases])), 3) for k in phases[0]},
               "exact_prof_ms": exact_split(log, warm, rounds), "sizes_U_P_N": sizes}
        res["extend"][f"num_neg_{num_neg}"] = row
        note(f"{name} num_neg {num_neg}: {row}")
    # the exact training step end to end with either object
    F = X.shape[1]
    tr = train.FullTrainer(graph, X, torch.from_numpy(labels), C, num_layers=fub.LAYERS, hidden=fub.H,
                           agg_func="MEAN", lr=0.01, seed=SEED)
    for kind in ("normal", "margin"):
        times = {"exact": [], "fast": []}
        for r in range(warm + rounds):
            ids = next_batch()
            for key, ul in (("exact", exact), ("fast", fast)):
                with StderrToFile(log):
                    t, _ = fub.host_ms(lambda: tr.unsup_step(ul, ids, unsup_loss=kind, learn_method="unsup"))
                if r >= warm:
                    times[key].append(t)
        row = {"exact_step_ms": stats(times["exact"]), "fast_step_ms": stats(times["fast"]),
               "exact_over_fast": stats([a / b for a, b in zip(times["exact"], times["fast"])])}
        res["unsup_step"][f"{kind}/unsup"] = row
        note(f"{name} unsup_step {kind}: {row}")
    res["F"] = F
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--configs", default="pubmed,rmat2m")
    ap.add_argument("--rounds", type=int, default=7, help="alternating rounds after two warm-up rounds")
    ap.add_argument("--out", default=None, help="JSON file; configurations already in it are kept")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fast_extend_bench needs a HIP device")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = {}
    if args.out and os.path.exists(args.out):
        with open(args.out) as f:
            res = json.load(f)
    with tempfile.TemporaryDirectory() as tmp:
        for name in args.configs.split(","):
            t0 = time.perf_counter()
            res[name] = measure(name, dev, args.rounds, os.path.join(tmp, "prof.log"))
            note(f"{name}: {time.perf_counter() - t0:.1f} s")
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "w") as f:
                    f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
