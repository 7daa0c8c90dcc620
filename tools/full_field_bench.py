#!/usr/bin/env python3
"""Measure exact training restricted to the receptive field of a mini-batch
against the full step on rmat2m ("Exact training on the receptive
field"), in one process, after warm-up, medians of alternating rounds.

The graph is that of tools/full_train_bench.py (rmat2m plus one edge for every
node without one), F = 256, hidden 128, 2 layers, fp32 MEAN, SGD.  For each
batch size B (the first B ids of one fixed permutation) it records

  sizes             n_L .. n_0 of the field
  entries           the CSR entries of the rows of R_l, per layer l = L .. 1:
                    what layer l's aggregate reads
  build_ms          FullTrainer.field(nodes, out=field): every launch of the
                    build and its one synchronisation
  field_step_build  the build, then step(nodes, field=): what a mini-batch
                    loop pays per batch (the layer-1 aggregate is recomputed:
                    its cache is keyed on the build)
  field_step_reuse  step(nodes, field=) with the field kept (and the cached
                    compact layer-1 aggregate with it)
  full_step         FullTrainer.step(nodes) without a field, on a trainer of
                    its own with cache_agg1 on, in the same rounds

Every time is a host clock around work that ends in a device synchronise
(the build synchronises by itself), so launch overhead is part of it.  The
crossover is the first B at which field_step_build is no faster than
full_step.

    python tools/full_field_bench.py --out profiles/full_field_bench.json

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
train = import_module("graphsage-pytorch_amd.train")
ops = import_module("graphsage-pytorch_amd.hip_ops")

SEED, H, LAYERS, CLASSES = 824, 128, 2, 16
BATCHES = [512, 4096, 32768, 262144, 1 << 20]


def note(msg):
    print(f"[full_field_bench] {msg}", file=sys.stderr, flush=True)


def host_ms(issue, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        issue()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def rounds_of(issuers, rounds, reps):
    """{name: [ms per call, one per round]}, the variants alternating inside each round."""
    for issue in issuers.values():
        issue()  # warm-up: code objects, workspaces, the node check
    out = {k: [] for k in issuers}
    for _ in range(rounds):
        for k, issue in issuers.items():
            out[k].append(round(host_ms(issue, reps), 4))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scale", type=int, default=21)
    ap.add_argument("--pairs", type=int, default=20_000_000)
    ap.add_argument("--feat", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5, help="alternating rounds")
    ap.add_argument("--reps", type=int, default=3, help="calls per round and variant")
    ap.add_argument("--batches", default=",".join(str(b) for b in BATCHES))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("full_field_bench needs a HIP device")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    n = 1 << args.scale
    src, dst = gs.rmat_pairs(args.scale, args.pairs, seed=SEED, n_threads=16)
    deg = gs.CSRGraph.from_pairs(src, dst, n, n_threads=16).degrees()
    lone = np.nonzero(deg == 0)[0].astype(np.int64)
    graph = gs.CSRGraph.from_pairs(np.concatenate([src, lone]), np.concatenate([dst, (lone + 1) % n]), n,
                                   n_threads=16)
    note(f"graph built: {n} nodes, {graph.n_entries} entries, {len(lone)} nodes given an edge")
    X = torch.empty(n, args.feat, dtype=torch.float32, device=dev)
    ops.fill_uniform(X, SEED)
    rs = np.random.RandomState(SEED)
    labels = torch.from_numpy(rs.randint(0, CLASSES, n))
    perm = rs.permutation(n).astype(np.int32)
    deg_d = torch.from_numpy(graph.degrees()).to(dev)
    kw = dict(num_layers=LAYERS, hidden=H, agg_func="MEAN", lr=0.01, cache_agg1=True)
    full = train.FullTrainer(graph, X, labels, CLASSES, **kw)
    rest = train.FullTrainer(graph, X, labels, CLASSES, **kw)
    res = {"graph": {"scale": args.scale, "pairs": args.pairs, "n": n, "entries": graph.n_entries,
                     "max_degree": graph.max_degree, "edges_added_for_nodes_without_one": int(len(lone))},
           "F": args.feat, "hidden": H, "layers": LAYERS, "agg": "MEAN", "classes": CLASSES, "rounds": args.rounds,
           "reps": args.reps, "seg_len": [rest.plan.seg_len, rest.tplan.seg_len], "ws_bytes": rest.ws_bytes,
           "batches": {}}
    crossover = None
    for B in (int(b) for b in args.batches.split(",")):
        nodes = torch.from_numpy(perm[:B].copy()).to(dev)
        field = rest.field(nodes)
        state = {"field": field}

        def build():
            state["field"] = rest.field(nodes, out=state["field"])

        def build_and_step():
            build()
            rest.step(nodes, field=state["field"])

        issuers = {"build": build, "field_step_build": build_and_step,
                   "field_step_reuse": lambda: rest.step(nodes, field=state["field"]),
                   "full_step": lambda: full.step(nodes)}
        times = rounds_of(issuers, args.rounds, args.reps)
        ms = {k: round(float(np.median(v)), 3) for k, v in times.items()}
        entries = [int(deg_d[field.rows(l).long()].sum()) for l in range(LAYERS, 0, -1)]
        res["batches"][str(B)] = {
            "sizes": list(field.sizes), "entries": entries,
            "items": [list(field.layer_counts(l)) for l in range(LAYERS, 0, -1)],
            "field_bytes": int(field._f.buf_bytes), "ms": ms, "ms_rounds": times,
            "full_over_field_build": round(ms["full_step"] / ms["field_step_build"], 2),
            "loss": [float(rest.loss), float(full.loss)]}
        if crossover is None and ms["field_step_build"] >= ms["full_step"]:
            crossover = B
        note(f"B = {B}: sizes {field.sizes}, entries {entries}, ms {ms}")
    res["crossover_B"] = crossover
    res["crossover_note"] = ("the first measured B at which the field step, build included, is no faster than the full "
                             "step; null: the field paid at every B measured")
    text = json.dumps(res, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
