#!/usr/bin/env python3
"""Measure what per-edge weights cost on the exact full-neighbourhood path on
rmat2m ("Per-edge weights"), in one process, after warm-up,
alternating rounds, HIP events -- the pattern of tools/full_train_bench.py,
whose graph (rmat2m plus one edge for every node without one) this reuses.

  aggregate   at F = 256 and 128, the default plans (forward seg_len
              hip_ops.FULL_SEG_LEN, transposed FULL_BWD_SEG_LEN): the forward
              hip_ops.agg_full and the backward hip_ops.agg_full_bwd (with its
              dSelf + Hprev epilogue), unweighted against edge_weight= with
              norm="mean" and norm="sum".  By bytes the weighted forms should
              cost the same: the forward reads 4 B more per entry next to a
              4 B id and a 512 B or 1 KB row, the backward reads den in place
              of cnt plus 4 B.
  step        train.FullTrainer (2 layers, hidden 128, F = 256, fp32, SGD),
              unweighted against edge_weight=: ms per step() over all N rows on
              half of the nodes, and per step(field=) on the receptive field
              of a batch of 512.

Weights are uniform in [0.5, 1.5].  Every pair is reported with the rounds,
the median, the range, the ratio of the medians and whether the two ranges
overlap; no bar is asserted.

    python tools/full_weighted_bench.py --out profiles/full_weighted_bench.json

Needs the GPU: there is no CPU path.  A measurement tool, not bench.py."""
import argparse
import json
import os
import sys
from importlib import import_module

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

gs = import_module("graphsage-pytorch_amd")
train = import_module("graphsage-pytorch_amd.train")
ops = import_module("graphsage-pytorch_amd.hip_ops")
fib = import_module("tools.full_infer_bench")

SEED, H = 824, 128


def note(msg):
    print(f"[full_weighted_bench] {msg}", file=sys.stderr, flush=True)


def pair(res, base, other):
    """The ratio of the medians and whether the ranges of the rounds overlap."""
    a, b = res[base]["ms_rounds"], res[other]["ms_rounds"]
    return {"ratio": round(float(np.median(b) / np.median(a)), 4), "ranges_overlap": bool(min(b) <= max(a) and
                                                                                         min(a) <= max(b)),
            "base_ms_range": [min(a), max(a)], "weighted_ms_range": [min(b), max(b)]}


def bench_aggregate(graph, w, F, rounds, reps, dev):
    n = graph.n_nodes
    g = torch.Generator(device="cpu").manual_seed(SEED + F)
    Hs = torch.rand(n, F, generator=g).sub_(0.3).to(dev)      # a relu-like table: ~30 % non-positive
    dA = torch.rand(n, F, generator=g).sub_(0.5).to(dev)
    dS = torch.rand(n, F, generator=g).sub_(0.5).to(dev)
    out, dH = torch.empty_like(Hs), torch.empty_like(Hs)
    plan = ops.agg_full_plan(graph)
    tplan = ops.agg_full_bwd_plan(graph)
    ws = torch.empty(max(16, plan.n_slots * F * 4, tplan.n_slots * F * 4), dtype=torch.uint8, device=dev)
    ews = {"mean": ops.EdgeWeights(plan, w, norm="mean"), "sum": ops.EdgeWeights(plan, w, norm="sum")}
    issuers = {"fwd": lambda: ops.agg_full("MEAN", Hs, plan, out, ws=ws),
               "bwd": lambda: ops.agg_full_bwd("MEAN", dA, tplan, dH, ws=ws, dSelf=dS, Hprev=Hs)}
    for k, ew in ews.items():
        issuers[f"fwd_weighted_{k}"] = lambda ew=ew: ops.agg_full("MEAN", Hs, plan, out, ws=ws, edge_weight=ew)
        issuers[f"bwd_weighted_{k}"] = lambda ew=ew: ops.agg_full_bwd("MEAN", dA, tplan, dH, ws=ws, dSelf=dS, Hprev=Hs,
                                                                      edge_weight=ew)
    # unit weights are the unweighted bits at this size too, before anything is timed
    unit = ops.EdgeWeights(plan, np.ones(plan.n_entries, np.float32))
    same_f = torch.equal(ops.agg_full("MEAN", Hs, plan, ws=ws), ops.agg_full("MEAN", Hs, plan, ws=ws, edge_weight=unit))
    same_b = torch.equal(ops.agg_full_bwd("MEAN", dA, tplan, ws=ws), ops.agg_full_bwd("MEAN", dA, tplan, ws=ws,
                                                                                       edge_weight=unit))
    del unit
    entries, row = graph.n_entries, F * 4
    nbytes = {"fwd": (entries + n) * row, "bwd": (entries + 3 * n) * row}
    times = fib.rounds_of(issuers, rounds, reps)
    res = {k: fib.summary({k: v}, nbytes[k[:3]])[k] for k, v in times.items()}
    return {"n": n, "entries": entries, "F": F, "seg_len": plan.seg_len, "bwd_seg_len": tplan.seg_len,
            "unit_weights_bitwise": {"fwd": bool(same_f), "bwd": bool(same_b)}, "timings": res,
            "weighted_over_unweighted": {k: pair(res, k[:3], k) for k in res if "weighted" in k}}


def bench_step(graph, w, X, labels, nodes, batch, rounds, dev):
    n, F = X.shape
    trs = {"unweighted": train.FullTrainer(graph, X, labels, 16, hidden=H, lr=0.01),
           "weighted": train.FullTrainer(graph, X, labels, 16, hidden=H, lr=0.01, edge_weight=w)}
    issuers = {}
    for k, t in trs.items():
        t.step(nodes)                                        # validates `nodes` once, fills the cache
        f = t.field(batch)
        t.step(batch, field=f)
        issuers[f"step_{k}"] = lambda t=t: t.step(nodes)
        issuers[f"field_step_{k}"] = lambda t=t, f=f: t.step(batch, field=f)
    res = fib.summary(fib.rounds_of(issuers, rounds, 1))
    f = trs["weighted"].field(batch)
    return {"n": n, "F": F, "hidden": H, "layers": 2, "classes": 16, "loss_nodes": int(nodes.numel()),
            "field_batch": int(batch.numel()), "field_sizes": list(f.sizes), "timings": res,
            "weighted_over_unweighted": {"step": pair(res, "step_unweighted", "step_weighted"),
                                         "field_step": pair(res, "field_step_unweighted", "field_step_weighted")}}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scale", type=int, default=21)
    ap.add_argument("--pairs", type=int, default=20_000_000)
    ap.add_argument("--feat", type=int, default=256)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=5, help="alternating rounds")
    ap.add_argument("--reps", type=int, default=3, help="aggregate calls per round and variant")
    ap.add_argument("--sections", default="aggregate,step", help="comma list of: aggregate, step")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("full_weighted_bench needs a HIP device")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    n = 1 << args.scale
    src, dst = gs.rmat_pairs(args.scale, args.pairs, seed=SEED, n_threads=16)
    deg = gs.CSRGraph.from_pairs(src, dst, n, n_threads=16).degrees()
    lone = np.nonzero(deg == 0)[0].astype(np.int64)
    graph = gs.CSRGraph.from_pairs(np.concatenate([src, lone]), np.concatenate([dst, (lone + 1) % n]), n,
                                   n_threads=16)
    note(f"graph built: {n} nodes, {graph.n_entries} entries, {len(lone)} nodes given an edge")
    rs = np.random.RandomState(SEED)
    w = rs.uniform(0.5, 1.5, graph.n_entries).astype(np.float32)
    res = {"graph": {"scale": args.scale, "pairs": args.pairs, "n": n, "entries": graph.n_entries,
                     "max_degree": graph.max_degree, "edges_added_for_nodes_without_one": int(len(lone))},
           "weights": "uniform in [0.5, 1.5]", "rounds": args.rounds, "reps": args.reps, "hbm_peak": fib.HBM_PEAK}
    sections = args.sections.split(",")
    for F in (256, 128) if "aggregate" in sections else ():
        res[f"aggregate_f{F}"] = bench_aggregate(graph, w, F, args.rounds, args.reps, dev)
        note(f"aggregate F={F} done")
        torch.cuda.empty_cache()
    if "step" in sections:
        X = torch.empty(n, args.feat, dtype=torch.float32, device=dev)
        ops.fill_uniform(X, SEED)
        labels = torch.from_numpy(rs.randint(0, 16, n))
        nodes = torch.from_numpy(rs.permutation(n)[:n // 2].astype(np.int32)).to(dev)
        batch = torch.from_numpy(rs.permutation(n)[:args.batch].astype(np.int32)).to(dev)
        res["step"] = bench_step(graph, w, X, labels, nodes, batch, args.rounds, dev)
        note("step done")
    text = json.dumps(res, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
