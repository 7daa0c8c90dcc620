#!/usr/bin/env python3
"""Measure exact full-batch training over full neighbourhoods on rmat2m
("Exact full-batch training"), in one process, after
warm-up, medians of alternating rounds, HIP events.

The graph is rmat2m plus one edge (v, v + 1) for every node without an edge,
the variant tools/full_infer_bench.py uses for MAX: train.FullTrainer refuses
a node with an empty neighbourhood under MEAN as well.

  aggregate   at width 128 (the hidden width, where the backward runs) and
              for seg_len in {64, 128, 256, 1024, no split}: the forward
              hip_ops.agg_full, the backward hip_ops.agg_full_bwd bare and with
              its dSelf + Hprev epilogue -- MEAN, and MAX with the
              argmax-recording forward.  us per call and the fraction of the
              8 TB/s HBM peak against the algorithmic bytes (forward: (entries
              + N) rows of F floats; backward: one gradient row per entry,
              two for MAX which reads an argmax row beside it, plus the N
              output rows and the epilogue's 2 N rows).
  step        train.FullTrainer (2 layers, hidden 128, fp32, SGD) on half of
              the nodes, MEAN and MAX: ms per step() with cache_agg1 on and
              off, each stage alone (forward, loss head, backward, update) and
              FullEmbedder.embed() at the same weights in the same run.

    python tools/full_train_bench.py --out profiles/full_train_bench.json

Needs the GPU: there is no CPU path.  A measurement tool, not bench.py; it
asserts nothing about speed."""
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
_lib = import_module("graphsage-pytorch_amd._lib")
fib = import_module("tools.full_infer_bench")

SEED, H = 824, 128
SEG_LENS = fib.SEG_LENS


def note(msg):
    print(f"[full_train_bench] {msg}", file=sys.stderr, flush=True)


def bench_aggregate(graph, agg, rounds, reps, dev):
    n = graph.n_nodes
    entries = graph.n_entries
    F = H
    g = torch.Generator(device="cpu").manual_seed(SEED)
    Hs = torch.rand(n, F, generator=g).sub_(0.3).to(dev)      # a relu-like table: ~30 % non-positive
    dA = torch.rand(n, F, generator=g).sub_(0.5).to(dev)
    dS = torch.rand(n, F, generator=g).sub_(0.5).to(dev)
    out, dH = torch.empty_like(Hs), torch.empty_like(Hs)
    am = torch.empty(n, F, dtype=torch.int32, device=dev) if agg == "MAX" else None
    issuers, info = {}, {}
    for name, seg_len in SEG_LENS.items():
        plan = ops.agg_full_plan(graph, seg_len=seg_len)
        tplan = plan.transposed()
        ws = torch.empty(max(16, 2 * plan.n_slots * F * 4, tplan.n_slots * F * 4), dtype=torch.uint8, device=dev)
        info[name] = {"forward": {"items": plan.n_items, "split_rows": plan.n_split, "partial_slots": plan.n_slots},
                      "transposed": {"items": tplan.n_items, "split_rows": tplan.n_split,
                                     "partial_slots": tplan.n_slots}}
        issuers[f"fwd_seg_{name}"] = lambda plan=plan, ws=ws: ops.agg_full(agg, Hs, plan, out, ws=ws)
        if agg == "MAX":
            issuers[f"fwd_argmax_seg_{name}"] = lambda plan=plan, ws=ws: ops.agg_full(agg, Hs, plan, out, ws=ws,
                                                                                      argmax=am)
        issuers[f"bwd_seg_{name}"] = lambda t=tplan, ws=ws: ops.agg_full_bwd(agg, dA, t, dH, argmax=am, ws=ws)
        issuers[f"bwd_epilogue_seg_{name}"] = lambda t=tplan, ws=ws: ops.agg_full_bwd(agg, dA, t, dH, argmax=am, ws=ws,
                                                                                      dSelf=dS, Hprev=Hs)
    if agg == "MAX":
        issuers["fwd_argmax_seg_256"]()                      # the argmax the backward variants read
    times = fib.rounds_of(issuers, rounds, reps)
    row = F * 4
    nbytes = {"fwd": (entries + n) * row, "fwd_argmax": (entries + 2 * n) * row,
              "bwd": (entries * (2 if agg == "MAX" else 1) + n) * row}
    nbytes["bwd_epilogue"] = nbytes["bwd"] + 2 * n * row
    res = {}
    for k, v in times.items():
        kind = k[:k.index("_seg_")]
        res[k] = fib.summary({k: v}, nbytes[kind])[k]
    return {"n": n, "entries": entries, "F": F, "agg": agg, "algorithmic_bytes": nbytes, "plans": info,
            "timings": res}


def bench_step(graph, X, labels, nodes, agg, rounds, dev):
    n, F = X.shape
    trs = {"cache_on": train.FullTrainer(graph, X, labels, 16, hidden=H, agg_func=agg, lr=0.01, cache_agg1=True),
           "cache_off": train.FullTrainer(graph, X, labels, 16, hidden=H, agg_func=agg, lr=0.01, cache_agg1=False)}
    a = trs["cache_on"]
    emb = train.FullEmbedder(graph, X, [w.clone() for w in a.weights()], agg_func=agg, seg_len=a.plan.seg_len)
    for t in trs.values():
        t.step(nodes)                                        # validates `nodes` once, fills the cache
    issuers = {f"step_{k}": (lambda t=t: t.step(nodes)) for k, t in trs.items()}
    b = trs["cache_off"]
    issuers["forward_cache_on"] = lambda: a.forward_backward(nodes, _lib.GS_TF_FORWARD)
    issuers["forward_cache_off"] = lambda: b.forward_backward(nodes, _lib.GS_TF_FORWARD)
    issuers["head"] = lambda: a.forward_backward(nodes, _lib.GS_TF_HEAD)
    issuers["backward"] = lambda: a.forward_backward(nodes, _lib.GS_TF_BACKWARD)
    issuers["update"] = a.apply_update
    issuers["full_embedder_embed"] = emb.embed
    res = fib.summary(fib.rounds_of(issuers, rounds, 1))
    ms = {k: round(v["us_median"] / 1e3, 3) for k, v in res.items()}
    return {"n": n, "F": F, "hidden": H, "layers": 2, "agg": agg, "classes": 16, "loss_nodes": int(nodes.numel()),
            "seg_len": a.plan.seg_len, "ws_bytes": a.ws_bytes, "ms": ms,
            "cache_agg1_saving_ms": round(ms["step_cache_off"] - ms["step_cache_on"], 3),
            "step_over_embed": round(ms["step_cache_on"] / ms["full_embedder_embed"], 3),
            "loss": float(a.loss), "timings": res}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scale", type=int, default=21)
    ap.add_argument("--pairs", type=int, default=20_000_000)
    ap.add_argument("--feat", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5, help="alternating rounds")
    ap.add_argument("--reps", type=int, default=3, help="aggregate calls per round and variant")
    ap.add_argument("--sections", default="aggregate,step", help="comma list of: aggregate, step")
    ap.add_argument("--aggs", default="MEAN,MAX", help="comma list of: MEAN, MAX")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("full_train_bench needs a HIP device")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    n = 1 << args.scale
    src, dst = gs.rmat_pairs(args.scale, args.pairs, seed=SEED, n_threads=16)
    deg = gs.CSRGraph.from_pairs(src, dst, n, n_threads=16).degrees()
    lone = np.nonzero(deg == 0)[0].astype(np.int64)
    graph = gs.CSRGraph.from_pairs(np.concatenate([src, lone]), np.concatenate([dst, (lone + 1) % n]), n,
                                   n_threads=16)
    note(f"graph built: {n} nodes, {graph.n_entries} entries, {len(lone)} nodes given an edge")
    res = {"graph": {"scale": args.scale, "pairs": args.pairs, "n": n, "entries": graph.n_entries,
                     "max_degree": graph.max_degree, "edges_added_for_nodes_without_one": int(len(lone))},
           "rounds": args.rounds, "reps": args.reps, "hbm_peak": fib.HBM_PEAK}
    sections, aggs = args.sections.split(","), args.aggs.split(",")
    for agg in aggs if "aggregate" in sections else ():
        res[f"aggregate_{agg.lower()}"] = bench_aggregate(graph, agg, args.rounds, args.reps, dev)
        note(f"aggregate {agg} done")
    X = torch.empty(n, args.feat, dtype=torch.float32, device=dev)
    ops.fill_uniform(X, SEED)
    rs = np.random.RandomState(SEED)
    labels = torch.from_numpy(rs.randint(0, 16, n))
    nodes = torch.from_numpy(rs.permutation(n)[:n // 2].astype(np.int32)).to(dev)
    for agg in aggs if "step" in sections else ():
        res[f"step_{agg.lower()}"] = bench_step(graph, X, labels, nodes, agg, args.rounds, dev)
        note(f"step {agg} done")
        torch.cuda.empty_cache()
    text = json.dumps(res, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
