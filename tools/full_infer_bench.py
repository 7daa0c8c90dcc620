#!/usr/bin/env python3
"""Measure exact full-neighbourhood inference on rmat2m ("Exact
full-neighbourhood inference"), in one process, after warm-up, medians of
alternating rounds:

  aggregate   hip_ops.agg_full over all rows of the feature table for seg_len
              in {64, 128, 256, 1024, no split}, against the existing kernel doing
              the same job: gs_agg_fwd in expand mode with ptr = the int32 row
              pointer, idx = the identity over absolute entries and dst_ids =
              arange (the entry count fits int32 at this size).  HIP events
              around --reps calls; us per call and the fraction of the 8 TB/s
              HBM peak against the algorithmic bytes (entries * F * b +
              N * F * b).  Two configurations: F = 256 fp32 MEAN on rmat2m as
              built, and bf16 MAX on rmat2m plus one edge (v, v + 1) for every
              node without an edge, because MAX refuses an empty neighbourhood.
  inference   train.FullEmbedder (2 layers, hidden 128, fp32 MEAN) for
              chunk_rows in {16384, 65536, 262144, N} at the default seg_len,
              and for each seg_len at one chunk (one plan serves both layers,
              whose rows are 1 KiB and 512 B): ms per embed() and nodes/s; per
              layer, the aggregate calls and the GEMM calls of
              all chunks timed as two separate passes (so their sum leaves out
              what the interleaved driver gains or loses in cache); and the
              sampled train.Embedder's node rate (fanouts 25, 10; 12 sampler
              streams) from the same run.

    python tools/full_infer_bench.py --out profiles/full_infer_bench.json

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

SEED, H, HBM_PEAK = 824, 128, 8.0e12
SEG_LENS = {"64": 64, "128": 128, "256": 256, "1024": 1024, "no_split": 0}


def ms_per_call(issue, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        issue()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def rounds_of(issuers, rounds, reps):
    """{name: [ms per call, one per round]}, the variants alternating inside each round."""
    for issue in issuers.values():
        issue()  # warm-up: code objects, plans, workspaces
    out = {k: [] for k in issuers}
    for _ in range(rounds):
        for k, issue in issuers.items():
            out[k].append(round(ms_per_call(issue, reps), 4))
    return out


def summary(times, nbytes=None):
    out = {}
    for k, v in times.items():
        med = float(np.median(v))
        out[k] = {"ms_rounds": v, "us_median": round(1e3 * med, 1), "spread": round((max(v) - min(v)) / med, 4)}
        if nbytes:
            out[k]["hbm_peak_fraction"] = round(nbytes / (med * 1e-3) / HBM_PEAK, 4)
    return out


def bench_aggregate(graph, X, agg, rounds, reps):
    n, F = X.shape
    dev = X.device
    rp = graph.row_ptr()
    entries = int(rp[-1])
    assert entries < 2 ** 31
    ptr32 = torch.from_numpy(rp.astype(np.int32)).to(dev)
    ident = torch.arange(entries, dtype=torch.int32, device=dev)
    dst = torch.arange(n, dtype=torch.int32, device=dev)
    _rp_d, col_d = graph.device_csr(dev)
    out = torch.empty_like(X)
    issuers = {"baseline_agg_fwd": lambda: ops.agg_fwd(agg, X, ptr32, ident, out, col=col_d, dst_ids=dst)}
    info = {}
    for name, seg_len in SEG_LENS.items():
        plan = ops.agg_full_plan(graph, seg_len=seg_len)
        need = max(16, plan.n_slots * F * 4)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        info[name] = {"items": plan.n_items, "split_rows": plan.n_split, "partial_slots": plan.n_slots}
        issuers[f"agg_full_seg_{name}"] = lambda plan=plan, ws=ws: ops.agg_full(agg, X, plan, out, ws=ws)
    # the results agree before anything is timed (MAX: bitwise; MEAN: the split changes the order of the sum)
    ref = issuers["baseline_agg_fwd"]().clone()
    for k, issue in issuers.items():
        got = issue()
        same = torch.equal(torch.nan_to_num(got.float(), nan=-7.0), torch.nan_to_num(ref.float(), nan=-7.0))
        err = float(torch.nan_to_num((got.float() - ref.float()).abs(), nan=0.0).max())
        info.setdefault(k.replace("agg_full_seg_", ""), {}).update({"bitwise_baseline": same, "max_abs_diff": err})
        assert same or (agg == "MEAN" and err < 1e-4), (k, err)
    nbytes = (entries + n) * F * X.element_size()
    res = summary(rounds_of(issuers, rounds, reps), nbytes)
    return {"n": n, "entries": entries, "F": F, "dtype": str(X.dtype), "agg": agg, "algorithmic_bytes": nbytes,
            "max_degree": graph.max_degree, "plans": info, "timings": res}


def bench_inference(graph, X, weights, chunks, rounds, streams, sampled_nodes):
    n, F = X.shape
    dev = X.device
    out = {"n": n, "F": F, "hidden": H, "layers": len(weights), "seg_len": ops.FULL_SEG_LEN, "chunk_rows": {}}
    embs = {str(c): train.FullEmbedder(graph, X, weights, chunk_rows=c) for c in chunks}
    total = summary(rounds_of({k: e.embed for k, e in embs.items()}, rounds, 1))
    plan = ops.agg_full_plan(graph)
    H1 = train.FullEmbedder(graph, X, weights[:1]).embed()
    ws = torch.empty(max(16, plan.n_slots * max(F, H) * 4), dtype=torch.uint8, device=dev)
    for c in chunks:
        A = torch.empty(min(c, n), max(F, H), dtype=torch.float32, device=dev)
        Hout = torch.empty(n, H, dtype=torch.float32, device=dev)
        passes = {}
        for l, (src, W) in enumerate(((X, weights[0]), (H1, weights[1])), 1):
            w = src.shape[1]

            def agg_pass(src=src, w=w):
                for r0 in range(0, n, c):
                    m = min(c, n - r0)
                    ops.agg_full("MEAN", src, plan, A[:m, :w], row0=r0, n_rows=m, ws=ws)

            def gemm_pass(src=src, w=w, W=W):
                for r0 in range(0, n, c):
                    m = min(c, n - r0)
                    ops.sage_linear_fwd(A[:m, :w], W, Hout[r0:r0 + m], Xs=src[r0:r0 + m])

            passes[f"layer{l}_aggregate"] = agg_pass
            passes[f"layer{l}_gemm"] = gemm_pass
        parts = summary(rounds_of(passes, rounds, 1))
        med = total[str(c)]["us_median"] * 1e-6
        out["chunk_rows"][str(c)] = {"embed": total[str(c)], "nodes_per_s": round(n / med),
                                     "ms_separate_passes": {k: round(v["us_median"] / 1e3, 3)
                                                            for k, v in parts.items()},
                                     "separate_passes": parts}
    by_seg = {k: train.FullEmbedder(graph, X, weights, seg_len=v, chunk_rows=n) for k, v in SEG_LENS.items()}
    out["seg_len_at_one_chunk"] = summary(rounds_of({k: e.embed for k, e in by_seg.items()}, rounds, 1))
    del by_seg
    # the sampled embedder on the same graph, features and weights
    emb = train.Embedder(graph, X, weights, (25, 10), "MEAN")
    ids = np.arange(min(n, sampled_nodes), dtype=np.int64)
    emb.embed(ids[:20000], 500, [train.make_rng(SEED + 1, 0, w) for w in range(streams)])
    rates = []
    for r in range(min(rounds, 3)):
        rngs = [train.make_rng(SEED + 2 + r, 0, w) for w in range(streams)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        emb.embed(ids, 500, rngs)
        torch.cuda.synchronize()
        rates.append(round(len(ids) / (time.perf_counter() - t0)))
    out["sampled_embedder"] = {"nodes": len(ids), "batch": 500, "fanouts": [25, 10], "sampler_streams": streams,
                               "nodes_per_s_rounds": rates, "nodes_per_s": float(np.median(rates))}
    return out


def note(msg):
    print(f"[full_infer_bench] {msg}", file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scale", type=int, default=21)
    ap.add_argument("--pairs", type=int, default=20_000_000)
    ap.add_argument("--feat", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5, help="alternating rounds")
    ap.add_argument("--reps", type=int, default=3, help="aggregate calls per round and variant")
    ap.add_argument("--streams", type=int, default=12)
    ap.add_argument("--sampled-nodes", type=int, default=400_000)
    ap.add_argument("--skip-max", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("full_infer_bench needs a HIP device")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    n = 1 << args.scale
    src, dst = gs.rmat_pairs(args.scale, args.pairs, seed=SEED, n_threads=16)
    graph = gs.CSRGraph.from_pairs(src, dst, n, n_threads=16)
    deg = graph.degrees()
    note(f"graph built: {n} nodes, {graph.n_entries} entries")
    X = torch.empty(n, args.feat, dtype=torch.float32, device=dev)
    ops.fill_uniform(X, SEED)
    weights = [w.to(dev) for w in train.reference_init(2, args.feat, H, 16, False, SEED)[0]]
    res = {"graph": {"scale": args.scale, "pairs": args.pairs, "n": n, "entries": graph.n_entries,
                     "max_degree": graph.max_degree, "nodes_without_edge": int((deg == 0).sum()),
                     "rows_longer_than": {str(k): int((deg > k).sum()) for k in (64, 256, 1024)}},
           "rounds": args.rounds, "reps": args.reps}
    res["aggregate_fp32_mean"] = bench_aggregate(graph, X, "MEAN", args.rounds, args.reps)
    note("aggregate fp32 MEAN done")
    chunks = sorted({c for c in (16384, 65536, 262144) if c < n} | {n})
    res["inference_fp32_mean"] = bench_inference(graph, X, weights, chunks, args.rounds, args.streams,
                                                 args.sampled_nodes)
    note("inference done")
    if not args.skip_max:
        del graph
        lone = np.nonzero(deg == 0)[0].astype(np.int64)
        g2 = gs.CSRGraph.from_pairs(np.concatenate([src, lone]), np.concatenate([dst, (lone + 1) % n]), n,
                                    n_threads=16)
        Xb = X.to(torch.bfloat16)
        del X
        res["aggregate_bf16_max"] = bench_aggregate(g2, Xb, "MAX", args.rounds, args.reps)
        res["aggregate_bf16_max"]["graph"] = f"rmat2m plus one edge (v, v + 1) for each of {len(lone)} nodes without one"
    text = json.dumps(res, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
