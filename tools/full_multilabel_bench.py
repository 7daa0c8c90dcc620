#!/usr/bin/env python3
"""Measure the multi-label (sigmoid BCE) head of the exact path on rmat2m
("Multi-label head"), in one process, after warm-up, medians and
ranges of alternating rounds, HIP events.

The graph and the model are tools/full_train_bench.py's (rmat2m plus one edge
per node without one; 2 layers, hidden 128, fp32, MEAN).

  1. The head alone at PPI's width, D = 128 and C = 121, over B = 512, 32,768
     and 1,048,576 rows of H_L in random order:
       head        E = H_L.index_select(ids), then hip_ops.cls_bce (loss, dE,
                   dWc, dbc; targets as packed bits read by node id)
       torch_head  the same on the same GPU in the same run: index_select,
                   addmm, binary_cross_entropy_with_logits (pos_weight, mean),
                   backward to E, Wc and bc; its float targets [B, C] are
                   gathered outside the timed region
     The two results are compared once per size.
  2. FullTrainer's head stage (stages=GS_TF_HEAD: gather, head, memset,
     scatter) with head="multilabel" against head="nll" at C = 16, same sizes.

    python tools/full_multilabel_bench.py --out profiles/full_multilabel_bench.json

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
import torch.nn.functional as F  # noqa: E402

gs = import_module("graphsage-pytorch_amd")
train = import_module("graphsage-pytorch_amd.train")
ops = import_module("graphsage-pytorch_amd.hip_ops")
_lib = import_module("graphsage-pytorch_amd._lib")
fib = import_module("tools.full_infer_bench")

SEED, H, C_HEAD, C_STEP = 824, 128, 121, 16
SIZES = [512, 32768, 1048576]


def note(msg):
    print(f"[full_multilabel_bench] {msg}", file=sys.stderr, flush=True)


def timed(issuers, rounds):
    for issue, _r in issuers.values():
        issue()
    times = {k: [] for k in issuers}
    for _ in range(rounds):
        for k, (issue, reps) in issuers.items():
            issue()   # an untimed call first: a window that follows a lighter variant otherwise starts at idle clocks
            times[k].append(round(fib.ms_per_call(issue, reps), 5))
    res = fib.summary(times)
    for k, v in res.items():
        v["ms_min"], v["ms_max"], v["calls_per_timing"] = min(times[k]), max(times[k]), issuers[k][1]
    return res


def compare(res, a, b):
    x, y = res[a], res[b]
    return {f"{a}_over_{b}": round(x["us_median"] / y["us_median"], 4),
            f"{a}_not_slower_than_{b}": x["us_median"] <= y["us_median"],
            "ranges_overlap": not (x["ms_max"] < y["ms_min"] or y["ms_max"] < x["ms_min"])}


def bench_head(HL, Y, words, Wc, bc, pw, nodes, rounds):
    B = int(nodes.numel())
    ids = nodes.long()
    yf = Y.index_select(0, ids).float()          # torch's targets, gathered outside the timed region
    Wt, bt = Wc.clone().requires_grad_(True), bc.clone().requires_grad_(True)

    def head():
        return ops.cls_bce(HL.index_select(0, ids), Wc, bc, words, roots=nodes, pos_weight=pw)

    def torch_head():
        E = HL.index_select(0, ids).requires_grad_(True)
        Wt.grad = bt.grad = None
        loss = F.binary_cross_entropy_with_logits(torch.addmm(bt, E, Wt.t()), yf, pos_weight=pw, reduction="mean")
        loss.backward()
        return loss.detach(), E.grad, Wt.grad, bt.grad

    a, b = head(), torch_head()
    torch.cuda.synchronize()
    agree = {"loss": float(a[0]), "torch_loss": float(b[0])}
    for name, u, v in zip(("dE", "dWc", "dbc"), a[1:], b[1:]):
        agree[f"{name}_max_abs_diff"] = float((u - v).abs().max())
        agree[f"{name}_max_abs"] = float(v.abs().max())
    reps = max(2, min(200, (1 << 21) // B))
    res = timed({"head": (head, reps), "torch_head": (torch_head, reps)}, rounds)
    flop = 3 * 2.0 * B * H * C_HEAD
    out = {"B": B, "D": H, "C": C_HEAD, "timings": res, "agreement": agree,
           "head_tflops": round(flop / (res["head"]["us_median"] * 1e-6) / 1e12, 3)}
    out.update(compare(res, "head", "torch_head"))
    return out


def bench_step_head(tr_ml, tr_nll, nodes, rounds):
    B = int(nodes.numel())
    for tr in (tr_ml, tr_nll):
        tr.forward_backward(nodes)               # validates `nodes`; H_L is in place from here on
    reps = max(2, min(100, (1 << 19) // B))
    res = timed({"multilabel": (lambda: tr_ml.forward_backward(nodes, _lib.GS_TF_HEAD), reps),
                 "nll": (lambda: tr_nll.forward_backward(nodes, _lib.GS_TF_HEAD), reps)}, rounds)
    out = {"B": B, "C": C_STEP, "timings": res}
    out.update(compare(res, "multilabel", "nll"))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scale", type=int, default=21)
    ap.add_argument("--pairs", type=int, default=20_000_000)
    ap.add_argument("--feat", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5, help="alternating rounds (five or more)")
    ap.add_argument("--sizes", default=",".join(map(str, SIZES)), help="comma list of row counts")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("full_multilabel_bench needs a HIP device")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    n = 1 << args.scale
    src, dst = gs.rmat_pairs(args.scale, args.pairs, seed=SEED, n_threads=16)
    deg = gs.CSRGraph.from_pairs(src, dst, n, n_threads=16).degrees()
    lone = np.nonzero(deg == 0)[0].astype(np.int64)
    graph = gs.CSRGraph.from_pairs(np.concatenate([src, lone]), np.concatenate([dst, (lone + 1) % n]), n,
                                   n_threads=16)
    note(f"graph built: {n} nodes, {graph.n_entries} entries")
    X = torch.empty(n, args.feat, dtype=torch.float32, device=dev)
    ops.fill_uniform(X, SEED)
    rs = np.random.RandomState(SEED)
    perm = rs.permutation(n).astype(np.int32)
    gen = torch.Generator(device=dev).manual_seed(SEED)
    tr_nll = train.FullTrainer(graph, X, torch.from_numpy(rs.randint(0, C_STEP, n)), C_STEP, hidden=H,
                               agg_func="MEAN", lr=0.01)
    Y16 = torch.rand(n, C_STEP, device=dev, generator=gen) < 0.3
    tr_ml = train.FullTrainer(graph, X, Y16, C_STEP, hidden=H, agg_func="MEAN", lr=0.01, head="multilabel")
    note("trainers built")
    half = torch.from_numpy(perm[:n // 2]).to(dev)
    tr_nll.step(half)                                         # parameters one step off their initial values
    tr_ml.step(half)
    # the head alone at PPI's width over the rows of H_L
    HL = tr_nll.hidden().clone()
    Y = torch.rand(n, C_HEAD, device=dev, generator=gen) < 0.3
    words = ops.pack_multilabel(Y)
    bound = float(np.sqrt(6.0 / (C_HEAD + H)))
    Wc = (torch.rand(C_HEAD, H, device=dev, generator=gen) * 2 - 1) * bound
    bc = (torch.rand(C_HEAD, device=dev, generator=gen) * 2 - 1) * 0.1
    pw = torch.rand(C_HEAD, device=dev, generator=gen) * 3.5 + 0.5
    res = {"graph": {"scale": args.scale, "pairs": args.pairs, "n": n, "entries": graph.n_entries},
           "model": {"layers": 2, "hidden": H, "F": args.feat, "agg": "MEAN"},
           "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "head": {}, "step_head": {}}
    for B in (int(s) for s in args.sizes.split(",")):
        nodes = torch.from_numpy(perm[:B].copy()).to(dev)
        res["head"][str(B)] = bench_head(HL, Y, words, Wc, bc, pw, nodes, args.rounds)
        res["step_head"][str(B)] = bench_step_head(tr_ml, tr_nll, nodes, args.rounds)
        note(f"B = {B} done")
    text = json.dumps(res, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
