#!/usr/bin/env python3
"""Measure the evaluation head of the exact path on rmat2m (DESIGN §4,
"Evaluation head"), in one process, after warm-up, medians and ranges of
alternating rounds, HIP events.

The graph and the model are tools/full_train_bench.py's (rmat2m plus one edge
per node without one; 2 layers, hidden 128, 16 classes, fp32, MEAN).  At
B = 512, 32,768 and 1,048,576 evaluated nodes:

  head            hip_ops.cls_eval over H_L[nodes] alone (the forward's H_L
                  is in place): loss, predictions and the confusion matrix
  head_sorted_ids, head_first_rows
                  the same head over the same ids in ascending order, and over
                  the first B rows of H_L without an id vector: what the random
                  order of the gather costs
  torch_head      the same result the only way the library could give it
                  before: hidden().index_select, @ Wc.T + bc, log_softmax,
                  argmax, the gathered NLL mean and a bincount confusion matrix
  evaluate        FullTrainer.evaluate as a whole (forward stage + head)
  torch_evaluate  the forward stage, then torch_head
  step_head       for context, the training step's GS_TF_HEAD stage (gather,
                  memset, forward + backward head, scatter)

and the head's byte floor B·D·4 bytes at the 8 TB/s HBM peak with the fraction
of it the head achieves.  The two heads' results are compared once per size
(equal predictions, loss difference).

    python tools/full_eval_bench.py --out profiles/full_eval_bench.json

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

SEED, H, C = 824, 128, 16
SIZES = [512, 32768, 1048576]


def note(msg):
    print(f"[full_eval_bench] {msg}", file=sys.stderr, flush=True)


def bench_size(tr, nodes, rounds):
    B = int(nodes.numel())
    head_p = tr.p.params[int(tr.p.offsets[tr.L]):]
    Wc, bc = tr.p.view(tr.L), tr.p.view(tr.L + 1)
    ids = nodes.long()
    labels = tr.labels.long()

    def forward():
        tr._forward_backward(nodes, _lib.GS_TF_FORWARD, None)

    def head():
        return ops.cls_eval(tr.hidden(), tr.labels, head_p, C, rows=nodes)

    def torch_head():
        E = tr.hidden().index_select(0, ids)
        z = E @ Wc.t() + bc
        logp = torch.log_softmax(z, 1)
        pred = z.argmax(1)
        y = labels.index_select(0, ids)
        loss = -logp.gather(1, y[:, None]).mean()
        return loss, torch.bincount(y * C + pred, minlength=C * C), pred

    def torch_evaluate():
        forward()
        return torch_head()

    tr.evaluate(nodes)                                       # validates `nodes` once; H_L is in place from here on
    loss, counts, pred, _ = head()
    tl, tconf, tpred = torch_head()
    torch.cuda.synchronize()
    agree = {"pred_equal_fraction": float((pred[0].long() == tpred).double().mean()),
             "loss": float(loss[0]), "torch_loss": float(tl),
             "confusion_equal": bool(torch.equal(counts[0, :C * C], tconf))}
    # calls per timing: enough work per window at the small sizes
    reps_head = max(2, min(200, (1 << 22) // B))
    # where the head's time goes: the same rows in ascending id order, and the first B rows without an id vector
    sorted_nodes = torch.sort(nodes).values
    issuers = {"head": (head, reps_head), "torch_head": (torch_head, reps_head),
               "head_sorted_ids": (lambda: ops.cls_eval(tr.hidden(), tr.labels, head_p, C, rows=sorted_nodes),
                                   reps_head),
               "head_first_rows": (lambda: ops.cls_eval(tr.hidden()[:B], tr.labels, head_p, C), reps_head),
               "evaluate": (lambda: tr.evaluate(nodes), 2), "torch_evaluate": (torch_evaluate, 2),
               "step_head": (lambda: tr.forward_backward(nodes, _lib.GS_TF_HEAD), max(2, reps_head // 8))}
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
    floor_ms = B * H * 4 / fib.HBM_PEAK * 1e3
    hm, tm = res["head"], res["torch_head"]
    em, tem = res["evaluate"], res["torch_evaluate"]
    return {"B": B, "timings": res, "agreement": agree,
            "head_byte_floor_ms": round(floor_ms, 5),
            "head_fraction_of_floor": round(floor_ms / (hm["us_median"] / 1e3), 4),
            "head_over_torch_head": round(hm["us_median"] / tm["us_median"], 4),
            "head_not_slower_than_torch_head": hm["us_median"] <= tm["us_median"],
            "head_ranges_overlap": not (hm["ms_max"] < tm["ms_min"] or tm["ms_max"] < hm["ms_min"]),
            "evaluate_over_torch_evaluate": round(em["us_median"] / tem["us_median"], 4),
            "evaluate_not_slower_than_torch_evaluate": em["us_median"] <= tem["us_median"],
            "evaluate_ranges_overlap": not (em["ms_max"] < tem["ms_min"] or tem["ms_max"] < em["ms_min"])}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scale", type=int, default=21)
    ap.add_argument("--pairs", type=int, default=20_000_000)
    ap.add_argument("--feat", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5, help="alternating rounds")
    ap.add_argument("--sizes", default=",".join(map(str, SIZES)), help="comma list of evaluated-node counts")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("full_eval_bench needs a HIP device")
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
    labels = torch.from_numpy(rs.randint(0, C, n))
    perm = rs.permutation(n).astype(np.int32)
    tr = train.FullTrainer(graph, X, labels, C, hidden=H, agg_func="MEAN", lr=0.01)
    tr.step(torch.from_numpy(perm[:n // 2]).to(dev))         # parameters one step off their initial values
    res = {"graph": {"scale": args.scale, "pairs": args.pairs, "n": n, "entries": graph.n_entries},
           "model": {"layers": 2, "hidden": H, "classes": C, "F": args.feat, "agg": "MEAN"},
           "rounds": args.rounds, "hbm_peak": fib.HBM_PEAK, "sizes": {}}
    for B in (int(s) for s in args.sizes.split(",")):
        res["sizes"][str(B)] = bench_size(tr, torch.from_numpy(perm[:B].copy()).to(dev), args.rounds)
        note(f"B = {B} done")
    text = json.dumps(res, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
