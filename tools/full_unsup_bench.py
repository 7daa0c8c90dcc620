#!/usr/bin/env python3
"""Measure the exact step under the unsupervised losses (FullTrainer.unsup_step,
DESIGN §4 "The unsupervised losses on the exact path") next to the module
path's utils.train_step and the supervised field step, in one process, after
warm-up, medians of alternating rounds.

Two configurations, each with batches of 512 training ids:

  pubmed   the golden Pubmed graph with test_gpu_pubmed.py's inputs: F = 500
           uniform features, hidden 128, 2 layers, 3 classes, fp32 MEAN, SGD
  rmat2m   tools/full_field_bench.py's graph (scale 21, 20 M pairs, one edge for
           every node without one), F = 256, hidden 128, 2 layers, 16 classes;
           the training set is the first 2^17 ids of a fixed permutation

Per configuration and variant (normal / margin x unsup / plus_unsup) every
round extends a fresh batch (extend_nodes draws from a seeded `random`), so
the exact step and the module step see batches from the same distribution but
not the same batch; the rounds alternate the variants.  Recorded per variant:

  step_ms          host clock around unsup_step (extend, plan, field build,
                   forward, head, backward, update) ending in a synchronise
  extend_ms        host clock around extend_nodes_array alone
  plan_ms          host clock around unsup_batch (plan build + upload)
  field_ms         host clock around FullTrainer.field (it synchronises)
  forward_ms, head_ms, backward_ms, update_ms
                   HIP events around the stages of the same batch, issued
                   stage by stage on a field that is kept
  sizes            n_L .. n_0 of the last batch's field, U and the plan's dims
  module_ms        host clock around utils.train_step (GraphSage module,
                   fanouts 10, 10, autograd, torch SGD) ending in a synchronise
  sup_field_ms     FullTrainer: extend, field, supervised step over the
                   extended batch, as apply_model_full's "sup" does

    python tools/full_unsup_bench.py --configs pubmed --out profiles/full_unsup_bench.json

Needs the GPU: there is no CPU path.  A measurement tool, not bench.py; it
asserts nothing about speed."""
import argparse
import json
import os
import random
import sys
import time
from importlib import import_module

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

gs = import_module("graphsage-pytorch_amd")
train = import_module("graphsage-pytorch_amd.train")
models = import_module("graphsage-pytorch_amd.models")
unsup = import_module("graphsage-pytorch_amd.unsup")
utils = import_module("graphsage-pytorch_amd.utils")
ops = import_module("graphsage-pytorch_amd.hip_ops")
_lib = import_module("graphsage-pytorch_amd._lib")

SEED, H, LAYERS, B = 824, 128, 2, 512
NUM_NEG = {"normal": 100, "margin": 6}
VARIANTS = [(k, m) for k in ("normal", "margin") for m in ("unsup", "plus_unsup")]


def note(msg):
    print(f"[full_unsup_bench] {msg}", file=sys.stderr, flush=True)


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def pubmed(dev):
    g = np.load(os.path.join(ROOT, "tests", "golden", "graphs.npz"))
    src, dst, n = g["pubmed_src"].astype(np.int64), g["pubmed_dst"].astype(np.int64), int(g["pubmed_n"][0])
    graph = gs.CSRGraph.from_pairs(src, dst, n)
    X = torch.empty(n, 500, dtype=torch.float32, device=dev)
    ops.fill_uniform(X, SEED)
    perm = np.random.RandomState(SEED).permutation(n)
    return graph, n, X, perm[n // 3 + n // 6:], (np.arange(n) % 3).astype(np.int64), 3, {}


def rmat2m(dev, scale=21, pairs=20_000_000):
    n = 1 << scale
    src, dst = gs.rmat_pairs(scale, pairs, seed=SEED, n_threads=16)
    deg = gs.CSRGraph.from_pairs(src, dst, n, n_threads=16).degrees()
    lone = np.nonzero(deg == 0)[0].astype(np.int64)
    graph = gs.CSRGraph.from_pairs(np.concatenate([src, lone]), np.concatenate([dst, (lone + 1) % n]), n,
                                   n_threads=16)
    X = torch.empty(n, 256, dtype=torch.float32, device=dev)
    ops.fill_uniform(X, SEED)
    rs = np.random.RandomState(SEED)
    labels = rs.randint(0, 16, n).astype(np.int64)
    train_ids = rs.permutation(n)[:1 << 17].astype(np.int64)
    return graph, n, X, train_ids, labels, 16, {"scale": scale, "pairs": pairs,
                                                "edges_added_for_nodes_without_one": int(len(lone))}


def measure(name, dev, rounds, with_module):
    graph, n, X, train_ids, labels, C, extra = {"pubmed": pubmed, "rmat2m": rmat2m}[name](dev)
    note(f"{name}: {n} nodes, {graph.n_entries} entries, {len(train_ids)} training ids")
    F = X.shape[1]
    tr = train.FullTrainer(graph, X, torch.from_numpy(labels), C, num_layers=LAYERS, hidden=H, agg_func="MEAN",
                           lr=0.01, seed=SEED)
    ul = unsup.UnsupervisedLoss(graph, train_ids, dev)
    order = np.random.RandomState(SEED + 1).permutation(train_ids)
    n_batches = len(order) // B
    cursor = [0]

    def next_batch():
        cursor[0] = (cursor[0] + 1) % n_batches
        return order[cursor[0] * B:(cursor[0] + 1) * B]

    random.seed(SEED)
    res = {"graph": dict(extra, n=n, entries=int(graph.n_entries), train_ids=int(len(train_ids))), "F": F,
           "hidden": H, "layers": LAYERS, "classes": C, "batch": B, "rounds": rounds, "ws_bytes": tr.ws_bytes,
           "variants": {}}
    issuers = {}
    for kind, method in VARIANTS:
        issuers[f"{kind}/{method}"] = (lambda kind=kind, method=method:
                                       tr.unsup_step(ul, next_batch(), unsup_loss=kind, learn_method=method))
    sup_field = [None]

    def sup_step():
        ids = tr._nodes(ul.extend_nodes_array(next_batch(), num_neg=100))
        sup_field[0] = tr.field(ids, out=sup_field[0])
        tr.step(ids, field=sup_field[0])

    issuers["sup_field"] = sup_step
    if with_module:
        torch.manual_seed(SEED)
        gsage = models.GraphSage(LAYERS, F, H, X, graph, dev, agg_func="MEAN", fanouts=[10, 10]).to(dev)
        cls = models.Classification(H, C).to(dev)
        opt = torch.optim.SGD([p for m in (gsage, cls) for p in m.parameters()], lr=0.01)
        for kind, method in VARIANTS:
            fn = {"normal": ul.get_loss_sage, "margin": ul.get_loss_margin}[kind]
            issuers[f"module {kind}/{method}"] = (
                lambda kind=kind, method=method, fn=fn:
                utils.train_step(gsage, cls, ul, opt, next_batch(), labels, NUM_NEG[kind], method, fn))
    for k, issue in issuers.items():                    # warm-up: code objects, workspaces, plans
        for _ in range(2):
            issue()
        note(f"{name}: warmed {k}")
    times = {k: [] for k in issuers}
    for _ in range(rounds):
        for k, issue in issuers.items():
            times[k].append(round(host_ms(issue)[0], 4))
    # the split of the exact step, stage by stage on one batch
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
    for kind, method in VARIANTS:
        split = {k: [] for k in ("extend_ms", "plan_ms", "field_ms", "forward_ms", "head_ms", "backward_ms",
                                 "update_ms")}
        field = batch = None
        for r in range(rounds + 1):
            ids = next_batch()
            t_ext, _ = host_ms(lambda: ul.extend_nodes_array(ids, num_neg=NUM_NEG[kind]))
            t_plan, batch = host_ms(lambda: tr.unsup_batch(ul, kind=kind, learn_method=method))
            t_field, field = host_ms(lambda: tr.field(batch.nodes, out=field))
            ev[0].record()
            for i, st in enumerate((_lib.GS_TF_FORWARD, _lib.GS_TF_HEAD, _lib.GS_TF_BACKWARD)):
                tr.forward_backward(batch.nodes, stages=st, field=field, unsup=batch)
                ev[i + 1].record()
            tr.apply_update()
            ev[4].record()
            torch.cuda.synchronize()
            if r == 0:
                continue                                 # the first round warms the staged calls
            for key, v in zip(split, (t_ext, t_plan, t_field, ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2]),
                                      ev[2].elapsed_time(ev[3]), ev[3].elapsed_time(ev[4]))):
                split[key].append(round(float(v), 4))
        key = f"{kind}/{method}"
        row = {"step_ms": round(float(np.median(times[key])), 3), "step_ms_rounds": times[key],
               "sizes": list(field.sizes), "U": int(batch.nodes.numel()), "dims": list(batch.dims),
               "loss_parts": [float(x) for x in tr.loss_parts()]}
        row.update({k: round(float(np.median(v)), 3) for k, v in split.items()})
        if with_module:
            mk = f"module {key}"
            row["module_ms"] = round(float(np.median(times[mk])), 3)
            row["module_ms_rounds"] = times[mk]
            row["module_over_exact"] = round(row["module_ms"] / row["step_ms"], 2)
        res["variants"][key] = row
        note(f"{name} {key}: {row}")
    res["sup_field_ms"] = round(float(np.median(times["sup_field"])), 3)
    res["sup_field_ms_rounds"] = times["sup_field"]
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--configs", default="pubmed,rmat2m")
    ap.add_argument("--rounds", type=int, default=7, help="alternating rounds")
    ap.add_argument("--no-module", action="store_true", help="leave the module path out")
    ap.add_argument("--out", default=None, help="JSON file; configurations already in it are kept")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("full_unsup_bench needs a HIP device")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = {}
    if args.out and os.path.exists(args.out):
        with open(args.out) as f:
            res = json.load(f)
    for name in args.configs.split(","):
        res[name] = measure(name, dev, args.rounds, not args.no_module)
        text = json.dumps(res, indent=1)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(text + "\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
