#!/usr/bin/env python3
"""Measure train_classification's loop against the classifier probe kernel
("Classifier probe"), on the Cora-shaped problem: N = 2708 nodes,
T = 1355 training ids, D = 128, C = 7, batches of 50 (28 steps per epoch).
Everything in one process, after warm-up, in alternating rounds.

  training    the training part alone for the same shuffled orders, at 8 and at
              800 epochs: the Python loop of utils.train_classification (gather,
              fused head, autograd backward, clip_grad_norm_, SGD.step per
              batch; no evaluate) and train.ClassifierProbe.run.  Host clock
              around the work plus a device synchronise; us per step for both.
  whole call  utils.train_classification on the Cora graph of the tests
              (64 uniform features, a 2-layer GraphSage of random weights) at
              --call-epochs epochs (reduced from the reference's 800: the loop
              and evaluate() cost the same every epoch), three ways:
              native=False, native=True, and native=True with
              evaluate_on="frozen"; seconds per call and per epoch, and the
              share of a call that is get_gnn_embeddings (timed alone).

    python tools/cls_probe_bench.py --out profiles/cls_probe_bench.json

Needs the GPU: there is no CPU path.  A measurement tool, not bench.py; it
asserts nothing about speed."""
import argparse
import contextlib
import io
import json
import math
import os
import random
import sys
import tempfile
import time
import types
from collections import defaultdict
from importlib import import_module

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

models = import_module("graphsage-pytorch_amd.models")
utils = import_module("graphsage-pytorch_amd.utils")
train = import_module("graphsage-pytorch_amd.train")

N, T, D, C, B, SEED = 2708, 1355, 128, 7, 50, 824


def orders(epochs, train_nodes):
    from sklearn.utils import shuffle
    np.random.seed(SEED)
    out = []
    for _ in range(epochs):
        train_nodes = shuffle(train_nodes)
        out.append(np.asarray(train_nodes))
    return np.stack(out)


def loop_training(features, labels, order, W, b):
    """The loop of utils.train_classification without evaluate(), over given orders."""
    classification = models.Classification(D, C).to(features.device)
    with torch.no_grad():
        classification.layer[0].weight.copy_(W)
        classification.layer[0].bias.copy_(b)
    c_optimizer = torch.optim.SGD(classification.parameters(), lr=0.5)
    for train_nodes in order:
        for index in range(math.ceil(len(train_nodes) / B)):
            nodes_batch = train_nodes[index * B:(index + 1) * B]
            loss = utils.supervised_loss(classification,
                                         features[torch.as_tensor(nodes_batch, device=features.device)],
                                         labels[nodes_batch])
            loss.backward()
            nn.utils.clip_grad_norm_(classification.parameters(), 5)
            c_optimizer.step()
            c_optimizer.zero_grad()
    torch.cuda.synchronize()
    return classification


def probe_training(features, labels, order, W, b):
    probe = train.ClassifierProbe(features, labels, C, weights=(W, b), lr=0.5, max_norm=5.0, batch=B)
    probe.run(order)
    torch.cuda.synchronize()
    return probe


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def training_rounds(device, epochs, rounds):
    rs = np.random.RandomState(SEED)
    features = torch.from_numpy(rs.standard_normal((N, D)).astype(np.float32)).to(device)
    labels = rs.randint(0, C, N).astype(np.int64)
    order = orders(epochs, rs.permutation(N)[:T])
    torch.manual_seed(SEED)
    lin = models.Classification(D, C).layer[0]
    W, b = lin.weight.detach().to(device), lin.bias.detach().to(device)
    steps = epochs * math.ceil(T / B)
    res = {"epochs": epochs, "steps": steps, "loop_s": [], "probe_s": []}
    loop_training(features, labels, order[:1], W, b)  # warm-up of both paths' code objects
    probe_training(features, labels, order[:1], W, b)
    for _ in range(rounds):
        dt, cls = timed(lambda: loop_training(features, labels, order, W, b))
        res["loop_s"].append(round(dt, 4))
        dt, probe = timed(lambda: probe_training(features, labels, order, W, b))
        res["probe_s"].append(round(dt, 5))
    # the two paths trained the same classifier (fp32 summation order apart)
    res["max_abs_param_difference"] = float((probe.weights()[0] - cls.layer[0].weight).abs().max())
    lo, pr = float(np.median(res["loop_s"])), float(np.median(res["probe_s"]))
    res["median"] = {"loop_s": lo, "probe_s": pr, "loop_us_per_step": round(1e6 * lo / steps, 2),
                     "probe_us_per_step": round(1e6 * pr / steps, 3), "speedup": round(lo / pr, 1)}
    return res


def cora_setup(device):
    g = np.load(os.path.join(ROOT, "tests", "golden", "graphs.npz"))
    adj = defaultdict(set)
    for a, b in zip(g["cora_src"].tolist(), g["cora_dst"].tolist()):
        adj[a].add(b)
        adj[b].add(a)
    rs = np.random.RandomState(SEED)
    perm = rs.permutation(N)
    t, v = N // 3, N // 6
    dc = types.SimpleNamespace(g_test=perm[:t], g_val=perm[t:t + v], g_train=perm[t + v:],
                               g_labels=rs.randint(0, C, N).astype(np.int64))
    feats = torch.from_numpy(rs.uniform(-1, 1, (N, 64)).astype(np.float32)).to(device)
    torch.manual_seed(SEED)
    gsage = models.GraphSage(2, 64, D, feats, adj, device).to(device)
    return dc, gsage


def whole_call_rounds(device, epochs, rounds):
    dc, gsage = cora_setup(device)
    ways = {"loop": dict(), "native": dict(native=True), "native_frozen": dict(native=True, evaluate_on="frozen")}
    res = {"epochs": epochs, "train_ids": len(dc.g_train), "embed_s": [], **{k + "_s": [] for k in ways}}

    def call(kw, n_epochs):
        torch.manual_seed(SEED)
        cls = models.Classification(D, C).to(device)
        random.seed(SEED)
        np.random.seed(SEED)
        with contextlib.redirect_stdout(io.StringIO()):
            return utils.train_classification(dc, gsage, cls, "g", device, 0.0, "bench", epochs=n_epochs, **kw)

    here = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)  # the checkpoints of improved epochs go here
        try:
            for kw in ways.values():
                call(kw, 1)
            for _ in range(rounds):
                random.seed(SEED)
                dt, _ = timed(lambda: utils.get_gnn_embeddings(gsage, dc, "g"))
                res["embed_s"].append(round(dt, 4))
                for k, kw in ways.items():
                    dt, _ = timed(lambda: call(kw, epochs))
                    res[k + "_s"].append(round(dt, 4))
        finally:
            os.chdir(here)
    med = {k: float(np.median(v)) for k, v in res.items() if isinstance(v, list)}
    res["median"] = med
    res["median_per_epoch_after_embeddings_s"] = {k[:-2]: round((med[k] - med["embed_s"]) / epochs, 5)
                                                  for k in med if k != "embed_s"}
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=3, help="alternating rounds")
    ap.add_argument("--epochs", type=int, nargs="+", default=[8, 800], help="epochs of the training-only comparison")
    ap.add_argument("--call-epochs", type=int, default=40, help="epochs of the whole train_classification calls")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cls_probe_bench needs a HIP device")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    res = {"problem": {"nodes": N, "train_ids": T, "D": D, "C": C, "batch": B, "steps_per_epoch": math.ceil(T / B)},
           "rounds": args.rounds, "training": {}}
    for e in args.epochs:
        res["training"][str(e)] = training_rounds(device, e, args.rounds)
    res["whole_call"] = whole_call_rounds(device, args.call_epochs, args.rounds)
    text = json.dumps(res, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
