"""Drop-in batch loop and embedding export of the reference's src/utils.py.

``apply_model``      utils.py:113-193 — one epoch: shuffle, per batch
                     extend_nodes (native, bit-exact), GraphSage forward/backward
                     (HIP), supervised head + NLL (fused HIP kernel), the
                     unsupervised losses (HIP), clip_grad_norm_(5) per model,
                     SGD(lr=0.7).
``get_gnn_embeddings`` utils.py:59-78 — every node's embedding in batches of
                     500 (the full-graph inference pass); with
                     sampler streams or several ranks, the native forward-only
                     pipeline sharded over ranks + one all-gather.
``evaluate``         utils.py:13-57 — validation / test micro-F1, checkpoint.
``train_classification`` utils.py:80-111 — classifier on frozen embeddings.

Same signatures, same randomness consumers in the same order: numpy's global
stream (sklearn ``shuffle``), Python's ``random`` (extend_nodes, then the
GraphSage sampler), so an epoch visits the reference's batches and samples.
"""
import math
import os
import random as _pyrandom
import sys

import numpy as np
import torch
import torch.distributed as dist
import torch.nn as nn

from . import hip_ops as ops

_NUM_NEG = {"margin": 6, "normal": 100}  # utils.py:119-122


class _SupervisedNLL(torch.autograd.Function):
    """-Σ log_softmax(E·Wᵀ + b)[i, y_i] / B (models.py:25-27, utils.py:159-164)
    in one fused HIP launch pair that also yields the gradients; backward only
    scales them by the incoming gradient."""

    @staticmethod
    def forward(ctx, E, W, b, labels):
        E_ = E.detach().contiguous()
        B, D = E_.shape
        C = W.shape[0]
        dev = E_.device
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        dE = torch.empty_like(E_)
        dW = torch.empty(C, D, dtype=torch.float32, device=dev)
        db = torch.empty(C, dtype=torch.float32, device=dev)
        ws = ops.cls_nll_workspace(B, D, C, dev)
        ops.cls_nll_fwd_bwd(E_, W.detach().contiguous(), b.detach().contiguous(), labels, loss, dE, dW, db, ws)
        ctx.save_for_backward(dE, dW, db)
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        dE, dW, db = ctx.saved_tensors
        return dE * g, dW * g, db * g, None


def supervised_loss(classification, embs, labels_batch):
    """The loss_sup of utils.py:159-164 through the fused head."""
    lin = classification.layer[0]
    y = torch.as_tensor(np.asarray(labels_batch), device=embs.device).to(torch.int32)
    return _SupervisedNLL.apply(embs, lin.weight, lin.bias, y)


def _trainable(models):
    return [p for m in models for p in m.parameters() if p.requires_grad]


def train_step(graphSage, classification, unsupervised_loss, optimizer, batch, labels, num_neg, learn_method,
               unsup):
    """The body of one apply_model batch (utils.py:146-191): extend, forward,
    losses, backward, clip per model, SGD.  Returns (loss, extended nodes);
    the loss stays on the device (no host sync)."""
    ext = getattr(unsupervised_loss, "extend_nodes_array", None)  # ours: the ids as an array
    nodes = (ext(batch, num_neg=num_neg) if ext is not None
             else np.asarray(list(unsupervised_loss.extend_nodes(batch, num_neg=num_neg))))
    embs = graphSage(nodes)
    parts = []
    if learn_method in ("sup", "plus_unsup"):
        parts.append(supervised_loss(classification, embs, labels[nodes]))
    if learn_method != "sup":
        parts.append(unsup(embs, nodes))
    loss = parts[0] if len(parts) == 1 else parts[0] + parts[1]
    loss.backward()
    models = [graphSage, classification]
    for m in models:
        nn.utils.clip_grad_norm_(m.parameters(), 5)
    optimizer.step()
    optimizer.zero_grad()
    for m in models:
        m.zero_grad()
    return loss.detach(), nodes


def apply_model(dataCenter, ds, graphSage, classification, unsupervised_loss, b_sz, unsup_loss, device,
                learn_method, verbose=True):
    """One training epoch, utils.py:113-193.  Returns (graphSage, classification)."""
    if unsup_loss not in _NUM_NEG:
        print("unsup_loss can be only 'margin' or 'normal'.")
        sys.exit(1)
    num_neg = _NUM_NEG[unsup_loss]
    train_nodes = getattr(dataCenter, ds + "_train")
    labels = getattr(dataCenter, ds + "_labels")
    from sklearn.utils import shuffle  # numpy's global stream, as the reference
    train_nodes = shuffle(train_nodes)

    models = [graphSage, classification]
    optimizer = torch.optim.SGD(_trainable(models), lr=0.7)
    optimizer.zero_grad()
    for m in models:
        m.zero_grad()
    unsup = {"margin": unsupervised_loss.get_loss_margin, "normal": unsupervised_loss.get_loss_sage}[unsup_loss]

    n_batches = math.ceil(len(train_nodes) / b_sz)
    seen = set()
    for index in range(n_batches):
        batch = train_nodes[index * b_sz:(index + 1) * b_sz]
        loss, nodes = train_step(graphSage, classification, unsupervised_loss, optimizer, batch, labels, num_neg,
                                 learn_method, unsup)
        seen.update(nodes.tolist())
        if verbose:
            print(f"Step [{index + 1}/{n_batches}], Loss: {loss.item():.4f}, "
                  f"Dealed Nodes [{len(seen)}/{len(train_nodes)}] ")
    return graphSage, classification


def apply_model_full(dataCenter, ds, trainer, unsupervised_loss, b_sz, unsup_loss, learn_method, verbose=True):
    """apply_model's epoch on the exact path: the same shuffle, batches,
    extend_nodes and print line, each batch one step of `trainer` (a
    train.FullTrainer, which holds both models' parameters, its own clip and
    optimiser) over the full neighbourhoods of the extended batch, restricted
    to its receptive field.  "unsup" / "plus_unsup": FullTrainer.unsup_step;
    "sup": extend_nodes, then the supervised step over the extended batch
    (utils.py:153-164).  Nothing but the shuffle and extend_nodes draws from a
    random stream.  Returns the trainer."""
    if unsup_loss not in _NUM_NEG:
        print("unsup_loss can be only 'margin' or 'normal'.")
        sys.exit(1)
    num_neg = _NUM_NEG[unsup_loss]
    train_nodes = getattr(dataCenter, ds + "_train")
    from sklearn.utils import shuffle  # numpy's global stream, as the reference
    train_nodes = shuffle(train_nodes)

    n_batches = math.ceil(len(train_nodes) / b_sz)
    seen = set()
    field = None
    for index in range(n_batches):
        batch = train_nodes[index * b_sz:(index + 1) * b_sz]
        if learn_method == "sup":
            nodes = unsupervised_loss.extend_nodes_array(batch, num_neg=num_neg)
            ids = trainer._nodes(nodes)
            field = trainer.field(ids, out=field)
            loss = trainer.step(ids, field=field)
        else:
            loss, nodes = trainer.unsup_step(unsupervised_loss, batch, unsup_loss=unsup_loss,
                                             learn_method=learn_method, num_neg=num_neg)
        seen.update(nodes.tolist())
        if verbose:
            print(f"Step [{index + 1}/{n_batches}], Loss: {loss.item():.4f}, "
                  f"Dealed Nodes [{len(seen)}/{len(train_nodes)}] ")
    return trainer


def _world(group):
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(group), dist.get_world_size(group)
    return 0, 1


def shard_ids(n, b_sz, rank, world):
    """Ids of the batches this rank embeds: the reference's batches of b_sz in
    id order (utils.py:63-68), batch i on rank i % world, concatenated."""
    n_batches = math.ceil(n / b_sz)
    parts = [np.arange(i * b_sz, min(n, (i + 1) * b_sz), dtype=np.int64) for i in range(rank, n_batches, world)]
    return np.concatenate(parts) if parts else np.zeros(0, np.int64)


def _embed_ids(gnn_model, ids, b_sz, rngs):
    """This rank's embeddings through the native inference pipeline."""
    from .train import Embedder
    weights = [getattr(gnn_model, f"sage_layer{i}").weight for i in range(1, gnn_model.num_layers + 1)]
    X = gnn_model.raw_features
    X = X if X.is_contiguous() else X.contiguous()
    emb = Embedder(gnn_model.graph, X, weights, gnn_model.fanouts, gnn_model.agg_func, gnn_model.gcn)
    return emb.embed(ids, b_sz, rngs)


def get_gnn_embeddings(gnn_model, dataCenter, ds, b_sz=500, *, sampler_streams=None, group=None, seed=None,
                       full_neighbourhood=False):
    """Embeddings of every node, utils.py:59-78 (batches of 500, in id order).

    Default (one process, no `sampler_streams`): the reference's loop — one
    GraphSage call per batch on the global `random` stream, bit-exact.

    Native pipeline (`sampler_streams` = S, or torch.distributed initialised
    with world W > 1): batch i goes to rank i % W; each rank
    runs its batches through the forward-only runner (train.Embedder) with S
    sampler streams, then one all-gather assembles [N, H] on every rank.  At
    W = 1, S = 1 the stream is the global `random` state (same result and
    same state afterwards as the default loop), or the module's own `rng`
    when it was given one; otherwise stream (r, w) is
    seeded train.rank_seed(seed, r, w) (seed defaults to 824), each one a
    reference stream on its own.

    `full_neighbourhood=True`: exact embeddings over every node's whole
    neighbourhood (train.FullEmbedder: the reference's num_sample=None branch,
    layer by layer over all nodes) instead of sampled ones.  Nothing is
    sampled, so `b_sz`, `sampler_streams` and `seed` are ignored and no
    `random` state is touched.  One process only: raises on world > 1."""
    n = len(getattr(dataCenter, ds + "_labels"))
    rank, world = _world(group)
    if full_neighbourhood:
        if world > 1:
            raise RuntimeError("get_gnn_embeddings(full_neighbourhood=True) runs on one GPU (world == 1)")
        from .train import FullEmbedder
        weights = [getattr(gnn_model, f"sage_layer{i}").weight for i in range(1, gnn_model.num_layers + 1)]
        X = gnn_model.raw_features
        X = X if X.is_contiguous() else X.contiguous()
        emb = FullEmbedder(gnn_model.graph, X, weights, gnn_model.agg_func, gnn_model.gcn)
        return emb.embed(None if n == gnn_model.graph.n_nodes else np.arange(n, dtype=np.int64)).detach()
    if world == 1 and not sampler_streams:
        out = []
        with torch.no_grad():
            for lo in range(0, n, b_sz):
                ids = np.arange(lo, min(n, lo + b_sz), dtype=np.int64)
                e = gnn_model(ids)
                assert len(e) == len(ids)
                out.append(e)
        embs = torch.cat(out, 0)
        assert len(embs) == n
        return embs.detach()

    from .sampler import RNG
    from .train import rank_seed
    S = int(sampler_streams or 1)
    ids = shard_ids(n, b_sz, rank, world)
    own = getattr(gnn_model, "rng", None)
    exact = world == 1 and S == 1 and own is None
    if exact:
        rngs = [RNG.from_python(_pyrandom)]
    elif world == 1 and S == 1:  # the module's own stream, as its forward would draw
        rngs = [own]
    else:
        base = 824 if seed is None else int(seed)
        rngs = [RNG(rank_seed(base, rank, w)) for w in range(S)]
    mine = _embed_ids(gnn_model, ids, b_sz, rngs)
    if exact:
        rngs[0].to_python(_pyrandom)
    if world == 1:
        return mine.detach()
    # all-gather: every rank knows every shard's ids, so pad to the largest
    H = mine.shape[1]
    lens = [len(shard_ids(n, b_sz, r, world)) for r in range(world)]
    buf = torch.zeros(max(lens), H, dtype=mine.dtype, device=mine.device)
    buf[:len(ids)].copy_(mine)
    parts = [torch.empty_like(buf) for _ in range(world)]
    dist.all_gather(parts, buf, group=group)
    embs = torch.empty(n, H, dtype=mine.dtype, device=mine.device)
    for r in range(world):
        rid = torch.from_numpy(shard_ids(n, b_sz, r, world)).to(mine.device)
        embs.index_copy_(0, rid, parts[r][:lens[r]])
    return embs.detach()


def evaluate(dataCenter, ds, graphSage, classification, device, max_vali_f1, name, cur_epoch):
    """Validation micro-F1, and test F1 + checkpoint when it improves
    (utils.py:13-57).  Same RNG use (GraphSage on the val nodes, then on the
    test nodes only when improved), same prints, same return value.  The
    checkpoint is torch.save([graphSage, classification]) as in the
    reference (GraphSage pickles without its native graph handle)."""
    from sklearn.metrics import f1_score
    test_nodes = getattr(dataCenter, ds + "_test")
    val_nodes = getattr(dataCenter, ds + "_val")
    labels = getattr(dataCenter, ds + "_labels")
    models = [graphSage, classification]
    params = []
    for model in models:
        for param in model.parameters():
            if param.requires_grad:
                param.requires_grad = False
                params.append(param)

    def predict(nodes):
        embs = graphSage(nodes)
        _, predicts = torch.max(classification(embs), 1)
        return predicts.cpu().numpy()

    predicts = predict(val_nodes)
    labels_val = labels[val_nodes]
    assert len(labels_val) == len(predicts)
    vali_f1 = f1_score(labels_val, predicts, average="micro")
    print("Validation F1:", vali_f1)
    if vali_f1 > max_vali_f1:
        max_vali_f1 = vali_f1
        predicts = predict(test_nodes)
        labels_test = labels[test_nodes]
        assert len(labels_test) == len(predicts)
        test_f1 = f1_score(labels_test, predicts, average="micro")
        print("Test F1:", test_f1)
        for param in params:
            param.requires_grad = True
        os.makedirs("models", exist_ok=True)
        torch.save(models, "models/model_best_{}_ep{}_{:.4f}.torch".format(name, cur_epoch, test_f1))
    for param in params:
        param.requires_grad = True
    return max_vali_f1


def evaluate_full(dataCenter, ds, trainer, max_vali_f1, name, cur_epoch, use_field=True):
    """evaluate's protocol (utils.py:13-57) on the exact path: validation
    micro-F1 of `trainer` (a train.FullTrainer) over the validation ids, and,
    when it improves on max_vali_f1, the test F1 and a checkpoint; the same
    prints and the same return value.  F1 is EvalResult.micro_f1 of
    FullTrainer.evaluate, over the receptive field of the ids (use_field) or
    over all N rows.  What differs from evaluate: nothing is sampled, so no
    `random` draw is made and no module is involved, and the checkpoint is
    torch.save(trainer.state_dict()), not a pickled pair of modules."""
    test_nodes = getattr(dataCenter, ds + "_test")
    val_nodes = getattr(dataCenter, ds + "_val")

    def f1_of(nodes):
        ids = trainer._nodes(np.asarray(nodes))
        return trainer.evaluate(ids, field=trainer.field(ids) if use_field else None).micro_f1

    vali_f1 = f1_of(val_nodes)
    print("Validation F1:", vali_f1)
    if vali_f1 > max_vali_f1:
        max_vali_f1 = vali_f1
        test_f1 = f1_of(test_nodes)
        print("Test F1:", test_f1)
        os.makedirs("models", exist_ok=True)
        torch.save(trainer.state_dict(), "models/model_best_{}_ep{}_{:.4f}.torch".format(name, cur_epoch, test_f1))
    return max_vali_f1


def micro_f1(labels, predicts):
    """Micro-averaged F1 of single-label multi-class predictions, which is the
    accuracy: every wrong prediction is one false positive (its class) and one
    false negative (the true class), so precision = recall = correct / n.
    sklearn's f1_score(average="micro") computes 2·p·r / (p + r) from them, which
    rounds its product and its quotient: the two values are equal up to those
    two roundings (2 ulp), not always bit for bit."""
    labels, predicts = np.asarray(labels), np.asarray(predicts)
    return float((labels == predicts).sum()) / float(labels.shape[-1])


def _set_classifier(classification, flat):
    """The flat probe parameters (W row-major, then b) into classification's own Parameters."""
    lin = classification.layer[0]
    nw = lin.weight.numel()
    with torch.no_grad():
        lin.weight.copy_(flat[:nw].view_as(lin.weight))
        lin.bias.copy_(flat[nw:].view_as(lin.bias))


def _train_classification_native(dataCenter, graphSage, classification, ds, device, max_vali_f1, name, epochs,
                                 evaluate_on):
    """train_classification's native path: every epoch's shuffle drawn up
    front, the whole run in train.ClassifierProbe, then the evaluation."""
    from sklearn.utils import shuffle
    from .train import ClassifierProbe
    print("Training Classification ...")
    b_sz = 50
    train_nodes = getattr(dataCenter, ds + "_train")
    labels = getattr(dataCenter, ds + "_labels")
    features = get_gnn_embeddings(graphSage, dataCenter, ds)
    if epochs < 1:  # the loop's range(epochs) is empty: nothing after the embeddings
        return classification, max_vali_f1
    lin = classification.layer[0]
    probe = ClassifierProbe(features, labels, lin.out_features, weights=(lin.weight.detach(), lin.bias.detach()),
                            lr=0.5, max_norm=5.0, batch=b_sz)
    order = []
    for epoch in range(epochs):  # chained as the loop chains them: numpy's stream ends where the loop leaves it
        train_nodes = shuffle(train_nodes)
        order.append(np.asarray(train_nodes))
    _, snapshots = probe.run(np.stack(order))
    if evaluate_on == "model":
        for epoch in range(epochs):
            _set_classifier(classification, snapshots[epoch])
            max_vali_f1 = evaluate(dataCenter, ds, graphSage, classification, device, max_vali_f1, name, epoch)
        return classification, max_vali_f1

    test_nodes = getattr(dataCenter, ds + "_test")
    val_nodes = getattr(dataCenter, ds + "_val")
    val_pred = probe.predict(val_nodes, snapshots).cpu().numpy()    # [epochs, n_val]
    test_pred = probe.predict(test_nodes, snapshots).cpu().numpy()
    labels_val, labels_test = np.asarray(labels)[val_nodes], np.asarray(labels)[test_nodes]
    models = [graphSage, classification]
    for epoch in range(epochs):
        vali_f1 = micro_f1(labels_val, val_pred[epoch])
        print("Validation F1:", vali_f1)
        if vali_f1 > max_vali_f1:
            max_vali_f1 = vali_f1
            test_f1 = micro_f1(labels_test, test_pred[epoch])
            print("Test F1:", test_f1)
            _set_classifier(classification, snapshots[epoch])
            os.makedirs("models", exist_ok=True)
            torch.save(models, "models/model_best_{}_ep{}_{:.4f}.torch".format(name, epoch, test_f1))
    _set_classifier(classification, snapshots[epochs - 1])
    return classification, max_vali_f1


def train_classification(dataCenter, graphSage, classification, ds, device, max_vali_f1, name, epochs=800,
                         native=False, evaluate_on="model"):
    """Classifier on frozen embeddings (utils.py:80-111): get_gnn_embeddings,
    then per epoch sklearn-shuffled batches of 50, -Σ logp[label] / n through
    the fused HIP head, clip_grad_norm_(5), SGD(lr=0.5), evaluate().

    `native=True`: the same run through train.ClassifierProbe.  Every epoch's
    shuffle is drawn up front (numpy's global stream has no other consumer in
    the loop, so it ends in the same state), all epochs' steps run in whole
    launches of one persistent kernel, then for each epoch in order its
    parameters are copied into `classification` and evaluate() is called
    exactly as the loop calls it: Python's `random` stream, the prints, the
    checkpoints and the return value are the loop's; only the fp32 summation
    order of a step differs.  A shape the kernel does not support raises
    ValueError; there is no fallback to the loop.

    `evaluate_on="frozen"` (with native=True only; ValueError otherwise) is
    NOT the reference's evaluation, which calls GraphSage on the validation
    (and test) nodes after every epoch and so re-samples their neighbourhoods
    each time.  Here the validation and test predictions of all epochs come
    from the frozen embeddings the classifier was trained on
    (ClassifierProbe.predict), micro-F1 is computed as accuracy (micro_f1:
    equal to sklearn's value up to sklearn's own rounding, so an F1 print or
    a checkpoint name can differ from evaluate's formatting in the last bit),
    and the epochs are walked in order: test F1, checkpoint and "Test F1"
    print only when validation improves, as evaluate does.  No `random` draw
    and no GraphSage forward after the embeddings."""
    if evaluate_on not in ("model", "frozen"):
        raise ValueError(f"evaluate_on must be 'model' or 'frozen', got {evaluate_on!r}")
    if evaluate_on == "frozen" and not native:
        raise ValueError("evaluate_on='frozen' needs native=True")
    if native:
        return _train_classification_native(dataCenter, graphSage, classification, ds, device, max_vali_f1, name,
                                            epochs, evaluate_on)
    from sklearn.utils import shuffle
    print("Training Classification ...")
    c_optimizer = torch.optim.SGD(classification.parameters(), lr=0.5)
    b_sz = 50
    train_nodes = getattr(dataCenter, ds + "_train")
    labels = getattr(dataCenter, ds + "_labels")
    features = get_gnn_embeddings(graphSage, dataCenter, ds)
    for epoch in range(epochs):
        train_nodes = shuffle(train_nodes)
        batches = math.ceil(len(train_nodes) / b_sz)
        for index in range(batches):
            nodes_batch = train_nodes[index * b_sz:(index + 1) * b_sz]
            loss = supervised_loss(classification, features[torch.as_tensor(nodes_batch, device=features.device)],
                                   labels[nodes_batch])
            loss.backward()
            nn.utils.clip_grad_norm_(classification.parameters(), 5)
            c_optimizer.step()
            c_optimizer.zero_grad()
        max_vali_f1 = evaluate(dataCenter, ds, graphSage, classification, device, max_vali_f1, name, epoch)
    return classification, max_vali_f1
