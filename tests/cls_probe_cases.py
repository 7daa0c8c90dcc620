"""Yardsticks for the classifier probe (hip_ops.cls_probe, its numpy mirror and
train.ClassifierProbe); no tests here.

`reference` restates the reference's train_classification loop
(utils.py:89-108) from its literal lines -- nn.Linear, torch.log_softmax,
loss.backward(), clip_grad_norm_(..., 5), torch.optim.SGD(lr=0.5) -- in torch
on the CPU with a dtype argument.  In float64 it is the reference every
implementation is compared with; in float32 its distance from the float64 run
(e32) is the unit the GPU tests measure the kernel in.

Shapes (D, C, batch, n_train, epochs) and what each exercises:
    128  7 50 137 3   Cora's shape, short last batch
      5  2 50  23 2   scalar path, n_train < batch
    100 41  1   9 2   batch of one
    256 16 64 200 2   largest guaranteed-supported
     16  3  8  64 4   n_train a multiple of batch; lde > D (a column slice of a wider table)
Each runs at two embedding scales (SCALES, per shape): at the small one no
step's gradient norm reaches the clip threshold, at the large one some steps'
do and others' do not (asserted on the float64 run's recorded norms,
tests/test_cls_probe_host.py).  Shapes 1 and
3 draw their labels from [0, C - 1): the last class never occurs.
"""
import functools

import numpy as np
import torch
import torch.nn as nn

LR, MAX_NORM = 0.5, 5.0

#         D    C  batch n_train epochs absent wide
SHAPES = [(128, 7, 50, 137, 3, False, False),
          (5, 2, 50, 23, 2, True, False),
          (100, 41, 1, 9, 2, False, False),
          (256, 16, 64, 200, 2, True, False),
          (16, 3, 8, 64, 4, False, True)]
SCALES = [(0.25, 3.0), (0.25, 8.0), (0.25, 1.0), (0.25, 2.0), (0.25, 3.0)]  # per shape: (no clip, mixed)
CASES = [(i, s) for i in range(len(SHAPES)) for s in SCALES[i]]


def clipped(norms):
    """Which steps clip_grad_norm_(MAX_NORM) scaled: coef = MAX_NORM / (norm + 1e-6) < 1."""
    return MAX_NORM / (np.asarray(norms) + 1e-6) < 1.0


def case_id(case):
    D, C, batch, n_train, epochs = SHAPES[case[0]][:5]
    return f"D{D}-C{C}-b{batch}-T{n_train}-e{epochs}-x{case[1]}"


class Case:
    """One problem: table [N, ld] fp32 whose columns [col0, col0 + D) are the
    embeddings E, labels [N], order [epochs, n_train] (every epoch a
    permutation of the same n_train training ids), and the initial W, b."""

    def __init__(self, shape, scale):
        D, C, batch, n_train, epochs, absent, wide = SHAPES[shape]
        rs = np.random.RandomState(1000 + 17 * shape)
        N = n_train + 11
        self.D, self.C, self.batch, self.n_train, self.epochs = D, C, batch, n_train, epochs
        self.col0 = 4 if wide else 0
        ld = D + 12 if wide else D
        self.table = (rs.standard_normal((N, ld)) * scale).astype(np.float32)
        self.labels = rs.randint(0, C - 1 if absent else C, N).astype(np.int64)
        train = rs.permutation(N)[:n_train]
        self.order = np.stack([rs.permutation(train) for _ in range(epochs)]).astype(np.int64)
        self.W = (rs.uniform(-1, 1, (C, D)) * np.sqrt(6.0 / (C + D))).astype(np.float32)
        self.b = rs.uniform(-0.1, 0.1, C).astype(np.float32)
        self.steps = -(-n_train // batch)

    @property
    def E(self):
        return self.table[:, self.col0:self.col0 + self.D]

    @property
    def params(self):
        return np.concatenate([self.W.reshape(-1), self.b])


@functools.lru_cache(maxsize=None)
def case(shape, scale):
    return Case(shape, scale)


class Result:
    def __init__(self, params, snapshots, losses, norms):
        self.params, self.snapshots, self.losses, self.norms = params, snapshots, losses, norms


def _flat(lin):
    return torch.cat([lin.weight.detach().reshape(-1), lin.bias.detach().reshape(-1)]).double().numpy()


@functools.lru_cache(maxsize=None)
def reference(shape, scale, dtype=torch.float64):
    """The loop of utils.py:89-108 on the case, in `dtype` on the CPU.  Returns
    a Result of float64 arrays: the final flat parameters, the parameters after
    each epoch, every step's loss, and every step's gradient norm as
    clip_grad_norm_ returned it.  Cached: callers must not modify it."""
    c = case(shape, scale)
    features = torch.from_numpy(c.E.copy()).to(dtype)
    labels = c.labels
    classification = nn.Sequential(nn.Linear(c.D, c.C)).to(dtype)  # Classification.layer
    lin = classification[0]
    with torch.no_grad():
        lin.weight.copy_(torch.from_numpy(c.W).to(dtype))
        lin.bias.copy_(torch.from_numpy(c.b).to(dtype))
    c_optimizer = torch.optim.SGD(classification.parameters(), lr=LR)
    b_sz = c.batch
    snapshots, losses, norms = [], [], []
    for epoch in range(c.epochs):
        train_nodes = c.order[epoch]
        for index in range(c.steps):
            nodes_batch = train_nodes[index * b_sz:(index + 1) * b_sz]
            labels_batch = labels[nodes_batch]
            embs_batch = features[nodes_batch]
            logists = torch.log_softmax(classification(embs_batch), 1)
            loss = -torch.sum(logists[range(logists.size(0)), labels_batch], 0)
            loss /= len(nodes_batch)
            loss.backward()
            norms.append(float(nn.utils.clip_grad_norm_(classification.parameters(), MAX_NORM)))
            c_optimizer.step()
            c_optimizer.zero_grad()
            losses.append(float(loss.detach()))
        snapshots.append(_flat(lin))
    return Result(_flat(lin), np.stack(snapshots), np.array(losses).reshape(c.epochs, c.steps), np.array(norms))
