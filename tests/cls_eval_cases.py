"""Tables of the evaluation head's tests (hip_ops.cls_eval, its numpy mirror
cls_eval_host, train.EvalResult); no tests here.

Shapes (B, D, C) and the branch each reaches in csrc/kernels/cls_eval.hip:
       1   1  1   a single row and class: logp = 0, loss = 0
      37 128  7   the float4 path, Cora's classes
     300  80  3   float4, a quarter of D that is no multiple of 8 floats
     257  50  2   the scalar loads, ldh = D + 3
    1000  16 17   a second class group holding one class
    4099 128 47   65 chunks of 64 rows, the last one partial: the fixed-order
                  loss sum has more than one term per thread round
      70  64  C*  C* = kEvalWcLds // (D + 1) + 1 = 127: C·(D + 1) exceeds the
                  kernel's LDS budget for Wc (the constant is read from the
                  kernel's source), so Wc is read through the cache; C·C also
                  exceeds the LDS histogram (kEvalHistLds), so the counts go
                  straight to memory
Every shape is run with `rows` a random subset (in random order) of a table
of B + 11 rows and labels indexed by row id, and with rows=None over the
first B rows.

Inputs: uniform_features-style rows (U(-1, 1) at 2^-23 resolution) times
SCALE, a xavier classifier and a bias in ±0.1, fixed seeds.  SCALE = 4 keeps
the logits of different classes apart: the float64 top-two margins are
recounted in tests/test_cls_eval_host.py against the cap of the GPU test.
"""
import functools
import os
import re

import numpy as np

from tests.golden.synth import uniform_features

_KERNEL = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "graphsage-pytorch_amd", "csrc",
                       "kernels", "cls_eval.hip")


def kernel_constant(name):
    """An integer constant of the kernel's source (a product of integer literals)."""
    m = re.search(r"constexpr\s+\w+\s+" + name + r"\s*=\s*([0-9* ]+);", open(_KERNEL).read())
    return int(np.prod([int(x) for x in m.group(1).split("*")]))


WC_LDS = kernel_constant("kEvalWcLds")
HIST_LDS = kernel_constant("kEvalHistLds")
CHUNK = kernel_constant("kEvalChunk")
SCALE = 4.0
EXTRA_ROWS = 11
SHAPES = [(1, 1, 1), (37, 128, 7), (300, 80, 3), (257, 50, 2), (1000, 16, 17), (4099, 128, 47),
          (70, 64, WC_LDS // (64 + 1) + 1)]
LDH = {(257, 50, 2): 50 + 3}          # row stride of the table (default: D)
FORMS = ["rows", "all"]
CASES = [(s, f) for s in SHAPES for f in FORMS]
MARGIN_CAP = 0.01                     # at most this share of a case's rows may fall below the margin


def case_id(case):
    (B, D, C), form = case
    return f"B{B}-D{D}-C{C}-{form}"


class Case:
    """table [N, ldh] fp32 (H = its first D columns), labels, rows (or None), W [C, D], b [C]."""

    def __init__(self, shape, form):
        B, D, C = shape
        self.B, self.D, self.C, self.form = B, D, C, form
        seed = 7000 + 131 * SHAPES.index(shape)
        rs = np.random.RandomState(seed)
        N = B + EXTRA_ROWS
        ldh = LDH.get(shape, D)
        self.table = np.full((N, ldh), np.nan, np.float32)   # the padding columns are never read
        self.table[:, :D] = uniform_features(seed, N, D) * np.float32(SCALE)
        self.labels = rs.randint(0, C, N).astype(np.int64)
        self.rows = rs.permutation(N)[:B].astype(np.int64) if form == "rows" else None
        self.W = (rs.uniform(-1, 1, (C, D)) * np.sqrt(6.0 / (C + D))).astype(np.float32)
        self.b = rs.uniform(-0.1, 0.1, C).astype(np.float32)

    @property
    def H(self):
        return self.table[:, :self.D] if self.rows is not None else self.table[:self.B, :self.D]

    @property
    def params(self):
        return np.concatenate([self.W.reshape(-1), self.b])

    @property
    def y(self):
        """The evaluated rows' labels, in output order."""
        return self.labels[self.rows] if self.rows is not None else self.labels[:self.B]


@functools.lru_cache(maxsize=None)
def case(shape, form):
    return Case(shape, form)


class Ref:
    def __init__(self, logp, pred, loss, conf, z):
        self.logp, self.pred, self.loss, self.conf, self.z = logp, pred, loss, conf, z


def torch_reference(H, rows, y, W, b, dtype):
    """torch on the CPU in `dtype`: log_softmax, argmax, the gathered NLL mean and a bincount confusion matrix
    (float64 numpy arrays; labels must lie in [0, C))."""
    import torch
    X = torch.from_numpy(np.ascontiguousarray(H if rows is None else H[rows])).to(dtype)
    Wt, bt = torch.from_numpy(W).to(dtype), torch.from_numpy(b).to(dtype)
    yt = torch.from_numpy(np.asarray(y, np.int64))
    C = W.shape[0]
    z = X.mm(Wt.t()) + bt
    logp = torch.log_softmax(z, 1)
    pred = z.argmax(1)
    loss = -torch.sum(logp[range(logp.size(0)), yt], 0) / logp.size(0)
    conf = torch.bincount(yt * C + pred, minlength=C * C).reshape(C, C)
    return Ref(logp.double().numpy(), pred.numpy(), float(loss.double()), conf.numpy(), z.double().numpy())


@functools.lru_cache(maxsize=None)
def reference(shape, form, fp32=False):
    """The case in torch float64 (or fp32: the yardstick e_torch).  Cached: callers must not modify it."""
    import torch
    c = case(shape, form)
    return torch_reference(c.H, c.rows, c.y, c.W, c.b, torch.float32 if fp32 else torch.float64)


def margins(z):
    """Per row, the float64 gap between the two largest logits (inf for one class)."""
    if z.shape[1] < 2:
        return np.full(z.shape[0], np.inf)
    top = np.sort(z, 1)[:, -2:]
    return top[:, 1] - top[:, 0]


def margin_rule(z64, z32):
    """The rows on which pred must equal the float64 argmax: margin >= 8 e_torch + 2^-22 max|z|, twice the
    per-logit bound of check_rule (e_torch: fp32 torch's largest logit error against float64)."""
    e_torch = float(np.max(np.abs(z32 - z64)))
    return margins(z64) >= 8.0 * e_torch + 2.0 ** -22 * float(np.max(np.abs(z64)))
