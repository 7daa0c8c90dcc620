"""Tables of the multi-label head's tests (hip_ops.cls_bce / cls_bce_eval, their
numpy mirrors, train.MultiLabelEvalResult); no tests here.

Shapes (B, D, C) and what each reaches in csrc/kernels/cls_bce.hip:
       1   4   1   one row, one label, 15 padded labels
      37 128   7   a partial row tile, one label group
      50  20  17   a second label group holding one label; D no multiple of 16
     257  50  33   D % 4 != 0, row stride D + 3 (unaligned rows), targets across
                   two words
    4099 128 121   PPI's width: four target words, many tiles and slabs, a
                   partial last tile
      70  64  C*   the largest C that gs_cls_bce_supported(64, .) accepts, read
                   from the library
Every shape runs with `rows` a random subset (in random order) of a table of
B + 11 rows and with rows=None over the first B rows, and with pos_weight None
and pos_weight in [0.5, 4].

Inputs: uniform_features rows (U(-1, 1) at 2^-23 resolution) times SCALE = 4, a
xavier classifier, a bias in +-0.1 and targets Bernoulli(0.3), fixed seeds.

Predictions: a bit must equal the float64 decision z64 > 0 wherever
|z64| >= 8 e_torch(z) + 2^-22 max|z64| (margin_rule); at most MARGIN_CAP of a
case's (row, label) elements may fall below that margin, which
tests/test_cls_bce_host.py recounts from the float64 reference alone.
"""
import functools
import importlib

import numpy as np

from tests.golden.synth import uniform_features

SCALE = 4.0
EXTRA_ROWS = 11
TARGET_P = 0.3
MARGIN_CAP = 0.01


@functools.lru_cache(maxsize=None)
def largest_c(D):
    """The largest C with gs_cls_bce_supported(D, C), from the library (no device work)."""
    lib = importlib.import_module("graphsage-pytorch_amd._lib").lib()
    C = 1
    assert lib.gs_cls_bce_supported(D, C)
    while lib.gs_cls_bce_supported(D, C + 1):
        C += 1
    return C


def shapes():
    return [(1, 4, 1), (37, 128, 7), (50, 20, 17), (257, 50, 33), (4099, 128, 121), (70, 64, largest_c(64))]


LD = {(257, 50, 33): 50 + 3}     # row stride of the table (default: D)
FORMS = ["rows", "all"]
PW = [False, True]


def cases():
    return [(s, f, p) for s in shapes() for f in FORMS for p in PW]


def case_id(case):
    (B, D, C), form, pw = case
    return f"B{B}-D{D}-C{C}-{form}-{'pw' if pw else 'nopw'}"


class Case:
    """table [N, ld] fp32 (its first D columns are the rows), targets [N, C] bool per table row, rows (or
    None), W [C, D], b [C], pos_weight [C] or None.  variant: "" | "x40" (features x 40) | "extreme" (all-zero
    and all-one target rows)."""

    def __init__(self, shape, form, pw, variant=""):
        B, D, C = shape
        self.B, self.D, self.C, self.form = B, D, C, form
        seed = 9100 + 17 * B + 3 * D + C
        rs = np.random.RandomState(seed)
        N = B + EXTRA_ROWS
        ld = LD.get(shape, D)
        scale = SCALE * (10.0 if variant == "x40" else 1.0)
        self.table = np.full((N, ld), np.nan, np.float32)   # the padding columns are never read
        self.table[:, :D] = uniform_features(seed, N, D) * np.float32(scale)
        self.targets = rs.uniform(0, 1, (N, C)) < TARGET_P
        if variant == "extreme":
            self.targets[0::3] = False
            self.targets[1::3] = True
        self.rows = rs.permutation(N)[:B].astype(np.int64) if form == "rows" else None
        self.W = (rs.uniform(-1, 1, (C, D)) * np.sqrt(6.0 / (C + D))).astype(np.float32)
        self.b = rs.uniform(-0.1, 0.1, C).astype(np.float32)
        self.pw = rs.uniform(0.5, 4.0, C).astype(np.float32) if pw else None

    @property
    def E(self):
        """The evaluated rows [B, D], in output order."""
        t = self.table[:, :self.D]
        return t[self.rows] if self.rows is not None else t[:self.B]

    @property
    def y(self):
        """The evaluated rows' targets [B, C] bool, in output order."""
        return self.targets[self.rows] if self.rows is not None else self.targets[:self.B]


@functools.lru_cache(maxsize=None)
def case(shape, form, pw, variant=""):
    return Case(shape, form, pw, variant)


class Ref:
    """loss (float), l [B, C] the loss terms, z, dE (unmasked), dW, db as float64 numpy; E the rows."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def dE_masked(self):
        return np.where(self.E <= 0, 0.0, self.dE)

    @property
    def pred(self):
        return self.z > 0


def torch_reference(E, y, W, b, pw, dtype):
    """binary_cross_entropy_with_logits (mean, pos_weight) and its autograd on the CPU in `dtype`."""
    import torch
    import torch.nn.functional as F
    Et = torch.from_numpy(np.ascontiguousarray(E)).to(dtype).requires_grad_(True)
    Wt = torch.from_numpy(W).to(dtype).requires_grad_(True)
    bt = torch.from_numpy(b).to(dtype).requires_grad_(True)
    yt = torch.from_numpy(np.asarray(y)).to(dtype)
    pwt = None if pw is None else torch.from_numpy(pw).to(dtype)
    z = torch.addmm(bt, Et, Wt.t())
    loss = F.binary_cross_entropy_with_logits(z, yt, pos_weight=pwt, reduction="mean")
    loss.backward()
    l = F.binary_cross_entropy_with_logits(z.detach(), yt, pos_weight=pwt, reduction="none")
    return Ref(loss=float(loss.detach().double()), l=l.double().numpy(), z=z.detach().double().numpy(),
               dE=Et.grad.double().numpy(), dW=Wt.grad.double().numpy(), db=bt.grad.double().numpy(),
               E=np.asarray(E, np.float64))


@functools.lru_cache(maxsize=None)
def reference(shape, form, pw, variant="", fp32=False):
    """The case in torch float64 (or fp32: the yardstick e_torch).  Cached: callers must not modify it."""
    import torch
    c = case(shape, form, pw, variant)
    return torch_reference(c.E, c.y, c.W, c.b, c.pw, torch.float32 if fp32 else torch.float64)


def loss_yardstick(ref, r32):
    """The fp32 yardstick of the loss for check_rule's `tor`.  The mean is one fp32 scalar, so its e_torch is one
    draw of rounding; where that draw is 0, the largest per-element error of the loss terms stands in (no fp32
    mean is expected to beat the error of the terms it averages)."""
    if r32.loss != ref.loss:
        return np.array([r32.loss])
    return np.array([ref.loss + float(np.max(np.abs(r32.l - ref.l)))])


def margin_rule(z64, z32):
    """The (row, label) elements on which the predicted bit must equal z64 > 0:
    |z64| >= 8 e_torch(z) + 2^-22 max|z64|, twice check_rule's per-logit bound."""
    e_torch = float(np.max(np.abs(z32 - z64)))
    return np.abs(z64) >= 8.0 * e_torch + 2.0 ** -22 * float(np.max(np.abs(z64)))


def counts_of(pred, y, keep=None):
    """[C, 3] true positives, false positives, false negatives over the kept elements."""
    pred, y = np.asarray(pred, bool), np.asarray(y, bool)
    k = np.ones_like(y) if keep is None else keep
    return np.stack([(pred & y & k).sum(0), (pred & ~y & k).sum(0), (~pred & y & k).sum(0)], 1).astype(np.int64)


def f1_restated(pred, y):
    """micro / macro F1, subset accuracy and per-label precision / recall / F1 of bool [B, C] arrays, stated
    directly (0 / 0 counts as 0)."""
    pred, y = np.asarray(pred, bool), np.asarray(y, bool)

    def div(a, b):
        return float(a) / float(b) if b else 0.0

    C = y.shape[1]
    tp = [(pred[:, c] & y[:, c]).sum() for c in range(C)]
    fp = [(pred[:, c] & ~y[:, c]).sum() for c in range(C)]
    fn = [(~pred[:, c] & y[:, c]).sum() for c in range(C)]
    prec = [div(tp[c], tp[c] + fp[c]) for c in range(C)]
    rec = [div(tp[c], tp[c] + fn[c]) for c in range(C)]
    f1 = [div(2 * tp[c], 2 * tp[c] + fp[c] + fn[c]) for c in range(C)]
    return {"micro_f1": div(2 * sum(tp), 2 * sum(tp) + sum(fp) + sum(fn)), "macro_f1": sum(f1) / C,
            "subset_accuracy": div((pred == y).all(1).sum(), y.shape[0]), "precision": np.array(prec),
            "recall": np.array(rec), "f1": np.array(f1)}
