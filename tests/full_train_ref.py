"""A float64 reference of one full-batch training step over full
neighbourhoods (no tests here, no GPU).

A plain restatement of what train.FullTrainer.forward_backward computes,
from the CSR alone and independent of oracle/: the layer-wise forward of
tests/full_ref.py over all N nodes (its neighbour_lists: a row's ids without
the row itself, plus the row exactly once under gcn), log_softmax + the NLL
mean over the rows `nodes` as tests/step_ref.py states them, and torch
autograd for the gradients.

MAX follows the reference's rule (models.py:325, torch.max(feat, 0)): a
per-destination torch.max(dim) over the gathered rows in visiting order, so
the gradient goes to the FIRST maximal entry -- not scatter_reduce("amax"),
whose backward splits a gradient evenly among ties.  The visiting order is
the kernels' (visit_lists): CSR row order with the row's own id skipped;
under gcn the own id stays where the row holds it and is appended last
where it does not.

`dtype` runs the same code in fp32: that run is the yardstick e_torch of
tests/adam_cases.check_rule.  bf16 features follow tests/step_ref.py: X
holds bf16 values, layer 1's aggregate and W1 enter the GEMM rounded to
bf16 in value only (the gradient reaches the fp32 W1).
"""
import numpy as np
import torch

from tests import full_ref
from tests.step_ref import _bf16_value


def visit_lists(row_ptr, col, gcn):
    """(destination per entry, source per entry) in the order the kernels
    visit a row's sources; as a set per row, full_ref.neighbour_lists."""
    row_ptr = np.asarray(row_ptr, np.int64)
    col = np.asarray(col, np.int64)
    n = len(row_ptr) - 1
    seg, ids = [], []
    for v in range(n):
        row = col[row_ptr[v]:row_ptr[v + 1]]
        if gcn:
            row = row if (row == v).any() else np.concatenate([row, [v]])
        else:
            row = row[row != v]
        seg.append(np.full(len(row), v, np.int64))
        ids.append(row)
    return np.concatenate(seg), np.concatenate(ids)


def padded_take(seg, n_dst):
    """[n_dst, kmax] entry positions, each list padded with its own first
    entry at the end (a repeat changes neither the max nor its first index)."""
    cnt = np.bincount(seg, minlength=n_dst)
    if n_dst and cnt.min() < 1:
        raise IndexError("MAX over an empty neighbourhood")
    start = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    k = np.arange(cnt.max())[None, :]
    return start[:, None] + np.where(k < cnt[:, None], k, 0)


def aggregate(rows, seg, ids, n_dst, agg, with_argmax=False):
    """rows[ids] reduced per destination (torch, differentiable)."""
    if agg == "MEAN":
        return full_ref.aggregate(rows, seg, ids, n_dst, "MEAN")
    if agg != "MAX":
        raise ValueError(agg)
    take = padded_take(seg, n_dst)
    src = ids[take]                                    # [n_dst, kmax] source ids
    m = rows[torch.from_numpy(src)].max(dim=1)         # first maximal entry wins
    if with_argmax:  # the winning entry's source id per (destination, column)
        return m.values, np.take_along_axis(src, m.indices.numpy(), 1)
    return m.values


def lists_for(row_ptr, col, gcn, agg):
    return visit_lists(row_ptr, col, gcn) if agg == "MAX" else full_ref.neighbour_lists(row_ptr, col, gcn)


def aggregate_backward(row_ptr, col, X, dA, agg, gcn, dSelf=None, Hprev=None, dtype=torch.float64):
    """(agg_full's output, its argmax or None, dH): dH is the gradient of
    sum(A * dA) with respect to X, plus dSelf, zeroed where Hprev <= 0."""
    n = len(row_ptr) - 1
    seg, ids = lists_for(row_ptr, col, gcn, agg)
    x = torch.from_numpy(np.asarray(X)).to(dtype).requires_grad_(True)
    am = None
    if agg == "MAX":
        a, am = aggregate(x, seg, ids, n, agg, with_argmax=True)
    else:
        a = aggregate(x, seg, ids, n, agg)
    (a * torch.from_numpy(np.asarray(dA)).to(dtype)).sum().backward()
    g = x.grad
    if dSelf is not None:
        g = g + torch.from_numpy(np.asarray(dSelf)).to(dtype)
    if Hprev is not None:
        g = torch.where(torch.from_numpy(np.asarray(Hprev)) <= 0, torch.zeros_like(g), g)
    return a.detach().double().numpy(), am, g.double().numpy()


def param_shapes(L, F, H, C, gcn):
    m = 1 if gcn else 2
    return [(H, m * (F if l == 1 else H)) for l in range(1, L + 1)] + [(C, H), (C,)]


def step_reference(row_ptr, col, X, labels, nodes, params, agg, gcn, bf16=False, dtype=torch.float64):
    """(loss, [gradient per tensor of params], [H_1 .. H_L]) as float64 numpy.

    params: [W_1, .., W_L, Wc, bc] (numpy, fp32 or float64 values); nodes:
    the unique ids the loss averages over; labels: one class per node."""
    n = len(row_ptr) - 1
    L = len(params) - 2
    seg, ids = lists_for(row_ptr, col, gcn, agg)
    leaves = [torch.from_numpy(np.asarray(p, np.float64).copy()).to(dtype).requires_grad_(True) for p in params]
    W, Wc, bc = leaves[:L], leaves[L], leaves[L + 1]
    h = torch.from_numpy(np.asarray(X)).to(dtype)
    hs = []
    for layer in range(1, L + 1):
        a = aggregate(h, seg, ids, n, agg)
        w = W[layer - 1]
        if bf16 and layer == 1:
            a, w = _bf16_value(a), _bf16_value(w)
        h = torch.relu((a if gcn else torch.cat([h, a], 1)).mm(w.t()))
        hs.append(h.detach().double().numpy())
    nodes = np.asarray(nodes, np.int64)
    emb = h[torch.from_numpy(nodes)]
    logp = torch.log_softmax(emb.mm(Wc.t()) + bc, 1)
    y = torch.from_numpy(np.asarray(labels, np.int64)[nodes])
    loss = -torch.sum(logp[range(logp.size(0)), y], 0) / logp.size(0)
    loss.backward()
    return float(loss.detach().double()), [p.grad.double().numpy() for p in leaves], hs
