"""A float64 reference of the exact path with per-edge weights (no tests here,
no GPU).

A plain restatement, from the CSR and the per-entry weights alone, of what
hip_ops.agg_full / agg_full_bwd compute with `edge_weight=` and of one
train.FullTrainer step with `edge_weight=`:

* the effective entries of destination v are those of
  full_train_ref.visit_lists (the kernels' visiting order): v's CSR row
  without the entries equal to v, whose weights are ignored; under gcn every
  entry of the row with its own weight, self entries included, and where the
  row holds no self entry v appended last with weight self_weight[v];
* S[v] = sum of w_e * rows[col_e]; norm "sum": out = S; norm "mean":
  out = S / den with den[v] = sum of w_e -- an index-add in the run's dtype;
* the layers, the heads (log_softmax + NLL mean, or
  binary_cross_entropy_with_logits mean with an optional pos_weight over
  multi-hot labels), the bf16 handling and torch autograd for the gradients
  are full_train_ref.step_reference's; the unsupervised head is
  full_unsup_ref.pair_loss on the weighted forward.

The weights are data: nothing here differentiates with respect to them.
`dtype` runs the same code in fp32: that run is the yardstick e_torch of
tests/adam_cases.check_rule.
"""
import numpy as np
import torch
import torch.nn.functional as F

from tests import full_train_ref as tref
from tests import full_unsup_ref as uref
from tests.step_ref import _bf16_value


def self_weights(self_weight, n):
    """A scalar or [n] self_weight as float64 [n]."""
    sw = np.asarray(self_weight, np.float64)
    return np.full(n, float(sw)) if sw.ndim == 0 else sw.reshape(n).copy()


def weighted_lists(row_ptr, col, w, gcn, self_weight=1.0):
    """(destination, source, weight) per effective entry, in the kernels'
    visiting order: the lists of full_train_ref.visit_lists with the weight
    each entry carries."""
    row_ptr = np.asarray(row_ptr, np.int64)
    col = np.asarray(col, np.int64)
    w = np.asarray(w, np.float64)
    n = len(row_ptr) - 1
    sw = self_weights(self_weight, n)
    wts = []
    for v in range(n):
        row = col[row_ptr[v]:row_ptr[v + 1]]
        wr = w[row_ptr[v]:row_ptr[v + 1]]
        if gcn:
            wr = wr if (row == v).any() else np.concatenate([wr, [sw[v]]])
        else:
            wr = wr[row != v]
        wts.append(wr)
    seg, ids = tref.visit_lists(row_ptr, col, gcn)
    wts = np.concatenate(wts) if wts else np.zeros(0)
    assert len(wts) == len(ids)
    return seg, ids, wts


def denominators(seg, wts, n):
    """den[v], the plain float64 sum of a row's effective weights."""
    return np.bincount(seg, weights=wts, minlength=n).astype(np.float64)


def aggregate(rows, seg, ids, wts, n_dst, norm):
    """The weighted sum or mean of rows[ids] per destination (torch, rows' dtype, differentiable in rows)."""
    seg_t, ids_t = torch.from_numpy(seg), torch.from_numpy(ids)
    wt = torch.from_numpy(wts).to(rows.dtype)
    out = torch.zeros(n_dst, rows.shape[1], dtype=rows.dtype).index_add(0, seg_t, rows[ids_t] * wt.unsqueeze(1))
    if norm == "sum":
        return out
    if norm != "mean":
        raise ValueError(norm)
    den = torch.zeros(n_dst, dtype=rows.dtype).index_add(0, seg_t, wt)
    return out / den.unsqueeze(1)


def aggregate_reference(row_ptr, col, w, X, gcn, norm, self_weight=1.0, bf16=False, dtype=torch.float64):
    """hip_ops.agg_full(edge_weight=)'s output for every row as float64 numpy, rounded to bf16 for a bf16 table."""
    n = len(row_ptr) - 1
    seg, ids, wts = weighted_lists(row_ptr, col, w, gcn, self_weight)
    a = aggregate(torch.from_numpy(np.asarray(X)).to(dtype), seg, ids, wts, n, norm)
    if bf16:
        a = _bf16_value(a)
    return a.double().numpy()


def aggregate_backward(row_ptr, col, w, X, dA, gcn, norm, self_weight=1.0, dSelf=None, Hprev=None,
                       dtype=torch.float64):
    """(the weighted aggregate, dH): dH is the gradient of sum(A * dA) with respect to X, plus dSelf, zeroed
    where Hprev <= 0 -- full_train_ref.aggregate_backward with weights."""
    n = len(row_ptr) - 1
    seg, ids, wts = weighted_lists(row_ptr, col, w, gcn, self_weight)
    x = torch.from_numpy(np.asarray(X)).to(dtype).requires_grad_(True)
    a = aggregate(x, seg, ids, wts, n, norm)
    (a * torch.from_numpy(np.asarray(dA)).to(dtype)).sum().backward()
    g = x.grad
    if dSelf is not None:
        g = g + torch.from_numpy(np.asarray(dSelf)).to(dtype)
    if Hprev is not None:
        g = torch.where(torch.from_numpy(np.asarray(Hprev)) <= 0, torch.zeros_like(g), g)
    return a.detach().double().numpy(), g.double().numpy()


def forward(lists, n, X, W, gcn, norm, bf16, dtype, keep=None):
    """H_L (torch, on the graph of the leaves W); `keep` collects every H_l as float64 numpy."""
    seg, ids, wts = lists
    h = torch.from_numpy(np.asarray(X)).to(dtype)
    for layer, w in enumerate(W, 1):
        a = aggregate(h, seg, ids, wts, n, norm)
        if bf16 and layer == 1:
            a, w = _bf16_value(a), _bf16_value(w)
        h = torch.relu((a if gcn else torch.cat([h, a], 1)).mm(w.t()))
        if keep is not None:
            keep.append(h.detach().double().numpy())
    return h


def _leaves(params, dtype):
    return [torch.from_numpy(np.asarray(p, np.float64).copy()).to(dtype).requires_grad_(True) for p in params]


def step_reference(row_ptr, col, w, X, labels, nodes, params, gcn, norm="mean", self_weight=1.0, bf16=False,
                   dtype=torch.float64, head="nll", pos_weight=None):
    """(loss, [gradient per tensor of params], [H_1 .. H_L]) as float64 numpy:
    full_train_ref.step_reference over the weighted aggregate.  head "nll":
    labels holds one class per node; "multilabel": a [N, C] multi-hot array."""
    n = len(row_ptr) - 1
    L = len(params) - 2
    leaves = _leaves(params, dtype)
    hs = []
    h = forward(weighted_lists(row_ptr, col, w, gcn, self_weight), n, X, leaves[:L], gcn, norm, bf16, dtype, hs)
    nodes = np.asarray(nodes, np.int64)
    z = h[torch.from_numpy(nodes)].mm(leaves[L].t()) + leaves[L + 1]
    if head == "nll":
        logp = torch.log_softmax(z, 1)
        y = torch.from_numpy(np.asarray(labels, np.int64)[nodes])
        loss = -torch.sum(logp[range(logp.size(0)), y], 0) / logp.size(0)
    elif head == "multilabel":
        y = torch.from_numpy(np.asarray(labels)[nodes]).to(dtype)
        pw = None if pos_weight is None else torch.from_numpy(np.asarray(pos_weight, np.float64)).to(dtype)
        loss = F.binary_cross_entropy_with_logits(z, y, pos_weight=pw, reduction="mean")
    else:
        raise ValueError(head)
    loss.backward()
    return float(loss.detach().double()), [p.grad.double().numpy() for p in leaves], hs


def unsup_step_reference(row_ptr, col, w, X, nodes, params, gcn, lists, kind, q, margin, norm="mean",
                         self_weight=1.0, bf16=False, dtype=torch.float64):
    """(loss, [gradient per tensor of params; zeros for the classifier]) of one "unsup" step:
    full_unsup_ref.pair_loss (kind "sage" or a margin kind) over the rows `nodes` of the weighted forward."""
    n = len(row_ptr) - 1
    L = len(params) - 2
    leaves = _leaves(params, dtype)
    h = forward(weighted_lists(row_ptr, col, w, gcn, self_weight), n, X, leaves[:L], gcn, norm, bf16, dtype)
    emb = h[torch.from_numpy(np.asarray(nodes, np.int64))]
    loss = uref.pair_loss(emb, lists, kind, q, margin)[0]
    loss.backward()
    return float(loss.detach().double()), [(torch.zeros_like(p) if p.grad is None else p.grad).double().numpy()
                                           for p in leaves]
