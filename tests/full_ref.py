"""A float64 reference of exact full-neighbourhood inference, layer by layer
over all nodes (no tests here, no GPU).

A plain restatement of what hip_ops.agg_full and train.FullEmbedder compute,
from the CSR alone and independent of oracle/ (which restates the reference's
dense-mask form; test_full_infer_host.py ties the two together):

* the sources of destination v are the ids of its CSR row without v itself,
  plus v exactly once under gcn (sparse lists: nothing of size N x N);
* MEAN is an index-add mean (a row without sources is 0/0 = NaN), MAX an
  element-wise maximum (IndexError when a row has no sources);
* H_l = relu(W_l . [H_{l-1} | agg]) for every node, or relu(W_l . agg) under
  gcn, with H_0 = X.

`dtype` runs the same code in fp32: that run is the yardstick e_torch of
tests/adam_cases.check_rule.  bf16 features (bf16=True), the handling of
tests/step_ref.py: X holds bf16 values, and layer 1's aggregate and W1 enter
the GEMM rounded to bf16; the layers above run unrounded.
"""
import numpy as np
import torch


def neighbour_lists(row_ptr, col, gcn, row0=0, n_rows=None):
    """(destination per entry, source id per entry) of the rows
    [row0, row0 + n_rows), destinations numbered from 0, in row order."""
    row_ptr = np.asarray(row_ptr, np.int64)
    n = len(row_ptr) - 1
    n_rows = n - row0 if n_rows is None else n_rows
    rp = row_ptr[row0:row0 + n_rows + 1]
    seg = np.repeat(np.arange(n_rows), np.diff(rp))
    ids = np.asarray(col, np.int64)[rp[0]:rp[-1]]
    keep = ids != seg + row0
    seg, ids = seg[keep], ids[keep]
    if gcn:
        seg = np.concatenate([seg, np.arange(n_rows)])
        ids = np.concatenate([ids, np.arange(row0, row0 + n_rows)])
        order = np.argsort(seg, kind="stable")
        seg, ids = seg[order], ids[order]
    return seg, ids


def aggregate(rows, seg, ids, n_dst, agg):
    """rows[ids] reduced per destination seg (torch, rows' dtype)."""
    seg_t, ids_t = torch.from_numpy(seg), torch.from_numpy(ids)
    cnt = np.bincount(seg, minlength=n_dst)
    if agg == "MEAN":
        out = torch.zeros(n_dst, rows.shape[1], dtype=rows.dtype).index_add(0, seg_t, rows[ids_t])
        return out / torch.from_numpy(cnt).to(rows.dtype).unsqueeze(1)
    if agg != "MAX":
        raise ValueError(agg)
    if n_dst and cnt.min() < 1:
        raise IndexError("MAX over an empty neighbourhood")
    out = torch.full((n_dst, rows.shape[1]), -np.inf, dtype=rows.dtype)
    return out.scatter_reduce(0, seg_t.unsqueeze(1).expand(-1, rows.shape[1]), rows[ids_t], "amax", include_self=True)


def _bf16_value(t):
    return t.to(torch.bfloat16).to(t.dtype)


def aggregate_reference(row_ptr, col, X, agg, gcn, row0=0, n_rows=None, bf16=False, dtype=torch.float64):
    """hip_ops.agg_full's output for the rows [row0, row0 + n_rows) as float64
    numpy: the aggregate of X's rows, rounded to bf16 when X is a bf16 table."""
    n = len(row_ptr) - 1
    n_rows = n - row0 if n_rows is None else n_rows
    seg, ids = neighbour_lists(row_ptr, col, gcn, row0, n_rows)
    a = aggregate(torch.from_numpy(np.asarray(X)).to(dtype), seg, ids, n_rows, agg)
    if bf16:
        a = _bf16_value(a)
    return a.double().numpy()


def full_reference(row_ptr, col, X, weights, agg, gcn, bf16=False, dtype=torch.float64):
    """[H_1, .., H_L] for every node (numpy float64, each [N, hidden]).

    X: the feature table (numpy fp32; bf16-representable when bf16);
    weights: the fp32 SageLayer weights, layer 1 first (numpy or torch)."""
    n = len(row_ptr) - 1
    seg, ids = neighbour_lists(row_ptr, col, gcn)
    h = torch.from_numpy(np.asarray(X)).to(dtype)
    outs = []
    for layer, w in enumerate(weights, 1):
        w = torch.as_tensor(np.asarray(w.detach().cpu() if isinstance(w, torch.Tensor) else w)).to(dtype)
        a = aggregate(h, seg, ids, n, agg)
        if bf16 and layer == 1:
            a, w = _bf16_value(a), _bf16_value(w)
        h = torch.relu((a if gcn else torch.cat([h, a], 1)).mm(w.t()))
        outs.append(h.double().numpy())
    return outs
