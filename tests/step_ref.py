"""A float64 reference of one supervised step, built from the pack (no tests
here, no GPU).

A plain restatement of what NativeTrainer.forward_backward + apply_update
compute for one batch, independent of oracle/ (which restates the reference's
dense-mask form from its own sampling) and of the sampler's rules: it decodes
the host view of a sample, `Sample.hop(j)`, in the layout DESIGN §3 and
tests/fullsize_parity.py describe, and does the arithmetic with torch on the
CPU, gradients from autograd:

* layer 1 (the last hop): destination r = dst_ids[r] reads the feature rows
  col[row_ptr[dst] + pos] of its sampled CSR entries, minus itself (plus
  itself under gcn);
* layers >= 2 (hop j = L - layer + 1): destination r reads the rows
  nbr[nbr_ptr[r]:nbr_ptr[r + 1]] of the previous layer's output (union-local
  ids, the self rule already applied) and its own row self[r];
* MEAN is an index-add mean, MAX a gather-max;
* h = relu(W . [self | agg]), or relu(W . agg) under gcn;
* log_softmax(emb . Wc^T + bc) and the NLL mean exactly as oracle.nll_loss
  states them.

`dtype` runs the same code in fp32: that run is the yardstick e_torch of
tests/adam_cases.check_rule.  bf16 features (bf16=True): X holds bf16 values,
and layer 1's aggregate and W1 enter the GEMM rounded to bf16 in value only
(the gradient reaches the fp32 W1), the rounding points of
oracle.forward_dense(bf16_layer1=True).

clip_sgd is the update: the per-group clip [sage weights], [Wc, bc] with
coef = min(max_norm / (norm + 1e-6), 1), then SGD, in float64 on a given raw
gradient.
"""
import numpy as np
import torch


def param_shapes(L, F, H, C, gcn):
    """Shapes of the flat parameter buffer's tensors: W1 .. WL, Wc, bc."""
    m = 1 if gcn else 2
    return [(H, m * (F if l == 1 else H)) for l in range(1, L + 1)] + [(C, H), (C,)]


def param_offsets(L, F, H, C, gcn):
    """Offsets of those tensors in the flat buffer (one more entry: the total)."""
    return np.concatenate([[0], np.cumsum([int(np.prod(s)) for s in param_shapes(L, F, H, C, gcn)])]).astype(np.int64)


def _lists(ptr, idx):
    """(segment id per entry, entries) of a CSR-style list-of-lists."""
    ptr = np.asarray(ptr, np.int64)
    return np.repeat(np.arange(len(ptr) - 1), np.diff(ptr)), np.asarray(idx, np.int64)


def layer1_lists(hop, row_ptr, col, gcn):
    """Per-destination neighbour ids of the last hop (node ids): the sampled
    CSR entries' ids without the destination itself; with it under gcn."""
    dst = np.asarray(hop.dst_ids, np.int64)
    seg, pos = _lists(hop.pos_ptr, hop.pos)
    ids = np.asarray(col, np.int64)[np.asarray(row_ptr, np.int64)[dst[seg]] + pos]
    keep = ids != dst[seg]
    seg, ids = seg[keep], ids[keep]
    if gcn:
        seg = np.concatenate([seg, np.arange(len(dst))])
        ids = np.concatenate([ids, dst])
        order = np.argsort(seg, kind="stable")
        seg, ids = seg[order], ids[order]
    return seg, ids, len(dst)


def _aggregate(rows, seg, idx, n_dst, agg):
    """rows[idx] reduced per destination seg: MEAN (index-add) or MAX (gather)."""
    seg_t, idx_t = torch.from_numpy(seg), torch.from_numpy(idx)
    cnt = np.bincount(seg, minlength=n_dst)
    if agg == "MEAN":
        out = torch.zeros(n_dst, rows.shape[1], dtype=rows.dtype).index_add(0, seg_t, rows[idx_t])
        return out / torch.from_numpy(cnt).to(rows.dtype).unsqueeze(1)
    if agg != "MAX":
        raise ValueError(agg)
    if cnt.min() < 1:
        raise IndexError("MAX over an empty neighbourhood")
    # pad every list to the longest with its own first entry: a max is unchanged by a repeat
    start = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    k = np.arange(cnt.max())[None, :]
    take = start[:, None] + np.where(k < cnt[:, None], k, 0)
    gathered = rows[torch.from_numpy(idx[take])]  # [n_dst, kmax, D]
    return gathered.max(dim=1).values


def _bf16_value(t):
    """t rounded to bf16 in value only; the gradient passes straight through."""
    r = t.detach().to(torch.bfloat16).to(t.dtype)
    return t + (r - t.detach())


def step_reference(sample, row_ptr, col, X, labels, roots, params, L, H, C, agg, gcn, bf16=False,
                   dtype=torch.float64):
    """One step's root embeddings [B, H], loss and flat gradient
    [W1 | .. | WL | Wc | bc] (numpy float64) from `params` (the flat
    parameters, fp32 or float64 values) and the host sample `sample` of `roots`.

    X: the feature table (numpy fp32; bf16-representable when bf16)."""
    F = X.shape[1]
    offs = param_offsets(L, F, H, C, gcn)
    shapes = param_shapes(L, F, H, C, gcn)
    params = np.asarray(params).astype(np.float64).reshape(-1)
    assert params.size == offs[-1]
    leaves = [torch.from_numpy(params[offs[i]:offs[i + 1]].copy()).to(dtype).reshape(s)
              .requires_grad_(True) for i, s in enumerate(shapes)]
    W, Wc, bc = leaves[:L], leaves[L], leaves[L + 1]
    Xt = torch.from_numpy(np.asarray(X)).to(dtype)
    h = None
    for layer in range(1, L + 1):
        j = L - layer + 1
        hop = sample.hop(j)
        if layer == 1:
            seg, idx, n_dst = layer1_lists(hop, row_ptr, col, gcn)
            src = Xt
            self_rows = Xt[torch.from_numpy(np.asarray(hop.dst_ids, np.int64))]
        else:
            seg, idx = _lists(hop.nbr_ptr, hop.nbr)
            n_dst = hop.n_dst
            src = h
            self_rows = h[torch.from_numpy(np.asarray(hop.self_local, np.int64))]
        a = _aggregate(src, seg, idx, n_dst, agg)
        w = W[layer - 1]
        if bf16 and layer == 1:
            a, w = _bf16_value(a), _bf16_value(w)
        h = torch.relu((a if gcn else torch.cat([self_rows, a], 1)).mm(w.t()))
    emb = h
    assert emb.shape == (len(roots), H)
    logp = torch.log_softmax(emb.mm(Wc.t()) + bc, 1)
    y = torch.from_numpy(np.asarray(labels, np.int64)[np.asarray(roots, np.int64)])
    loss = -torch.sum(logp[range(logp.size(0)), y], 0) / logp.size(0)
    loss.backward()
    grad = np.concatenate([p.grad.double().numpy().reshape(-1) for p in leaves])
    return emb.detach().double().numpy(), float(loss.detach().double()), grad


def clip_sgd(params, grad, group_off, lr, max_norm):
    """The update in float64: per group [group_off[g], group_off[g + 1]) the
    gradient is scaled by min(max_norm / (norm + 1e-6), 1), then p -= lr * g.
    Returns (parameters, clipped gradient)."""
    p = np.asarray(params).astype(np.float64).reshape(-1)
    g = np.asarray(grad).astype(np.float64).reshape(-1).copy()
    for lo, hi in zip(group_off[:-1], group_off[1:]):
        lo, hi = int(lo), int(hi)
        norm = np.sqrt(np.sum(g[lo:hi] * g[lo:hi]))
        g[lo:hi] *= min(max_norm / (norm + 1e-6), 1.0)
    return p - lr * g, g


def clip_sgd_torch_fp32(params, grad, group_off, lr, max_norm):
    """The same update as fp32 torch on the CPU does it (clip_grad_norm_ per
    group + SGD): check_rule's yardstick for the update.  float64 numpy out."""
    p = torch.from_numpy(np.asarray(params, np.float32).reshape(-1).copy())
    g = torch.from_numpy(np.asarray(grad, np.float32).reshape(-1).copy())
    qs = []
    for lo, hi in zip(group_off[:-1], group_off[1:]):
        q = p[int(lo):int(hi)].clone().requires_grad_(True)
        q.grad = g[int(lo):int(hi)].clone()
        torch.nn.utils.clip_grad_norm_([q], max_norm)
        qs.append(q)
    with torch.no_grad():
        for q in qs:
            q.add_(q.grad, alpha=-lr)
    return (torch.cat([q.detach() for q in qs]).double().numpy(),
            torch.cat([q.grad for q in qs]).double().numpy())
