"""A float64 reference of one exact training step under the unsupervised
losses (no tests here, no GPU).

The forward is full_train_ref's (its lists_for, aggregate and bf16 rounding),
over all N nodes; on the rows h[nodes] goes the loss loop of
unsup_loss_cases.reference -- get_loss_sage / get_loss_margin of
models.py:65-132 with the reference's own calls -- and, for "plus_unsup", the
NLL mean over the same rows (utils.py:153-169), added sup first.  torch
autograd carries the loss to every parameter.  `dtype` runs the same code in
fp32: the unit e_torch of adam_cases.check_rule.
"""
import numpy as np
import torch
import torch.nn.functional as F

from tests import unsup_loss_cases as ulc
from tests.full_train_ref import aggregate, lists_for
from tests.step_ref import _bf16_value


def forward(row_ptr, col, X, W, agg, gcn, bf16, dtype):
    """H_L (torch, on the graph of the leaves W) of full_train_ref.step_reference's forward."""
    n = len(row_ptr) - 1
    seg, ids = lists_for(row_ptr, col, gcn, agg)
    h = torch.from_numpy(np.asarray(X)).to(dtype)
    for layer, w in enumerate(W, 1):
        a = aggregate(h, seg, ids, n, agg)
        if bf16 and layer == 1:
            a, w = _bf16_value(a), _bf16_value(w)
        h = torch.relu((a if gcn else torch.cat([h, a], 1)).mm(w.t()))
    return h


def pair_loss(emb, lists, kind, q, margin):
    """unsup_loss_cases.reference's loop on the rows of the torch tensor `emb` (kept on its graph).
    Returns (loss, cos tensors [positive lists, then negative lists], scores, selection dict)."""
    pos_lists, neg_lists = lists
    zero = torch.tensor(0.0, dtype=emb.dtype)
    nodes_score, cps, cns = [], [], []
    sel = {k: [] for k in ("sel_pos", "sel_neg", "ext_pos", "ext_neg", "h", "gap_pos", "gap_neg", "gap2_pos",
                           "gap2_neg", "ties_pos", "ties_neg")}
    p0 = n0 = 0
    for pps, nps in zip(pos_lists, neg_lists):
        indexs = [list(x) for x in zip(*pps)]
        pos_cos = F.cosine_similarity(emb[indexs[0]], emb[indexs[1]])
        indexs = [list(x) for x in zip(*nps)]
        neg_cos = F.cosine_similarity(emb[indexs[0]], emb[indexs[1]])
        pos_cos.retain_grad()
        neg_cos.retain_grad()
        cps.append(pos_cos)
        cns.append(neg_cos)
        if kind == "sage":
            neg_score = q * torch.mean(torch.log(torch.sigmoid(-neg_cos)), 0)
            pos_score = torch.log(torch.sigmoid(pos_cos))
            nodes_score.append(torch.mean(-pos_score - neg_score).view(1, -1))
        else:
            pos_ls, neg_ls = torch.log(torch.sigmoid(pos_cos)), torch.log(torch.sigmoid(neg_cos))
            pos_score, pi = torch.min(pos_ls, 0)
            neg_score, ni = torch.max(neg_ls, 0)
            h = neg_score - pos_score + margin
            nodes_score.append(torch.max(zero, h).view(1, -1))
            pi, ni = int(pi), int(ni)
            gp, gp2, tp = ulc._extreme(pos_ls.detach().double().numpy(), pi)
            gn, gn2, tn = ulc._extreme(neg_ls.detach().double().numpy(), ni)
            for k, v in (("sel_pos", p0 + pi), ("sel_neg", n0 + ni), ("ext_pos", pos_score.item()),
                         ("ext_neg", neg_score.item()), ("h", h.item()), ("gap_pos", gp), ("gap_neg", gn),
                         ("gap2_pos", gp2), ("gap2_neg", gn2), ("ties_pos", tp), ("ties_neg", tn)):
                sel[k].append(v)
        p0 += len(pps)
        n0 += len(nps)
    scores = torch.cat(nodes_score, 0)
    loss = torch.mean(scores) if kind == "sage" else torch.mean(scores, 0)
    return loss.sum(), cps + cns, scores, sel


def step_reference(row_ptr, col, X, labels, nodes, params, agg, gcn, lists=None, kind=None, q=ulc.Q,
                   margin=ulc.MARGIN, with_sup=False, bf16=False, dtype=torch.float64):
    """One step's loss and gradients as float64 numpy, in a dict:
    loss, loss_sup, loss_net; grads [per tensor of params; zeros where the loss does not reach]; E = h[nodes];
    dE (d loss / d E), dE_net (of the pair loss alone), dZ (dE masked by E > 0: the rows of dZ_L); coef
    (d loss_net / d cos per pair, positive pairs first), score per node and, for a margin kind, the
    selection entries of unsup_loss_cases.reference.  kind None: the supervised loss alone
    (full_train_ref.step_reference restated); otherwise "sage" or any margin kind."""
    L = len(params) - 2
    leaves = [torch.from_numpy(np.asarray(p, np.float64).copy()).to(dtype).requires_grad_(True) for p in params]
    W, Wc, bc = leaves[:L], leaves[L], leaves[L + 1]
    h = forward(row_ptr, col, X, W, agg, gcn, bf16, dtype)
    nodes = np.asarray(nodes, np.int64)
    emb = h[torch.from_numpy(nodes)]
    emb.retain_grad()
    out = {}
    loss_sup = loss_net = None
    if kind is None or with_sup:
        logp = torch.log_softmax(emb.mm(Wc.t()) + bc, 1)
        y = torch.from_numpy(np.asarray(labels, np.int64)[nodes])
        loss_sup = -torch.sum(logp[range(logp.size(0)), y], 0) / logp.size(0)
    if kind is not None:
        loss_net, coss, scores, sel = pair_loss(emb, lists, kind, q, margin)
        out["dE_net"] = torch.autograd.grad(loss_net, emb, retain_graph=True)[0].double().numpy()
        emb.grad = None                 # retain_grad's hooks saw that pass too
        for c in coss:
            c.grad = None
    loss = loss_sup if loss_net is None else (loss_net if loss_sup is None else loss_sup + loss_net)
    loss.backward()
    if kind is not None:
        out["coef"] = torch.cat([torch.zeros_like(c) if c.grad is None else c.grad for c in coss]).double().numpy()
        out["score"] = scores.detach().reshape(-1).double().numpy()
        if kind != "sage":
            for k, v in sel.items():
                out[k] = v if k.startswith("ties") else np.asarray(v, np.int64 if k.startswith("sel") else np.float64)
    E = emb.detach().double().numpy()
    out.update(
        loss=float(loss.detach().double()),
        loss_sup=0.0 if loss_sup is None else float(loss_sup.detach().double()),
        loss_net=0.0 if loss_net is None else float(loss_net.detach().double()),
        grads=[(torch.zeros_like(p) if p.grad is None else p.grad).double().numpy() for p in leaves],
        E=E, dE=emb.grad.double().numpy())
    out["dZ"] = np.where(E > 0, out["dE"], 0.0)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return out
