"""train.FullTrainer(head="multilabel") on the GPU: the exact step with the
sigmoid BCE head (gs_cls_bce_fwd_bwd inside gs_train_full_*) against a float64
restatement -- the forward of tests/full_train_ref.py with
binary_cross_entropy_with_logits on the rows `nodes` and torch autograd --, full
and with `field=`, under SGD and Adam, with `unsup=`, and its evaluation
(MultiLabelEvalResult) against the numpy mirror.

Tolerance (adam_cases.check_rule): err <= 4 * e_torch + 2^-23 * max|ref|, with
e_torch the error of the restatement's own fp32 run on the CPU against its
float64 run, per compared quantity; the loss's yardstick where fp32 torch hits
the float64 mean exactly is the largest error of its terms
(cls_bce_cases.loss_yardstick).
"""
import importlib
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import adam_cases as ac
from tests import cls_bce_cases as K
from tests import full_cases as fc
from tests import full_field_cases as ffc
from tests import full_train_cases as tc
from tests import full_train_ref as tref
from tests import full_unsup_cases as uc
from tests import full_unsup_ref as uref
from tests import step_ref
from tests.adam_cases import check_rule

pytestmark = pytest.mark.gpu

ops = importlib.import_module("graphsage-pytorch_amd.hip_ops")
train = importlib.import_module("graphsage-pytorch_amd.train")
utils = importlib.import_module("graphsage-pytorch_amd.utils")
_lib = importlib.import_module("graphsage-pytorch_amd._lib")
DEV = torch.device("cuda", 0)
_MEMO = {}


def _case(id, graph, L, Fd, H, C, agg, gcn, pw):
    return {"id": id, "graph": graph, "L": L, "F": Fd, "H": H, "C": C, "agg": agg, "gcn": gcn, "pw": pw,
            "bf16": False, "seg_len": tc.SEG_LEN}


CASES = [
    _case("mean_c5", "hub_max", 2, 64, 80, 5, "MEAN", False, False),
    _case("max_c40", "rmat", 2, 128, 80, 40, "MAX", False, True),
    _case("gcn_c40", "hub_max", 2, 50, 16, 40, "MEAN", True, True),
    _case("l3_c5", "directed", 3, 64, 80, 5, "MEAN", False, True),
]
BY_ID = {c["id"]: c for c in CASES}
IDS = [c["id"] for c in CASES]


def _np(t):
    return t.detach().cpu().numpy()


def _setup(case):
    """graph, n, rp, col, X, Xd, Y [n, C] bool, nodes, params, pos_weight (or None)."""
    key = ("setup", case["id"])
    if key not in _MEMO:
        graph, n, rp, col = ffc.graph_of(case["graph"])
        X = fc.features(n, case["F"])
        rs = np.random.RandomState(100 + case["C"])
        Y = rs.uniform(0, 1, (n, case["C"])) < 0.3
        pw = rs.uniform(0.5, 4.0, case["C"]).astype(np.float32) if case["pw"] else None
        nodes = tc.nodes_of(n, k=min(tc.N_NODES_SUBSET, n - 5))
        _MEMO[key] = (graph, n, rp, col, X, torch.from_numpy(X).to(DEV), Y, nodes, tc.params_of(case), pw)
    return _MEMO[key]


def _trainer(case, params=None, head="multilabel", labels=None, **kw):
    graph, n, rp, col, X, Xd, Y, nodes, params0, pw = _setup(case)
    params = params0 if params is None else params
    L = case["L"]
    w = ([torch.from_numpy(np.array(p)) for p in params[:L]], torch.from_numpy(np.array(params[L])),
         torch.from_numpy(np.array(params[L + 1])))
    args = {"seg_len": case["seg_len"]}
    if head == "multilabel":
        args.update(head=head, pos_weight=None if pw is None else torch.from_numpy(pw))
        labels = torch.from_numpy(Y) if labels is None else labels
    elif head is not None:
        args["head"] = head
    args.update(kw)
    return train.FullTrainer(graph, Xd, labels, case["C"], num_layers=L, hidden=case["H"], agg_func=case["agg"],
                             gcn=case["gcn"], weights=w, **args)


def ml_reference(case, params, dtype=torch.float64, lists=None, kind=None, q=uc.Q, margin=uc.MARGIN, nodes=None):
    """One step with the BCE head as float64 numpy: the forward of full_train_ref (its lists_for and aggregate),
    binary_cross_entropy_with_logits (mean, pos_weight) over the rows `nodes`, plus (kind) the pair loss of
    full_unsup_ref over the same rows, and autograd.  A dict: loss, loss_sup, loss_net, l (the BCE terms), z,
    grads, H (every H_l)."""
    graph, n, rp, col, X, Xd, Y, nodes0, _p, pw = _setup(case)
    nodes = np.asarray(nodes0 if nodes is None else nodes, np.int64)
    L = case["L"]
    seg, ids = tref.lists_for(rp, col, case["gcn"], case["agg"])
    leaves = [torch.from_numpy(np.asarray(p, np.float64).copy()).to(dtype).requires_grad_(True) for p in params]
    W, Wc, bc = leaves[:L], leaves[L], leaves[L + 1]
    h = torch.from_numpy(np.asarray(X)).to(dtype)
    hs = []
    for w in W:
        a = tref.aggregate(h, seg, ids, n, case["agg"])
        h = torch.relu((a if case["gcn"] else torch.cat([h, a], 1)).mm(w.t()))
        hs.append(h.detach().double().numpy())
    emb = h[torch.from_numpy(nodes)]
    z = emb.mm(Wc.t()) + bc
    y = torch.from_numpy(Y[nodes]).to(dtype)
    pwt = None if pw is None else torch.from_numpy(pw).to(dtype)
    loss_sup = F.binary_cross_entropy_with_logits(z, y, pos_weight=pwt, reduction="mean")
    l = F.binary_cross_entropy_with_logits(z.detach(), y, pos_weight=pwt, reduction="none")
    loss_net = None
    if kind is not None:
        loss_net = uref.pair_loss(emb, lists, kind, q, margin)[0]
    loss = loss_sup if loss_net is None else loss_sup + loss_net
    loss.backward()
    return types.SimpleNamespace(
        loss=float(loss.detach().double()), loss_sup=float(loss_sup.detach().double()),
        loss_net=0.0 if loss_net is None else float(loss_net.detach().double()), l=l.double().numpy(),
        z=z.detach().double().numpy(), H=hs,
        grads=[(torch.zeros_like(p) if p.grad is None else p.grad).double().numpy() for p in leaves])


def _refs(case):
    key = ("ref", case["id"])
    if key not in _MEMO:
        p = _setup(case)[8]
        _MEMO[key] = (ml_reference(case, p), ml_reference(case, p, torch.float32))
    return _MEMO[key]


def _check_grads(tag, tr, r64, r32, L, skip_cls=False):
    for i, pname in enumerate(tc.names_of(L)):
        got = _np(tr.p.view(i, grad=True))
        if skip_cls and i >= L:
            continue
        assert got.shape == r64.grads[i].shape and np.abs(r64.grads[i]).max() > 0
        check_rule(f"{tag} d{pname}", got, r64.grads[i].reshape(-1), r32.grads[i].reshape(-1))


# ------------------------------------------------------------ 1. one step, full and field
@pytest.mark.parametrize("case_id", IDS)
def test_step_matches_float64_full_and_field(gs, case_id):
    case = BY_ID[case_id]
    graph, n, rp, col, X, Xd, Y, nodes, params, pw = _setup(case)
    r64, r32 = _refs(case)
    L = case["L"]
    tr = _trainer(case)
    assert tr.labels.dtype == torch.int32 and tuple(tr.labels.shape) == (n, (case["C"] + 31) // 32)
    assert torch.equal(ops.unpack_multilabel(tr.labels, case["C"]).cpu(), torch.from_numpy(Y))
    before = tr.p.params.clone()
    loss = tr.forward_backward(nodes).clone()
    torch.cuda.synchronize()
    assert torch.equal(tr.p.params, before)
    tag = f"multilabel step {case_id}"
    yard = K.loss_yardstick(types.SimpleNamespace(loss=r64.loss_sup, l=r64.l),
                            types.SimpleNamespace(loss=r32.loss_sup, l=r32.l))
    check_rule(f"{tag} loss", [float(loss)], np.array([r64.loss]), yard)
    check_rule(f"{tag} H_L", _np(tr.hidden()), r64.H[-1].reshape(-1), r32.H[-1].reshape(-1))
    _check_grads(tag, tr, r64, r32, L)
    full_grads = tr.p.grads.clone()
    again = tr.forward_backward(nodes).clone()
    assert torch.equal(again, loss) and torch.equal(tr.p.grads, full_grads)      # bitwise repeatable

    ft = _trainer(case)
    field = ft.field(nodes)
    assert all(s <= n for s in field.sizes)
    floss = ft.forward_backward(nodes, field=field).clone()
    torch.cuda.synchronize()
    check_rule(f"{tag} field loss", [float(floss)], np.array([r64.loss]), yard)
    _check_grads(f"{tag} field", ft, r64, r32, L)
    # the head sees bitwise the same rows of H_L on both paths and is a function of its operands alone
    assert torch.equal(floss, loss)
    for i in (L, L + 1):
        assert torch.equal(ft.p.view(i, grad=True), tr.p.view(i, grad=True)), tr.p.names[i]


# ------------------------------------------------------------ 2. three updates
@pytest.mark.parametrize("optimizer", ["sgd", "adam"])
@pytest.mark.parametrize("case_id", ["mean_c5", "max_c40"])
def test_three_updates(gs, case_id, optimizer):
    """Teacher-forced as test_gpu_full_train.py does it: at the parameters the device holds, every raw gradient
    against the float64 step, then every parameter after apply_update against the float64 update of that raw
    gradient."""
    case = BY_ID[case_id]
    graph, n, rp, col, X, Xd, Y, nodes, params, pw = _setup(case)
    L = case["L"]
    g0 = _refs(case)[0].grads
    offs = np.concatenate([[0], np.cumsum([p.size for p in params])]).astype(np.int64)
    goff = np.array([0, offs[L], offs[-1]], np.int64)
    flat0 = np.concatenate([g.reshape(-1) for g in g0])
    norms = [np.sqrt((flat0[goff[k]:goff[k + 1]] ** 2).sum()) for k in range(2)]
    max_norm = ac.f32(0.25 * min(norms))                   # both groups clip at step 1
    lr, betas, eps, wd = ac.f32(0.05), (ac.f32(0.9), ac.f32(0.999)), ac.f32(1e-8), ac.f32(0.01)
    tr = _trainer(case, lr=lr, max_norm=max_norm, optimizer=optimizer, betas=betas, eps=eps, weight_decay=wd)
    assert np.array_equal(tr.p.group_off, goff)
    nodes_d = torch.from_numpy(nodes.astype(np.int32)).to(DEV)
    for t in range(1, 4):
        p0 = _np(tr.p.params)
        cur = [p0[offs[i]:offs[i + 1]].reshape(params[i].shape) for i in range(L + 2)]
        r64, r32 = ml_reference(case, cur), ml_reference(case, cur, torch.float32)
        st = tr.optimizer_state()
        assert st["step"] == t - 1
        tr.forward_backward(nodes_d)
        graw = _np(tr.p.grads)
        for i, pname in enumerate(tc.names_of(L)):
            check_rule(f"multilabel {optimizer} {case_id} step {t} d{pname}", graw[offs[i]:offs[i + 1]],
                       r64.grads[i].reshape(-1), r32.grads[i].reshape(-1))
        if optimizer == "sgd":
            want = step_ref.clip_sgd(p0, graw, goff, lr, max_norm)[0]
            tor = step_ref.clip_sgd_torch_fp32(p0, graw, goff, lr, max_norm)[0]
        else:
            m0, v0 = _np(st["m"]), _np(st["v"])
            want = ac.reference_adamw(p0, graw, m0, v0, t, lr, betas, eps, wd, goff, 1.0, max_norm)[0]
            tor = ac.torch_adamw(p0, graw, m0, v0, t, lr, betas, eps, wd, goff, 1.0, max_norm, torch.float32)[0]
        tr.apply_update()
        torch.cuda.synchronize()
        got = _np(tr.p.params)
        assert not np.array_equal(got, p0)
        for i, pname in enumerate(tc.names_of(L)):
            lo, hi = offs[i], offs[i + 1]
            check_rule(f"multilabel {optimizer} {case_id} step {t} {pname}", got[lo:hi], want[lo:hi], tor[lo:hi])
    assert tr.optimizer_state()["step"] == 3


# ------------------------------------------------------------ 3. with the unsupervised losses
UNSUP_CASE = "l2_h16-hub_max"


def _unsup_setup():
    """full_unsup_cases' case (its graph, extended batch and pair plan) with C = 5 multi-hot labels."""
    s = uc.setup(UNSUP_CASE)
    case = dict(_case("unsup_c5", s["graph"], s["L"], s["F"], s["H"], 5, s["agg"], s["gcn"], True))
    return s, case


@pytest.mark.parametrize("path", ["full", "field"])
def test_plus_unsup_adds_the_bce_mean(gs, path):
    s, case = _unsup_setup()
    graph, n, rp, col, X, Xd, Y, _nodes, params, pw = _setup(case)
    assert np.array_equal(X, s["X"])
    tr = _trainer(case)
    plan = torch.from_numpy(s["plan"].copy()).to(DEV)
    b = tr.unsup_batch((plan, s["dims"], s["nodes"]), kind="normal", learn_method="plus_unsup", q=uc.Q,
                       margin=uc.MARGIN)
    field = tr.field(b.nodes) if path == "field" else None
    loss = tr.forward_backward(b.nodes, field=field, unsup=b)
    torch.cuda.synchronize()
    r64 = ml_reference(case, params, lists=s["lists"], kind="sage", nodes=s["nodes"])
    r32 = ml_reference(case, params, torch.float32, lists=s["lists"], kind="sage", nodes=s["nodes"])
    total, sup, net = (float(x) for x in tr.loss_parts())
    tag = f"multilabel plus_unsup {path}"
    yard = K.loss_yardstick(types.SimpleNamespace(loss=r64.loss_sup, l=r64.l),
                            types.SimpleNamespace(loss=r32.loss_sup, l=r32.l))
    check_rule(f"{tag} loss_sup", [sup], np.array([r64.loss_sup]), yard)
    assert total == float(np.float32(sup) + np.float32(net)) and float(loss) == total
    # the pair loss reads E alone: bitwise the single-label trainer's at the same parameters (test_gpu_full_unsup.py
    # holds that one against float64)
    nl = _trainer(case, head="nll", labels=torch.from_numpy(tc.labels_of(n, case["C"])))
    nb = nl.unsup_batch((plan, s["dims"], s["nodes"]), kind="normal", learn_method="plus_unsup", q=uc.Q,
                        margin=uc.MARGIN)
    nl.forward_backward(nb.nodes, field=nl.field(nb.nodes) if path == "field" else None, unsup=nb)
    torch.cuda.synchronize()
    assert float(nl.loss_parts()[2]) == net and net > 0
    _check_grads(tag, tr, r64, r32, case["L"])


@pytest.mark.parametrize("optimizer", ["sgd", "adam"])
def test_unsup_still_leaves_the_classifier_alone(gs, optimizer):
    s, case = _unsup_setup()
    params = _setup(case)[8]
    L = case["L"]
    tr = _trainer(case, optimizer=optimizer, lr=0.05, weight_decay=0.01 if optimizer == "adam" else 0.0)
    tr.step(s["nodes"])                                         # a supervised step first: Adam moments exist
    plan = torch.from_numpy(s["plan"].copy()).to(DEV)
    b = tr.unsup_batch((plan, s["dims"], s["nodes"]), kind="normal", learn_method="unsup")
    cls = [tr.p.view(i).clone() for i in (L, L + 1)]
    lo = int(tr.p.offsets[L])
    mom = None if tr.opt_m is None else (tr.opt_m[lo:].clone(), tr.opt_v[lo:].clone())
    sage = tr.p.view(0).clone()
    tr.step(b.nodes, unsup=b)
    torch.cuda.synchronize()
    assert not torch.equal(tr.p.view(0), sage)
    assert all(torch.equal(tr.p.view(i), c) for i, c in zip((L, L + 1), cls))
    assert not bool(tr.p.grads[lo:].any()) and float(tr.loss_parts()[1]) == 0.0
    if mom is not None:
        assert torch.equal(tr.opt_m[lo:], mom[0]) and torch.equal(tr.opt_v[lo:], mom[1])


# ------------------------------------------------------------ 4. evaluation
@pytest.mark.parametrize("case_id", IDS)
def test_evaluate_against_the_mirror(gs, case_id):
    case = BY_ID[case_id]
    graph, n, rp, col, X, Xd, Y, nodes, params, pw = _setup(case)
    L, C = case["L"], case["C"]
    tr = _trainer(case, lr=0.05)
    for _ in range(2):
        tr.step(nodes)
    state = (tr.p.params.clone(), tr.p.grads.clone(), tr.optimizer_state()["step"])
    ev = np.setdiff1d(np.arange(n), nodes)[:41].astype(np.int64)      # rows the steps did not train on
    res = tr.evaluate(ev, want_logp=True)
    assert isinstance(res, train.MultiLabelEvalResult)
    torch.cuda.synchronize()
    assert torch.equal(tr.p.params, state[0]) and torch.equal(tr.p.grads, state[1])
    assert tr.optimizer_state()["step"] == state[2]
    H = _np(tr.hidden())
    Wc, bc = _np(tr.p.view(L)), _np(tr.p.view(L + 1))
    m_loss, m_counts, m_exact, m_pred, m_z = ops.cls_bce_eval_host(H, Y[ev], Wc, bc, rows=ev, pos_weight=pw)
    r64 = K.torch_reference(H[ev], Y[ev], Wc, bc, pw, torch.float64)
    r32 = K.torch_reference(H[ev], Y[ev], Wc, bc, pw, torch.float32)
    assert abs(m_loss - r64.loss) < 1e-12 and np.abs(m_z - r64.z).max() < 1e-10
    tag = f"multilabel evaluate {case_id}"
    check_rule(f"{tag} loss", [float(res.loss)], np.array([m_loss]), K.loss_yardstick(r64, r32))
    check_rule(f"{tag} logits", _np(res.logits), m_z.reshape(-1), r32.z.reshape(-1))
    keep = K.margin_rule(r64.z, r32.z)
    assert (~keep).sum() <= K.MARGIN_CAP * keep.size
    bits = _np(res.pred)
    assert bits.shape == (len(ev), C) and bits.dtype == bool
    np.testing.assert_array_equal(bits[keep], m_pred[keep])
    counts = _np(res.counts)
    np.testing.assert_array_equal(counts, K.counts_of(bits, Y[ev]))
    assert res.n_exact == int((bits == Y[ev]).all(1).sum())
    if keep.all():
        np.testing.assert_array_equal(counts, m_counts)
        assert res.n_exact == m_exact
    want = K.f1_restated(bits, Y[ev])
    for k in ("micro_f1", "macro_f1", "subset_accuracy"):
        assert abs(getattr(res, k) - want[k]) < 1e-14, k
    np.testing.assert_allclose(res.per_label["f1"], want["f1"], rtol=0, atol=1e-14)
    # through the field of the evaluated rows: the same rows of H_L, so the same result bit for bit
    fres = tr.evaluate(ev, field=tr.field(ev), want_logp=True)
    assert torch.equal(fres.loss, res.loss) and torch.equal(fres.counts, res.counts)
    assert torch.equal(fres.pred_words, res.pred_words) and torch.equal(fres.logits, res.logits)
    assert fres.n_exact == res.n_exact and fres.micro_f1 == res.micro_f1


def test_evaluate_full_accepts_a_multilabel_trainer(gs, tmp_path, monkeypatch, capsys):
    case = BY_ID["mean_c5"]
    graph, n, rp, col, X, Xd, Y, nodes, params, pw = _setup(case)
    tr = _trainer(case, lr=0.05)
    perm = np.random.RandomState(4).permutation(n)
    dc = types.SimpleNamespace(g_val=perm[:60], g_test=perm[60:150])
    tr.step(perm[150:])
    monkeypatch.chdir(tmp_path)
    want_val, want_test = tr.evaluate(dc.g_val).micro_f1, tr.evaluate(dc.g_test).micro_f1
    capsys.readouterr()
    m = utils.evaluate_full(dc, "g", tr, -1.0, "ml", 3)
    assert m == want_val and 0.0 <= want_val <= 1.0
    assert capsys.readouterr().out.splitlines() == [f"Validation F1: {want_val}", f"Test F1: {want_test}"]
    assert (tmp_path / "models" / "model_best_ml_ep3_{:.4f}.torch".format(want_test)).exists()


# ------------------------------------------------------------ 5. the single-label head beside it
@pytest.mark.parametrize("case_id", ["mean_c5", "max_c40"])
def test_nll_head_is_unchanged_and_state_moves_between_heads(gs, case_id):
    case = BY_ID[case_id]
    graph, n, rp, col, X, Xd, Y, nodes, params, pw = _setup(case)
    L, C = case["L"], case["C"]
    y1 = torch.from_numpy(tc.labels_of(n, C))
    ml = _trainer(case, lr=0.05)                                           # built beside the two below
    a = _trainer(case, head="nll", labels=y1, lr=0.05, optimizer="adam")
    b = _trainer(case, head=None, labels=y1, lr=0.05, optimizer="adam")   # the call of before: `head` omitted
    assert a.head == b.head == "nll" and a.cfg.head == 0 and ml.cfg.head == 1 and a.ws_bytes == b.ws_bytes
    for _ in range(3):
        la, lb = a.step(nodes).clone(), b.step(nodes).clone()
        ml.step(nodes)
        assert torch.equal(la, lb) and torch.equal(a.p.grads, b.p.grads) and torch.equal(a.p.params, b.p.params)
    assert torch.equal(a.opt_m, b.opt_m) and torch.equal(a.opt_v, b.opt_v)
    r = a.evaluate(nodes)
    assert isinstance(r, train.EvalResult) and 0.0 <= r.micro_f1 <= 1.0
    # state_dict between the heads: same names, shapes and places
    assert list(ml.state_dict()) == list(a.state_dict()) == tc.names_of(L)
    assert not torch.equal(ml.p.params, a.p.params)
    ml.load_state_dict(a.state_dict())
    assert torch.equal(ml.p.params, a.p.params)
    fresh = _trainer(case, lr=0.05)
    fresh.load_state_dict(a.state_dict())
    assert torch.equal(ml.step(nodes).clone(), fresh.step(nodes).clone()) and torch.equal(ml.p.params, fresh.p.params)
    a.load_state_dict(ml.state_dict())
    assert torch.equal(a.p.params, ml.p.params) and np.isfinite(float(a.step(nodes)))


def test_refusals(gs):
    case = BY_ID["mean_c5"]
    graph, n, rp, col, X, Xd, Y, nodes, params, pw = _setup(case)
    y1 = torch.from_numpy(tc.labels_of(n, case["C"]))
    with pytest.raises(ValueError, match="one class per node"):
        _trainer(case, head="nll", labels=torch.from_numpy(Y))
    with pytest.raises(ValueError, match="multi-hot"):
        _trainer(case, labels=y1)
    with pytest.raises(ValueError, match="multi-hot"):
        _trainer(case, labels=torch.from_numpy(Y[:, :-1]))
    with pytest.raises(ValueError, match="0 or 1"):
        _trainer(case, labels=torch.from_numpy(Y).float() * 0.5)
    with pytest.raises(ValueError, match="head"):
        _trainer(case, head="softmax", labels=y1)
    with pytest.raises(ValueError, match="pos_weight"):
        _trainer(case, head="nll", labels=y1, pos_weight=torch.ones(case["C"]))
    with pytest.raises(ValueError, match="pos_weight"):
        _trainer(case, pos_weight=torch.ones(case["C"] + 1))
    # a raw config with an unknown head is refused by the library
    tr = _trainer(case)
    tr.cfg.head = 2
    with pytest.raises(ValueError):
        tr.forward_backward(nodes)
    tr.cfg.head = 1
    assert np.isfinite(float(tr.forward_backward(nodes)))
