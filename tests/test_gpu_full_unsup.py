"""The exact step under the unsupervised losses (train.FullTrainer with
`unsup=`, gs_train_full_unsup_forward_backward) on the MI355X against the
float64 reference of tests/full_unsup_ref.py on the cases of
tests/full_unsup_cases.py, bitwise against the pieces it is made of
(hip_ops.unsup_loss_fwd / unsup_loss_bwd, the supervised step), and end to end
with a real UnsupervisedLoss on the golden Cora graph.

Tolerance (adam_cases.check_rule): err <= factor * e_torch + 2^-23 * max|ref|,
with e_torch the error of the reference's own fp32 run on the CPU against its
float64 run and factor 4 unless full_unsup_cases.FACTOR names the row.  The
loss_net scalar is bounded by 4 * e_torch(score) + 2^-23 * |loss|, as
test_gpu_unsup_loss.py bounds it.  What selects (the margin kinds' pairs) is
compared exactly: the cases have clear winners (test_full_unsup_host.py).
"""
import importlib
import random

import numpy as np
import pytest
import torch

from tests import adam_cases as ac
from tests import full_unsup_cases as uc
from tests import full_unsup_ref as uref
from tests import unsup_cases as UC
from tests import unsup_loss_cases as ulc
from tests.adam_cases import check_rule

pytestmark = pytest.mark.gpu

ops = importlib.import_module("graphsage-pytorch_amd.hip_ops")
train = importlib.import_module("graphsage-pytorch_amd.train")
unsup = importlib.import_module("graphsage-pytorch_amd.unsup")
utils = importlib.import_module("graphsage-pytorch_amd.utils")
gsp = importlib.import_module("graphsage-pytorch_amd")
_lib = importlib.import_module("graphsage-pytorch_amd._lib")
DEV = torch.device("cuda", 0)
KIND_ARG = {"sage": "normal", "margin": "margin", "split": "margin"}
_MEMO = {}


def _np(t):
    return t.detach().cpu().numpy()


def _dev_inputs(case_id):
    key = ("in", case_id)
    if key not in _MEMO:
        s = uc.setup(case_id)
        Xd = torch.from_numpy(s["X"]).to(DEV)
        _MEMO[key] = (Xd.to(torch.bfloat16) if s["bf16"] else Xd, torch.from_numpy(s["plan"].copy()).to(DEV))
    return _MEMO[key]


def _trainer(case_id, params=None, **kw):
    s = uc.setup(case_id)
    L = s["L"]
    params = s["params"] if params is None else params
    w = ([torch.from_numpy(np.array(p)) for p in params[:L]], torch.from_numpy(np.array(params[L])),
         torch.from_numpy(np.array(params[L + 1])))
    return train.FullTrainer(s["graph_obj"], _dev_inputs(case_id)[0], torch.from_numpy(s["labels"]), s["C"],
                             num_layers=L, hidden=s["H"], agg_func=s["agg"], gcn=s["gcn"], weights=w,
                             seg_len=s["seg_len"], **kw)


def _batch(tr, case_id, method, kind):
    s = uc.setup(case_id)
    return tr.unsup_batch((_dev_inputs(case_id)[1], s["dims"], s["nodes"]), kind=KIND_ARG[kind], learn_method=method,
                          q=uc.Q, margin=uc.margin_of(case_id, kind))


def _dz_rows(tr, b, field):
    """The rows of dZ_L that belong to b.nodes, in their order, and the buffer itself."""
    buf = tr.hidden(which=2)
    if field is None:
        return buf.index_select(0, b.nodes.long()), buf
    return buf.index_select(0, field.pos(tr.L).index_select(0, b.nodes.long()).long()), buf


def _state(tr, b, field):
    """Everything one step leaves, as bytes-comparable numpy ("dZ": the rows of dZ_L's buffer, which holds
    dZ_L itself up to two layers and what the backward's ping-pong left there above that)."""
    torch.cuda.synchronize()
    return {"loss": _np(tr._loss3).copy(), "grads": _np(tr.p.grads).copy(), "pairs": _np(b.pair_state()).copy(),
            "dE": _np(b.d_embeddings(tr.H)).copy(), "dZ": _np(_dz_rows(tr, b, field)[0]).copy()}


def _same(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in a)


# ------------------------------------------------------------ 1. float64 matrix
def _step_refs(case_id, method, kind, params, lr, max_norm):
    """(r64, r32, parameters after one clip + SGD update in float64 and in fp32 torch)."""
    r64, r32 = uc.ref(case_id, method, kind), uc.ref(case_id, method, kind, torch.float32)
    s = uc.setup(case_id)
    L = s["L"]
    goff = np.cumsum([0] + [p.size for p in params])
    groups = [0, int(goff[L])] + ([int(goff[-1])] if method == "plus_unsup" else [])
    out = []
    for r, dt in ((r64, np.float64), (r32, np.float32)):
        flat = np.concatenate([np.asarray(p, dt).reshape(-1) for p in params])
        g = np.concatenate([np.asarray(x, dt).reshape(-1) for x in r["grads"]])
        for lo, hi in zip(groups[:-1], groups[1:]):
            norm = np.sqrt(np.sum(g[lo:hi] * g[lo:hi], dtype=dt))
            coef = min(dt(max_norm) / (norm + dt(1e-6)), dt(1.0))
            flat[lo:hi] = flat[lo:hi] - dt(lr) * (g[lo:hi] * coef)
        out.append(flat.astype(np.float64))
    return r64, r32, out[0], out[1]


@pytest.mark.parametrize("path", ["full", "field"])
@pytest.mark.parametrize("kind", uc.KINDS)
@pytest.mark.parametrize("method", uc.METHODS)
@pytest.mark.parametrize("case_id", uc.IDS)
def test_step_matches_float64_reference(gs, case_id, method, kind, path):
    s = uc.setup(case_id)
    L, U = s["L"], s["U"]
    lr, max_norm = ac.f32(0.7), 5.0
    tr = _trainer(case_id, lr=lr, max_norm=max_norm)
    b = _batch(tr, case_id, method, kind)
    field = tr.field(b.nodes) if path == "field" else None
    before = tr.p.params.clone()
    # forward and head first: with three layers the backward's ping-pong reuses the buffer of dZ_L
    tr.forward_backward(b.nodes, stages=_lib.GS_TF_FORWARD | _lib.GS_TF_HEAD, field=field, unsup=b)
    dz = _dz_rows(tr, b, field)[0].clone()
    loss = tr.forward_backward(b.nodes, stages=_lib.GS_TF_BACKWARD, field=field, unsup=b)
    torch.cuda.synchronize()
    assert torch.equal(tr.p.params, before) and loss.data_ptr() == tr.loss_parts()[0].data_ptr()
    r64, r32, p64, p32 = _step_refs(case_id, method, kind, s["params"], lr, max_norm)
    tag = f"unsup step {case_id} {method} {kind} {path}"
    failures = []

    def rule(name, got, a, c):
        try:
            check_rule(f"{tag} {name}", got, np.asarray(a).reshape(-1), np.asarray(c).reshape(-1),
                       factor=uc.factor(case_id, method, kind, path, name))
        except AssertionError as e:
            failures.append(str(e))

    total, sup, net = (float(x) for x in tr.loss_parts())
    e_score = float(np.max(np.abs(r32["score"] - r64["score"])))
    err, bound = abs(net - r64["loss_net"]), 4.0 * e_score + 2.0 ** -23 * abs(r64["loss_net"])
    msg = f"{tag} loss_net: err {err:.3e}, e_torch(score) {e_score:.3e}, bound {bound:.3e}"
    print(msg)
    if not err <= bound:
        failures.append(msg)
    if method == "plus_unsup":
        rule("loss_sup", [sup], [r64["loss_sup"]], [r32["loss_sup"]])
        assert total == float(np.float32(sup) + np.float32(net))
    else:
        assert sup == 0.0 and total == net
    rule("E", _np(tr.hidden().index_select(0, b.nodes.long())), r64["E"], r32["E"])
    rule("dZ_L", _np(dz), r64["dZ"], r32["dZ"])
    rule("dE_net", _np(b.d_embeddings(tr.H)), r64["dE_net"], r32["dE_net"])
    pairs = _np(b.pair_state())
    rule("coef", pairs[:, 0], r64["coef"], r32["coef"])
    if kind != "sage":
        on = r64["h"] > 0
        want = np.sort(np.concatenate([r64["sel_pos"][on], s["dims"][1] + r64["sel_neg"][on]]))
        if not np.array_equal(np.nonzero(pairs[:, 0])[0], want):
            failures.append(f"{tag}: the pairs with a coefficient differ from the reference's")
    for i, g in enumerate(r64["grads"]):
        got = _np(tr.p.view(i, grad=True))
        if method == "unsup" and i >= L:
            assert not np.any(got) and not np.any(g)
            continue
        assert np.abs(g).max() > 0
        rule(f"d{tr.p.names[i]}", got, g, r32["grads"][i])
    tr.apply_update()
    torch.cuda.synchronize()
    rule("params after one update", _np(tr.p.params), p64, p32)
    assert not failures, "\n".join(failures)


# -------------------------------------------------- 2. bitwise ties to existing code
@pytest.mark.parametrize("kind", ["sage", "split"])
@pytest.mark.parametrize("method", uc.METHODS)
@pytest.mark.parametrize("case_id", ["l2_h16-hub_max", "max_h80-bounded", "h256-hub_max", "bf16_max-directed"])
def test_head_is_bitwise_its_pieces(gs, case_id, method, kind):
    s = uc.setup(case_id)
    tr = _trainer(case_id)
    b = _batch(tr, case_id, method, kind)
    tr.p.grads.fill_(float("nan"))
    tr.forward_backward(b.nodes, unsup=b)
    got = _state(tr, b, None)
    _dz, buf = _dz_rows(tr, b, None)
    buf = _np(buf).copy()
    # the pair loss on the embeddings FullEmbedder gives
    E = tr.embed(s["nodes"]).contiguous()
    assert torch.equal(E, tr.hidden().index_select(0, b.nodes.long()))
    M, P, N, U = s["dims"]
    ws = ops.unsup_loss_workspace(M, P, N, DEV)
    loss = ops.unsup_loss_fwd(ulc.KIND_ID[kind], E, _dev_inputs(case_id)[1], s["dims"], uc.Q,
                              uc.margin_of(case_id, kind), ws)
    dE = torch.full_like(E, float("nan"))
    ops.unsup_loss_bwd(E, _dev_inputs(case_id)[1], s["dims"], ws, torch.ones(1, device=DEV), dE)
    torch.cuda.synchronize()
    assert got["loss"][2:].tobytes() == _np(loss).reshape(1).tobytes()
    assert got["dE"].tobytes() == _np(dE).tobytes()
    assert got["pairs"].tobytes() == _np(ws[:4 * (P + N)]).tobytes()
    # rows of dZ_L outside `nodes` are exactly zero; the unpaired rows too under 'unsup'
    outside = np.setdiff1d(np.arange(s["n"]), s["nodes"])
    assert not np.any(buf[outside]) and np.all(np.isfinite(buf))
    if method == "unsup":
        assert not np.any(got["dZ"][U - uc.FREE_ROWS:]) and np.any(got["dZ"][0])
        L = s["L"]
        assert not np.any(_np(tr.p.grads)[int(tr.p.offsets[L]):])
    else:  # loss_sup and the classifier's gradients are the supervised step's over the same nodes
        sup = _trainer(case_id)
        sup.forward_backward(b.nodes)
        torch.cuda.synchronize()
        L = s["L"]
        lo = int(tr.p.offsets[L])
        assert got["loss"][1:2].tobytes() == _np(sup.loss).tobytes()
        assert got["grads"][lo:].tobytes() == _np(sup.p.grads)[lo:].tobytes()
        assert np.any(got["dZ"][U - uc.FREE_ROWS:])


# ------------------------------------------------------ 3. the classifier under 'unsup'
def _sage_loop(case_id, kind, optimizer, n_steps, hp, dtype):
    """n_steps of (reference gradients, clip, update) on the sage group in `dtype`; returns the flat sage
    parameters after every step as float64."""
    s = uc.setup(case_id)
    L = s["L"]
    npdt = np.float64 if dtype == torch.float64 else np.float32
    params = [np.asarray(p, np.float64) for p in s["params"]]
    sizes = [p.size for p in params[:L]]
    n_sage = int(sum(sizes))
    m, v = np.zeros(n_sage), np.zeros(n_sage)
    out = []
    for t in range(1, n_steps + 1):
        r = uref.step_reference(s["rp"], s["col"], s["X"], s["labels"], s["nodes"], params, s["agg"], s["gcn"],
                                lists=s["lists"], kind=kind, margin=uc.margin_of(case_id, kind), bf16=s["bf16"],
                                dtype=dtype)
        g = np.concatenate([x.reshape(-1) for x in r["grads"][:L]])
        flat = np.concatenate([p.reshape(-1) for p in params[:L]])
        goff = [0, n_sage]
        if optimizer == "adam":
            if dtype == torch.float64:
                flat, _g, m, v = ac.reference_adamw(flat, g, m, v, t, hp["lr"], hp["betas"], hp["eps"], hp["wd"],
                                                    goff, 1.0, hp["max_norm"])
            else:
                flat, _g, m, v = ac.torch_adamw(flat, g, m, v, t, hp["lr"], hp["betas"], hp["eps"], hp["wd"], goff,
                                                1.0, hp["max_norm"], dtype)
        else:
            g = g.astype(npdt)
            norm = np.sqrt(np.sum(g * g, dtype=npdt))
            coef = min(npdt(hp["max_norm"]) / (norm + npdt(1e-6)), npdt(1.0))
            flat = (flat.astype(npdt) - npdt(hp["lr"]) * (g * coef)).astype(np.float64)
        out.append(flat.copy())
        o = 0
        for i, n in enumerate(sizes):
            params[i] = flat[o:o + n].reshape(params[i].shape)
            o += n
    return out


@pytest.mark.parametrize("optimizer", ["sgd", "adam"])
def test_unsup_leaves_the_classifier_alone(gs, optimizer):
    case_id, kind = "l2_h16-hub_max", "sage"
    s = uc.setup(case_id)
    L = s["L"]
    hp = {"lr": ac.f32(0.7 if optimizer == "sgd" else 0.01), "betas": (ac.f32(0.9), ac.f32(0.999)),
          "eps": ac.f32(1e-8), "wd": ac.f32(0.01), "max_norm": 5.0}
    tr = _trainer(case_id, optimizer=optimizer, lr=hp["lr"], betas=hp["betas"], eps=hp["eps"],
                  weight_decay=hp["wd"], max_norm=hp["max_norm"])
    lo = int(tr.p.offsets[L])
    if optimizer == "adam":   # moments a supervised step left behind
        tr.step(s["nodes"])
        tr.load_state_dict({n: torch.from_numpy(np.array(p)) for n, p in zip(tr.p.names, s["params"])})
        tr.opt_m[:lo].zero_()
        tr.opt_v[:lo].zero_()
        tr._opt_step = 0
        assert bool(tr.opt_m[lo:].abs().max() > 0)
        m0, v0 = tr.opt_m[lo:].clone(), tr.opt_v[lo:].clone()
    cls0 = tr.p.params[lo:].clone()
    b = _batch(tr, case_id, "unsup", kind)
    ref64 = _sage_loop(case_id, kind, optimizer, 3, hp, torch.float64)
    ref32 = _sage_loop(case_id, kind, optimizer, 3, hp, torch.float32)
    for t in range(3):
        tr.p.grads[lo:].fill_(float("nan"))
        tr.step(b.nodes, unsup=b)
        torch.cuda.synchronize()
        assert not bool(tr.p.grads[lo:].ne(0).any())                # exactly zero, NaN gone
        assert torch.equal(tr.p.params[lo:], cls0)
        if optimizer == "adam":
            assert torch.equal(tr.opt_m[lo:], m0) and torch.equal(tr.opt_v[lo:], v0)
        check_rule(f"unsup {optimizer} update {t + 1} sage params", _np(tr.p.params[:lo]), ref64[t], ref32[t])
    assert tr.optimizer_state()["step"] == 3                         # the one counter advances
    tr.step(s["nodes"])                                              # a supervised step updates it again
    torch.cuda.synchronize()
    assert not torch.equal(tr.p.params[lo:], cls0)


# ------------------------------------------------ 4. repeatability and isolation
@pytest.mark.parametrize("path", ["full", "field"])
@pytest.mark.parametrize("case_id", ["max_h80-bounded", "gcn_h128-bounded", "l3_h80-hub_max"])
def test_repeatable_isolated_and_staged(gs, case_id, path):
    s = uc.setup(case_id)

    def fresh(params, what, cache=True):
        tr = _trainer(case_id, params=params, cache_agg1=cache)
        b = _batch(tr, case_id, "plus_unsup", "split")
        field = tr.field(b.nodes) if path == "field" else None
        if what == "sup":
            tr.forward_backward(b.nodes, field=field)
            torch.cuda.synchronize()
            return {"loss": _np(tr.loss).copy(), "grads": _np(tr.p.grads).copy()}, tr
        tr.forward_backward(b.nodes, field=field, unsup=b)
        return _state(tr, b, field), tr

    p0 = s["params"]
    want_u, tr = fresh(p0, "unsup")
    want_s, _ = fresh(p0, "sup")
    b = _batch(tr, case_id, "plus_unsup", "split")
    field = tr.field(b.nodes) if path == "field" else None
    tr.forward_backward(b.nodes, field=field, unsup=b)               # again on the same trainer (A_1 cached)
    assert _same(_state(tr, b, field), want_u)
    off, _ = fresh(p0, "unsup", cache=False)
    assert _same(off, want_u)
    # supervised, unsup, supervised in turn on one trainer at the same weights
    for what in ("sup", "unsup", "sup"):
        if what == "sup":
            tr.forward_backward(b.nodes, field=field)
            torch.cuda.synchronize()
            assert _np(tr.loss).tobytes() == want_s["loss"].tobytes()
            assert _np(tr.p.grads).tobytes() == want_s["grads"].tobytes()
        else:
            tr.forward_backward(b.nodes, field=field, unsup=b)
            assert _same(_state(tr, b, field), want_u)
    # the three stages as three calls
    tr2 = _trainer(case_id)
    b2 = _batch(tr2, case_id, "plus_unsup", "split")
    f2 = tr2.field(b2.nodes) if path == "field" else None
    for st in (_lib.GS_TF_FORWARD, _lib.GS_TF_HEAD, _lib.GS_TF_BACKWARD):
        tr2.forward_backward(b2.nodes, stages=st, field=f2, unsup=b2)
    assert _same(_state(tr2, b2, f2), want_u)
    # embed with unsup= is the forward stage: the rows of the step's own E
    E = tr2.embed(b2.nodes, field=f2, unsup=b2)
    assert torch.equal(E, tr.hidden().index_select(0, b.nodes.long()))


# ------------------------------------------------------------------ 5. end to end
def _cora():
    if "cora" not in _MEMO:
        g = UC.graphs()
        n = int(g["cora_n"][0])
        graph = gsp.CSRGraph.from_pairs(g["cora_src"].astype(np.int64), g["cora_dst"].astype(np.int64), n)
        from tests import full_cases as fc
        from tests import full_train_cases as tc
        case = {"L": 2, "F": 64, "H": 16, "C": 7, "gcn": False}
        X = fc.features(n, 64)
        _MEMO["cora"] = (graph, n, graph.row_ptr(), graph.col(), X, torch.from_numpy(X).to(DEV),
                         tc.labels_of(n, 7), tc.params_of(case), UC.extend_case("cora_n6")[1])
    return _MEMO["cora"]


def _cora_trainer(params):
    graph, n, rp, col, X, Xd, labels, _p, train_ids = _cora()
    w = ([torch.from_numpy(np.array(p)) for p in params[:2]], torch.from_numpy(np.array(params[2])),
         torch.from_numpy(np.array(params[3])))
    return train.FullTrainer(graph, Xd, torch.from_numpy(labels), 7, num_layers=2, hidden=16, agg_func="MEAN",
                             weights=w)


@pytest.mark.parametrize("unsup_loss,method", [("normal", "unsup"), ("normal", "plus_unsup"), ("margin", "unsup"),
                                               ("margin", "plus_unsup")])
def test_unsup_step_end_to_end_on_cora(gs, unsup_loss, method):
    """extend_nodes with num_neg 100 (normal) / 6 (margin), then unsup_step against the float64 reference fed
    the same extended lists; the exact path draws nothing from `random`."""
    graph, n, rp, col, X, Xd, labels, params, train_ids = _cora()
    num_neg = {"normal": 100, "margin": 6}[unsup_loss]
    batch = train_ids[:20]
    ul = unsup.UnsupervisedLoss(graph, train_ids, DEV)
    random.seed(11)
    ul.extend_nodes(batch, num_neg=num_neg)
    state_after_extend = random.getstate()
    lists = ulc.lists_of_object(ul)
    nodes = np.asarray(ul.unique_nodes_batch, np.int64)
    kind = "sage" if unsup_loss == "normal" else "margin"
    refs = [uref.step_reference(rp, col, X, labels, nodes, params, "MEAN", False, lists=lists[:2], kind=kind,
                                q=float(ul.Q), margin=float(ul.MARGIN), with_sup=method == "plus_unsup", dtype=dt)
            for dt in (torch.float64, torch.float32)]
    if kind == "margin":                                            # this batch has clear winners
        e_ext = max(np.abs(refs[1][k] - refs[0][k]).max() for k in ("ext_pos", "ext_neg"))
        assert uc.conditions(refs[0], lists[:2], 100 * e_ext, 100 * np.abs(refs[1]["h"] - refs[0]["h"]).max()) == []
    tr = _cora_trainer(params)
    random.seed(11)
    loss, ext = tr.unsup_step(ul, batch, unsup_loss=unsup_loss, learn_method=method)
    assert random.getstate() == state_after_extend
    torch.cuda.synchronize()
    assert np.array_equal(ext, nodes) and tr._unsup_field is not None and tr._unsup_field.sizes[0] == len(nodes)
    failures = []
    e_score = float(np.max(np.abs(refs[1]["score"] - refs[0]["score"])))
    net = float(tr.loss_parts()[2])
    err, bound = abs(net - refs[0]["loss_net"]), 4.0 * e_score + 2.0 ** -23 * abs(refs[0]["loss_net"])
    print(f"cora {unsup_loss} {method} loss_net: err {err:.3e}, e_torch(score) {e_score:.3e}, bound {bound:.3e}")
    if not err <= bound:
        failures.append("loss_net")
    if method == "unsup":
        assert not np.any(_np(tr.p.grads)[int(tr.p.offsets[2]):])
    # the step leaves the clipped gradients behind; a second trainer, forward_backward only, has the raw ones
    tr2 = _cora_trainer(params)
    b = tr2.unsup_batch(ul, kind=unsup_loss, learn_method=method)
    tr2.forward_backward(b.nodes, field=tr2.field(b.nodes), unsup=b)
    torch.cuda.synchronize()
    assert float(tr2.loss_parts()[0]) == float(loss)
    for i, g in enumerate(refs[0]["grads"]):
        if method == "unsup" and i >= 2:
            continue
        try:
            check_rule(f"cora {unsup_loss} {method} d{tr2.p.names[i]}", _np(tr2.p.view(i, grad=True)), g.reshape(-1),
                       refs[1]["grads"][i].reshape(-1))
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, "\n".join(failures)


def test_apply_model_full_runs_two_batches(gs, capsys):
    graph, n, rp, col, X, Xd, labels, params, train_ids = _cora()

    class DC:
        pass

    dc = DC()
    dc.cora_train, dc.cora_labels = np.asarray(train_ids[:40]), labels
    ul = unsup.UnsupervisedLoss(graph, train_ids, DEV)     # negatives come from the whole training set
    tr = _cora_trainer(params)
    np.random.seed(3)
    random.seed(3)
    assert utils.apply_model_full(dc, "cora", tr, ul, 20, "margin", "plus_unsup") is tr
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("Step [")]
    assert len(lines) == 2 and lines[0].startswith("Step [1/2], Loss: ") and lines[1].startswith("Step [2/2], Loss: ")
    assert lines[1].endswith("/40] ") and "Dealed Nodes [" in lines[0]
    assert tr.optimizer_state()["step"] == 2
    utils.apply_model_full(dc, "cora", tr, ul, 20, "normal", "sup", verbose=False)
    assert tr.optimizer_state()["step"] == 4
    with pytest.raises(SystemExit):
        utils.apply_model_full(dc, "cora", tr, ul, 20, "other", "unsup")
    assert "unsup_loss can be only 'margin' or 'normal'." in capsys.readouterr().out


# ------------------------------------------------------------------- 6. refusals
def test_refusals_launch_nothing(gs):
    case_id = "l2_h16-hub_max"
    s = uc.setup(case_id)
    tr = _trainer(case_id)
    plan = _dev_inputs(case_id)[1]
    M, P, N, U = s["dims"]

    def untouched(fn, exc, match=None):
        tr._loss3.fill_(float("nan"))
        tr.p.grads.fill_(float("nan"))
        tr._ws.fill_(0xFF)
        tr.invalidate_cache()
        if tr._uws is not None:
            tr._uws.fill_(0xFF)
        with pytest.raises(exc, match=match):
            fn()
        torch.cuda.synchronize()
        assert bool(torch.isnan(tr._loss3).all()) and bool(torch.isnan(tr.p.grads).all())
        assert bool((tr._ws == 0xFF).all()) and (tr._uws is None or bool((tr._uws == 0xFF).all()))

    good = _batch(tr, case_id, "plus_unsup", "margin")
    # Python's refusals
    untouched(lambda: tr.unsup_batch((plan, s["dims"], s["nodes"]), kind="sage"), ValueError, "kind")
    untouched(lambda: tr.unsup_batch((plan, s["dims"], s["nodes"]), learn_method="sup"), ValueError, "learn_method")
    untouched(lambda: tr.unsup_batch((plan, (0, P, N, U), s["nodes"])), ValueError, "non-empty list")
    untouched(lambda: tr.unsup_batch((plan, (M, 0, N, U), s["nodes"])), ValueError, "pair")
    untouched(lambda: tr.unsup_batch((plan, s["dims"], s["nodes"][:-1])), ValueError, "rows")
    untouched(lambda: tr.unsup_batch((plan[:-1], s["dims"], s["nodes"])), ValueError, "plan")
    untouched(lambda: tr.unsup_batch((plan.cpu(), s["dims"], s["nodes"])), ValueError, "plan")
    untouched(lambda: tr.forward_backward(s["nodes"][::-1].copy(), unsup=good), ValueError, "own nodes")
    untouched(lambda: tr.forward_backward(s["nodes"][:-1], unsup=good), ValueError, "own nodes")
    untouched(lambda: tr.forward_backward(good.nodes, unsup=object()), TypeError, "unsup_batch")
    untouched(lambda: tr.unsup_step(None, s["nodes"][:4], unsup_loss="other"), ValueError, "unsup_loss")
    untouched(lambda: tr.unsup_step(None, s["nodes"][:4], learn_method="sup"), ValueError, "learn_method")
    other = tr.field(np.sort(s["nodes"])[:-1].copy())
    untouched(lambda: tr.forward_backward(good.nodes, field=other, unsup=good), ValueError, "other nodes")
    deeper = ops.ReceptiveField(tr.plan, tr.tplan, tr.L + 1, DEV).build(good.nodes)
    untouched(lambda: tr.forward_backward(good.nodes, field=deeper, unsup=good), ValueError, "layers")
    # the native call's own refusals, behind Python's
    call = lambda: tr._forward_backward(good.nodes, _lib.GS_TF_ALL, None, good)   # noqa: E731
    good.desc.kind = 2
    untouched(call, ValueError, "kind")
    good.desc.kind = 1
    for name in ("M", "P", "N"):
        keep = getattr(good.desc, name)
        setattr(good.desc, name, 0)
        untouched(call, ValueError, "at least 1")
        setattr(good.desc, name, keep)
    good.uws_bytes -= 256
    untouched(call, ValueError, "unsup workspace")
    good.uws_bytes += 256
    good.uws_ptr += 16
    untouched(call, ValueError, "unsup workspace")
    good.uws_ptr -= 16
    tr._check_field = lambda field, nodes: None                      # Python's own check out of the way
    try:
        untouched(lambda: tr._forward_backward(good.nodes, _lib.GS_TF_ALL, other, good), ValueError,
                  "another set of nodes")
        untouched(lambda: tr._forward_backward(good.nodes, _lib.GS_TF_ALL, deeper, good), ValueError,
                  "another number of layers")
    finally:
        del tr._check_field
    keep = tr.cfg.max_nodes
    tr.cfg.max_nodes = U - 1
    untouched(call, ValueError, "max_nodes")
    tr.cfg.max_nodes = keep
    # and the descriptor, restored, runs
    tr.forward_backward(good.nodes, unsup=good)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(tr._loss3).all()) and bool(torch.isfinite(tr.p.grads).all())
