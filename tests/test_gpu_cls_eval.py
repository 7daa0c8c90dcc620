"""The evaluation head on the GPU (hip_ops.cls_eval, gs_cls_eval) against
float64, and what is built on it: FullTrainer.evaluate, ClassifierProbe.evaluate
and utils.evaluate_full.

Tolerances.  logp and loss: adam_cases.check_rule, err <= 4 e_torch + 2^-23
max|ref|, with e_torch the error of fp32 torch on the CPU against float64,
never measured from the kernel.  pred: equal to the float64 argmax on every row
whose float64 top-two margin is at least 8 e_torch + 2^-22 max|z| (twice the
per-logit bound; e_torch here is fp32 torch's largest logit error), and a case
fails when more than 1 % of its rows fall below that margin.  counts: exactly
a bincount of (labels, the device's own pred).  GS_CLS_EVAL_FIGURES=<path>
writes the observed ratios err / e_torch as JSON.
"""
import ctypes
import importlib
import json
import os
import types

import numpy as np
import pytest
import torch

from tests import cls_eval_cases as K
from tests import cls_probe_cases as PK
from tests import full_cases as fc
from tests import full_train_cases as tc
from tests import full_train_ref as tref
from tests.adam_cases import check_rule

pytestmark = pytest.mark.gpu

ops = importlib.import_module("graphsage-pytorch_amd.hip_ops")
train = importlib.import_module("graphsage-pytorch_amd.train")
utils = importlib.import_module("graphsage-pytorch_amd.utils")
_lib = importlib.import_module("graphsage-pytorch_amd._lib")
DEV = torch.device("cuda", 0)
_FIGURES = []
_MEMO = {}


@pytest.fixture(scope="module", autouse=True)
def _write_figures():
    yield
    path = os.environ.get("GS_CLS_EVAL_FIGURES")
    if path and _FIGURES:
        with open(path, "w") as f:
            json.dump({"rule": "err <= 4 * e_torch + 2^-23 * max|ref|; ratio = err / e_torch",
                       "largest_ratio": max(r[3] for r in _FIGURES if np.isfinite(r[3])),
                       "figures": [{"what": w, "err": e, "e_torch": t, "ratio": r, "bound": b}
                                   for w, e, t, r, b in _FIGURES]}, f, indent=1)


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def _inputs(c):
    """(H view, labels, rows or None, params) on the device for a Case."""
    table = _dev(c.table)
    if c.rows is not None:
        return table[:, :c.D], _dev(c.labels, torch.int32), _dev(c.rows, torch.int32), _dev(c.params)
    return table[:c.B, :c.D], _dev(c.y, torch.int32), None, _dev(c.params)


def _run(case, **kw):
    key = ("run", case, tuple(sorted(kw.items())))
    if key not in _MEMO:
        c = K.case(*case)
        H, labels, rows, params = _inputs(c)
        out = ops.cls_eval(H, labels, params, c.C, rows=rows, want_logp=True, **kw)
        torch.cuda.synchronize()
        _MEMO[key] = tuple(t.cpu().numpy() for t in out)
    return _MEMO[key]


def _check_pred(what, pred, z64, z32):
    """The margin rule of the module docstring; returns the rows it covers."""
    keep = K.margin_rule(z64, z32)
    left_out = int((~keep).sum())
    print(f"{what}: {left_out} of {len(keep)} rows below the margin")
    assert left_out <= K.MARGIN_CAP * len(keep), what
    np.testing.assert_array_equal(pred[keep], z64.argmax(1)[keep], err_msg=what)
    return keep


def _check_counts(counts, y, pred, C):
    y = np.asarray(y, np.int64)
    has = (y >= 0) & (y < C)
    assert counts.dtype == np.int64
    np.testing.assert_array_equal(counts[:C * C], np.bincount(y[has] * C + pred[has], minlength=C * C))
    assert counts[C * C] == has.sum() and counts[C * C + 1] == (~has).sum()
    assert counts[C * C] + counts[C * C + 1] == len(y)


# ---------------------------------------------------------------- 1. the operator
def test_kernel_constants_are_the_library_s():
    assert K.WC_LDS == int(_lib.lib().gs_cls_eval_wc_lds_floats())


@pytest.mark.parametrize("case", K.CASES, ids=K.case_id)
def test_operator_matches_float64(case):
    c, ref, r32 = K.case(*case), K.reference(*case), K.reference(case[0], case[1], True)
    loss, counts, pred, logp = _run(case)
    assert loss.shape == (1,) and counts.shape == (1, c.C * c.C + 2) and pred.shape == (1, c.B)
    assert logp.shape == (1, c.B, c.C) and pred.dtype == np.int32 and logp.dtype == np.float32
    tag = f"cls_eval {K.case_id(case)}"
    check_rule(f"{tag} logp", logp[0], ref.logp.reshape(-1), r32.logp.reshape(-1), _FIGURES)
    check_rule(f"{tag} loss", loss, np.array([ref.loss]), np.array([r32.loss]), _FIGURES)
    _check_pred(tag, pred[0], ref.z, r32.z)
    _check_counts(counts[0], c.y, pred[0], c.C)
    assert (pred[0] >= 0).all() and (pred[0] < c.C).all()
    if case[0] == (1, 1, 1):
        assert logp[0, 0, 0] == 0.0 and loss[0] == 0.0
    # without logp and without pred: the same loss and counts, bit for bit
    H, labels, rows, params = _inputs(c)
    l2, c2, p2, g2 = ops.cls_eval(H, labels, params, c.C, rows=rows, want_pred=False)
    assert p2 is None and g2 is None
    assert np.array_equal(l2.cpu().numpy().view(np.uint32), loss.view(np.uint32))
    assert np.array_equal(c2.cpu().numpy(), counts)


@pytest.mark.parametrize("case", K.CASES, ids=K.case_id)
def test_operator_is_bitwise_repeatable(case):
    c = K.case(*case)
    base = _run(case)
    H, labels, rows, params = _inputs(c)
    again = ops.cls_eval(H, labels, params, c.C, rows=rows, want_logp=True)
    for a, b in zip(base, again):
        assert np.array_equal(_bits(a), _bits(b.cpu().numpy()))


@pytest.mark.parametrize("shape", [(37, 128, 7), (257, 50, 2), (4099, 128, 47), K.SHAPES[-1]],
                         ids=lambda s: "x".join(map(str, s)))
def test_three_sets_equal_three_single_calls(shape):
    """n_sets = 3 at a stride wider than a set: every output of set s is bitwise that of the call on set s alone."""
    c = K.case(shape, "rows")
    rs = np.random.RandomState(5)
    P = c.params.size
    sets = np.stack([c.params, c.params + rs.uniform(-0.05, 0.05, P).astype(np.float32), c.params * np.float32(2)])
    stride = P + 5
    wide = np.full((3, stride), np.nan, np.float32)
    wide[:, :P] = sets
    H, labels, rows, _p = _inputs(c)
    out = ops.cls_eval(H, labels, _dev(wide.reshape(-1)), c.C, rows=rows, n_sets=3, set_stride=stride, want_logp=True)
    out = [t.cpu().numpy() for t in out]
    assert out[0].shape == (3,) and out[2].shape == (3, c.B) and out[3].shape == (3, c.B, c.C)
    assert not np.array_equal(out[3][0], out[3][2])
    # the single calls pass the same set_stride: where Wc is read through the cache, the load path (float4 or
    # scalar) follows the alignment of (params, set_stride), whatever n_sets is, so that set s alone and set s
    # among three take the same path.  P + 5 is a multiple of 4 for the last shape and odd for (257, 50, 2).
    for s in range(3):
        one = ops.cls_eval(H, labels, _dev(wide[s]), c.C, rows=rows, set_stride=stride, want_logp=True)
        for a, b in zip(out, one):
            assert np.array_equal(_bits(a[s]), _bits(b.cpu().numpy()[0])), s


@pytest.mark.parametrize("D", [8, 6])
def test_ties_and_nans_follow_numpy_argmax(D):
    """Small integers: every sum is exact and many rows tie, so pred is
    np.argmax exactly and logp is the float64 value rounded once.  A row with
    a NaN logit predicts its first NaN class and makes the loss NaN."""
    C, B = 21, 500
    rs = np.random.RandomState(3 + D)
    H = rs.randint(-2, 3, (B, D)).astype(np.float32)
    W = rs.randint(-1, 2, (C, D)).astype(np.float32)
    b = rs.randint(-1, 2, C).astype(np.float32)
    y = rs.randint(0, C, B)
    z = H.astype(np.float64) @ W.T.astype(np.float64) + b
    assert ((z == z.max(1, keepdims=True)).sum(1) > 1).sum() > 100
    params = np.concatenate([W.reshape(-1), b])
    loss, counts, pred, logp = ops.cls_eval(_dev(H), _dev(y, torch.int32), _dev(params), C)
    np.testing.assert_array_equal(pred.cpu().numpy()[0], np.argmax(z, 1))
    _check_counts(counts.cpu().numpy()[0], y, np.argmax(z, 1), C)
    assert np.isfinite(float(loss[0]))
    # a NaN in H: the whole row is NaN, its first class wins; a NaN bias at class 18 (the second class group)
    Hn = H.copy()
    Hn[7, 1] = np.nan
    loss, counts, pred, logp = ops.cls_eval(_dev(Hn), _dev(y, torch.int32), _dev(params), C, want_logp=True)
    want = np.argmax(z, 1)
    want[7] = 0
    np.testing.assert_array_equal(pred.cpu().numpy()[0], want)
    assert np.isnan(float(loss[0])) and bool(torch.isnan(logp[0, 7]).all()) and bool(torch.isfinite(logp[0, 8]).all())
    pn = params.copy()
    pn[C * D + 18] = np.nan
    loss, counts, pred, logp = ops.cls_eval(_dev(H), _dev(y, torch.int32), _dev(pn), C)
    assert bool((pred[0] == 18).all()) and np.isnan(float(loss[0]))
    zn = z.copy()
    zn[:, 18] = np.nan
    np.testing.assert_array_equal(pred.cpu().numpy()[0], np.argmax(zn, 1))


@pytest.mark.parametrize("D", [4000, 4001])
def test_rows_too_wide_for_wc_beside_them_read_wc_through_the_cache(D):
    """D = 4,000 with two classes: Wc would fit its LDS budget, but not beside
    the waves' row tiles, so it is read through the cache (one row per group);
    float4 and scalar loads.  The same rule against float64."""
    C, B = 2, 9
    assert C * (D + 4) <= K.WC_LDS
    rs = np.random.RandomState(D)
    H = rs.uniform(-1, 1, (B, D)).astype(np.float32)
    W = (rs.uniform(-1, 1, (C, D)) * np.sqrt(6.0 / (C + D))).astype(np.float32)
    b = rs.uniform(-0.1, 0.1, C).astype(np.float32)
    y = rs.randint(0, C, B)
    ref = K.torch_reference(H, None, y, W, b, torch.float64)
    r32 = K.torch_reference(H, None, y, W, b, torch.float32)
    p = np.concatenate([W.reshape(-1), b])
    p = np.concatenate([p, np.zeros(-len(p) % 4, np.float32)])   # a stride that is a multiple of 4: float4 reads of Wc
    loss, counts, pred, logp = ops.cls_eval(_dev(H), _dev(y, torch.int32), _dev(p), C, set_stride=len(p),
                                            want_logp=True)
    tag = f"cls_eval wide D={D}"
    check_rule(f"{tag} logp", logp.cpu().numpy()[0], ref.logp.reshape(-1), r32.logp.reshape(-1), _FIGURES)
    check_rule(f"{tag} loss", loss.cpu().numpy(), np.array([ref.loss]), np.array([r32.loss]), _FIGURES)
    keep = K.margin_rule(ref.z, r32.z)
    np.testing.assert_array_equal(pred.cpu().numpy()[0][keep], ref.pred[keep])
    _check_counts(counts.cpu().numpy()[0], y, pred.cpu().numpy()[0], C)


def _raw_call(c, labels, rows, guard=64):
    """gs_cls_eval on caller-owned buffers, each between two guard regions; returns (loss, counts, pred) and
    asserts that no guard word changed."""
    table = _dev(c.table)
    H = table[:, :c.D]
    B, C = len(rows), c.C
    params = _dev(c.params)
    rows_d, labels_d = _dev(rows, torch.int32), _dev(labels, torch.int32)
    need = int(_lib.lib().gs_cls_eval_ws_bytes(B, c.D, C, 1))
    assert need > 0 and need % 16 == 0
    bufs = {"loss": (torch.float32, 1), "counts": (torch.int64, C * C + 2), "pred": (torch.int32, B),
            "ws": (torch.float32, need // 4)}
    store = {}
    for k, (dt, n) in bufs.items():
        t = torch.zeros(n + 2 * guard, dtype=dt, device=DEV)
        t[:guard] = 77
        t[n + guard:] = 77
        store[k] = t
    view = {k: store[k][guard:guard + bufs[k][1]] for k in bufs}
    assert view["ws"].data_ptr() % 16 == 0
    _lib.check(_lib.lib().gs_cls_eval(B, c.D, C, H.data_ptr(), H.stride(0), rows_d.data_ptr(), labels_d.data_ptr(), 1,
                                      params.data_ptr(), 1, C * c.D + C, view["pred"].data_ptr(), None,
                                      view["loss"].data_ptr(), view["counts"].data_ptr(), view["ws"].data_ptr(), need,
                                      _lib.stream_ptr(DEV)))
    torch.cuda.synchronize()
    for k, t in store.items():
        n = bufs[k][1]
        assert bool((t[:guard] == 77).all()) and bool((t[n + guard:] == 77).all()), k
    np.testing.assert_array_equal(table.cpu().numpy().view(np.uint32), c.table.view(np.uint32))  # H is read only
    return view["loss"].cpu().numpy(), view["counts"].cpu().numpy(), view["pred"].cpu().numpy()


@pytest.mark.parametrize("shape", [(300, 80, 3), (4099, 128, 47), K.SHAPES[-1]], ids=lambda s: "x".join(map(str, s)))
def test_bad_labels_are_counted_and_left_out(shape):
    """Labels -1 and C at two known rows: n_bad = 2, and the loss and the
    matrix are those of the call without the two rows; nothing outside the
    outputs and the workspace is written (guard words around each)."""
    c = K.case(shape, "rows")
    at = [5, min(211, c.B - 2)]
    labels = c.labels.copy()
    labels[c.rows[at[0]]], labels[c.rows[at[1]]] = -1, c.C
    loss, counts, pred = _raw_call(c, labels, c.rows)
    CC = c.C * c.C
    assert counts[CC] == c.B - 2 and counts[CC + 1] == 2
    _check_counts(counts, labels[c.rows], pred, c.C)
    ref = K.reference(shape, "rows")
    keep = np.delete(np.arange(c.B), at)
    loss_k, counts_k, pred_k = _raw_call(c, c.labels, c.rows[keep])
    np.testing.assert_array_equal(counts[:CC], counts_k[:CC])
    np.testing.assert_array_equal(pred[keep], pred_k)          # a row's values depend on the row alone
    # the two sums cut their rows into other chunks: both within the rule of the float64 mean over the kept rows
    want = -ref.logp[keep, c.y[keep]].mean()
    r32 = K.reference(shape, "rows", True)
    tor = -r32.logp[keep, c.y[keep]].mean()
    check_rule(f"bad labels {shape} loss", loss, np.array([want]), np.array([tor]))
    check_rule(f"bad labels {shape} loss without the rows", loss_k, np.array([want]), np.array([tor]))
    # an all-bad batch: NaN loss, an all-zero matrix
    loss_a, counts_a, _p = _raw_call(c, np.full_like(c.labels, c.C), c.rows)
    assert np.isnan(loss_a[0]) and not counts_a[:CC].any() and counts_a[CC] == 0 and counts_a[CC + 1] == c.B


def test_refusals_come_before_any_launch():
    c = K.case((37, 128, 7), "rows")
    H, labels, rows, params = _inputs(c)
    for bad in (dict(H=H.cpu()), dict(H=H.double()), dict(H=H.t()), dict(rows=rows.long()), dict(labels=labels.long()),
                dict(params=params[:-1]), dict(C=0), dict(n_sets=2), dict(set_stride=c.C * c.D), dict(labels=labels[:5])):
        kw = dict(H=H, labels=labels, params=params, C=c.C, rows=rows)
        kw.update(bad)
        with pytest.raises((ValueError, TypeError, RuntimeError)):
            ops.cls_eval(**kw)
    L = _lib.lib()
    loss, counts = torch.zeros(1, device=DEV), torch.zeros(51, dtype=torch.int64, device=DEV)
    need = int(L.gs_cls_eval_ws_bytes(c.B, c.D, c.C, 1))
    ws = torch.zeros(need + 16, dtype=torch.uint8, device=DEV)
    good = [c.B, c.D, c.C, H.data_ptr(), H.stride(0), rows.data_ptr(), labels.data_ptr(), 1, params.data_ptr(), 1,
            c.C * c.D + c.C, None, None, loss.data_ptr(), counts.data_ptr(), ws.data_ptr(), need, _lib.stream_ptr(DEV)]
    assert L.gs_cls_eval(*good) == _lib.GS_OK
    for i, v in ((0, 0), (1, 0), (2, 0), (3, None), (4, c.D - 1), (6, None), (8, None), (9, 0), (10, c.C * c.D),
                 (13, None), (14, None), (15, None), (15, ws.data_ptr() + 4), (16, need - 1)):
        args = list(good)
        args[i] = v
        assert L.gs_cls_eval(*args) == _lib.GS_EINVAL, i
    assert L.gs_cls_eval_ws_bytes(0, 1, 1, 1) < 0
    torch.cuda.synchronize()
    assert float(loss[0]) == float(loss[0])  # the good call ran; the refused ones wrote nothing after it
    assert int(counts[49]) == c.B


# -------------------------------------------------------- 2. FullTrainer.evaluate
EVAL_IDS = ["l1", "l2", "l3_h80", "h16_f50", "gcn", "max", "max_gcn", "bf16_f100"]


def _setup(case, gname):
    graph, n, rp, col = fc.graph_of(gname)
    X = fc.features(n, case["F"], case["bf16"])
    Xd = torch.from_numpy(X).to(DEV)
    if case["bf16"]:
        Xd = Xd.to(torch.bfloat16)
    return graph, n, rp, col, X, Xd, tc.labels_of(n, case["C"]), tc.params_of(case)


def _trainer(case, graph, Xd, labels, params, **kw):
    L = case["L"]
    w = ([torch.from_numpy(p) for p in params[:L]], torch.from_numpy(params[L]), torch.from_numpy(params[L + 1]))
    args = {"seg_len": case["seg_len"]}
    args.update(kw)
    return train.FullTrainer(graph, Xd, torch.from_numpy(labels), case["C"], num_layers=L, hidden=case["H"],
                             agg_func=case["agg"], gcn=case["gcn"], weights=w, **args)


def _ref(case, rp, col, X, labels, nodes, params, dtype):
    loss, _g, hs = tref.step_reference(rp, col, X, labels, nodes, params, case["agg"], case["gcn"], bf16=case["bf16"],
                                       dtype=dtype)
    Wc, bc = (np.asarray(p, np.float64) for p in params[-2:])
    return loss, hs[-1][nodes] @ Wc.T + bc


@pytest.mark.parametrize("case_id", EVAL_IDS)
@pytest.mark.parametrize("name", ["hub_max", "rmat"])
def test_full_trainer_evaluate(gs, name, case_id):
    case = tc.STEP_BY_ID[case_id]
    graph, n, rp, col, X, Xd, labels, params = _setup(case, name)
    tr = _trainer(case, graph, Xd, labels, params, optimizer="adam", lr=0.01)
    sub = tc.nodes_of(n)
    tr.step(sub)                                             # gradients, moments and the step counter are now set
    torch.cuda.synchronize()
    p0 = tr.p.params.cpu().numpy()
    offs = tr.p.offsets
    cur = [p0[offs[i]:offs[i + 1]].reshape(params[i].shape) for i in range(case["L"] + 2)]
    for what, nodes in (("subset", sub), ("all", np.arange(n, dtype=np.int64))):
        tag = f"evaluate {name} {case_id} {what}"
        loss64, z64 = _ref(case, rp, col, X, labels, nodes, cur, torch.float64)
        loss32, z32 = _ref(case, rp, col, X, labels, nodes, cur, torch.float32)
        nodes_d = _dev(nodes, torch.int32)
        res = tr.evaluate(nodes_d, want_logp=True)
        assert isinstance(res, train.EvalResult) and res.loss.dim() == 0 and tuple(res.pred.shape) == (len(nodes),)
        assert tuple(res.logp.shape) == (len(nodes), case["C"]) and tuple(res.counts.shape) == (case["C"] ** 2 + 2,)
        check_rule(f"{tag} loss", [float(res.loss)], np.array([loss64]), np.array([loss32]), _FIGURES)
        pred = res.pred.cpu().numpy()
        keep = _check_pred(tag, pred, z64, z32)
        assert keep.all(), tag                               # the reference leaves out no row of these cases
        _check_counts(res.counts.cpu().numpy(), labels[nodes], pred, case["C"])
        np.testing.assert_array_equal(res.confusion, np.bincount(labels[nodes] * case["C"] + pred,
                                                                 minlength=case["C"] ** 2).reshape(case["C"], -1))
        assert res.n == len(nodes) and res.n_bad == 0 and res.micro_f1 == float(np.mean(pred == labels[nodes]))
        # with the batch's receptive field: bitwise the same
        resf = tr.evaluate(nodes_d, field=tr.field(nodes_d), want_logp=True)
        for a, b in ((res.loss, resf.loss), (res.pred, resf.pred), (res.logp, resf.logp), (res.counts, resf.counts)):
            assert torch.equal(a, b), tag
        # the training head's loss at the same parameters: another kernel, the same rule
        lfb = float(tr.forward_backward(nodes_d, _lib.GS_TF_FORWARD | _lib.GS_TF_HEAD))
        check_rule(f"{tag} forward_backward loss", [lfb], np.array([loss64]), np.array([loss32]), _FIGURES)
        # and the two kernels' losses against each other, under the same rule (not bitwise: other kernels)
        bound = 4.0 * abs(loss32 - loss64) + 2.0 ** -23 * abs(loss64)
        print(f"{tag} evaluate - forward_backward: {abs(float(res.loss) - lfb):.3e}, bound {bound:.3e}")
        assert abs(float(res.loss) - lfb) <= bound, tag
    # evaluate, with and without a field, touches no parameter, gradient or moment
    tr.forward_backward(sub)
    torch.cuda.synchronize()
    state = [t.clone() for t in (tr.p.params, tr.p.grads, tr.opt_m, tr.opt_v)]
    assert float(tr.p.grads.abs().max()) > 0 and float(tr.opt_v.abs().max()) > 0
    res = tr.evaluate(sub)
    tr.evaluate(nodes_d, field=tr.field(nodes_d), want_logp=True)
    torch.cuda.synchronize()
    for before, after in zip(state, (tr.p.params, tr.p.grads, tr.opt_m, tr.opt_v)):
        assert torch.equal(before, after)
    assert tr.optimizer_state()["step"] == 1 and tr._cls_frozen is False and res.logp is None


@pytest.mark.parametrize("fields", [False, True], ids=["full", "field"])
@pytest.mark.parametrize("cache", [True, False], ids=["cache", "nocache"])
@pytest.mark.parametrize("case_id", ["l2", "max", "bf16_f100"])
def test_evaluate_between_two_steps_changes_no_bit(gs, case_id, cache, fields):
    """step(a, fa); evaluate(v, fv); step(a, fa) ends in bitwise the
    parameters of the two steps alone: the layer-1 cache is never reused
    across paths."""
    case = tc.STEP_BY_ID[case_id]
    graph, n, rp, col, X, Xd, labels, params = _setup(case, "rmat")
    a_ids = _dev(tc.nodes_of(n), torch.int32)
    v_ids = _dev(tc.nodes_of(n, k=29, seed=99), torch.int32)
    ends = []
    for with_eval in (True, False):
        tr = _trainer(case, graph, Xd, labels, params, cache_agg1=cache)
        fa = tr.field(a_ids) if fields else None
        tr.step(a_ids, field=fa)
        if with_eval:
            res = tr.evaluate(v_ids, field=tr.field(v_ids) if fields else None)
            assert 0 <= res.micro_f1 <= 1
            if not fields:                                   # also the other path's rows in between
                tr.evaluate(v_ids, field=tr.field(v_ids))
        loss = tr.step(a_ids, field=fa).clone()
        torch.cuda.synchronize()
        ends.append((tr.p.params.clone(), loss))
    assert torch.equal(ends[0][0], ends[1][0]) and torch.equal(ends[0][1], ends[1][1])
    assert not torch.equal(ends[0][0], _trainer(case, graph, Xd, labels, params).p.params)


# ---------------------------------------------------- 3. ClassifierProbe.evaluate
def test_classifier_probe_evaluate():
    shape = int(np.argmin([s[0] * s[1] for s in PK.SHAPES]))   # the smallest shape (D = 5, C = 2)
    c = PK.case(shape, PK.SCALES[shape][1])
    rs = np.random.RandomState(2)
    order = np.stack([rs.permutation(c.order[0]) for _ in range(3)])
    E = _dev(c.E)
    probe = train.ClassifierProbe(E, c.labels, c.C, weights=(torch.from_numpy(c.W), torch.from_numpy(c.b)),
                                  lr=PK.LR, max_norm=PK.MAX_NORM, batch=c.batch)
    _losses, snaps = probe.run(order)
    nodes = rs.permutation(len(c.E))[:len(c.E) - 3]
    res = probe.evaluate(nodes, snaps)
    assert tuple(res.loss.shape) == (3,) and tuple(res.pred.shape) == (3, len(nodes)) and res.logp is None
    assert tuple(res.counts.shape) == (3, c.C * c.C + 2) and res.confusion.shape == (3, c.C, c.C)
    pred = res.pred.cpu().numpy()
    want = probe.predict(nodes, snaps).cpu().numpy()
    S = snaps.cpu().numpy()
    X64 = c.E[nodes].astype(np.float64)
    for e in range(3):
        W, b = S[e, :c.C * c.D].reshape(c.C, c.D), S[e, c.C * c.D:]
        z64 = X64 @ W.T.astype(np.float64) + b
        z32 = (torch.from_numpy(np.ascontiguousarray(c.E[nodes])) @ torch.from_numpy(W).t() + torch.from_numpy(b)).numpy()
        keep = _check_pred(f"probe epoch {e}", pred[e], z64, z32.astype(np.float64))
        np.testing.assert_array_equal(pred[e][keep], want[e][keep])
        _check_counts(res.counts[e].cpu().numpy(), c.labels[nodes], pred[e], c.C)
        assert res.accuracy[e] == float(np.mean(pred[e] == c.labels[nodes]))
    one = probe.evaluate(nodes)                              # the current parameters are the last snapshot
    assert one.loss.dim() == 0 and torch.equal(one.pred, res.pred[2]) and torch.equal(one.counts, res.counts[2])
    assert torch.equal(one.loss, res.loss[2]) and isinstance(one.macro_f1, float)
    assert torch.equal(probe.evaluate(_dev(nodes)).pred, one.pred)
    for bad in ([0, len(c.E)], [-1]):
        with pytest.raises(IndexError):
            probe.evaluate(bad)
    with pytest.raises(ValueError):
        probe.evaluate(nodes, snaps[:, :-1])


# ------------------------------------------------------- 4. utils.evaluate_full
def test_evaluate_full_protocol(gs, tmp_path, monkeypatch, capsys):
    case = tc.STEP_BY_ID["l2"]
    graph, n, rp, col, X, Xd, labels, params = _setup(case, "hub_max")
    tr = _trainer(case, graph, Xd, labels, params)
    perm = np.random.RandomState(4).permutation(n)
    dc = types.SimpleNamespace(g_val=perm[:60], g_test=perm[60:150], g_labels=labels)
    for _ in range(3):
        tr.step(perm[150:])
    monkeypatch.chdir(tmp_path)
    want_val = float(np.mean(tr.evaluate(dc.g_val).pred.cpu().numpy() == labels[dc.g_val]))
    want_test = float(np.mean(tr.evaluate(dc.g_test).pred.cpu().numpy() == labels[dc.g_test]))
    capsys.readouterr()
    for use_field in (True, False):
        m = utils.evaluate_full(dc, "g", tr, -1.0, f"t{int(use_field)}", 7, use_field=use_field)
        assert m == want_val
        assert capsys.readouterr().out.splitlines() == [f"Validation F1: {want_val}", f"Test F1: {want_test}"]
        path = tmp_path / "models" / "model_best_t{}_ep7_{:.4f}.torch".format(int(use_field), want_test)
        assert path.exists()
        saved = torch.load(path)
        sd = tr.state_dict()
        assert sorted(saved) == sorted(sd) and all(torch.equal(saved[k].to(DEV), sd[k]) for k in sd)
    files = sorted(os.listdir(tmp_path / "models"))
    assert len(files) == 2
    m = utils.evaluate_full(dc, "g", tr, 2.0, "t9", 8)       # no improvement: one print, nothing written
    assert m == 2.0 and capsys.readouterr().out.splitlines() == [f"Validation F1: {want_val}"]
    assert sorted(os.listdir(tmp_path / "models")) == files
