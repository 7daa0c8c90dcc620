"""Per-edge weights on the exact path, on the device: hip_ops.agg_full /
agg_full_bwd with `edge_weight=` and train.FullTrainer / FullEmbedder with
`edge_weight=`, on the graphs of tests/full_cases.py and the directed graph of
tests/full_train_cases.py.

Two kinds of check.  With unit weights (and unit self_weight, norm="mean")
every result is BITWISE the unweighted one: the operators at every lane-group
width and dtype, with and without a field, and a whole trainer step.  With
random weights the results are held against the float64 reference of
tests/full_weight_ref.py under adam_cases.check_rule: err <= 4 * e_torch +
2^-23 * max|ref|, e_torch being the error of the reference's own fp32 run.

FACTOR: the 4 of the rule unless a row says otherwise here, with its reason.
One exception is computed, not tabulated (bf16_output_factor): the bare
operator over a bf16 table writes a bf16 row, the fp32 sum rounded once.
Where that sum and the float64 sum straddle a bf16 rounding boundary the two
rounded values differ by one whole bf16 ulp of THAT element, whatever the size
of the fp32 error, so the kernel's largest error is one ulp of whichever
element flips -- at most ulp_bf16(max|ref|).  e_torch is the same event in the
reference's own fp32 run, at whichever element flips there (or 0 when none
does), so err / e_torch compares the binades of two elements, not two errors:
with weights in [-2, 2] and norm="sum" the rows span several binades.  The
factor is therefore raised to ulp_bf16(max|ref|) / e_torch where that exceeds
4 -- from the references and the format alone, never from the kernel's output
-- and every element must also lie within one bf16 ulp of its own reference.
"""
import importlib

import numpy as np
import pytest
import torch

from tests import full_cases as fc
from tests import full_field_cases as ffc
from tests import full_train_cases as tc
from tests import full_unsup_cases as uc
from tests import full_weight_ref as wref
from tests.adam_cases import check_rule

pytestmark = pytest.mark.gpu

ops = importlib.import_module("graphsage-pytorch_amd.hip_ops")
train = importlib.import_module("graphsage-pytorch_amd.train")
DEV = torch.device("cuda", 0)
SEG_LENS = [fc.SEG_LEN, None]
FACTOR = {}              # {(test, case id): (factor, reason)}
_MEMO = {}


def factor(test, case_id):
    return FACTOR.get((test, case_id), (4.0, ""))[0]


def _np(t):
    return t.detach().float().cpu().numpy()


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _same(a, b):
    """Bitwise equality, NaN rows included."""
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(_bits(a), _bits(b)))


def _plans(name, gcn, seg_len):
    """(forward plan, its transpose, n, row_ptr, col); "directed" through a bare-CSR graph object."""
    key = ("plan", name, gcn, seg_len)
    if key not in _MEMO:
        graph, n, rp, col = ffc.graph_of(name)
        plan = ops.agg_full_plan(graph, gcn=gcn, seg_len=seg_len)
        _MEMO[key] = (plan, plan.transposed(), n, np.asarray(rp, np.int64), np.asarray(col, np.int64))
    return _MEMO[key]


def _inputs(n, F):
    """X, dA, dSelf, Hprev as fp32 numpy, fixed per shape."""
    key = ("in", n, F)
    if key not in _MEMO:
        rs = np.random.RandomState(57 + F)
        _MEMO[key] = [rs.uniform(-1, 1, (n, F)).astype(np.float32) for _ in range(4)]
    return _MEMO[key]


def _weights(name, kind):
    """(w [n_entries], self_weight [n]) fp32 of a graph: "mean" in [0.25, 4] (den well away from 0), "sum" in
    [-2, 2]; the self weights are a non-unit vector of the same range."""
    key = ("w", name, kind)
    if key not in _MEMO:
        _g, n, rp, _col = ffc.graph_of(name)
        rs = np.random.RandomState(len(name) + (0 if kind == "mean" else 100))
        lo, hi = (0.25, 4.0) if kind == "mean" else (-2.0, 2.0)
        _MEMO[key] = (rs.uniform(lo, hi, int(rp[-1])).astype(np.float32), rs.uniform(lo, hi, n).astype(np.float32))
    return _MEMO[key]


def _bf16_ulp(x):
    """The spacing of bf16 values at magnitude |x| (8 significant bits), elementwise."""
    x = np.maximum(np.abs(np.asarray(x, np.float64)), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(x)) - 7)


def bf16_output_factor(base, ref, tor):
    """check_rule's factor for a bf16 output row (the module docstring): one bf16 ulp at max|ref| over e_torch,
    where that exceeds `base`; an fp32 run without any error keeps `base`."""
    e_torch = float(np.max(np.abs(tor - ref)))
    ulp = float(_bf16_ulp(np.abs(ref).max()))
    return max(base, ulp / e_torch) if e_torch > 0 else base


def _field(plan, tplan, n, L=2):
    return ops.full_field(plan, tplan, tc.nodes_of(n), L, device=DEV)


# --------------------------------------- 1. unit weights: bitwise the unweighted path
@pytest.mark.parametrize("gcn", [False, True], ids=["sage", "gcn"])
@pytest.mark.parametrize("dt,F", fc.OP_SHAPES, ids=[f"{d}-{f}" for d, f in fc.OP_SHAPES])
@pytest.mark.parametrize("name", ["hub", "hub_max", "directed"])
def test_unit_weights_forward_is_bitwise_the_unweighted(gs, name, dt, F, gcn):
    """agg_full over all rows, over a window and over a field's rows; "hub" keeps its NaN rows."""
    for seg_len in SEG_LENS:
        plan, tplan, n, _rp, _col = _plans(name, gcn, seg_len)
        ew = ops.EdgeWeights(plan, np.ones(plan.n_entries, np.float32))
        Xd = _dev(_inputs(n, F)[0])
        if dt == "bf16":
            Xd = Xd.to(torch.bfloat16)
        want = ops.agg_full("MEAN", Xd, plan)
        got = ops.agg_full("MEAN", Xd, plan, edge_weight=ew)
        assert _same(got, want), seg_len
        assert _same(ops.agg_full("MEAN", Xd, plan, row0=3, n_rows=n - 8, edge_weight=ew), want[3:n - 5])
        f = _field(plan, tplan, n)
        for l in (1, 2):
            a = ops.agg_full("MEAN", Xd, plan, field=f, layer=l)
            b = ops.agg_full("MEAN", Xd, plan, field=f, layer=l, edge_weight=ew)
            assert _same(a, b) and _same(b, want[f.rows(l).long()]), (seg_len, l)


@pytest.mark.parametrize("gcn", [False, True], ids=["sage", "gcn"])
@pytest.mark.parametrize("F", [128, 50])
@pytest.mark.parametrize("name", ["hub_max", "directed"])
def test_unit_weights_backward_is_bitwise_the_unweighted(gs, name, F, gcn):
    for seg_len in SEG_LENS:
        plan, tplan, n, _rp, _col = _plans(name, gcn, seg_len)
        ew = ops.EdgeWeights(plan, np.ones(plan.n_entries, np.float32))
        _X, dA, dSelf, Hprev = (_dev(a) for a in _inputs(n, F))
        for kw in ({}, {"dSelf": dSelf, "Hprev": Hprev}):
            want = ops.agg_full_bwd("MEAN", dA, tplan, **kw)
            assert _same(ops.agg_full_bwd("MEAN", dA, tplan, edge_weight=ew, **kw), want), (seg_len, bool(kw))
        assert tplan.n_split >= 1 or seg_len is None
        f = _field(plan, tplan, n)
        for l in (1, 2):
            rows = f.rows(l).long()
            kw = {"dSelf": dSelf[rows].contiguous(), "Hprev": Hprev, "field": f, "layer": l}
            a = ops.agg_full_bwd("MEAN", dA[rows].contiguous(), tplan, **kw)
            b = ops.agg_full_bwd("MEAN", dA[rows].contiguous(), tplan, edge_weight=ew, **kw)
            assert _same(a, b), (seg_len, l)


# ------------------------------------------------ 2. random weights against float64
W_KINDS = ["mean", "sum"]


@pytest.mark.parametrize("gcn", [False, True], ids=["sage", "gcn"])
@pytest.mark.parametrize("kind", W_KINDS)
@pytest.mark.parametrize("dt,F", [("f32", 256), ("f32", 50), ("bf16", 100)], ids=["f32-256", "f32-50", "bf16-100"])
@pytest.mark.parametrize("name", ["hub_max", "directed", "rmat"])
def test_weighted_forward_matches_float64_reference(gs, name, dt, F, kind, gcn):
    """norm="mean" with weights in [0.25, 4] and norm="sum" with weights in [-2, 2], a non-unit self_weight
    vector (read under gcn only), at seg_len 8 and the default; two runs are bitwise equal."""
    bf16 = dt == "bf16"
    w, sw = _weights(name, kind)
    _p, _t, n, rp, col = _plans(name, gcn, None)
    X = fc.features(n, F, bf16)
    Xd = _dev(X).to(torch.bfloat16) if bf16 else _dev(X)
    ref = wref.aggregate_reference(rp, col, w, X, gcn, kind, sw, bf16=bf16)
    tor = wref.aggregate_reference(rp, col, w, X, gcn, kind, sw, bf16=bf16, dtype=torch.float32)
    for seg_len in SEG_LENS:
        plan = _plans(name, gcn, seg_len)[0]
        if seg_len == fc.SEG_LEN:
            assert plan.n_split >= 4  # the split path runs
        ew = ops.EdgeWeights(plan, w, norm=kind, self_weight=sw)
        out = torch.full((n, F), float("nan"), dtype=Xd.dtype, device=DEV)
        ops.agg_full("MEAN", Xd, plan, out, edge_weight=ew)
        again = ops.agg_full("MEAN", Xd, plan, edge_weight=ew)
        torch.cuda.synchronize()
        assert _same(out, again)
        fac = factor("op_fwd", f"{name}-{dt}-{F}-{kind}-{gcn}")
        if bf16:
            fac = bf16_output_factor(fac, ref, tor)
            got = _np(out).astype(np.float64)
            assert (np.abs(got - ref) <= _bf16_ulp(np.maximum(np.abs(got), np.abs(ref)))).all()
        check_rule(f"weighted agg_full {name} {dt} F={F} {kind} gcn={gcn} seg_len={seg_len}", _np(out),
                   ref.reshape(-1), tor.reshape(-1), factor=fac)


@pytest.mark.parametrize("gcn", [False, True], ids=["sage", "gcn"])
@pytest.mark.parametrize("kind", W_KINDS)
@pytest.mark.parametrize("F", [256, 50])
@pytest.mark.parametrize("name", ["hub_max", "directed", "rmat"])
def test_weighted_backward_matches_float64_reference(gs, name, F, kind, gcn):
    """agg_full_bwd bare and with the dSelf + Hprev epilogue."""
    w, sw = _weights(name, kind)
    _p, _t, n, rp, col = _plans(name, gcn, None)
    X, dA, dSelf, Hprev = _inputs(n, F)
    dAd, dSd, Hpd = _dev(dA), _dev(dSelf), _dev(Hprev)
    for epi in (False, True):
        kw = {"dSelf": dSelf, "Hprev": Hprev} if epi else {}
        ref = wref.aggregate_backward(rp, col, w, X, dA, gcn, kind, sw, **kw)[1]
        tor = wref.aggregate_backward(rp, col, w, X, dA, gcn, kind, sw, dtype=torch.float32, **kw)[1]
        for seg_len in SEG_LENS:
            plan, tplan, _n, _rp, _col = _plans(name, gcn, seg_len)
            ew = ops.EdgeWeights(plan, w, norm=kind, self_weight=sw)
            dkw = {"dSelf": dSd, "Hprev": Hpd} if epi else {}
            dH = torch.full((n, F), float("nan"), dtype=torch.float32, device=DEV)
            ops.agg_full_bwd("MEAN", dAd, tplan, dH, edge_weight=ew, **dkw)
            again = ops.agg_full_bwd("MEAN", dAd, plan, edge_weight=ew, **dkw)   # a forward plan: its own transpose
            torch.cuda.synchronize()
            assert _same(dH, again)
            check_rule(f"weighted agg_full_bwd {name} F={F} {kind} gcn={gcn} seg_len={seg_len} epilogue={epi}",
                       _np(dH), ref.reshape(-1), tor.reshape(-1), factor=factor("op_bwd", f"{name}-{F}-{kind}-{gcn}"))
            if epi:
                assert bool((dH[Hpd <= 0] == 0).all())


@pytest.mark.parametrize("gcn", [False, True], ids=["sage", "gcn"])
@pytest.mark.parametrize("kind", W_KINDS)
@pytest.mark.parametrize("name", ["hub_max", "directed"])
def test_field_rows_are_bitwise_the_unrestricted_weighted_rows(gs, name, kind, gcn):
    """agg_full and agg_full_bwd on the field of a 37-node batch: a restricted forward row is the full call's
    row, and the restricted backward is the full backward of a dA that is zero off R_l, on the rows R_{l-1}."""
    F = 50 if name == "directed" else 128
    w, sw = _weights(name, kind)
    for seg_len in SEG_LENS:
        plan, tplan, n, _rp, _col = _plans(name, gcn, seg_len)
        ew = ops.EdgeWeights(plan, w, norm=kind, self_weight=sw)
        X, dA, dSelf, Hprev = (_dev(a) for a in _inputs(n, F))
        f = _field(plan, tplan, n)
        full = ops.agg_full("MEAN", X, plan, edge_weight=ew)
        for l in (1, 2):
            rows, prev = f.rows(l).long(), f.rows(l - 1).long()
            assert _same(ops.agg_full("MEAN", X, plan, field=f, layer=l, edge_weight=ew), full[rows]), (seg_len, l)
            keep = torch.zeros(n, 1, device=DEV)
            keep[rows] = 1
            want = ops.agg_full_bwd("MEAN", dA * keep, tplan, dSelf=dSelf * keep, Hprev=Hprev, edge_weight=ew)[prev]
            got = ops.agg_full_bwd("MEAN", dA[rows].contiguous(), tplan, dSelf=dSelf[rows].contiguous(), Hprev=Hprev,
                                   field=f, layer=l, edge_weight=ew)
            assert _same(got, want), (seg_len, l)


# ------------------------------------------------------------------ 3. the trainer
def _case(id, L, F, H, C, gcn, kind="mean", bf16=False, head="nll", graph="hub_max", seg_len=fc.SEG_LEN):
    return {"id": id, "L": L, "F": F, "H": H, "C": C, "gcn": gcn, "kind": kind, "bf16": bf16, "head": head,
            "graph": graph, "seg_len": seg_len, "agg": "MEAN"}


STEP_CASES = [
    _case("l1", 1, 256, 128, 3, False),
    _case("l2", 2, 256, 128, 7, False),
    _case("l2_default", 2, 256, 128, 3, False, seg_len=None),
    _case("l3_h80", 3, 64, 80, 7, False),
    _case("h16_f50_sum", 2, 50, 16, 3, False, kind="sum"),
    _case("gcn", 2, 256, 128, 7, True),
    _case("gcn_h80_sum", 2, 64, 80, 3, True, kind="sum"),
    _case("gcn_l3_f50", 3, 50, 16, 7, True),
    _case("directed_l2", 2, 64, 80, 3, False, graph="directed"),
    _case("bf16", 2, 256, 128, 3, False, bf16=True),
    _case("multilabel", 2, 64, 80, 5, False, head="multilabel"),
]
STEP_BY_ID = {c["id"]: c for c in STEP_CASES}
STEP_IDS = [c["id"] for c in STEP_CASES]


def _setup(case):
    """graph, n, rp, col, X, Xd, labels (one class per node, or [n, C] bool), nodes, params, w, sw."""
    key = ("setup", case["id"])
    if key not in _MEMO:
        graph, n, rp, col = ffc.graph_of(case["graph"])
        X = fc.features(n, case["F"], case["bf16"])
        Xd = _dev(X).to(torch.bfloat16) if case["bf16"] else _dev(X)
        if case["head"] == "multilabel":
            labels = np.random.RandomState(100 + case["C"]).uniform(0, 1, (n, case["C"])) < 0.3
        else:
            labels = tc.labels_of(n, case["C"])
        w, sw = _weights(case["graph"], case["kind"])
        _MEMO[key] = (graph, n, rp, col, X, Xd, labels, tc.nodes_of(n), tc.params_of(case), w, sw)
    return _MEMO[key]


def _trainer(case, w="case", params=None, **kw):
    graph, n, rp, col, X, Xd, labels, nodes, params0, w0, sw = _setup(case)
    params = params0 if params is None else params
    L = case["L"]
    weights = ([torch.from_numpy(np.array(p)) for p in params[:L]], torch.from_numpy(np.array(params[L])),
               torch.from_numpy(np.array(params[L + 1])))
    args = {"seg_len": case["seg_len"], "head": case["head"]}
    if w is not None:
        args.update(edge_weight=w0 if isinstance(w, str) and w == "case" else w, edge_norm=case["kind"],
                    self_weight=sw)
    args.update(kw)
    return train.FullTrainer(graph, Xd, torch.from_numpy(labels), case["C"], num_layers=L, hidden=case["H"],
                             agg_func="MEAN", gcn=case["gcn"], weights=weights, **args)


def _refs(case):
    key = ("ref", case["id"])
    if key not in _MEMO:
        graph, n, rp, col, X, Xd, labels, nodes, params, w, sw = _setup(case)
        args = (rp, col, w, X, labels, nodes, params, case["gcn"])
        kw = {"norm": case["kind"], "self_weight": sw, "bf16": case["bf16"], "head": case["head"]}
        _MEMO[key] = (wref.step_reference(*args, **kw), wref.step_reference(*args, dtype=torch.float32, **kw))
    return _MEMO[key]


def _dev_nodes(nodes):
    return torch.from_numpy(np.asarray(nodes).astype(np.int32)).to(DEV)


def _check_step(tag, case, tr, loss, rows_of=None):
    (loss64, g64, h64), (loss32, g32, h32) = _refs(case)
    fac = factor("step", case["id"])
    check_rule(f"{tag} loss", [float(loss)], np.array([loss64]), np.array([loss32]), factor=fac)
    for l in range(1, case["L"] + 1):
        rows = slice(None) if rows_of is None else _np(rows_of(l)).astype(np.int64)
        check_rule(f"{tag} H_{l}", _np(tr.hidden(l))[rows], h64[l - 1][rows].reshape(-1), h32[l - 1][rows].reshape(-1),
                   factor=fac)
    for i, pname in enumerate(tc.names_of(case["L"])):
        got = _np(tr.p.view(i, grad=True))
        assert got.shape == g64[i].shape and np.abs(g64[i]).max() > 0
        check_rule(f"{tag} d{pname}", got, g64[i].reshape(-1), g32[i].reshape(-1), factor=fac)


@pytest.mark.parametrize("case_id", ["l2", "gcn", "l2_default", "multilabel"])
def test_unit_weights_trainer_step_is_bitwise_the_unweighted(gs, case_id):
    """Loss, flat gradient and every H_l after one forward_backward, full and through a field, and the
    parameters after the whole step."""
    case = STEP_BY_ID[case_id]
    n = _setup(case)[1]
    nodes = _dev_nodes(tc.nodes_of(n))
    plain = _trainer(case, w=None)
    unit = _trainer(case, w=np.ones(plain.plan.n_entries, np.float32), self_weight=1.0, edge_norm="mean")
    assert unit.edge_weights is not None and plain.edge_weights is None
    for use_field in (False, True):
        kw_p = {"field": plain.field(nodes)} if use_field else {}
        kw_u = {"field": unit.field(nodes)} if use_field else {}
        a = plain.forward_backward(nodes, **kw_p).clone()
        b = unit.forward_backward(nodes, **kw_u).clone()
        torch.cuda.synchronize()
        assert _same(a, b) and _same(plain.p.grads, unit.p.grads) and float(unit.p.grads.abs().max()) > 0
        if not use_field:
            for l in range(1, case["L"] + 1):
                assert _same(plain.hidden(l), unit.hidden(l))
    plain.step(nodes)
    unit.step(nodes)
    assert _same(plain.p.params, unit.p.params)
    assert _same(plain.embed(), unit.embed())


@pytest.mark.parametrize("case_id", STEP_IDS)
def test_weighted_step_matches_float64_reference(gs, case_id):
    """Loss, every H_l and every gradient tensor of one forward_backward on a 37-node subset, each under the
    rule on its own; a second run is bitwise the first."""
    case = STEP_BY_ID[case_id]
    n = _setup(case)[1]
    nodes = _dev_nodes(tc.nodes_of(n))
    tr = _trainer(case)
    before = tr.p.params.clone()
    loss = tr.forward_backward(nodes).clone()
    torch.cuda.synchronize()
    assert torch.equal(tr.p.params, before)
    _check_step(f"weighted step {case_id}", case, tr, loss)
    grads = tr.p.grads.clone()
    again = _trainer(case, cache_agg1=False)
    loss2 = again.forward_backward(nodes)
    assert _same(loss2, loss) and _same(again.p.grads, grads)


@pytest.mark.parametrize("case_id", ["l2", "gcn", "l3_h80", "gcn_h80_sum", "directed_l2", "multilabel"])
def test_weighted_field_step_matches_float64_reference(gs, case_id):
    """The same step with field=: the same function, so the same reference -- loss, gradients and the rows
    R_l of every H_l under the rule, as the unweighted field step is checked."""
    case = STEP_BY_ID[case_id]
    n = _setup(case)[1]
    nodes = _dev_nodes(tc.nodes_of(n))
    tr = _trainer(case)
    field = tr.field(nodes)
    loss = tr.forward_backward(nodes, field=field).clone()
    torch.cuda.synchronize()
    _check_step(f"weighted field step {case_id}", case, tr, loss, rows_of=field.rows)
    g = tr.p.grads.clone()
    assert _same(tr.forward_backward(nodes, field=field), loss) and _same(tr.p.grads, g)   # repeatable, cached A_1


@pytest.mark.parametrize("case_id", ["l2", "gcn"])
def test_set_edge_weight_is_a_fresh_trainer(gs, case_id):
    """set_edge_weight(w2) then a step: bitwise a trainer constructed with w2 (a stale cached A_1 would show),
    full and through a field; embed() and evaluate() follow the new weights too."""
    case = STEP_BY_ID[case_id]
    graph, n, rp, col, X, Xd, labels, nodes_h, params, w, sw = _setup(case)
    nodes = _dev_nodes(nodes_h)
    w2 = np.random.RandomState(77).uniform(0.25, 4.0, len(w)).astype(np.float32)
    tr = _trainer(case, cache_agg1=True)
    tr.forward_backward(nodes)                                  # fills the cache with w's A_1
    tr.forward_backward(nodes, field=tr.field(nodes))
    e_old = tr.embed().clone()
    tr.set_edge_weight(w2, edge_norm=case["kind"], self_weight=sw)
    fresh = _trainer(case, w=w2, cache_agg1=False)
    for use_field in (False, True):
        a = tr.forward_backward(nodes, **({"field": tr.field(nodes)} if use_field else {})).clone()
        b = fresh.forward_backward(nodes, **({"field": fresh.field(nodes)} if use_field else {})).clone()
        torch.cuda.synchronize()
        assert _same(a, b) and _same(tr.p.grads, fresh.p.grads), use_field
    e_new = tr.embed()
    assert _same(e_new, fresh.embed()) and not torch.equal(e_new, e_old)
    ra, rb = tr.evaluate(nodes), fresh.evaluate(nodes)
    assert _same(ra.loss, rb.loss) and torch.equal(ra.pred, rb.pred)
    ref = wref.step_reference(rp, col, w2, X, labels, nodes_h, params, case["gcn"], norm=case["kind"], self_weight=sw)
    tor = wref.step_reference(rp, col, w2, X, labels, nodes_h, params, case["gcn"], norm=case["kind"], self_weight=sw,
                              dtype=torch.float32)
    check_rule(f"evaluate after set_edge_weight {case_id}", [float(ra.loss)], np.array([ref[0]]), np.array([tor[0]]))
    check_rule(f"embed after set_edge_weight {case_id}", _np(e_new), ref[2][-1].reshape(-1), tor[2][-1].reshape(-1))
    tr.set_edge_weight(None)                                    # and back to the unweighted trainer
    plain = _trainer(case, w=None)
    assert _same(tr.forward_backward(nodes).clone(), plain.forward_backward(nodes)) and _same(tr.p.grads, plain.p.grads)


def test_weighted_embedder_is_the_trainers_forward(gs):
    case = STEP_BY_ID["gcn"]
    graph, n, rp, col, X, Xd, labels, nodes_h, params, w, sw = _setup(case)
    tr = _trainer(case)
    tr.forward_backward(_dev_nodes(nodes_h))
    emb = train.FullEmbedder(graph, Xd, tr.weights(), gcn=True, seg_len=case["seg_len"], edge_weight=w,
                             self_weight=sw).embed()
    assert _same(emb, tr.hidden()) and _same(emb, tr.embed())


@pytest.mark.parametrize("name", ["hub_max", "directed"])
def test_sym_weights_give_the_normalised_adjacency_product(gs, name):
    """edge_weight="sym" with gcn: H_1 = relu((D^-1/2 (A + I) D^-1/2 X) W_1^T), the dense product in float64."""
    case = _case(f"sym-{name}", 1, 64, 80, 3, True, graph=name)
    graph, n, rp, col, X, Xd, labels, nodes_h, params, _w, _sw = _setup(case)
    tr = _trainer(case, w="sym")
    assert tr.edge_weights.norm == "sum"
    tr.forward_backward(_dev_nodes(nodes_h))
    A = np.zeros((n, n))
    A[np.repeat(np.arange(n), np.diff(rp)), col] = 1.0
    A[np.arange(n), np.arange(n)] = 1.0
    d = A.sum(1)
    An = A / np.sqrt(d[:, None] * d[None, :])
    ref = np.maximum((An @ X.astype(np.float64)) @ params[0].astype(np.float64).T, 0)
    tor = torch.relu((torch.from_numpy(An).float() @ torch.from_numpy(X)) @ torch.from_numpy(params[0]).t()).double().numpy()
    check_rule(f"sym H_1 {name}", _np(tr.hidden(1)), ref.reshape(-1), tor.reshape(-1), factor=factor("sym", name))


def test_weighted_unsup_step_matches_float64_reference(gs):
    """One unsup= step ("normal", "unsup") with weights: the pair loss of full_unsup_ref over the weighted forward."""
    s = uc.setup("l2_h16-hub_max")
    assert s["agg"] == "MEAN" and not s["gcn"] and not s["bf16"]
    w, sw = _weights("hub_max", "mean")
    L = s["L"]
    weights = ([torch.from_numpy(np.array(p)) for p in s["params"][:L]], torch.from_numpy(np.array(s["params"][L])),
               torch.from_numpy(np.array(s["params"][L + 1])))
    tr = train.FullTrainer(s["graph_obj"], _dev(s["X"]), torch.from_numpy(s["labels"]), s["C"], num_layers=L,
                           hidden=s["H"], agg_func="MEAN", gcn=False, weights=weights, seg_len=s["seg_len"],
                           edge_weight=w)
    b = tr.unsup_batch((torch.from_numpy(s["plan"].copy()).to(DEV), s["dims"], s["nodes"]), kind="normal",
                       learn_method="unsup", q=uc.Q, margin=uc.MARGIN)
    args = (s["rp"], s["col"], w, s["X"], s["nodes"], s["params"], False, s["lists"], "sage", uc.Q, uc.MARGIN)
    loss64, g64 = wref.unsup_step_reference(*args)
    loss32, g32 = wref.unsup_step_reference(*args, dtype=torch.float32)
    for field in (None, tr.field(b.nodes)):
        loss = tr.forward_backward(b.nodes, field=field, unsup=b).clone()
        torch.cuda.synchronize()
        tag = f"weighted unsup step field={field is not None}"
        check_rule(f"{tag} loss", [float(loss)], np.array([loss64]), np.array([loss32]), factor=factor("unsup", "loss"))
        for i, pname in enumerate(tc.names_of(L)[:L]):
            assert np.abs(g64[i]).max() > 0
            check_rule(f"{tag} d{pname}", _np(tr.p.view(i, grad=True)), g64[i].reshape(-1), g32[i].reshape(-1),
                       factor=factor("unsup", pname))


def test_refusals_come_before_any_launch(gs):
    case = STEP_BY_ID["l2"]
    graph, n, rp, col, X, Xd, labels, nodes_h, params, w, sw = _setup(case)
    plan, tplan, _n, _rp, _col = _plans("hub_max", False, fc.SEG_LEN)
    ew = ops.EdgeWeights(plan, w)
    out = torch.full((n, case["F"]), 7.0, device=DEV)
    with pytest.raises(ValueError, match="MAX"):
        ops.agg_full("MAX", Xd, plan, out, edge_weight=ew)
    with pytest.raises(ValueError, match="MAX"):
        ops.agg_full_bwd("MAX", Xd, tplan, out, edge_weight=ew, argmax=torch.zeros(n, case["F"], dtype=torch.int32,
                                                                                  device=DEV))
    with pytest.raises(ValueError, match="another plan"):
        ops.agg_full("MEAN", Xd, _plans("hub_max", True, fc.SEG_LEN)[0], out, edge_weight=ew)
    with pytest.raises(ValueError, match="another plan"):
        ops.agg_full_bwd("MEAN", Xd, _plans("hub_max", True, fc.SEG_LEN)[1], out, edge_weight=ew)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    with pytest.raises(ValueError, match="MAX"):
        train.FullTrainer(graph, Xd, torch.from_numpy(labels), case["C"], agg_func="MAX", edge_weight=w)
    with pytest.raises(ValueError, match="MAX"):
        train.FullEmbedder(graph, Xd, [torch.from_numpy(p) for p in params[:2]], agg_func="MAX", edge_weight=w)
    neg = w.copy()
    neg[rp[3]:rp[4]] = -1.0                                     # node 3's row sums to a negative den
    with pytest.raises(ValueError, match="weight sum"):
        _trainer(case, w=neg)
    with pytest.raises(ValueError, match="weight sum"):
        train.FullEmbedder(graph, Xd, [torch.from_numpy(p) for p in params[:2]], edge_weight=neg)
    assert _trainer(case, w=neg, edge_norm="sum").edge_weights.norm == "sum"       # the sum takes them
    tr = _trainer(case)
    with pytest.raises(ValueError, match="weight sum"):
        tr.set_edge_weight(neg)
    assert tr.edge_weights is not None and np.array_equal(tr.edge_weights.w, w)    # and the old set stays
    # the bare operator returns what IEEE gives: a row whose weights sum to 0 divides by 0
    zero = w.copy()
    zero[rp[3]:rp[4]] = 0.0
    got = ops.agg_full("MEAN", Xd, plan, edge_weight=ops.EdgeWeights(plan, zero))
    assert bool(torch.isnan(got[3]).all()) and bool(torch.isfinite(got[:3]).all())
