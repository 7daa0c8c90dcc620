"""Exact training restricted to the receptive field of a mini-batch on the
device (hip_ops.full_field, agg_full / agg_full_bwd with field=,
train.FullTrainer with field=) against the CPU mirror
hip_ops.full_field_host, the unrestricted kernels (bitwise) and the float64
reference of tests/full_train_ref.py, on the inputs of
tests/full_field_cases.py.

Tolerance (adam_cases.check_rule): err <= 4 * e_torch + 2^-23 * max|ref|, with
e_torch the error of the reference's own fp32 run on the CPU against its
float64 run, never measured from the kernel.  What indexes or selects (the
field's rows, maps and items, restricted aggregate rows, MAX on ties) must be
exact.
"""
import importlib

import numpy as np
import pytest
import torch

from tests import adam_cases as ac
from tests import full_cases as fc
from tests import full_field_cases as ffc
from tests import full_train_cases as tc
from tests import full_train_ref as tref
from tests import step_ref
from tests.adam_cases import check_rule

pytestmark = pytest.mark.gpu

ops = importlib.import_module("graphsage-pytorch_amd.hip_ops")
train = importlib.import_module("graphsage-pytorch_amd.train")
_lib = importlib.import_module("graphsage-pytorch_amd._lib")
DEV = torch.device("cuda", 0)
STEP_GRAPH_CASES = ["hub_four", "hub_one", "hub_seg", "rmat5"]
_MEMO = {}


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype)


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def _plans(gname, gcn, seg_len):
    key = ("plan", gname, gcn, seg_len)
    if key not in _MEMO:
        graph, n, rp, col = ffc.graph_of(gname)
        plan = ops.agg_full_plan(graph, gcn=gcn, seg_len=seg_len)
        _MEMO[key] = (plan, plan.transposed(), n, rp, col)
    return _MEMO[key]


def _np(t):
    return t.cpu().numpy()


def _snapshot(f):
    """Everything a built field exposes, as numpy."""
    out = {"sizes": f.sizes}
    for l in range(f.n_layers + 1):
        out["rows", l], out["pos", l] = _np(f.rows(l)), _np(f.pos(l))
    for l in range(1, f.n_layers + 1):
        out["items", l], out["split", l] = _np(f.items(l)), _np(f.split(l))
        out["t_items", l], out["t_split", l] = _np(f.t_items(l)), _np(f.t_split(l))
        out["counts", l] = f.layer_counts(l)
    return out


def _same(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)


# ------------------------------------------------ 1. the field against its mirror
@pytest.mark.parametrize("L", [1, 2, 3])
@pytest.mark.parametrize("gcn", [False, True], ids=["sage", "gcn"])
@pytest.mark.parametrize("case_id", ffc.FIELD_IDS)
def test_device_field_is_the_host_mirror(gs, case_id, gcn, L):
    """rows_l, pos_l and the counts equal full_field_host's, and the compacted
    items and split rows, forward and transposed, equal a numpy filter of the
    plans' host arrays (unsorted `nodes`, seg_len 8 and the default)."""
    case = ffc.FIELD_BY_ID[case_id]
    for seg_len in (ffc.SEG_LEN, None):
        plan, tplan, n, rp, col = _plans(case["graph"], gcn, seg_len)
        host = ops.full_field_host(rp, col, case["nodes"], L, gcn)
        f = ops.full_field(plan, tplan, case["nodes"], L, device=DEV)
        assert f.sizes == host.sizes and f.n_layers == L
        for l in range(L + 1):
            assert np.array_equal(_np(f.rows(l)), host.rows(l)) and f.rows(l).dtype == torch.int32
            assert np.array_equal(_np(f.pos(l)), host.pos(l)) and f.pos(l).dtype == torch.int32
        for l in range(1, L + 1):
            items, split = ffc.filter_plan(plan, host.pos(l))
            t_items, t_split = ffc.filter_plan(tplan, host.pos(l - 1))
            assert f.layer_counts(l) == (len(items), len(split), len(t_items), len(t_split))
            assert np.array_equal(_np(f.items(l)), items) and np.array_equal(_np(f.split(l)), split)
            assert np.array_equal(_np(f.t_items(l)), t_items) and np.array_equal(_np(f.t_split(l)), t_split)
        if seg_len == ffc.SEG_LEN and L == case["L"] and case["split_at_r1"]:
            assert f.layer_counts(1)[1] >= 1           # the split path is part of the case


def _features(n, F, bf16):
    key = ("X", n, F, bf16)
    if key not in _MEMO:
        X = fc.features(n, F, bf16)
        Xd = torch.from_numpy(X).to(DEV)
        _MEMO[key] = (X, Xd.to(torch.bfloat16) if bf16 else Xd)
    return _MEMO[key]


def _setup(case, gname):
    graph, n, rp, col = ffc.graph_of(gname)
    X, Xd = _features(n, case["F"], case["bf16"])
    return graph, n, rp, col, X, Xd, tc.labels_of(n, case["C"]), tc.params_of(case)


def _trainer(case, graph, Xd, labels, params, **kw):
    L = case["L"]
    w = ([torch.from_numpy(p) for p in params[:L]], torch.from_numpy(params[L]), torch.from_numpy(params[L + 1]))
    args = {"seg_len": case["seg_len"]}
    args.update(kw)
    return train.FullTrainer(graph, Xd, torch.from_numpy(labels), case["C"], num_layers=L, hidden=case["H"],
                             agg_func=case["agg"], gcn=case["gcn"], weights=w, **args)


def test_two_fields_rebuilt_alternately_on_one_trainer(gs):
    """A, B, A, B into one ReceptiveField (the maps reset by walking the old
    rows) and A, B as objects of their own: every build is bitwise the first
    build of its nodes."""
    case = tc.STEP_BY_ID["l2"]
    graph, n, rp, col, X, Xd, labels, params = _setup(case, "hub_max")
    tr = _trainer(case, graph, Xd, labels, params)
    A, B = ffc.FIELD_BY_ID["hub_four"]["nodes"], np.array([0, 3, 200, 17, 125])
    fa, fb = tr.field(A), tr.field(B)
    first = {"A": _snapshot(fa), "B": _snapshot(fb)}
    assert first["A"]["sizes"] == (4, 90, 213) and not _same(first["A"], first["B"])
    f, ids = None, []
    for which, nodes in (("A", A), ("B", B), ("A", A), ("B", B)):
        f = tr.field(nodes, out=f)
        assert _same(_snapshot(f), first[which]), which
        ids.append(f.build_id)
    assert len(set(ids)) == 4 and _same(_snapshot(fa), first["A"]) and _same(_snapshot(fb), first["B"])
    host = ops.full_field_host(rp, col, B, 2)
    assert all(np.array_equal(first["B"]["pos", l], host.pos(l)) for l in range(3))


# --------------------------------------------------- 2. the restricted aggregate
def _op_inputs(n, F, ties=False):
    key = ("in", n, F, ties)
    if key not in _MEMO:
        rs = np.random.RandomState(31 + F)
        if ties:
            arrs = [rs.randint(0, 3, (n, F)), rs.randint(-4, 5, (n, F)), rs.randint(-4, 5, (n, F)),
                    rs.randint(-1, 2, (n, F))]
        else:
            arrs = [rs.uniform(-1, 1, (n, F)) for _ in range(4)]
        _MEMO[key] = [a.astype(np.float32) for a in arrs]
    return _MEMO[key]


OP_CASES = ["hub_four", "hub_seg", "rmat5", "directed"]


@pytest.mark.parametrize("F", [128, 50])
@pytest.mark.parametrize("gcn", [False, True], ids=["sage", "gcn"])
@pytest.mark.parametrize("agg", ["MEAN", "MAX"])
@pytest.mark.parametrize("case_id", OP_CASES)
def test_restricted_aggregate_rows_are_bitwise_the_full_rows(gs, case_id, agg, gcn, F):
    case = ffc.FIELD_BY_ID[case_id]
    L = case["L"]
    for seg_len in (ffc.SEG_LEN, None):
        plan, tplan, n, rp, col = _plans(case["graph"], gcn, seg_len)
        Xd = _dev(_op_inputs(n, F)[0])
        f = ops.full_field(plan, tplan, case["nodes"], L, device=DEV)
        am_full = torch.full((n, F), -7, dtype=torch.int32, device=DEV) if agg == "MAX" else None
        full = ops.agg_full(agg, Xd, plan, argmax=am_full)
        for l in range(1, L + 1):
            rows = f.rows(l).long()
            am = torch.full((f.size(l), F), -7, dtype=torch.int32, device=DEV) if agg == "MAX" else None
            out = torch.full((f.size(l), F), float("nan"), dtype=torch.float32, device=DEV)
            ops.agg_full(agg, Xd, plan, out, field=f, layer=l, argmax=am)
            torch.cuda.synchronize()
            assert torch.equal(out, full[rows]), (seg_len, l)
            if agg == "MAX":
                assert torch.equal(am, am_full[rows]), (seg_len, l)       # global source ids
                plain = ops.agg_full(agg, Xd, plan, field=f, layer=l)     # without argmax: the same rows
                assert torch.equal(plain, out)
        Xb = Xd.to(torch.bfloat16)                                        # the bf16 form of layer 1
        assert torch.equal(ops.agg_full(agg, Xb, plan, field=f, layer=1), ops.agg_full(agg, Xb, plan)[f.rows(1).long()])


# ------------------------------------------- 3. the restricted backward aggregate
def _restricted_bwd(case_id, agg, gcn, F, ties):
    """Yields (tag, device dH [n_{l-1}, F], float64 reference rows, fp32 reference rows) per seg_len and layer."""
    case = ffc.FIELD_BY_ID[case_id]
    L = case["L"]
    _p, _t, n, rp, col = _plans(case["graph"], gcn, None)
    X, dA, dSelf, Hprev = _op_inputs(n, F, ties)
    Xd, Hpd = _dev(X), _dev(Hprev)
    host = ops.full_field_host(rp, col, case["nodes"], L, gcn)
    for l in range(1, L + 1):
        keep = (host.pos(l) >= 0)[:, None]
        dA_l, dS_l = np.where(keep, dA, 0).astype(np.float32), np.where(keep, dSelf, 0).astype(np.float32)
        ref = tref.aggregate_backward(rp, col, X, dA_l, agg, gcn, dSelf=dS_l, Hprev=Hprev)[2][host.rows(l - 1)]
        tor = tref.aggregate_backward(rp, col, X, dA_l, agg, gcn, dSelf=dS_l, Hprev=Hprev,
                                      dtype=torch.float32)[2][host.rows(l - 1)]
        for seg_len in (ffc.SEG_LEN, None):
            plan, tplan, _n, _rp, _col = _plans(case["graph"], gcn, seg_len)
            f = ops.full_field(plan, tplan, case["nodes"], L, device=DEV)
            rows = host.rows(l)
            am = None
            if agg == "MAX":
                am = torch.full((len(rows), F), -7, dtype=torch.int32, device=DEV)
                ops.agg_full("MAX", Xd, plan, field=f, layer=l, argmax=am)
            dH = torch.full((f.size(l - 1), F), float("nan"), dtype=torch.float32, device=DEV)
            ops.agg_full_bwd(agg, _dev(dA[rows]), tplan, dH, dSelf=_dev(dSelf[rows]), argmax=am, Hprev=Hpd, field=f,
                             layer=l)
            again = ops.agg_full_bwd(agg, _dev(dA[rows]), tplan, dSelf=_dev(dSelf[rows]), argmax=am, Hprev=Hpd,
                                     field=f, layer=l)
            torch.cuda.synchronize()
            assert torch.equal(dH, again)                     # bitwise repeatable
            yield f"{case_id} {agg} gcn={gcn} F={F} seg_len={seg_len} layer={l}", dH, ref, tor


@pytest.mark.parametrize("F", [128, 50])
@pytest.mark.parametrize("gcn", [False, True], ids=["sage", "gcn"])
@pytest.mark.parametrize("agg", ["MEAN", "MAX"])
@pytest.mark.parametrize("case_id", OP_CASES)
def test_restricted_backward_matches_float64_reference(gs, case_id, agg, gcn, F):
    """agg_full_bwd(field=, layer=) on the rows R_{l-1} against
    full_train_ref.aggregate_backward fed a dA (and dSelf) that is zero off R_l."""
    for tag, dH, ref, tor in _restricted_bwd(case_id, agg, gcn, F, ties=False):
        check_rule(f"agg_full_bwd field {tag}", _np(dH), ref.reshape(-1), tor.reshape(-1),
                   factor=ffc.factor("op_bwd", f"{case_id}-{agg}-{gcn}-{F}"))


@pytest.mark.parametrize("F", [128, 50])
@pytest.mark.parametrize("gcn", [False, True], ids=["sage", "gcn"])
@pytest.mark.parametrize("case_id", OP_CASES)
def test_restricted_max_on_ties_is_the_reference_choice_exactly(gs, case_id, gcn, F):
    for tag, dH, ref, _tor in _restricted_bwd(case_id, "MAX", gcn, F, ties=True):
        assert np.array_equal(_np(dH).astype(np.float64), ref), tag


# ------------------------------------------------- 4. the step against float64
def _ref_step(case, rp, col, X, labels, nodes, params, dtype=torch.float64):
    return tref.step_reference(rp, col, X, labels, nodes, params, case["agg"], case["gcn"], bf16=case["bf16"],
                               dtype=dtype)


def _refs(case, gname, nodes):
    """(float64 step, fp32 step) of the reference, computed once per input."""
    key = ("ref", case["id"], gname, tuple(int(v) for v in nodes))
    if key not in _MEMO:
        graph, n, rp, col, X, Xd, labels, params = _setup(case, gname)
        _MEMO[key] = (_ref_step(case, rp, col, X, labels, nodes, params),
                      _ref_step(case, rp, col, X, labels, nodes, params, dtype=torch.float32))
    return _MEMO[key]


def _check_step(tag, tr, field, loss, refs, case, fac, key=None, labels=None):
    """`key`: the FACTOR rows ("step_loss", key) and ("step_head", key) hold for the loss head's outputs."""
    (loss64, g64, h64), (loss32, g32, h32) = refs
    L = case["L"]

    def head_factor(test, what, ref, tor):
        f = ffc.factor(test, key) if key else fac
        if f != ffc.PROPAGATED:
            return fac if f == 4.0 else f
        Wc, bc = (_np(tr.p.view(i)) for i in (L, L + 1))
        return ffc.propagated_head_factor(what, h64[-1], h32[-1], _np(field.rows(L)), labels, Wc, bc, ref, tor)

    check_rule(f"{tag} loss", [float(loss)], np.array([loss64]), np.array([loss32]),
               factor=head_factor("step_loss", "loss", loss64, loss32))
    for l in range(1, L + 1):
        rows = _np(field.rows(l)).astype(np.int64)
        check_rule(f"{tag} H_{l} on R_{l}", _np(tr.hidden(l))[rows], h64[l - 1][rows].reshape(-1),
                   h32[l - 1][rows].reshape(-1), factor=fac)
    for i, pname in enumerate(tc.names_of(L)):
        got = _np(tr.p.view(i, grad=True))
        assert got.shape == g64[i].shape and np.abs(g64[i]).max() > 0
        check_rule(f"{tag} d{pname}", got, g64[i].reshape(-1), g32[i].reshape(-1),
                   factor=head_factor("step_head", pname, g64[i], g32[i]) if i >= L else fac)


STEP_PAIRS = [(g, c) for g in STEP_GRAPH_CASES for c in tc.STEP_IDS] + \
    [("directed", c) for c in ("l2", "gcn", "max")]


@pytest.mark.parametrize("field_id,case_id", STEP_PAIRS)
def test_field_step_matches_float64_reference(gs, field_id, case_id):
    """Loss, every gradient tensor and the rows R_l of every H_l of one
    forward_backward(nodes, field=), each under the rule on its own; the depth
    is the step case's."""
    case, fcase = tc.STEP_BY_ID[case_id], ffc.FIELD_BY_ID[field_id]
    nodes = fcase["nodes"]
    graph, n, rp, col, X, Xd, labels, params = _setup(case, fcase["graph"])
    tr = _trainer(case, graph, Xd, labels, params)
    before = tr.p.params.clone()
    field = tr.field(nodes)
    assert field.sizes == ops.full_field_host(rp, col, nodes, case["L"], case["gcn"]).sizes
    assert all(s < n for s in field.sizes[:-1])                # restricted at every layer that computes
    loss = tr.forward_backward(nodes, field=field)
    torch.cuda.synchronize()
    assert torch.equal(tr.p.params, before)                    # no update before apply_update
    _check_step(f"field step {field_id} {case_id}", tr, field, loss, _refs(case, fcase["graph"], nodes), case,
                ffc.factor("step", f"{field_id}-{case_id}"), key=f"{field_id}-{case_id}", labels=labels)


# --------------------------------------------------- 5. a poisoned workspace
@pytest.mark.parametrize("case_id", ["l2", "max", "bf16_max"])
@pytest.mark.parametrize("field_id", ["hub_four", "rmat5"])
def test_field_step_reads_no_row_outside_the_field(gs, field_id, case_id):
    """The whole workspace filled with 0xFF bytes (NaN as fp32, -1 as int32)
    before a field step: a read of any row the step did not write itself
    shows, where the left-overs of an earlier full step would hide it."""
    case, fcase = tc.STEP_BY_ID[case_id], ffc.FIELD_BY_ID[field_id]
    nodes = fcase["nodes"]
    graph, n, rp, col, X, Xd, labels, params = _setup(case, fcase["graph"])
    tr = _trainer(case, graph, Xd, labels, params)
    tr.forward_backward(nodes)                                 # a full step's left-overs first
    tr._ws.fill_(0xFF)
    tr.p.grads.fill_(float("nan"))
    tr.invalidate_cache()
    field = tr.field(nodes)
    loss = tr.forward_backward(nodes, field=field)
    torch.cuda.synchronize()
    _check_step(f"poisoned {field_id} {case_id}", tr, field, loss, _refs(case, fcase["graph"], nodes), case,
                ffc.factor("step", f"{field_id}-{case_id}"), key=f"{field_id}-{case_id}", labels=labels)
    outside = np.setdiff1d(np.arange(n), _np(field.rows(1)))
    assert np.isnan(_np(tr.hidden(1))[outside]).all()          # and no row outside R_1 was written


# ------------------------------------------- 6. full and field paths interleaved
@pytest.mark.parametrize("case_id", ["l2", "max", "bf16_max"])
def test_full_and_field_steps_interleaved(gs, case_id):
    """full, field, full on one trainer with cache_agg1=True, an update after
    each: every step equals a fresh trainer's at the same weights (bitwise;
    the field step also under the rule against float64), so neither path
    reuses the other's layer-1 aggregate."""
    case, fcase = tc.STEP_BY_ID[case_id], ffc.FIELD_BY_ID["hub_four"]
    nodes = fcase["nodes"]
    graph, n, rp, col, X, Xd, labels, params = _setup(case, "hub_max")
    tr = _trainer(case, graph, Xd, labels, params, cache_agg1=True, lr=0.05)
    field = tr.field(nodes)
    for kind in ("full", "field", "field", "full", "full"):
        sd = {k: v.clone() for k, v in tr.state_dict().items()}
        fresh = _trainer(case, graph, Xd, labels, params, cache_agg1=False)
        fresh.load_state_dict(sd)
        kw = {"field": field} if kind == "field" else {}
        loss = tr.forward_backward(nodes, **kw).clone()
        want = fresh.forward_backward(nodes, **({"field": fresh.field(nodes)} if kind == "field" else {})).clone()
        torch.cuda.synchronize()
        assert torch.equal(loss, want) and torch.equal(tr.p.grads, fresh.p.grads), kind
        assert tr._agg1 == (train._FULL_AGG1 if kind == "full" else field.build_id)
        if kind == "field":
            L = case["L"]
            p0 = _np(tr.p.params)
            offs = np.concatenate([[0], np.cumsum([p.size for p in params])]).astype(np.int64)
            cur = [p0[offs[i]:offs[i + 1]].reshape(params[i].shape) for i in range(L + 2)]
            refs = (_ref_step(case, rp, col, X, labels, nodes, cur),
                    _ref_step(case, rp, col, X, labels, nodes, cur, dtype=torch.float32))
            _check_step(f"interleaved {case_id}", tr, field, loss, refs, case, ffc.factor("step", f"mix-{case_id}"))
        tr.apply_update()
    tr.invalidate_cache()
    assert tr._agg1 is None


def test_cache_follows_full_and_two_fields(gs):
    """full, A, A, B, full, invalidate_cache(), A on one trainer with
    cache_agg1=True and two different fields A and B: after each call the loss
    and the gradients are bitwise those of a trainer with cache_agg1=False
    given the same calls -- the order in which a stale compact A_1 (the other
    field's, or the N-row one) would be reused if the one cache variable named
    the wrong owner."""
    case = tc.STEP_BY_ID["l2"]
    graph, n, rp, col, X, Xd, labels, params = _setup(case, "hub_max")
    batch = {"A": ffc.FIELD_BY_ID["hub_four"]["nodes"], "B": np.array([0, 3, 200, 17, 125, 64])}
    tr = _trainer(case, graph, Xd, labels, params, cache_agg1=True, lr=0.05)
    plain = _trainer(case, graph, Xd, labels, params, cache_agg1=False, lr=0.05)
    fields = {t: {k: t.field(v) for k, v in batch.items()} for t in (tr, plain)}
    assert fields[tr]["A"].sizes != fields[tr]["B"].sizes and all(s < n for s in fields[tr]["B"].sizes[:-1])
    owner = {"full": train._FULL_AGG1, "A": fields[tr]["A"].build_id, "B": fields[tr]["B"].build_id}
    for call in ("full", "A", "A", "B", "full", "invalidate", "A"):
        if call == "invalidate":
            tr.invalidate_cache()
            plain.invalidate_cache()
            assert tr._agg1 is None
            continue
        got, want = [], []
        for t, res in ((tr, got), (plain, want)):
            if call == "full":
                loss = t.forward_backward(batch["A"])
            else:
                loss = t.forward_backward(batch[call], field=fields[t][call])
            res.extend((loss.clone(), t.p.grads.clone()))
            t.apply_update()
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), call
        assert float(got[1].abs().max()) > 0 and tr._agg1 == owner[call], call
    assert torch.equal(tr.p.params, plain.p.params)


@pytest.mark.parametrize("case_id", ["l2", "max_gcn"])
def test_every_node_through_a_field(gs, case_id):
    """nodes = arange(N): every n_l is N, and the step passes the rule."""
    case = tc.STEP_BY_ID[case_id]
    graph, n, rp, col, X, Xd, labels, params = _setup(case, "hub_max")
    nodes = np.arange(n)
    tr = _trainer(case, graph, Xd, labels, params)
    field = tr.field(nodes)
    assert field.sizes == (n,) * (case["L"] + 1)
    loss = tr.forward_backward(nodes, field=field)
    torch.cuda.synchronize()
    _check_step(f"all nodes {case_id}", tr, field, loss, _refs(case, "hub_max", nodes), case,
                ffc.factor("step", f"all-{case_id}"))


# ----------------------------------------------------------- 7. three updates
def _flat(xs):
    return np.concatenate([np.asarray(x, np.float64).reshape(-1) for x in xs])


@pytest.mark.parametrize("optimizer", ["sgd", "adam"])
@pytest.mark.parametrize("case_id", ["l2", "l3_h80", "gcn", "max", "bf16_max"])
def test_field_trainer_three_updates(gs, case_id, optimizer):
    """Three step(nodes_t, field=) calls, a different mini-batch each (the
    field rebuilt in place), the clip active: teacher-forced exactly as
    test_gpu_full_train.test_full_trainer_three_updates -- at the parameters
    the device holds, every raw gradient tensor against the float64 step of
    that mini-batch, then every parameter tensor after the update against the
    float64 update of that raw gradient."""
    case = tc.STEP_BY_ID[case_id]
    graph, n, rp, col, X, Xd, labels, params = _setup(case, "hub_max")
    L = case["L"]
    batches = [ffc.FIELD_BY_ID["hub_four"]["nodes"], np.array([0, 3, 200, 17, 125, 64]), np.array([1, 296, 5])]
    _l, g0, _h = _ref_step(case, rp, col, X, labels, batches[0], params)
    sizes = [p.size for p in params]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    goff = np.array([0, offs[L], offs[-1]], np.int64)
    norms = [np.sqrt((_flat(g0)[goff[k]:goff[k + 1]] ** 2).sum()) for k in range(2)]
    max_norm = ac.f32(0.25 * min(norms))                   # both groups clip at step 1
    lr, betas, eps, wd = ac.f32(0.05), (ac.f32(0.9), ac.f32(0.999)), ac.f32(1e-8), ac.f32(0.01)
    tr = _trainer(case, graph, Xd, labels, params, lr=lr, max_norm=max_norm, optimizer=optimizer, betas=betas,
                  eps=eps, weight_decay=wd)
    fac = ffc.factor("update", case_id)
    field = None
    for t in range(1, 4):
        nodes = batches[t - 1]
        p0 = _np(tr.p.params)
        cur = [p0[offs[i]:offs[i + 1]].reshape(params[i].shape) for i in range(L + 2)]
        g64 = _ref_step(case, rp, col, X, labels, nodes, cur)[1]
        g32 = _ref_step(case, rp, col, X, labels, nodes, cur, dtype=torch.float32)[1]
        if t == 1:
            assert all(np.sqrt((_flat(g64)[goff[k]:goff[k + 1]] ** 2).sum()) > max_norm for k in range(2))
        st = tr.optimizer_state()
        assert st["step"] == t - 1
        field = tr.field(nodes, out=field)
        assert field.size(1) < n
        tr.forward_backward(nodes, field=field)
        graw = _np(tr.p.grads)                                 # unclipped until apply_update
        for i, pname in enumerate(tc.names_of(L)):
            check_rule(f"field {optimizer} {case_id} step {t} d{pname}", graw[offs[i]:offs[i + 1]],
                       g64[i].reshape(-1), g32[i].reshape(-1), factor=fac)
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
            check_rule(f"field {optimizer} {case_id} step {t} {pname}", got[lo:hi], want[lo:hi], tor[lo:hi],
                       factor=fac)
    assert tr.optimizer_state()["step"] == 3
    b = _trainer(case, graph, Xd, labels, params, lr=lr, max_norm=max_norm, optimizer=optimizer, betas=betas,
                 eps=eps, weight_decay=wd)                     # step(nodes, field=) is the same three updates
    for nodes in batches:
        b.step(nodes, field=b.field(nodes))
    assert torch.equal(b.p.params, tr.p.params)


# ------------------------------------------------------------ 8. determinism
@pytest.mark.parametrize("case_id", ["l2", "max_l3", "bf16_f100"])
def test_field_step_is_bitwise_repeatable(gs, case_id):
    case, fcase = tc.STEP_BY_ID[case_id], ffc.FIELD_BY_ID["rmat5"]
    nodes = fcase["nodes"]
    graph, n, rp, col, X, Xd, labels, params = _setup(case, "rmat")
    tr = _trainer(case, graph, Xd, labels, params, cache_agg1=False)
    field = tr.field(nodes)
    runs = []
    for _run in range(2):
        loss = tr.forward_backward(nodes, field=field).clone()
        runs.append((loss, tr.p.grads.clone(), tr.hidden().clone()))
    assert all(torch.equal(a, b) for a, b in zip(*runs)) and float(runs[0][1].abs().max()) > 0
    perm = tr.field(nodes[::-1].copy())                        # a permutation of the nodes: the same field
    assert _same(_snapshot(perm), _snapshot(field))
    loss = tr.forward_backward(nodes[::-1].copy(), field=field)   # ... and a field covers its nodes in any order
    (loss64, _g, _h), (loss32, _g32, _h32) = _refs(case, "rmat", nodes)
    check_rule(f"permuted nodes loss {case_id}", [float(loss)], np.array([loss64]), np.array([loss32]))


@pytest.mark.parametrize("case_id", ["l2", "max"])
def test_field_stages_one_by_one_are_the_whole_step(gs, case_id):
    """forward, head and backward issued as three calls leave bitwise what GS_TF_ALL leaves."""
    case, nodes = tc.STEP_BY_ID[case_id], ffc.FIELD_BY_ID["hub_four"]["nodes"]
    graph, n, rp, col, X, Xd, labels, params = _setup(case, "hub_max")
    tr = _trainer(case, graph, Xd, labels, params, cache_agg1=False)
    field = tr.field(nodes)
    loss = tr.forward_backward(nodes, field=field).clone()
    grads = tr.p.grads.clone()
    tr.p.grads.zero_()
    for stage in (_lib.GS_TF_FORWARD, _lib.GS_TF_HEAD, _lib.GS_TF_BACKWARD):
        tr.forward_backward(nodes, stages=stage, field=field)
    assert torch.equal(tr.loss, loss) and torch.equal(tr.p.grads, grads) and float(grads.abs().max()) > 0


def test_embed_through_a_field(gs):
    """embed(nodes, field=): the forward stage alone, the rows `nodes` of H_L in the order given."""
    for case_id in ("l2", "max", "bf16_max"):
        case, fcase = tc.STEP_BY_ID[case_id], ffc.FIELD_BY_ID["hub_four"]
        nodes = fcase["nodes"]
        graph, n, rp, col, X, Xd, labels, params = _setup(case, "hub_max")
        tr = _trainer(case, graph, Xd, labels, params)
        grads = tr.p.grads.clone()
        got = tr.embed(nodes, field=tr.field(nodes))
        (_l, _g, h64), (_l32, _g32, h32) = _refs(case, "hub_max", nodes)
        assert got.shape == (len(nodes), case["H"]) and torch.equal(tr.p.grads, grads)
        check_rule(f"embed field {case_id}", _np(got), h64[-1][nodes].reshape(-1), h32[-1][nodes].reshape(-1))
        assert torch.equal(got, tr.embed(nodes))               # the full path's rows, bit for bit


# ------------------------------------------------------------------ 9. refusals
def test_field_refusals_come_before_any_launch(gs):
    case = tc.STEP_BY_ID["l2"]
    graph, n, rp, col, X, Xd, labels, params = _setup(case, "hub_max")
    nodes = ffc.FIELD_BY_ID["hub_four"]["nodes"]
    tr = _trainer(case, graph, Xd, labels, params)
    field = tr.field(nodes)
    tr.forward_backward(nodes, field=field)
    torch.cuda.synchronize()
    p, g, loss, ws, snap = tr.p.params.clone(), tr.p.grads.clone(), tr.loss.clone(), tr._ws.clone(), _snapshot(field)
    other_nodes = tr.field(np.array([2, 4, 125, 8]))
    l3 = tc.STEP_BY_ID["l3_h80"]
    other_depth = _trainer(l3, graph, _features(n, l3["F"], False)[1], tc.labels_of(n, l3["C"]),
                           tc.params_of(l3)).field(nodes)
    other_seg = _trainer(case, graph, Xd, labels, params, seg_len=None).field(nodes)
    other_gcn = _trainer(tc.STEP_BY_ID["gcn"], graph, _features(n, 128, False)[1], tc.labels_of(n, 7),
                         tc.params_of(tc.STEP_BY_ID["gcn"])).field(nodes)
    g2, n2, rp2, col2 = ffc.graph_of("rmat")
    other_graph = _trainer(case, g2, _features(n2, case["F"], False)[1], tc.labels_of(n2, case["C"]),
                           params).field(nodes)
    for bad, match in ((other_nodes, "other nodes"), (other_depth, "3 layers"), (other_seg, "another plan"),
                       (other_gcn, "another plan"), (other_graph, "another plan")):
        for call in (tr.forward_backward, tr.step, tr.embed):
            with pytest.raises(ValueError, match=match):
                call(nodes, field=bad)
    with pytest.raises(ValueError, match="other nodes"):
        tr.forward_backward(np.array([2, 4, 125]), field=field)        # a subset of the field's nodes
    with pytest.raises(TypeError, match="ReceptiveField"):
        tr.forward_backward(nodes, field=ops.full_field_host(rp, col, nodes, 2))
    for bad_nodes, exc in ((np.array([2, 4, 125, 7, 4]), ValueError), (np.array([2, n]), IndexError),
                           (_i32([2, 4, 4]), ValueError), (_i32([-1, 4]), IndexError)):
        with pytest.raises(exc):
            tr.field(bad_nodes)
        with pytest.raises(exc):
            tr.field(bad_nodes, out=field)
        with pytest.raises(exc):
            ops.full_field(tr.plan, tr.tplan, bad_nodes, 2, device=DEV)
        with pytest.raises(exc):
            tr.forward_backward(bad_nodes, field=field)
    with pytest.raises(ValueError, match="another plan or depth"):
        tr.field(nodes, out=other_depth)
    with pytest.raises(ValueError, match="layer"):
        ops.agg_full("MEAN", Xd, tr.plan, field=field, layer=3)
    with pytest.raises(ValueError, match="another plan"):
        ops.agg_full("MEAN", Xd, other_seg.plan, field=field, layer=1)
    torch.cuda.synchronize()
    assert torch.equal(tr.p.params, p) and torch.equal(tr.p.grads, g) and torch.equal(tr.loss, loss)
    assert torch.equal(tr._ws, ws) and _same(_snapshot(field), snap)
