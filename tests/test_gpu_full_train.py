"""Full-batch training over full neighbourhoods on the device
(hip_ops.agg_full(argmax=), hip_ops.agg_full_bwd, train.FullTrainer) against
the float64 reference of tests/full_train_ref.py, on the graphs of
tests/full_cases.py and the directed graph of tests/full_train_cases.py.

Tolerance (adam_cases.check_rule): err <= 4 * e_torch + 2^-23 * max|ref|, with
e_torch the error of the reference's own fp32 run on the CPU against its
float64 run, never measured from the kernel; gradients are checked per named
parameter.  What selects (MAX values, the argmax, a MAX backward of small
integers) must equal the reference exactly.
"""
import importlib

import numpy as np
import pytest
import torch

from tests import adam_cases as ac
from tests import full_cases as fc
from tests import full_train_cases as tc
from tests import full_train_ref as tref
from tests import step_ref
from tests.adam_cases import check_rule

pytestmark = pytest.mark.gpu

ops = importlib.import_module("graphsage-pytorch_amd.hip_ops")
models = importlib.import_module("graphsage-pytorch_amd.models")
train = importlib.import_module("graphsage-pytorch_amd.train")
sampler = importlib.import_module("graphsage-pytorch_amd.sampler")
DEV = torch.device("cuda", 0)
OP_WIDTHS = [128, 32, 16, 50]          # lane groups of 64, 32 and 16, and the scalar path
_MEMO = {}


def _plans(name, gcn, seg_len):
    """(forward plan, its transpose, n, row_ptr, col); the tuple graph through a FullPlan."""
    key = ("plan", name, gcn, seg_len)
    if key not in _MEMO:
        graph, n, rp, col = tc.csr_of(name)
        plan = ops.FullPlan(graph, gcn=gcn, seg_len=seg_len) if isinstance(graph, tuple) else \
            ops.agg_full_plan(graph, gcn=gcn, seg_len=seg_len)
        _MEMO[key] = (plan, plan.transposed(), n, rp, col)
    return _MEMO[key]


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype)


def _op_inputs(n, F, ties=False):
    """X, dA, dSelf, Hprev as fp32 numpy (fixed per shape); with `ties`
    small integers, so that many entries tie and every sum is exact."""
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


# ------------------------------------------------- 1. the backward operator
@pytest.mark.parametrize("F", OP_WIDTHS)
@pytest.mark.parametrize("gcn", [False, True], ids=["sage", "gcn"])
@pytest.mark.parametrize("agg", ["MEAN", "MAX"])
@pytest.mark.parametrize("name", ["hub_max", "rmat", "directed"])
def test_agg_full_bwd_matches_float64_reference(gs, name, agg, gcn, F):
    """agg_full_bwd at seg_len 8 and the default, bare and with the dSelf +
    Hprev epilogue; MAX reads the argmax agg_full recorded."""
    n = tc.csr_of(name)[1]
    X, dA, dSelf, Hprev = _op_inputs(n, F)
    Xd, dAd, dSd, Hpd = (_dev(a) for a in (X, dA, dSelf, Hprev))
    for epi in (False, True):
        kw = {"dSelf": dSelf, "Hprev": Hprev} if epi else {}
        _plan, _t, _n, rp, col = _plans(name, gcn, None)
        _a, am_ref, ref = tref.aggregate_backward(rp, col, X, dA, agg, gcn, **kw)
        _a, _am, tor = tref.aggregate_backward(rp, col, X, dA, agg, gcn, dtype=torch.float32, **kw)
        for seg_len in (tc.SEG_LEN, None):
            plan, tplan, _n, _rp, _col = _plans(name, gcn, seg_len)
            if seg_len == tc.SEG_LEN:
                assert tplan.n_split >= 4  # the split path runs
            am = None
            if agg == "MAX":
                am = torch.full((n, F), -7, dtype=torch.int32, device=DEV)
                ops.agg_full("MAX", Xd, plan, argmax=am)
                assert np.array_equal(am.cpu().numpy(), am_ref)  # distinct values: the one maximal entry
            dkw = {"dSelf": dSd, "Hprev": Hpd} if epi else {}
            outs = []
            for _run in range(2):
                dH = torch.full((n, F), float("nan"), dtype=torch.float32, device=DEV)
                ops.agg_full_bwd(agg, dAd, tplan, dH, argmax=am, **dkw)
                outs.append(dH)
            torch.cuda.synchronize()
            assert torch.equal(outs[0], outs[1])  # bitwise repeatable
            what = f"agg_full_bwd {name} {agg} gcn={gcn} F={F} seg_len={seg_len} epilogue={epi}"
            check_rule(what, outs[0].cpu().numpy(), ref.reshape(-1), tor.reshape(-1),
                       factor=tc.factor("op_bwd", f"{name}-{agg}-{gcn}-{F}"))
            if epi:
                assert bool((outs[0][Hpd <= 0] == 0).all())


@pytest.mark.parametrize("F", [128, 50])
def test_mean_backward_quotient_is_the_division(gs, F):
    """Every element of the MEAN backward is dA / count as IEEE division
    rounds it (numpy's float32 quotient), bit for bit: destinations v = 0 ..
    99 read v + 1 sources each and no source is read twice, so dH[u] is one
    quotient, for the counts 1 .. 100 and gradients over 40 binades."""
    K = 100
    n_src = K * (K + 1) // 2
    n = K + n_src
    deg = np.concatenate([np.arange(1, K + 1), np.zeros(n_src, np.int64)])
    row_ptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    col = (K + np.arange(n_src)).astype(np.int32)          # destination v owns the next v + 1 sources
    rs = np.random.RandomState(41 + F)
    dA = (rs.uniform(-1, 1, (n, F)) * 2.0 ** rs.randint(-20, 21, (n, F))).astype(np.float32)
    plan = ops.FullPlan((row_ptr, col), seg_len=tc.SEG_LEN)
    dH = ops.agg_full_bwd("MEAN", _dev(dA), plan)
    torch.cuda.synchronize()
    want = np.zeros((n, F), np.float32)
    owner = np.repeat(np.arange(K), np.arange(1, K + 1))   # the one destination that reads source K + i
    want[K:] = dA[owner] / (owner + 1).astype(np.float32)[:, None]
    got = dH.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), int((got != want).sum())


@pytest.mark.parametrize("F", OP_WIDTHS)
@pytest.mark.parametrize("gcn", [False, True], ids=["sage", "gcn"])
@pytest.mark.parametrize("name", ["hub_max", "rmat", "directed"])
def test_max_on_ties_is_the_reference_choice_exactly(gs, name, gcn, F):
    """Integer-valued inputs with many ties: values, argmax (the reference's
    first-index choice in visiting order) and the backward are all exact."""
    n = tc.csr_of(name)[1]
    X, dA, dSelf, Hprev = _op_inputs(n, F, ties=True)
    Xd, dAd, dSd, Hpd = (_dev(a) for a in (X, dA, dSelf, Hprev))
    _plan, _t, _n, rp, col = _plans(name, gcn, None)
    a_ref, am_ref, dh_ref = tref.aggregate_backward(rp, col, X, dA, "MAX", gcn, dSelf=dSelf, Hprev=Hprev)
    for seg_len in (tc.SEG_LEN, None):
        plan, tplan, _n, _rp, _col = _plans(name, gcn, seg_len)
        am = torch.full((n, F), -7, dtype=torch.int32, device=DEV)
        out = ops.agg_full("MAX", Xd, plan, argmax=am)
        dH = ops.agg_full_bwd("MAX", dAd, tplan, argmax=am, dSelf=dSd, Hprev=Hpd)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().astype(np.float64), a_ref), seg_len
        assert np.array_equal(am.cpu().numpy(), am_ref), seg_len
        assert np.array_equal(dH.cpu().numpy().astype(np.float64), dh_ref), seg_len


# ----------------------------------------------------- 2. the argmax forward
@pytest.mark.parametrize("F", OP_WIDTHS)
@pytest.mark.parametrize("gcn", [False, True], ids=["sage", "gcn"])
@pytest.mark.parametrize("name", ["hub_max", "rmat", "directed"])
def test_argmax_forward(gs, name, gcn, F):
    n = tc.csr_of(name)[1]
    X = _op_inputs(n, F)[0]
    Xd = _dev(X)
    for seg_len in (tc.SEG_LEN, None):
        plan, _t, _n, rp, col = _plans(name, gcn, seg_len)
        plain = ops.agg_full("MAX", Xd, plan)
        am = torch.full((n, F), -7, dtype=torch.int32, device=DEV)
        out = ops.agg_full("MAX", Xd, plan, argmax=am)
        torch.cuda.synchronize()
        assert torch.equal(out, plain)                                    # bitwise agg_full's without argmax
        amc = am.cpu().numpy().astype(np.int64)
        assert np.array_equal(X[amc, np.arange(F)[None, :]], out.cpu().numpy())   # X[argmax[v, f], f] == out[v, f]
        seg, ids = tref.visit_lists(rp, col, gcn)
        member = np.zeros((n, n), bool)
        member[seg, ids] = True
        assert member[np.arange(n)[:, None], amc].all()                   # a member of the effective neighbourhood


def test_argmax_first_wins_across_a_segment_boundary(gs):
    """All-equal rows: every element ties, so argmax is the first id the
    kernel visits -- for the hub rows of four segments under gcn, the own id
    where it sorts first (first segment), and the row's first neighbour where
    the own id sorts last (last segment); never a later segment's entry."""
    graph, n, rp, col = fc.graph_of("hub_max")
    Xd = torch.ones(n, 32, dtype=torch.float32, device=DEV)
    for gcn in (False, True):
        seg, ids = tref.visit_lists(rp, col, gcn)
        first = np.array([ids[seg == v][0] for v in range(n)])
        for seg_len in (tc.SEG_LEN, None):
            am = torch.full((n, 32), -7, dtype=torch.int32, device=DEV)
            ops.agg_full("MAX", Xd, graph, gcn=gcn, seg_len=seg_len, argmax=am)
            assert np.array_equal(am.cpu().numpy(), np.repeat(first[:, None], 32, 1)), (gcn, seg_len)
    sf, sl = fc.HUB_SPECIAL["self_first"], fc.HUB_SPECIAL["self_last"]
    assert col[rp[sf]] == sf and col[rp[sl + 1] - 1] == sl and rp[sf + 1] - rp[sf] == 3 * tc.SEG_LEN + 5
    assert first[sf] == sf and first[sl] == col[rp[sl]] != sl   # (gcn, the loop's last pass)


# ------------------------------------------------- 3. the step against float64
def _features(n, F, bf16):
    key = ("X", n, F, bf16)
    if key not in _MEMO:
        X = fc.features(n, F, bf16)
        Xd = torch.from_numpy(X).to(DEV)
        if bf16:
            Xd = Xd.to(torch.bfloat16)
        _MEMO[key] = (X, Xd)
    return _MEMO[key]


def _setup(case, gname):
    graph, n, rp, col = fc.graph_of(gname)
    X, Xd = _features(n, case["F"], case["bf16"])
    return graph, n, rp, col, X, Xd, tc.labels_of(n, case["C"]), tc.nodes_of(n), tc.params_of(case)


def _trainer(case, graph, Xd, labels, params, **kw):
    L = case["L"]
    w = ([torch.from_numpy(p) for p in params[:L]], torch.from_numpy(params[L]), torch.from_numpy(params[L + 1]))
    args = {"seg_len": case["seg_len"]}
    args.update(kw)
    return train.FullTrainer(graph, Xd, torch.from_numpy(labels), case["C"], num_layers=L, hidden=case["H"],
                             agg_func=case["agg"], gcn=case["gcn"], weights=w, **args)


def _ref_step(case, rp, col, X, labels, nodes, params, dtype=torch.float64):
    return tref.step_reference(rp, col, X, labels, nodes, params, case["agg"], case["gcn"], bf16=case["bf16"],
                               dtype=dtype)


def _flat(xs):
    return np.concatenate([np.asarray(x, np.float64).reshape(-1) for x in xs])


@pytest.mark.parametrize("case_id", tc.STEP_IDS)
@pytest.mark.parametrize("name", ["hub_max", "rmat"])
def test_full_step_matches_float64_reference(gs, name, case_id):
    """Loss, H_L and every gradient tensor of one forward_backward on a
    37-node subset, each under the rule on its own."""
    case = tc.STEP_BY_ID[case_id]
    graph, n, rp, col, X, Xd, labels, nodes, params = _setup(case, name)
    loss64, g64, h64 = _ref_step(case, rp, col, X, labels, nodes, params)
    loss32, g32, h32 = _ref_step(case, rp, col, X, labels, nodes, params, dtype=torch.float32)
    tr = _trainer(case, graph, Xd, labels, params)
    before = tr.p.params.clone()
    loss = tr.forward_backward(torch.from_numpy(nodes.astype(np.int32)).to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(tr.p.params, before)                # no update before apply_update
    fac = tc.factor("step", case_id)
    tag = f"full step {name} {case_id}"
    check_rule(f"{tag} loss", [float(loss)], np.array([loss64]), np.array([loss32]), factor=fac)
    check_rule(f"{tag} H_L", tr.hidden().cpu().numpy(), h64[-1].reshape(-1), h32[-1].reshape(-1), factor=fac)
    for i, pname in enumerate(tc.names_of(case["L"])):
        got = tr.p.view(i, grad=True).cpu().numpy()
        assert got.shape == g64[i].shape and np.abs(g64[i]).max() > 0
        check_rule(f"{tag} d{pname}", got, g64[i].reshape(-1), g32[i].reshape(-1), factor=fac)
    assert tr.ws_bytes > 0 and tr.hidden(1).shape == (n, case["H"])


@pytest.mark.parametrize("optimizer", ["sgd", "adam"])
@pytest.mark.parametrize("case_id", tc.STEP_IDS)
def test_full_trainer_three_updates(gs, case_id, optimizer):
    """Three steps with the clip active, teacher-forced as
    test_gpu_step_matrix.py does it: at the parameters the device holds, every
    raw gradient tensor against the float64 step under the rule, then every
    parameter tensor after apply_update against the float64 update
    (step_ref.clip_sgd / adam_cases.reference_adamw) of that raw gradient.
    (The update is checked on the device's own gradient because Adam's first
    steps divide by |g|: an element with |g| near eps turns a gradient error
    inside the rule into a parameter error of any size.  Measured with the
    float64 gradient fed to the reference instead: l2, Adam, step 1,
    layer.0.weight err / e_torch 4.79.)"""
    case = tc.STEP_BY_ID[case_id]
    graph, n, rp, col, X, Xd, labels, nodes, params = _setup(case, "hub_max")
    L = case["L"]
    _l, g0, _h = _ref_step(case, rp, col, X, labels, nodes, params)
    sizes = [p.size for p in params]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    goff = np.array([0, offs[L], offs[-1]], np.int64)
    norms = [np.sqrt((_flat(g0)[goff[k]:goff[k + 1]] ** 2).sum()) for k in range(2)]
    max_norm = ac.f32(0.25 * min(norms))                   # both groups clip at step 1
    lr, betas, eps, wd = ac.f32(0.05), (ac.f32(0.9), ac.f32(0.999)), ac.f32(1e-8), ac.f32(0.01)
    tr = _trainer(case, graph, Xd, labels, params, lr=lr, max_norm=max_norm, optimizer=optimizer, betas=betas,
                  eps=eps, weight_decay=wd)
    assert np.array_equal(tr.p.group_off, goff)
    nodes_d = torch.from_numpy(nodes.astype(np.int32)).to(DEV)
    fac = tc.factor("update", case_id)
    for t in range(1, 4):
        p0 = tr.p.params.cpu().numpy()
        cur = [p0[offs[i]:offs[i + 1]].reshape(params[i].shape) for i in range(L + 2)]
        g64 = _ref_step(case, rp, col, X, labels, nodes, cur)[1]
        g32 = _ref_step(case, rp, col, X, labels, nodes, cur, dtype=torch.float32)[1]
        if t == 1:  # the clip is active: the reference's own norms exceed max_norm
            assert all(np.sqrt((_flat(g64)[goff[k]:goff[k + 1]] ** 2).sum()) > max_norm for k in range(2))
        st = tr.optimizer_state()
        assert st["step"] == t - 1
        tr.forward_backward(nodes_d)
        graw = tr.p.grads.cpu().numpy()                    # unclipped until apply_update
        for i, pname in enumerate(tc.names_of(L)):
            check_rule(f"full {optimizer} {case_id} step {t} d{pname}", graw[offs[i]:offs[i + 1]],
                       g64[i].reshape(-1), g32[i].reshape(-1), factor=fac)
        if optimizer == "sgd":
            want = step_ref.clip_sgd(p0, graw, goff, lr, max_norm)[0]
            tor = step_ref.clip_sgd_torch_fp32(p0, graw, goff, lr, max_norm)[0]
        else:
            m0, v0 = st["m"].cpu().numpy(), st["v"].cpu().numpy()
            want = ac.reference_adamw(p0, graw, m0, v0, t, lr, betas, eps, wd, goff, 1.0, max_norm)[0]
            tor = ac.torch_adamw(p0, graw, m0, v0, t, lr, betas, eps, wd, goff, 1.0, max_norm, torch.float32)[0]
        tr.apply_update()
        torch.cuda.synchronize()
        got = tr.p.params.cpu().numpy()
        assert not np.array_equal(got, p0)
        for i, pname in enumerate(tc.names_of(L)):
            lo, hi = offs[i], offs[i + 1]
            check_rule(f"full {optimizer} {case_id} step {t} {pname}", got[lo:hi], want[lo:hi], tor[lo:hi], factor=fac)
    assert tr.optimizer_state()["step"] == 3


# ------------------------------------------------------ 4. ties to what exists
@pytest.mark.parametrize("case_id", ["l2", "l3_h80", "gcn", "max", "bf16_max"])
def test_embed_is_bitwise_full_embedder(gs, case_id):
    case = tc.STEP_BY_ID[case_id]
    graph, n, rp, col, X, Xd, labels, nodes, params = _setup(case, "hub_max")
    tr = _trainer(case, graph, Xd, labels, params)
    tr.step(nodes)
    W = [w.clone() for w in tr.weights()]
    want = train.FullEmbedder(graph, Xd, W, agg_func=case["agg"], gcn=case["gcn"], seg_len=case["seg_len"]).embed()
    assert torch.equal(tr.embed(), want) and float(want.abs().max()) > 0
    assert torch.equal(tr.embed([3, 0, 3]), want[[3, 0, 3]])
    tr.forward_backward(nodes)                             # the step's own H_L, at the same weights
    torch.cuda.synchronize()
    assert torch.equal(tr.hidden(), want)


@pytest.mark.parametrize("gcn", [False, True], ids=["sage", "gcn"])
@pytest.mark.parametrize("agg", ["MEAN", "MAX"])
def test_full_step_agrees_with_the_sampled_step(gs, agg, gcn):
    """On `bounded` fanouts of 15 take every neighbourhood whole, so
    NativeTrainer.forward_backward on the same nodes computes the same loss
    and gradients: both under the rule against the one float64 reference."""
    case = {"L": 2, "F": 64, "H": 64, "C": 5, "agg": agg, "gcn": gcn, "bf16": False, "seg_len": tc.SEG_LEN}
    graph, n, rp, col, X, Xd, labels, nodes, params = _setup(case, "bounded")
    loss64, g64, _h = _ref_step(case, rp, col, X, labels, nodes, params)
    loss32, g32, _h = _ref_step(case, rp, col, X, labels, nodes, params, dtype=torch.float32)
    tr = _trainer(case, graph, Xd, labels, params)
    w = ([torch.from_numpy(p) for p in params[:2]], torch.from_numpy(params[2]), torch.from_numpy(params[3]))
    nt = train.NativeTrainer(graph, Xd, torch.from_numpy(labels), 5, num_layers=2, hidden=64, fanouts=(15, 15),
                             agg_func=agg, gcn=gcn, weights=w)
    s = sampler.sample(graph, sampler.RNG(3), nodes, [15, 15], gcn=gcn)
    assert [s.n_empty(j) for j in (1, 2)] == [0, 0]
    nodes_d = torch.from_numpy(nodes.astype(np.int32)).to(DEV)
    l_full = float(tr.forward_backward(nodes_d))
    l_samp = float(nt.forward_backward(models.DeviceSample(s, DEV), nodes_d))
    torch.cuda.synchronize()
    for tag, l, p in (("full", l_full, tr.p), ("sampled", l_samp, nt.p)):
        check_rule(f"bounded {agg} gcn={gcn} {tag} loss", [l], np.array([loss64]), np.array([loss32]))
        for i, pname in enumerate(tc.names_of(2)):
            check_rule(f"bounded {agg} gcn={gcn} {tag} d{pname}", p.view(i, grad=True).cpu().numpy(),
                       g64[i].reshape(-1), g32[i].reshape(-1))


@pytest.mark.parametrize("case_id", ["l2", "max", "bf16_max"])
def test_cache_agg1_changes_no_bit(gs, case_id):
    case = tc.STEP_BY_ID[case_id]
    graph, n, rp, col, X, Xd, labels, nodes, params = _setup(case, "rmat")
    a = _trainer(case, graph, Xd, labels, params, cache_agg1=True)
    b = _trainer(case, graph, Xd, labels, params, cache_agg1=False)
    for _step in range(2):
        la, lb = a.forward_backward(nodes).clone(), b.forward_backward(nodes).clone()
        assert torch.equal(a.p.grads, b.p.grads) and torch.equal(la, lb) and float(a.p.grads.abs().max()) > 0
        a.apply_update()
        b.apply_update()
    assert torch.equal(a.p.params, b.p.params) and a._agg1 == train._FULL_AGG1 and torch.equal(a.hidden(1, 1), b.hidden(1, 1))
    a.hidden(1, 1).zero_()                                 # a stale cache would now show
    a.invalidate_cache()
    a.forward_backward(nodes)
    b.forward_backward(nodes)
    assert torch.equal(a.p.grads, b.p.grads)


def test_state_dict_round_trip_through_native_trainer(gs):
    case = tc.STEP_BY_ID["l2"]
    graph, n, rp, col, X, Xd, labels, nodes, params = _setup(case, "hub_max")
    tr = _trainer(case, graph, Xd, labels, params, optimizer="adam", lr=0.01)
    tr.step(nodes)
    sd, st = tr.state_dict(), tr.optimizer_state()
    assert list(sd) == tc.names_of(2) and st["step"] == 1
    nt = train.NativeTrainer(graph, Xd, torch.from_numpy(labels), case["C"], num_layers=2, hidden=case["H"],
                             fanouts=(5, 5), optimizer="adam", seed=1)
    assert not torch.equal(nt.p.params, tr.p.params)
    nt.load_state_dict(sd)
    nt.load_optimizer_state(st)
    assert torch.equal(nt.p.params, tr.p.params) and nt.optimizer_state()["step"] == 1
    back = _trainer(case, graph, Xd, labels, tc.params_of(case, seed=5), optimizer="adam", lr=0.01)
    back.load_state_dict(nt.state_dict())
    back.load_optimizer_state(nt.optimizer_state())
    assert torch.equal(back.p.params, tr.p.params) and torch.equal(back.opt_m, tr.opt_m)
    la, lb = tr.step(nodes).clone(), back.step(nodes).clone()
    assert torch.equal(la, lb) and torch.equal(back.p.params, tr.p.params)    # training continues bit for bit


# ------------------------------------------------------------------ 5. refusals
def test_refusals_come_before_any_launch(gs):
    graph, n, _rp, _col = fc.graph_of("hub")
    Xd = _features(n, 32, False)[1]
    labels = torch.zeros(n, dtype=torch.int64)
    with pytest.raises(ValueError, match="4 nodes have an empty neighbourhood.*gcn"):
        train.FullTrainer(graph, Xd, labels, 3, hidden=16, seg_len=tc.SEG_LEN)
    with pytest.raises(IndexError, match="empty neighbourhood"):
        train.FullTrainer(graph, Xd, labels, 3, hidden=16, agg_func="MAX", seg_len=tc.SEG_LEN)
    train.FullTrainer(graph, Xd, labels, 3, hidden=16, gcn=True, seg_len=tc.SEG_LEN)   # gcn is the remedy

    case = tc.STEP_BY_ID["h16_f50"]
    graph, n, rp, col, X, Xd, labels, nodes, params = _setup(case, "hub_max")
    with pytest.raises(RuntimeError, match="HIP device"):
        _trainer(case, graph, Xd.cpu(), labels, params)
    bad = [p.copy() for p in params]
    bad[1] = bad[1][:, :-1]
    with pytest.raises(ValueError, match=r"weights\[1\]"):
        _trainer(case, graph, Xd, labels, bad)
    tr = _trainer(case, graph, Xd, labels, params)
    tr.forward_backward(nodes)
    torch.cuda.synchronize()
    grads, loss, ws = tr.p.grads.clone(), tr.loss.clone(), tr._ws.clone()
    dup = np.concatenate([nodes, nodes[:1]])
    for bad_nodes, exc in ((dup, ValueError), (torch.from_numpy(dup.astype(np.int32)).to(DEV), ValueError),
                           (torch.from_numpy(nodes.astype(np.int32)), RuntimeError),
                           (torch.from_numpy(nodes).to(DEV), TypeError),
                           (torch.from_numpy(nodes.astype(np.int32)).to(DEV).reshape(1, -1), TypeError),
                           (np.array([0, n]), IndexError), (nodes.astype(np.float32), TypeError)):
        with pytest.raises(exc):
            tr.forward_backward(bad_nodes)
    torch.cuda.synchronize()
    assert torch.equal(tr.p.grads, grads) and torch.equal(tr.loss, loss) and torch.equal(tr._ws, ws)

    Xb = _features(n, 32, True)[1]
    am = torch.full((n, 32), -7, dtype=torch.int32, device=DEV)
    out = torch.full((n, 32), 3.0, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(ValueError, match="float32"):
        ops.agg_full("MAX", Xb, graph, out, argmax=am)
    with pytest.raises(ValueError, match="MAX"):
        ops.agg_full("MEAN", Xb.float(), graph, argmax=am)
    torch.cuda.synchronize()
    assert bool((am == -7).all()) and bool((out == 3.0).all())
    with pytest.raises(ValueError, match="argmax"):
        ops.agg_full_bwd("MAX", Xb.float(), graph)
