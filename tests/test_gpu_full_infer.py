"""Exact full-neighbourhood inference on the device (hip_ops.agg_full,
train.FullEmbedder, get_gnn_embeddings(full_neighbourhood=True)) against the
float64 reference of tests/full_ref.py, on the graphs of tests/full_cases.py.

Tolerance (adam_cases.check_rule): err <= 4 * e_torch + 2^-23 * max|ref|, with
e_torch the error of the reference's own fp32 run on the CPU against its
float64 run, never measured from the kernel.  MAX of representable values is
exact: the operator must equal the reference bitwise.  Rows whose
neighbourhood is empty are NaN under MEAN (0/0) in exactly the reference's
places, and are left out of the rule.
"""
import importlib
import random
import types

import numpy as np
import pytest
import torch

from tests import full_cases as fc
from tests import full_ref
from tests.adam_cases import check_rule

pytestmark = pytest.mark.gpu

ops = importlib.import_module("graphsage-pytorch_amd.hip_ops")
models = importlib.import_module("graphsage-pytorch_amd.models")
train = importlib.import_module("graphsage-pytorch_amd.train")
utils = importlib.import_module("graphsage-pytorch_amd.utils")
sampler = importlib.import_module("graphsage-pytorch_amd.sampler")
DEV = torch.device("cuda", 0)
_X = {}


def _features(n, F, bf16):
    """(numpy fp32 values, device tensor in the table's dtype); built once."""
    key = (n, F, bf16)
    if key not in _X:
        X = fc.features(n, F, bf16)
        Xd = torch.from_numpy(X).to(DEV)
        if bf16:
            Xd = Xd.to(torch.bfloat16)
            assert torch.equal(Xd.float().cpu(), torch.from_numpy(X))
        _X[key] = (X, Xd)
    return _X[key]


def _rule_rows(what, got, ref, tor, factor=4.0):
    """NaN rows exactly the reference's; check_rule on the others."""
    got = np.asarray(got, np.float64)
    nan = np.isnan(ref).any(1)
    assert np.array_equal(np.isnan(got).any(1), nan), f"{what}: NaN rows differ from the reference's"
    assert np.array_equal(np.isnan(got).all(1), nan)
    assert np.array_equal(np.isnan(tor).any(1), nan)
    return check_rule(what, got[~nan], ref[~nan].reshape(-1), tor[~nan].reshape(-1), factor=factor)


# ---------------------------------------------------------------- 1. operator
@pytest.mark.parametrize("gcn", [False, True], ids=["sage", "gcn"])
@pytest.mark.parametrize("agg", ["MEAN", "MAX"])
@pytest.mark.parametrize("dt,F", fc.OP_SHAPES, ids=[f"{d}-{f}" for d, f in fc.OP_SHAPES])
@pytest.mark.parametrize("name", ["hub", "rmat"])
def test_agg_full_matches_float64_reference(gs, name, dt, F, agg, gcn):
    """agg_full at seg_len 8 and the default, over the whole graph and over a
    window that starts and ends off every block multiple."""
    bf16 = dt == "bf16"
    gname = fc.graph_for(name, agg, gcn)
    graph, n, row_ptr, col = fc.graph_of(gname)
    X, Xd = _features(n, F, bf16)
    ref = full_ref.aggregate_reference(row_ptr, col, X, agg, gcn, bf16=bf16)
    tor = full_ref.aggregate_reference(row_ptr, col, X, agg, gcn, bf16=bf16, dtype=torch.float32)
    if name == "hub" and not gcn and agg == "MEAN":
        assert int(np.isnan(ref).any(1).sum()) == 4
    for seg_len in fc.OP_SEG_LENS:
        plan = ops.agg_full_plan(graph, gcn=gcn, seg_len=seg_len)
        if seg_len == fc.SEG_LEN:
            assert plan.n_split >= 4  # the split path runs
        for row0, tail in fc.OP_WINDOWS:
            n_rows = n - row0 - tail
            out = torch.full((n_rows, F), float("nan"), dtype=Xd.dtype, device=DEV)
            ops.agg_full(agg, Xd, graph, out, gcn=gcn, seg_len=seg_len, row0=row0, n_rows=n_rows)
            torch.cuda.synchronize()
            got = out.float().cpu().numpy().astype(np.float64)
            what = f"agg_full {gname} {dt} F={F} {agg} gcn={gcn} seg_len={seg_len} rows {row0}..{row0 + n_rows}"
            r, t = ref[row0:row0 + n_rows], tor[row0:row0 + n_rows]
            if agg == "MAX":
                assert np.array_equal(got, r), what  # a max of representable values is exact
            else:
                _rule_rows(what, got, r, t, fc.factor("op", f"{gname}-{dt}-{F}-{gcn}"))


def test_agg_full_max_refuses_an_empty_row_in_the_window(gs):
    graph, n, _row_ptr, _col = fc.graph_of("hub")
    _X_, Xd = _features(n, 32, False)
    out = ops.agg_full("MAX", Xd, graph, seg_len=fc.SEG_LEN, row0=0, n_rows=fc.HUB_SELF_ONLY)
    assert bool(torch.isfinite(out).all())
    with pytest.raises(IndexError, match="empty neighbourhood"):
        ops.agg_full("MAX", Xd, graph, seg_len=fc.SEG_LEN, row0=0, n_rows=fc.HUB_SELF_ONLY + 1)
    with pytest.raises(ValueError):
        ops.agg_full("MEAN", Xd, graph, row0=n - 2, n_rows=3)


# ---------------------------------------------------------------- 2. pipeline
def _embedder(case, gname, L=None, **kw):
    graph, n, _rp, _col = fc.graph_of(gname)
    _Xn, Xd = _features(n, case["F"], case["bf16"])
    W = fc.weights(case["L"], case["F"], case["H"], case["gcn"])[:L or case["L"]]
    args = {"seg_len": case["seg_len"], "chunk_rows": case["chunk_rows"]}
    args.update(kw)
    return train.FullEmbedder(graph, Xd, [torch.from_numpy(w) for w in W], agg_func=case["agg"], gcn=case["gcn"],
                              **args)


@pytest.mark.parametrize("case_id", fc.PIPE_IDS)
@pytest.mark.parametrize("name", ["hub", "rmat"])
def test_full_embedder_matches_float64_reference(gs, name, case_id):
    """Every layer's output H_l (the embedder of the first l layers) under the
    rule; under MAX the hub graph is the one without its empty rows."""
    case = fc.PIPE_BY_ID[case_id]
    gname = fc.graph_for(name, case["agg"], case["gcn"])
    _graph, n, row_ptr, col = fc.graph_of(gname)
    X, _Xd = _features(n, case["F"], case["bf16"])
    W = fc.weights(case["L"], case["F"], case["H"], case["gcn"])
    args = (row_ptr, col, X, W, case["agg"], case["gcn"])
    ref = full_ref.full_reference(*args, bf16=case["bf16"])
    tor = full_ref.full_reference(*args, bf16=case["bf16"], dtype=torch.float32)
    for l in range(1, case["L"] + 1):
        got = _embedder(case, gname, L=l).embed()
        torch.cuda.synchronize()
        assert got.shape == (n, case["H"]) and got.dtype == torch.float32
        _rule_rows(f"full {gname} {case_id} H_{l}", got.cpu().numpy(), ref[l - 1], tor[l - 1],
                   fc.factor("pipe", case_id))
    rows = np.array([n - 1, 0, 7, 7, 33], np.int64)
    sel = _embedder(case, gname).embed(rows)
    want = got.cpu()[torch.from_numpy(rows)]  # embed(nodes): those rows of the same embeddings, NaN rows included
    assert sel.shape == want.shape and torch.equal(torch.nan_to_num(sel.cpu(), nan=-1.0),
                                                   torch.nan_to_num(want, nan=-1.0))


# ------------------------------------------------- 3. against the sampled path
@pytest.mark.parametrize("gcn", [False, True], ids=["sage", "gcn"])
@pytest.mark.parametrize("agg", ["MEAN", "MAX"])
def test_full_embedder_agrees_with_the_sampled_forward(gs, agg, gcn):
    """On the bounded graph (no row longer than 14 entries) fanouts (15, 15)
    sample every neighbourhood whole, so NativeTrainer.forward on a host
    sample of all nodes computes the same function: both under the rule
    against the one float64 reference."""
    graph, n, row_ptr, col = fc.graph_of("bounded")
    F, H, L = 64, 64, 2
    X, Xd = _features(n, F, False)
    W = fc.weights(L, F, H, gcn)
    ref = full_ref.full_reference(row_ptr, col, X, W, agg, gcn)[-1]
    tor = full_ref.full_reference(row_ptr, col, X, W, agg, gcn, dtype=torch.float32)[-1]
    Wt = [torch.from_numpy(w) for w in W]
    full = train.FullEmbedder(graph, Xd, Wt, agg_func=agg, gcn=gcn, seg_len=fc.SEG_LEN, chunk_rows=64).embed()
    tr = train.NativeTrainer(graph, Xd, torch.zeros(1, dtype=torch.int32), 1, num_layers=L, hidden=H,
                             fanouts=(15, 15), agg_func=agg, gcn=gcn,
                             weights=(Wt, torch.zeros(1, H), torch.zeros(1)))
    s = sampler.sample(graph, sampler.RNG(3), np.arange(n, dtype=np.int64), [15, 15], gcn=gcn)
    assert [s.n_empty(j) for j in (1, 2)] == [0, 0]
    out = torch.full((n, H), float("nan"), dtype=torch.float32, device=DEV)
    tr.forward(models.DeviceSample(s, DEV), out)
    torch.cuda.synchronize()
    tag = f"bounded {agg} gcn={gcn}"
    _rule_rows(f"{tag} full", full.cpu().numpy(), ref, tor)
    _rule_rows(f"{tag} sampled", out.cpu().numpy(), ref, tor)


# ------------------------------------------------------------- 4. invariance
@pytest.mark.parametrize("case_id", ["l2", "max", "bf16_max", "h16_f50"])
def test_full_embedder_is_bitwise_invariant(gs, case_id):
    """chunk_rows 7, 64 and N give identical bits, as do two runs; seg_len
    above every degree equals a plan that never splits."""
    case = fc.PIPE_BY_ID[case_id]
    gname = fc.graph_for("hub", case["agg"], case["gcn"])
    n = fc.graph_of(gname)[1]
    base_emb = _embedder(case, gname, chunk_rows=n)
    base = base_emb.embed().clone()
    again = base_emb.embed()
    torch.cuda.synchronize()
    keep = ~torch.isnan(base).any(1)
    assert int((~keep).sum()) == (4 if case["agg"] == "MEAN" and not case["gcn"] else 0)
    assert float(base[keep].abs().max()) > 0
    assert torch.equal(base[keep], again[keep]) and torch.equal(torch.isnan(base), torch.isnan(again))
    for chunk in (7, 64):
        e = _embedder(case, gname, chunk_rows=chunk).embed()
        assert torch.equal(base[keep], e[keep]) and torch.equal(torch.isnan(base), torch.isnan(e)), chunk
    big = _embedder(case, gname, seg_len=1000, chunk_rows=64)
    none = _embedder(case, gname, seg_len=0, chunk_rows=64)
    assert big.plan.n_split == 0 and none.plan.n_split == 0 and base_emb.plan.n_split > 0
    a, b = big.embed(), none.embed()
    assert torch.equal(a[keep], b[keep]) and torch.equal(torch.isnan(a), torch.isnan(b))


# ------------------------------------------------------ 5. get_gnn_embeddings
def test_get_gnn_embeddings_full_neighbourhood(gs):
    graph, n, _rp, _col = fc.graph_of("rmat")
    F, H = 64, 32
    _Xn, Xd = _features(n, F, False)
    torch.manual_seed(824)
    model = models.GraphSage(2, F, H, Xd, graph, DEV, agg_func="MEAN", fanouts=[25, 10])
    model.to(DEV)
    dc = types.SimpleNamespace(g_labels=np.zeros(n, np.int64))
    random.seed(9)
    before = utils.get_gnn_embeddings(model, dc, "g").clone()
    random.seed(11)
    state = random.getstate()
    E = utils.get_gnn_embeddings(model, dc, "g", b_sz=13, sampler_streams=3, full_neighbourhood=True)
    assert random.getstate() == state
    W = [model.sage_layer1.weight, model.sage_layer2.weight]
    want = train.FullEmbedder(graph, Xd, W, agg_func="MEAN").embed()
    assert E.shape == (n, H) and torch.equal(E, want)
    assert not torch.equal(E, before)  # exact neighbourhoods, not 25 / 10 sampled ones
    random.seed(9)
    after = utils.get_gnn_embeddings(model, dc, "g")
    assert torch.equal(after, before)  # the default path is unchanged
    part = types.SimpleNamespace(g_labels=np.zeros(100, np.int64))
    assert torch.equal(utils.get_gnn_embeddings(model, part, "g", full_neighbourhood=True), want[:100])
