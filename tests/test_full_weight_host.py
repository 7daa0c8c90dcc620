"""The host side of per-edge weights on the exact path, without a GPU: the
transposed plan's T_SRC array, hip_ops.EdgeWeights.host() (den and the
transposed weights), edge_weights_from_pairs, sym_norm_weights and the
refusals, on the graphs of tests/full_cases.py and the directed graph of
tests/full_train_cases.py.
"""
import importlib

import numpy as np
import pytest

from tests import full_cases as fc
from tests import full_train_cases as tc
from tests import full_weight_ref as wref

ops = importlib.import_module("graphsage-pytorch_amd.hip_ops")
_lib = importlib.import_module("graphsage-pytorch_amd._lib")

GRAPHS = ["directed", "hub", "hub_max", "rmat"]
SEG_LENS = [fc.SEG_LEN, None]


def _plan(name, gcn, seg_len):
    graph, n, rp, col = tc.csr_of(name)
    return ops.FullPlan(graph, gcn=gcn, seg_len=seg_len), n, np.asarray(rp, np.int64), np.asarray(col, np.int64)


def _weights(n_entries, seed=3, lo=0.25, hi=4.0):
    return np.random.RandomState(seed).uniform(lo, hi, n_entries).astype(np.float32)


# --------------------------------------------------------------------- T_SRC
@pytest.mark.parametrize("seg_len", SEG_LENS, ids=["seg8", "default"])
@pytest.mark.parametrize("gcn", [False, True], ids=["sage", "gcn"])
@pytest.mark.parametrize("name", GRAPHS)
def test_t_src_names_the_forward_entry_of_every_transposed_entry(gs, name, gcn, seg_len):
    plan, n, rp, col = _plan(name, gcn, seg_len)
    t = plan.transposed()
    t_rp, t_col, t_src = t.row_ptr, t.col, t.array(_lib.GS_FP_T_SRC)
    assert t_src.dtype == np.int64 and len(t_src) == len(t_col) == t_rp[-1]
    owner = np.repeat(np.arange(n), np.diff(rp))               # the forward row that owns each forward entry
    t_row = np.repeat(np.arange(n), np.diff(t_rp))             # the transposed row u of each transposed entry
    fwd = t_src >= 0
    s = t_src[fwd]
    assert (col[s] == t_row[fwd]).all()                        # col[s] == u
    assert (owner[s] == t_col[fwd]).all()                      # the forward row owning s is t_col[j]
    assert len(np.unique(s)) == len(s)                         # distinct
    is_self = col[:len(owner)] == owner
    want = np.nonzero(~is_self | gcn)[0]                       # every non-self entry once; under gcn the self entries too
    assert np.array_equal(np.sort(s), want)
    has_self = np.zeros(n, bool)
    has_self[owner[is_self]] = True
    added = ~fwd
    if gcn:                                                    # -1 exactly at the self entries gcn added
        assert (t_col[added] == t_row[added]).all()
        assert np.array_equal(np.sort(t_row[added]), np.nonzero(~has_self)[0])
    else:
        assert not added.any()
    # the array does not depend on the transposed plan's seg_len
    assert np.array_equal(plan.transposed(3).array(_lib.GS_FP_T_SRC), t_src)
    with pytest.raises(ValueError):
        plan.array(_lib.GS_FP_T_SRC)                           # a forward plan owns none


# -------------------------------------------------------------- EdgeWeights
@pytest.mark.parametrize("gcn", [False, True], ids=["sage", "gcn"])
@pytest.mark.parametrize("name", GRAPHS)
def test_edge_weights_host_arrays(gs, name, gcn):
    plan, n, rp, col = _plan(name, gcn, fc.SEG_LEN)
    w = _weights(plan.n_entries)
    sw = np.random.RandomState(5).uniform(0.5, 2.0, n).astype(np.float32)
    ew = ops.EdgeWeights(plan, w, norm="mean", self_weight=sw)
    w_h, den, w_t = ew.host()
    assert np.array_equal(w_h, w) and den.dtype == np.float32 and w_t.dtype == np.float32
    # den: a plain Python float64 loop over the effective entries, in entry order, rounded once
    want = np.zeros(n, np.float32)
    for v in range(n):
        s = 0.0
        for e in range(rp[v], rp[v + 1]):
            if gcn or col[e] != v:
                s += float(w[e])
        if gcn and not (col[rp[v]:rp[v + 1]] == v).any():
            s += float(sw[v])
        want[v] = np.float32(s)
    assert np.array_equal(den, want)
    seg, _ids, wts = wref.weighted_lists(rp, col, w, gcn, sw)  # and the reference's lists say the same
    np.testing.assert_allclose(den, wref.denominators(seg, wts, n), rtol=2.0 ** -23)
    # w_t is w carried through T_SRC, the added self entries taking self_weight
    t = plan.transposed()
    t_src = t.array(_lib.GS_FP_T_SRC)
    t_row = np.repeat(np.arange(n), np.diff(t.row_ptr))
    assert np.array_equal(w_t, np.where(t_src >= 0, w[np.maximum(t_src, 0)], sw[t_row]))
    # sum over the transposed entries of each destination == den (same multiset of weights)
    back = np.bincount(t.col, weights=w_t.astype(np.float64), minlength=n)
    np.testing.assert_allclose(back, den, rtol=1e-6)


@pytest.mark.parametrize("gcn", [False, True], ids=["sage", "gcn"])
@pytest.mark.parametrize("name", GRAPHS)
def test_unit_weights_give_the_plan_counts_exactly(gs, name, gcn):
    plan, n, _rp, _col = _plan(name, gcn, None)
    ew = ops.EdgeWeights(plan, np.ones(plan.n_entries, np.float32))
    w, den, w_t = ew.host()
    assert np.array_equal(den, plan.array(_lib.GS_FP_COUNT).astype(np.float32))
    assert (w_t == 1).all() and len(w_t) == plan.transposed().n_entries
    assert np.array_equal(ew.bad_rows(), plan.array(_lib.GS_FP_EMPTY_ROWS))


def test_self_entry_weights_are_ignored_without_gcn(gs):
    plan, n, rp, col = _plan("directed", False, fc.SEG_LEN)
    owner = np.repeat(np.arange(n), np.diff(rp))
    is_self = col == owner
    assert is_self.sum() == 2                                  # nodes 5 and 11
    w = _weights(plan.n_entries)
    w2 = w.copy()
    w2[is_self] = -1234.5
    a, b = ops.EdgeWeights(plan, w), ops.EdgeWeights(plan, w2)
    assert np.array_equal(a.host()[1], b.host()[1]) and np.array_equal(a.host()[2], b.host()[2])
    gplan = _plan("directed", True, fc.SEG_LEN)[0]             # under gcn they count
    assert not np.array_equal(ops.EdgeWeights(gplan, w).host()[1], ops.EdgeWeights(gplan, w2).host()[1])


# ---------------------------------------------------- edge_weights_from_pairs
def test_edge_weights_from_pairs_round_trip_on_a_csrgraph(gs):
    graph, n, rp, col = fc.graph_of("hub")
    rp, col = np.asarray(rp, np.int64), np.asarray(col, np.int64)
    owner = np.repeat(np.arange(n), np.diff(rp))
    w = _weights(len(owner))
    perm = np.random.RandomState(9).permutation(len(owner))    # the triples in any order
    got = ops.edge_weights_from_pairs(rp, col, owner[perm], col[perm], w[perm])
    assert got.dtype == np.float32 and np.array_equal(got, w)


def test_edge_weights_from_pairs_symmetric_missing_default_duplicate(gs):
    src, dst, n = fc.pairs_of("hub")
    graph, _n, rp, col = fc.graph_of("hub")
    key = np.minimum(src, dst) * n + np.maximum(src, dst)
    _u, first = np.unique(key, return_index=True)              # every undirected edge once
    s, d = src[first], dst[first]
    w = _weights(len(s), seed=4)
    got = ops.edge_weights_from_pairs(rp, col, d, s, w, symmetric=True)
    lut = {}
    for a, b, x in zip(s.tolist(), d.tolist(), w.tolist()):
        lut[(a, b)] = lut[(b, a)] = np.float32(x)
    owner = np.repeat(np.arange(n), np.diff(rp))
    assert np.array_equal(got, np.array([lut[(int(v), int(u))] for v, u in zip(owner, col)], np.float32))
    with pytest.raises(KeyError):                              # one direction only: the reverse entries are missing
        ops.edge_weights_from_pairs(rp, col, d, s, w)
    half = ops.edge_weights_from_pairs(rp, col, d, s, w, default=0.5)
    assert set(np.unique(half[half != got]).tolist()) == {0.5} and (half == got).any()
    with pytest.raises(ValueError):                            # a triple twice
        ops.edge_weights_from_pairs(rp, col, np.concatenate([d, d[:1]]), np.concatenate([s, s[:1]]),
                                    np.concatenate([w, w[:1]]), symmetric=True)
    off = np.nonzero(s != d)[0][0]
    with pytest.raises(ValueError):                            # both directions given, and mirrored on top
        ops.edge_weights_from_pairs(rp, col, np.concatenate([d, s[off:off + 1]]),
                                    np.concatenate([s, d[off:off + 1]]), np.concatenate([w, w[:1]]), symmetric=True)
    with pytest.raises(IndexError):
        ops.edge_weights_from_pairs(rp, col, [n], [0], [1.0])


# ----------------------------------------------------------- sym_norm_weights
@pytest.mark.parametrize("name", ["directed", "hub_max", "rmat"])
def test_sym_norm_weights_against_the_dense_normalised_adjacency(gs, name):
    plan, n, rp, col = _plan(name, True, fc.SEG_LEN)
    w, sw = ops.sym_norm_weights(plan)
    assert w.dtype == np.float32 and sw.dtype == np.float32
    A = np.zeros((n, n))
    owner = np.repeat(np.arange(n), np.diff(rp))
    A[owner, col] = 1.0
    A[np.arange(n), np.arange(n)] = 1.0                        # A + I, self exactly once
    d = A.sum(1)
    assert np.array_equal(d, plan.array(_lib.GS_FP_COUNT))
    want = A / np.sqrt(d[:, None] * d[None, :])                # D^-1/2 (A + I) D^-1/2
    seg, ids, wts = wref.weighted_lists(rp, col, w, True, sw)
    got = np.zeros((n, n))
    np.add.at(got, (seg, ids), wts)
    np.testing.assert_allclose(got, want, rtol=2.0 ** -23, atol=0)
    ew = ops.EdgeWeights(plan, w, norm="sum", self_weight=sw)  # finite: accepted
    assert np.isfinite(ew.host()[1]).all()


# ------------------------------------------------------------------ refusals
def test_refusals(gs):
    plan, n, rp, col = _plan("directed", False, fc.SEG_LEN)
    w = _weights(plan.n_entries)
    with pytest.raises(ValueError):
        ops.EdgeWeights(plan, w[:-1])                          # wrong length
    with pytest.raises(ValueError):
        ops.EdgeWeights(plan, np.concatenate([w, w[:1]]))
    bad = w.copy()
    bad[7] = np.nan
    with pytest.raises(ValueError):
        ops.EdgeWeights(plan, bad)                             # NaN weight
    bad[7] = np.inf
    with pytest.raises(ValueError):
        ops.EdgeWeights(plan, bad)
    with pytest.raises(ValueError):
        ops.EdgeWeights(plan, w, self_weight=np.ones(n - 1, np.float32))
    with pytest.raises(ValueError):
        ops.EdgeWeights(plan, w, self_weight=float("nan"))
    with pytest.raises(ValueError):
        ops.EdgeWeights(plan, w, norm="max")
    with pytest.raises(ValueError):
        ops.EdgeWeights(plan.transposed(), w)                  # a forward plan expected
    ew = ops.EdgeWeights(plan, w)
    with pytest.raises(ValueError):                            # MAX, refused before any device is touched
        ops._check_edge_weight("agg_full", ew, plan, "MAX")
    with pytest.raises(ValueError):                            # another plan
        ops._check_edge_weight("agg_full", ew, _plan("directed", False, None)[0], "MEAN")
    with pytest.raises(TypeError):
        ops._check_edge_weight("agg_full", w, plan, "MEAN")
    neg = ops.EdgeWeights(plan, -w)                            # negative weights are allowed ...
    assert len(neg.bad_rows()) == n and len(ew.bad_rows()) == 0    # ... and bad_rows names what "mean" cannot take
    train = importlib.import_module("graphsage-pytorch_amd.train")
    with pytest.raises(ValueError):
        train._edge_weights("FullTrainer", plan, "MAX", w, "mean", 1.0)
    with pytest.raises(ValueError):
        train._edge_weights("FullTrainer", plan, "MEAN", -w, "mean", 1.0)      # den <= 0 under mean
    assert train._edge_weights("FullTrainer", plan, "MEAN", -w, "sum", 1.0).norm == "sum"
    assert train._edge_weights("FullTrainer", plan, "MEAN", None, "mean", 1.0) is None
