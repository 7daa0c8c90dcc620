"""The counter-based extend_nodes, host mirror (DESIGN §5e;
graphsage-pytorch_amd/csrc/host/unsup.cpp, gs_unsup_extend_fast with no device
attached): every array and the subset flag against the plain-Python
restatement of tests/fast_extend_cases.py, properties that do not depend on the
rule, purity, uniformity of the chosen subsets and the argument errors."""
import itertools
import random

import numpy as np
import pytest

from tests import fast_cases as fc
from tests import fast_extend_cases as xc


def _loss(train, G=None, **kw):
    return xc.make_loss(G if G is not None else xc.far_graph(), xc.TRAIN[train] if isinstance(train, str) else train,
                        None, **kw)


@pytest.mark.parametrize("case", xc.CASES, ids=xc.CASE_IDS)
def test_mirror_equals_restatement(case):
    t, B, k, hops, walks, parts = case
    G = xc.far_graph()
    seed, bi = xc.case_seed(case)
    ul = _loss(t, seed=seed, n_walk_len=hops, walks=walks)
    nodes = xc.nodes_for(B)
    got = xc.run(ul, nodes, k, parts, bi)
    want = xc.rule_extend(G, xc.TRAIN[t], seed, bi, nodes, k, hops, walks, parts)
    xc.assert_same(got, want, xc.CASE_IDS[xc.CASES.index(case)])
    # what the cases are there for
    if t == "A" and parts & 2 and k:
        assert got["neg_cnt"].min() == k                       # Floyd everywhere (far lists of 1,667-2,000)
    if t == "B" and B >= 64 and parts & 2 and hops == 5 and k == 100:
        assert set(got["neg_cnt"].tolist()) >= {30, 89}         # whole lists of the star and of the lattice


def test_edge_batches():
    G = xc.far_graph()
    ul = _loss("B", seed=3)
    for nodes, k in ((np.zeros(0, np.int64), 6), (np.array([2995], np.int64), 6), (np.array([2450, 2450], np.int64), 0)):
        xc.assert_same(xc.run(ul, nodes, k, 3, 4), xc.rule_extend(G, xc.T_B, 3, 4, nodes, k), str(nodes))
    # an empty far list: T_C's star nodes; 2450 has neither kind of pair, so the subset flag is off
    ulc = _loss("C", seed=3)
    nodes = np.array([2405, 2450, 100], np.int64)
    got = xc.run(ulc, nodes, 6, 3, 0)
    xc.assert_same(got, xc.rule_extend(G, xc.T_C, 3, 0, nodes, 6))
    assert got["neg_cnt"].tolist() == [0, 0, 6] and not got["ok"] and 2450 not in got["unique"]
    with pytest.raises(AssertionError):
        ulc.extend_nodes(nodes, num_neg=6)
    # an empty train set
    ule = _loss(np.zeros(0, np.int64))
    got = xc.run(ule, xc.nodes_for(64), 6)
    assert len(got["unique"]) == 0 and not got["ok"] and got["has_pos"].any()


def test_directed_dead_end():
    G = xc.directed_graph()
    ul = _loss(xc.T_DIRECTED, G=G, seed=5, walks=(3, 4), n_walk_len=2)
    nodes = np.array([xc.PATH_HI - 2, xc.PATH_HI, xc.PATH_LO, 5], np.int64)
    got = xc.run(ul, nodes, 6, 3, 1)
    xc.assert_same(got, xc.rule_extend(G, xc.T_DIRECTED, 5, 1, nodes, 6, 2, (3, 4)))
    # every walk from 2947 stops after two steps, at the dead end 2949: one train node (2948) on the way
    assert got["pos_cnt"].tolist() == [3, 0, 6, 0] and got["has_pos"].tolist() == [True, False, True, False]
    # balls follow out-edges: 2900's ball is {2900, 2901, 2902}, so 2900 and 2902 are not far
    far0 = set(xc.T_DIRECTED.tolist()) - {2900, 2902}
    assert set(xc.run(ul, nodes[2:3], 100, 2)["neg"][:, 1].tolist()) == far0


@pytest.mark.parametrize("t,k,walks", [("A", 65, (6, 1)), ("B", 6, (6, 1)), ("B", 100, (3, 2))])
def test_properties_independent_of_the_rule(t, k, walks):
    G = xc.far_graph()
    rp, col = G.row_ptr(), G.col()
    train = set(xc.TRAIN[t].tolist())
    ul = _loss(t, seed=11, walks=walks)
    nodes = xc.nodes_for(130)
    got = xc.run(ul, nodes, k, 3, 9)
    no = np.concatenate([[0], np.cumsum(got["neg_cnt"])])
    po = np.concatenate([[0], np.cumsum(got["pos_cnt"])])
    for r, v in enumerate(nodes.tolist()):
        ball = xc.ball(G, v, 5)
        mine = got["neg"][no[r]:no[r + 1]]
        assert np.all(mine[:, 0] == v)
        picked = mine[:, 1].tolist()
        assert len(set(picked)) == len(picked) == min(k, len(train - ball))
        assert all(x in train and x not in ball for x in picked)
        pairs = got["pos"][po[r]:po[r + 1]]
        assert np.all(pairs[:, 0] == v) and all(x in train and x != v for x in pairs[:, 1].tolist())
        if walks[1] == 1:
            assert set(pairs[:, 1].tolist()) <= set(col[rp[v]:rp[v + 1]].tolist())
        assert got["has_pos"][r] == (rp[v + 1] > rp[v])
    assert np.all(np.diff(got["unique"]) > 0)
    assert set(got["unique"].tolist()) == set(got["pos"].reshape(-1).tolist()) | set(got["neg"].reshape(-1).tolist())


def test_purity():
    ul = _loss("A", seed=824)
    nodes = xc.nodes_for(65)
    random.seed(4)
    state = random.getstate()
    a = xc.run(ul, nodes, 6, 3, 7)
    xc.assert_same(xc.run(ul, nodes, 6, 3, 7), a)
    ul1 = _loss("A", seed=824, n_threads=1)
    xc.assert_same(xc.run(ul1, nodes, 6, 3, 7), a, "one thread")
    for seed, bi in ((824, 8), (825, 7), (824, 7 + 2 ** 32), (824 + 2 ** 32, 7)):
        c = xc.run(ul, nodes, 6, 3, bi, seed=seed)
        assert not np.array_equal(c["neg"], a["neg"]) and not np.array_equal(c["pos"], a["pos"]), (seed, bi)
    # the public calls: extend_nodes* advance batch_index, the part calls read it
    ul.seed, ul.batch_index = 824, 7
    u = ul.extend_nodes_array(nodes, num_neg=6)
    assert ul.batch_index == 8 and np.array_equal(u, a["unique"])
    assert ul.positive_pairs == [tuple(p) for p in a["pos"].tolist()]
    assert ul.negtive_pairs == [tuple(p) for p in a["neg"].tolist()]
    assert ul.extend_nodes(nodes, num_neg=6) != a["unique"].tolist() and ul.batch_index == 9
    ul.batch_index = 7
    assert ul.get_negtive_nodes(nodes, 6)[-len(a["neg"]):] == [tuple(p) for p in a["neg"].tolist()]
    assert ul.get_positive_nodes(nodes)[-len(a["pos"]):] == [tuple(p) for p in a["pos"].tolist()]
    assert ul.batch_index == 7
    assert random.getstate() == state


@pytest.mark.parametrize("far,k,M,band", [(5, 2, 4000, 18.97), (7, 3, 7000, 13.94)], ids=["5c2", "7c3"])
def test_uniformity(far, k, M, band):
    """A star node whose far list is `far` lattice train ids, over M batch indices at seed 7: each of the
    C(far, k) subsets is drawn M / C(far, k) times in expectation and stays within 4 standard deviations
    (`band` is one) of it.  The same check over the deliberately biased rule (x mod k) must fail."""
    train = np.array([10 + 80 * i for i in range(far)], np.int64)
    ul = _loss(train, seed=7)
    node = np.array([2450], np.int64)
    subsets = {s: 0 for s in itertools.combinations(train.tolist(), k)}
    wrong = dict(subsets)
    expect = M / len(subsets)
    assert abs(band - np.sqrt(M * (1 / len(subsets)) * (1 - 1 / len(subsets)))) < 0.01
    for bi in range(M):
        got = xc.run(ul, node, k, 2, bi)
        subsets[tuple(sorted(got["neg"][:, 1].tolist()))] += 1
        w = fc.draw_words(7, bi, 1, xc.HOP_NEG, k)[0]
        wrong[tuple(sorted(train[fc.rule_positions(w, far, k, wrong="mod")].tolist()))] += 1
    dev = max(abs(c - expect) for c in subsets.values())
    print(f"C({far},{k}) over {M}: largest deviation {dev:.1f} = {dev / band:.2f} sigma")
    assert sum(subsets.values()) == M and dev <= 4 * band
    assert max(abs(c - expect) for c in wrong.values()) > 4 * band


def test_arguments():
    G = xc.far_graph()
    ul = _loss("B")
    nodes = xc.nodes_for(64)
    with pytest.raises(ValueError, match="1024"):
        xc.run(ul, nodes, 1025)
    xc.run(ul, nodes, 1024)
    with pytest.raises(ValueError, match="Sample larger"):
        xc.run(ul, nodes, -1)
    with pytest.raises(IndexError):
        xc.run(ul, np.array([xc.N], np.int64), 6)
    with pytest.raises(ValueError):
        xc.run(ul, nodes, 6, parts=0)
    big = _loss("B", walks=(257, 256))
    with pytest.raises(ValueError, match="65536"):
        xc.run(big, nodes[:2], 6)
    xc.run(_loss("B", walks=(256, 256)), nodes[:2], 6)
    with pytest.raises(ValueError):
        xc.unsup.UnsupervisedLoss(G, xc.T_B, None, extend="fast", rng=xc.gs.RNG(1))
    with pytest.raises(ValueError):
        xc.unsup.UnsupervisedLoss(G, xc.T_B, None, extend="quick")
    assert xc.unsup.UnsupervisedLoss(G, xc.T_B, None).extend == "exact"
