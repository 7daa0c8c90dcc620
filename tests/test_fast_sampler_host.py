"""Counter-based (Philox) sampler, host mirror (DESIGN §5d;
graphsage-pytorch_amd/csrc/host/fsample.cpp): known answers of the generator,
every pack against a plain-Python statement of the rule and the structural
properties the kernels rely on, purity, and uniformity of the chosen subsets."""
import importlib

import numpy as np
import pytest

from tests import fast_cases as fc

gs = importlib.import_module("graphsage-pytorch_amd")
S = importlib.import_module("graphsage-pytorch_amd.sampler")
L = importlib.import_module("graphsage-pytorch_amd._lib")

KNOWN = [  # the published Random123 vectors: counter, key, output
    ([0] * 4, [0] * 2, "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ([0xffffffff] * 4, [0xffffffff] * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0],
     "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


@pytest.fixture(scope="module")
def graph():
    return fc.special_graph()


@pytest.mark.parametrize("ctr,key,want", KNOWN)
def test_philox_known_answers(ctr, key, want):
    want = [int(w, 16) for w in want.split()]
    assert S.philox4x32(ctr, key).tolist() == want
    # the tests' own numpy restatement (fast_cases.philox_np) is held to the same vectors
    assert fc.philox_np(*[[c] for c in ctr], *key)[0].tolist() == want


@pytest.mark.parametrize("gcn", [False, True])
@pytest.mark.parametrize("fanouts", fc.FANOUT_SETS, ids=lambda f: "-".join(map(str, f)))
@pytest.mark.parametrize("B", [1, 7, 64, 130])
def test_pack_structure(graph, B, fanouts, gcn):
    roots = fc.roots_for(B)
    seed, bi = 824 + B, 3 * B + len(fanouts)
    pack, sizes, offs, used = S.fast_sample(graph, seed, bi, roots, fanouts, gcn=gcn)
    n_empty = fc.check_structure(graph, pack.numpy(), sizes, offs, used, roots, fanouts, gcn, seed, bi)
    # without fail_empty the isolated root's empty neighbourhood is sampled and counted, not an error
    assert (n_empty >= 1) == (not gcn and fc.ISOLATED in roots)


@pytest.mark.parametrize("fanouts", [[1], [32]], ids=lambda f: str(f[0]))
def test_layout_equals_host_sample(graph, fanouts):
    """One hop: both samplers take min(deg, k) entries per root, so the sizes
    agree and gs_sample_pack_layout of the bit-exact sample must give the
    fast pack's offsets and total."""
    roots = fc.roots_for(64)
    pack, sizes, offs, used = S.fast_sample(graph, 1, 0, roots, fanouts)
    s = S.sample(graph, gs.RNG(5), roots, fanouts)
    assert tuple(int(x) for x in sizes[0]) == s.sizes(1)
    assert offs[0].tolist() == s.offsets[0]
    assert used == s.pack_total + len(roots)


@pytest.mark.parametrize("gcn", [False, True])
def test_saturating_frontier(gcn):
    G = fc.dense_graph(40)
    roots = np.array([3, 17, 17, 39], np.int64)
    fanouts = [10, 10, 4]
    pack, sizes, offs, used = S.fast_sample(G, 9, 2, roots, fanouts, gcn=gcn)
    assert sizes[1, 2] == 40 and sizes[2, 0] == 40  # F2 is every node
    fc.check_structure(G, pack.numpy(), sizes, offs, used, roots, fanouts, gcn, 9, 2)


def test_fail_empty(graph):
    roots = np.array([fc.ISOLATED, 8], np.int64)
    for fanouts in ([10], [5, 4]):
        with pytest.raises(IndexError):
            S.fast_sample(graph, 0, 0, roots, fanouts, fail_empty=True)
        S.fast_sample(graph, 0, 0, roots, fanouts, fail_empty=True, gcn=True)  # self is always there
        S.fast_sample(graph, 0, 0, roots[1:], fanouts, fail_empty=True)


def test_arguments(graph):
    roots = np.array([1, 2], np.int64)
    for bad in ([0], [33], [10, -1], [None]):
        with pytest.raises(ValueError):
            S.fast_sample(graph, 0, 0, roots, bad)
    with pytest.raises(IndexError):
        S.fast_sample(graph, 0, 0, np.array([fc.N], np.int64), [5])
    with pytest.raises(ValueError):
        S.fast_sample(graph, 0, 0, np.zeros(0, np.int64), [5])


def test_purity(graph):
    roots = fc.roots_for(64)
    fan = [25, 10]
    a = S.fast_sample(graph, 824, 7, roots, fan)
    b = S.fast_sample(graph, 824, 7, roots, fan)
    assert a[3] == b[3] and np.array_equal(a[0].numpy(), b[0].numpy())
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    for seed, bi in ((824, 8), (825, 7), (824, 7 + 2 ** 32), (824 + 2 ** 32, 7)):
        c = S.fast_sample(graph, seed, bi, roots, fan)
        assert c[3] != a[3] or not np.array_equal(a[0].numpy(), c[0].numpy()), (seed, bi)


# 99.9th percentile of chi-square with 39 and with 10 degrees of freedom
CHI2_999 = {39: 72.055, 10: 29.588}


def _chi2(counts, expected):
    return float(((counts - expected) ** 2 / expected).sum())


@pytest.mark.parametrize("node,k,wrong_rule", [(fc.DEG40, 10, "mod"), (fc.SPECIAL[11], 10, "range")],
                         ids=["deg40", "deg11"])
def test_uniformity(graph, node, k, wrong_rule):
    """One root over M = 4000 batch indices: every row position is chosen
    M k / deg times in expectation; Σ (O - E)² / E stays under the 99.9th
    percentile of χ²(deg - 1).  The negatively correlated counts of
    without-replacement sampling only lower the statistic.  The same
    statistic over a deliberately wrong rule (x mod k; at deg = k + 1, where
    that is almost the identity, x drawn below m instead of m + 1) must exceed
    the cap, so this test can fail."""
    M, seed = 4000, 824
    deg = int(graph.degrees()[node])
    rp = graph.row_ptr()
    counts = np.zeros(deg)
    roots = np.array([node], np.int64)
    for bi in range(M):
        pack, sizes, offs, used = S.fast_sample(graph, seed, bi, roots, [k])
        o = int(offs[0, L.GS_PK_POS])
        counts[pack[o:o + k].numpy() - rp[node]] += 1
    E = M * k / deg
    cap = CHI2_999[deg - 1]
    stat = _chi2(counts, E)
    print(f"chi2(deg={deg}, k={k}) = {stat:.2f}, cap {cap}")
    assert counts.sum() == M * k
    assert stat < cap
    wrong = np.zeros(deg)
    for bi in range(M):
        w = fc.draw_words(seed, bi, 1, 1, k)[0]
        wrong[fc.rule_positions(w, deg, k, wrong=wrong_rule)] += 1
    print(f"wrong rule '{wrong_rule}': chi2 = {_chi2(wrong, E):.2f}")
    assert _chi2(wrong, E) > cap
