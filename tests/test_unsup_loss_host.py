"""The yardsticks of test_gpu_unsup_loss.py, checked on the CPU
(tests/unsup_loss_cases.py):

* build_plan against gs_unsup_loss_plan on every batch of every golden extend
  case, and on a batch with repeated nodes (the dicts' last-occurrence rule);
* reference in fp32 against the loss and gradient captured from the reference
  model on the two golden embeddings;
* the case table: which instance of the kernels each width reaches, the plan's
  edges, and the conditions on the margin cases (clear winners, clear hinges,
  the split half on and half off) -- conditions on the inputs, no tolerances;
* the tie cases: torch.min / torch.max over dim 0 select the first of the tied.
"""
import random

import numpy as np
import pytest
import torch

from tests import unsup_cases as UC
from tests import unsup_loss_cases as C
from tests.test_unsup_native import U as unsup
from tests.test_unsup_native import _graph, _replay


def _native_plan(ul):
    plan, dims = ul._device_plan(torch.device("cpu"))
    return plan.numpy(), tuple(int(x) for x in dims)


def _assert_same_plan(ul):
    pos_lists, neg_lists, n_rows = C.lists_of_object(ul)
    mine, dims = C.build_plan(pos_lists, neg_lists, n_rows)
    native, ndims = _native_plan(ul)
    assert dims == ndims[:4]
    assert ndims[4:] == (len(ul.node_positive_pairs), len(ul.node_negtive_pairs))
    assert mine.dtype == native.dtype and np.array_equal(mine, native)
    return dims, pos_lists, neg_lists


@pytest.mark.parametrize("tag", UC.extend_tags())
def test_build_plan_equals_native_plan(tag):
    name, train, (_b_sz, num_neg, _nb, seed), batches = UC.extend_case(tag)
    ul = unsup.UnsupervisedLoss(_graph(name), train, "cpu", n_threads=4)
    random.seed(seed)
    for b in batches:
        if int(b["error"]):
            with pytest.raises(AssertionError):
                ul.extend_nodes(b["nodes"], num_neg=num_neg)
        else:
            ul.extend_nodes(b["nodes"], num_neg=num_neg)
        _assert_same_plan(ul)


def test_golden_plans_hold_the_edges():
    """What the golden cases contribute: skipped nodes and duplicate pairs."""
    skipped = dups = 0
    for tag in UC.loss_tags():
        ul = _replay(tag)
        dims, pos_lists, _neg = _assert_same_plan(ul)
        skipped += len(ul.node_positive_pairs) - dims[0]
        dups += sum(len(x) - len(set(x)) for x in pos_lists)
    assert skipped > 0 and dups > 0


def test_build_plan_repeated_nodes():
    """A batch that names nodes twice: a key sits at its first occurrence and holds its last one's pairs."""
    name, train, (_b_sz, num_neg, _nb, seed), batches = UC.extend_case("cora_n6")
    ul = unsup.UnsupervisedLoss(_graph(name), train, "cpu", n_threads=4)
    random.seed(seed)
    nodes = np.concatenate([batches[0]["nodes"], batches[0]["nodes"][:7]])
    ul.extend_nodes(nodes, num_neg=num_neg)
    assert len(ul.node_negtive_pairs) == len(batches[0]["nodes"])
    _assert_same_plan(ul)


@pytest.mark.parametrize("tag", UC.loss_tags())
@pytest.mark.parametrize("kind", ["sage", "margin"])
def test_reference_reproduces_golden_loss(tag, kind):
    """The tolerances of test_unsup_native.test_unsup_losses_match_reference."""
    G = UC.extend_file()
    pos_lists, neg_lists, n_rows = C.lists_of_object(_replay(tag))
    emb = G[f"{tag}__emb"]
    assert emb.shape[0] == n_rows
    r = C.reference(emb, (pos_lists, neg_lists), kind, C.Q, C.MARGIN, torch.float32)
    want = float(G[f"{tag}__{kind}_loss"])
    assert abs(r["loss"] - want) <= 1e-5 * max(1.0, abs(want))
    torch.testing.assert_close(torch.tensor(r["dE"], dtype=torch.float32), torch.from_numpy(G[f"{tag}__{kind}_grad"]),
                               atol=1e-6, rtol=1e-5)


# ------------------------------------------------------------------ the table
@pytest.mark.parametrize("D", C.WIDTHS)
def test_width_reaches_its_instance(D):
    _E, _lists, plan, dims = C.base(D)
    got = C.predicates(D, dims, plan)
    assert C.accepted(D)
    for k, v in C.EXPECT[D].items():
        assert got[k] == v, (D, k, got[k], v)
    # the plan's edges, the same at every width
    assert dims == (C.M, 580, 1008, C.U)
    assert got["max_pos"] == 40 and got["max_neg"] == 70 and got["pair_rounds"] == 5
    assert got["row_rounds"] >= 5 and got["memberless_rows"] == C.FREE_ROWS
    v = C.plan_views(plan, dims)
    tptr = v["tptr"]
    assert tptr[1] - tptr[0] == 2 * C.M                      # row 0: a partner in every list, five rounds
    assert np.all(v["pa"] != 0) and np.all(v["na"] != 0)     # and owner of nothing
    assert np.all(np.diff(tptr)[-C.FREE_ROWS:] == 0) and np.all(np.diff(tptr)[:-C.FREE_ROWS] > 0)
    assert sorted(set(np.diff(v["pos_ptr"]).tolist())) == sorted(C.POS_COUNTS)
    assert sorted(set(np.diff(v["neg_ptr"]).tolist())) == sorted(C.NEG_COUNTS)
    for m in range(C.M):                                     # partners without replacement
        for ptr_, b in ((v["pos_ptr"], v["pb"]), (v["neg_ptr"], v["nb"])):
            part = b[ptr_[m]:ptr_[m + 1]]
            assert len(set(part.tolist())) == len(part)


def test_every_instance_is_reached():
    by_nc = {}
    for D in C.WIDTHS:
        by_nc.setdefault(C.chunks_for(D), []).append(D)
    assert sorted(by_nc) == [2, 4, 8, 16]
    # both sides of every boundary, a partly filled last chunk and a full one in every instance
    assert (128, 132) == (max(by_nc[2]), min(by_nc[4])) and (256, 260) == (max(by_nc[4]), min(by_nc[8]))
    assert (512, 516) == (max(by_nc[8]), min(by_nc[16])) and max(by_nc[16]) == 1024
    for nc, ws in by_nc.items():
        lanes = {C.EXPECT[D]["lanes_last_chunk"] for D in ws}
        assert 1 in lanes and 16 in lanes, (nc, lanes)
    assert not any(C.accepted(D) for D in (0, 2, 6, 1028))


@pytest.mark.parametrize("D", C.WIDTHS)
@pytest.mark.parametrize("kind", ["margin", "split"])
def test_margin_case_has_clear_winners(D, kind):
    r = C.ref(D, kind)
    assert C.conditions(r) == []
    assert all(len(t) == 1 for t in r["ties_pos"] + r["ties_neg"])
    active = C.active_fraction(r)
    if kind == "split":
        assert 0.25 <= active <= 0.75
        assert C.margin_of(D, kind) == float(np.float32(C.margin_of(D, kind)))
    else:
        assert active == 1.0 and r["h"].min() >= 2.0
    # the fp32 run of the reference then selects the same pairs and the same hinges
    t = C.ref(D, kind, torch.float32)
    assert np.array_equal(t["sel_pos"], r["sel_pos"]) and np.array_equal(t["sel_neg"], r["sel_neg"])
    assert np.array_equal(t["h"] > 0, r["h"] > 0)
    # selected pairs carry the coefficient, nothing else does; a node with the hinge off has none
    on = r["h"] > 0
    nz = np.nonzero(r["coef"])[0]
    want = np.sort(np.concatenate([r["sel_pos"][on], 580 + r["sel_neg"][on]]))
    assert np.array_equal(nz, want)
    assert np.all(r["score"][~on] == 0.0)


@pytest.mark.parametrize("D", C.TIE_WIDTHS)
def test_tie_cases_select_the_first(D):
    _E, _lists, plan, dims, sites = C.tie_case(D)
    v = C.plan_views(plan, dims)
    assert {(s, j2 - j) for _m, s, j, j2 in sites} == {("pos", 1), ("pos", 16), ("neg", 1), ("neg", 16)}
    r = C.tie_ref(D)
    tied_nodes = [(m, s) for m, s, _j, _j2 in sites]
    assert C.conditions(r, tied_nodes) == []
    assert np.all(r["h"] > 0)
    # the fp32 run is the unit of the GPU test's rule: it must select what float64 selects (its cosines of two
    # equal rows need not be bitwise equal, so it may see no tie at all)
    t = C.tie_ref(D, torch.float32)
    assert np.array_equal(t["sel_pos"], r["sel_pos"]) and np.array_equal(t["sel_neg"], r["sel_neg"])
    assert np.array_equal(np.nonzero(t["coef"])[0], np.nonzero(r["coef"])[0])
    for m, s, j, j2 in sites:
        lo = v[f"{s}_ptr"][m]
        assert r[f"ties_{s}"][m].tolist() == [j, j2]
        assert r[f"sel_{s}"][m] == lo + j                    # the first of the tied
        g = (0 if s == "pos" else dims[1]) + lo
        assert r["coef"][g + j] != 0.0 and r["coef"][g + j2] == 0.0
        assert r["cos"][g + j] == r["cos"][g + j2]
    for m in range(C.M):
        for s in ("pos", "neg"):
            if (m, s) not in tied_nodes:
                assert len(r[f"ties_{s}"][m]) == 1


# ------------------------------------------------------ the class off width 128
@pytest.mark.parametrize("D", sorted(C.CLASS_SEED))
def test_class_inputs_have_clear_winners(D):
    ul = _replay(C.CLASS_TAG)
    pos_lists, neg_lists, n_rows = C.lists_of_object(ul)
    emb = C.class_embedding(D, n_rows, UC.extend_file())
    r = C.reference(emb, (pos_lists, neg_lists), "margin", C.Q, C.MARGIN, torch.float64)
    # the walks list a pair more than once: copies of the winner tie, and select the same two rows
    assert C.conditions(r, lists=(pos_lists, neg_lists)) == []
