"""The float64 reference of the exact step under the unsupervised losses
(tests/full_unsup_ref.py) and the claims of tests/full_unsup_cases.py, on the
CPU: the reference's gradients against central finite differences, its
supervised restatement against full_train_ref.step_reference, the margin
cases' clear winners, and the rows no pair touches.
"""
import numpy as np
import pytest
import torch

from tests import full_train_ref as tref
from tests import full_unsup_cases as uc
from tests import full_unsup_ref as uref
from tests import unsup_loss_cases as ulc


def test_case_table_reaches_every_branch():
    assert {c["graph"] for c in uc.CASES} == {"hub_max", "bounded", "directed"}
    assert {c["L"] for c in uc.CASES} == {1, 2, 3} and {c["agg"] for c in uc.CASES} == {"MEAN", "MAX"}
    assert any(c["gcn"] for c in uc.CASES) and any(c["bf16"] for c in uc.CASES)
    assert {ulc.chunks_for(c["H"]) for c in uc.CASES} == {2, 4}
    assert [c["H"] for c in uc.CASES if ulc.chunks_for(c["H"]) == 4] == [256]
    assert uc.FACTOR == {} or all(len(v) == 2 and v[1] for v in uc.FACTOR.values())
    for cid in uc.IDS:
        s = uc.setup(cid)
        assert 37 <= s["U"] <= 96 and s["U"] < s["n"]
        M, P, N, U = s["dims"]
        v = ulc.plan_views(s["plan"], s["dims"])
        assert (M, U) == (s["M"], s["U"])
        pos, neg = np.diff(v["pos_ptr"]), np.diff(v["neg_ptr"])
        assert [int(x) for x in pos[:6]] == list(uc.POS_COUNTS) and [int(x) for x in neg[:5]] == list(uc.NEG_COUNTS)
        members = np.diff(v["tptr"])
        assert members[0] == 2 * M                                  # row 0: a partner in every list
        assert np.all(members[U - uc.FREE_ROWS:] == 0) and np.sum(members == 0) >= 2
        assert set(v["pb"].tolist()) >= {0} and not np.any(v["pa"] == 0)


@pytest.mark.parametrize("method,kind", [("unsup", "sage"), ("plus_unsup", "sage"), ("unsup", "margin"),
                                         ("plus_unsup", "split")])
def test_reference_gradients_agree_with_central_differences(method, kind):
    """Three entries of every parameter tensor the loss reaches, on the 48-node case, in float64."""
    cid = uc.FD_CASE
    s = uc.setup(cid)
    assert s["n"] == 48
    r = uc.ref(cid, method, kind)
    margin = uc.margin_of(cid, kind)

    def loss_at(params):
        return uref.step_reference(s["rp"], s["col"], s["X"], s["labels"], s["nodes"], params, s["agg"], s["gcn"],
                                   lists=s["lists"], kind=kind, margin=margin,
                                   with_sup=method == "plus_unsup")["loss"]

    rs = np.random.RandomState(3)
    eps = 1e-6
    base = [np.asarray(p, np.float64) for p in s["params"]]
    for i, g in enumerate(r["grads"]):
        if method == "unsup" and i >= s["L"]:
            assert not np.any(g)                                    # the classifier takes no part
            continue
        big = np.argsort(np.abs(g).reshape(-1))[-8:]
        for j in rs.choice(big, 3, replace=False):
            hi, lo = [p.copy() for p in base], [p.copy() for p in base]
            hi[i].reshape(-1)[j] += eps
            lo[i].reshape(-1)[j] -= eps
            fd = (loss_at(hi) - loss_at(lo)) / (2 * eps)
            assert abs(fd - g.reshape(-1)[j]) <= 1e-6 * max(1.0, abs(fd)), (i, j, fd, g.reshape(-1)[j])


@pytest.mark.parametrize("case_id", uc.IDS)
def test_supervised_restatement_is_full_train_ref(case_id):
    s = uc.setup(case_id)
    mine = uref.step_reference(s["rp"], s["col"], s["X"], s["labels"], s["nodes"], s["params"], s["agg"], s["gcn"],
                               bf16=s["bf16"])
    loss, grads, hs = tref.step_reference(s["rp"], s["col"], s["X"], s["labels"], s["nodes"], s["params"], s["agg"],
                                          s["gcn"], bf16=s["bf16"])
    assert mine["loss"] == loss and mine["loss_net"] == 0.0 and mine["loss_sup"] == loss
    assert all(np.array_equal(a, b) for a, b in zip(mine["grads"], grads))
    assert np.array_equal(mine["E"], hs[-1][s["nodes"]])


@pytest.mark.parametrize("kind", ["margin", "split"])
@pytest.mark.parametrize("case_id", uc.IDS)
def test_margin_cases_have_clear_winners(case_id, kind):
    """Best to runner-up and |h| at least 100 times the fp32 reference's own error in those quantities,
    measured for this case; copies of the winner are one candidate (the first index is taken)."""
    s = uc.setup(case_id)
    gap_min, h_min = uc.thresholds(case_id, kind)
    assert gap_min > 0 and h_min > 0
    r = uc.ref(case_id, "unsup", kind)
    assert uc.conditions(r, s["lists"], gap_min, h_min) == []
    r32 = uc.ref(case_id, "unsup", kind, torch.float32)
    pairs = [p for side in s["lists"] for lst in side for p in lst]
    P = s["dims"][1]
    for k, off in (("sel_pos", 0), ("sel_neg", P)):                 # fp32 picks the same pairs
        assert [pairs[off + i] for i in r[k]] == [pairs[off + i] for i in r32[k]]
    for k, side in (("pos", 0), ("neg", 1)):                        # torch takes the first of tied copies
        start = np.concatenate([[0], np.cumsum([len(x) for x in s["lists"][side]])])
        for m, tied in enumerate(r[f"ties_{k}"]):
            assert r[f"sel_{k}"][m] - start[m] == tied[0]
    on = float(np.mean(r["h"] > 0))
    if kind == "split":
        assert 0.25 <= on <= 0.75
        assert uc.margin_of(case_id, kind) == float(np.float32(uc.margin_of(case_id, kind)))
    else:
        assert on == 1.0


@pytest.mark.parametrize("kind", uc.KINDS)
@pytest.mark.parametrize("case_id", uc.IDS)
def test_rows_in_no_pair_have_no_gradient(case_id, kind):
    s = uc.setup(case_id)
    r = uc.ref(case_id, "unsup", kind)
    free = slice(s["U"] - uc.FREE_ROWS, s["U"])
    assert not np.any(r["dE"][free]) and not np.any(r["dE_net"][free]) and not np.any(r["dZ"][free])
    assert np.array_equal(r["dE"], r["dE_net"]) and r["loss"] == r["loss_net"] and r["loss_sup"] == 0.0
    assert np.any(r["dE"][0])                                       # the row every list holds
    rp = uc.ref(case_id, "plus_unsup", kind)
    assert np.array_equal(rp["dE_net"], r["dE_net"]) and np.any(rp["dE"][free])
    assert rp["loss"] == rp["loss_sup"] + rp["loss_net"]
