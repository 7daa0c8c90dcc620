"""The counter-based extend_nodes on the MI355X (DESIGN §5e;
graphsage-pytorch_amd/csrc/kernels/unsup_fast.hip):

* every array and the subset flag equal the host mirror's bit for bit — the
  mirror is itself held to a plain-Python statement of the rule in
  test_fast_extend_host.py;
* the loss kernels over the plan of such an extend against the float64 loop of
  full_unsup_ref.pair_loss on the object's own pair dicts, with the bound of
  test_gpu_unsup_loss.py;
* FullTrainer.unsup_step with such an object on the golden Cora batch, held as
  test_gpu_full_unsup.py holds the exact one."""
import importlib
import random

import numpy as np
import pytest
import torch

from tests import fast_extend_cases as xc
from tests import full_unsup_cases as uc
from tests import full_unsup_ref as uref
from tests import test_gpu_full_unsup as tfu
from tests import unsup_loss_cases as ulc
from tests.adam_cases import check_rule

pytestmark = pytest.mark.gpu

unsup = importlib.import_module("graphsage-pytorch_amd.unsup")
DEV = torch.device("cuda", 0)
_OBJ = {}

# The batch index of the Cora margin step: the first one (seed 7, searched on the CPU with the host mirror)
# whose batch has clear winners by full_unsup_cases.conditions, as the exact test's batch has.
CORA_SEED, CORA_MARGIN_BATCH_INDEX = 7, 0


def _pair(G, train, seed, hops=5, walks=(6, 1)):
    """(device object, host-mirror object) over one graph and train set, kept for the module."""
    key = (id(G), train.tobytes())
    if key not in _OBJ:
        _OBJ[key] = (xc.make_loss(G, train, DEV), xc.make_loss(G, train, DEV, device_balls=False))
    for ul in _OBJ[key]:
        ul.seed, ul.N_WALK_LEN, (ul.N_WALKS, ul.WALK_LEN) = seed, hops, walks
    assert _OBJ[key][0].device_balls and not _OBJ[key][1].device_balls
    return _OBJ[key]


@pytest.mark.parametrize("case", xc.CASES, ids=xc.CASE_IDS)
def test_device_equals_mirror(case):
    t, B, k, hops, walks, parts = case
    seed, bi = xc.case_seed(case)
    dev, host = _pair(xc.far_graph(), xc.TRAIN[t], seed, hops, walks)
    nodes = xc.nodes_for(B)
    xc.assert_same(xc.run(dev, nodes, k, parts, bi), xc.run(host, nodes, k, parts, bi))


def test_big_lattice_three_scan_blocks():
    dev, host = _pair(xc.big_lattice(), xc.T_BIG, 17)
    nodes = xc.big_nodes(65)
    got = xc.run(dev, nodes, 100, 3, 5)
    xc.assert_same(got, xc.run(host, nodes, 100, 3, 5))
    assert got["unique"].min() < 32768 < 65536 < got["unique"].max() and got["neg_cnt"].min() == 100


def test_directed_dead_end():
    dev, host = _pair(xc.directed_graph(), xc.T_DIRECTED, 5, 2, (3, 4))
    nodes = np.array([xc.PATH_HI - 2, xc.PATH_HI, xc.PATH_LO, 5], np.int64)
    got = xc.run(dev, nodes, 6, 3, 1)
    xc.assert_same(got, xc.run(host, nodes, 6, 3, 1))
    assert got["pos_cnt"].tolist() == [3, 0, 6, 0]


def test_empty_far_list_raises():
    dev, host = _pair(xc.far_graph(), xc.T_C, 3)
    nodes = np.array([2405, 2450, 100], np.int64)
    got = xc.run(dev, nodes, 6, 3, 0)
    xc.assert_same(got, xc.run(host, nodes, 6, 3, 0))
    assert not got["ok"] and got["neg_cnt"].tolist() == [0, 0, 6]
    dev.batch_index = 0
    with pytest.raises(AssertionError):
        dev.extend_nodes(nodes, num_neg=6)
    assert dev.batch_index == 1


def test_smaller_second_batch_sees_nothing_stale():
    dev, host = _pair(xc.far_graph(), xc.T_A, 21)
    for B, k, bi in ((130, 100, 0), (7, 6, 1), (130, 100, 0)):
        nodes = xc.nodes_for(B)
        xc.assert_same(xc.run(dev, nodes, k, 3, bi), xc.run(host, nodes, k, 3, bi), f"B={B}")
    # the unique bitmap is all zero between calls: an isolated node without negatives and an empty batch
    # extend to nothing
    for nodes, k in ((np.array([2995], np.int64), 0), (np.zeros(0, np.int64), 6)):
        got = xc.run(dev, nodes, k, 3, 2)
        assert len(got["unique"]) == len(got["pos"]) == len(got["neg"]) == 0 and not got["ok"]
        xc.assert_same(got, xc.run(host, nodes, k, 3, 2))
    with pytest.raises(ValueError, match="1024"):
        xc.run(dev, xc.nodes_for(7), 1025)
    xc.assert_same(xc.run(dev, xc.nodes_for(7), 1024, 3, 3), xc.run(host, xc.nodes_for(7), 1024, 3, 3))


@pytest.mark.parametrize("kind,num_neg", [("sage", 100), ("margin", 6)])
def test_losses_after_a_fast_extend(kind, num_neg):
    D = 64
    dev, _host = _pair(xc.far_graph(), xc.T_A, 13)
    dev.batch_index = 4
    random.seed(2)
    state = random.getstate()
    nodes = xc.nodes_for(80)
    nodes = nodes[xc.far_graph().degrees()[nodes] > 0][:65]     # the loss loops refuse a node without neighbours
    assert len(nodes) == 65
    uniq = dev.extend_nodes_array(nodes, num_neg=num_neg)
    pos_lists, neg_lists, U = ulc.lists_of_object(dev)
    assert U == len(uniq) and len(pos_lists) > 40
    E = np.random.RandomState(D + num_neg).standard_normal((U, D)).astype(np.float32)
    refs = []
    for dt in (torch.float64, torch.float32):
        emb = torch.from_numpy(E).to(dt).requires_grad_(True)
        loss, _cos, scores, _sel = uref.pair_loss(emb, (pos_lists, neg_lists), kind, float(dev.Q), float(dev.MARGIN))
        loss.backward()
        refs.append({"loss": float(loss.detach().double()), "score": scores.detach().double().numpy().reshape(-1),
                     "dE": emb.grad.double().numpy().reshape(-1)})
    r64, r32 = refs
    emb = torch.from_numpy(E).to(DEV).requires_grad_(True)
    loss = (dev.get_loss_sage if kind == "sage" else dev.get_loss_margin)(emb, uniq)
    loss.sum().backward()
    assert random.getstate() == state
    failures = []
    try:
        check_rule(f"fast extend {kind} dE", emb.grad.cpu().numpy(), r64["dE"], r32["dE"])
    except AssertionError as e:
        failures.append(str(e))
    e_score = float(np.max(np.abs(r32["score"] - r64["score"])))
    err = abs(float(loss.detach().reshape(-1)[0]) - r64["loss"])
    bound = 4.0 * e_score + 2.0 ** -23 * abs(r64["loss"])
    msg = f"fast extend {kind} loss: err {err:.3e}, e_torch(score) {e_score:.3e}, bound {bound:.3e}"
    print(msg)
    if not err <= bound:
        failures.append(msg)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("unsup_loss,method", [("normal", "unsup"), ("normal", "plus_unsup"), ("margin", "unsup"),
                                               ("margin", "plus_unsup")])
def test_unsup_step_with_a_fast_extend_on_cora(gs, unsup_loss, method):
    """test_unsup_step_end_to_end_on_cora with extend="fast": the float64 / float32 references fed the fast
    lists, the same bounds; `random` is not touched by the whole step."""
    graph, n, rp, col, X, Xd, labels, params, train_ids = tfu._cora()
    num_neg = {"normal": 100, "margin": 6}[unsup_loss]
    bi = CORA_MARGIN_BATCH_INDEX if unsup_loss == "margin" else 0
    batch = train_ids[:20]
    ul = unsup.UnsupervisedLoss(graph, train_ids, DEV, extend="fast", seed=CORA_SEED)
    assert ul.device_balls                                          # attached whatever the graph's size
    random.seed(11)
    state = random.getstate()
    ul.batch_index = bi
    ul.extend_nodes(batch, num_neg=num_neg)
    lists = ulc.lists_of_object(ul)
    nodes = np.asarray(ul.unique_nodes_batch, np.int64)
    kind = "sage" if unsup_loss == "normal" else "margin"
    refs = [uref.step_reference(rp, col, X, labels, nodes, params, "MEAN", False, lists=lists[:2], kind=kind,
                                q=float(ul.Q), margin=float(ul.MARGIN), with_sup=method == "plus_unsup", dtype=dt)
            for dt in (torch.float64, torch.float32)]
    if kind == "margin":                                            # this batch has clear winners
        e_ext = max(np.abs(refs[1][k] - refs[0][k]).max() for k in ("ext_pos", "ext_neg"))
        assert uc.conditions(refs[0], lists[:2], 100 * e_ext, 100 * np.abs(refs[1]["h"] - refs[0]["h"]).max()) == []
    tr = tfu._cora_trainer(params)
    ul.batch_index = bi
    loss, ext = tr.unsup_step(ul, batch, unsup_loss=unsup_loss, learn_method=method)
    assert ul.batch_index == bi + 1
    torch.cuda.synchronize()
    assert np.array_equal(ext, nodes) and tr._unsup_field is not None and tr._unsup_field.sizes[0] == len(nodes)
    failures = []
    e_score = float(np.max(np.abs(refs[1]["score"] - refs[0]["score"])))
    net = float(tr.loss_parts()[2])
    err, bound = abs(net - refs[0]["loss_net"]), 4.0 * e_score + 2.0 ** -23 * abs(refs[0]["loss_net"])
    print(f"cora fast {unsup_loss} {method} loss_net: err {err:.3e}, e_torch(score) {e_score:.3e}, bound {bound:.3e}")
    if not err <= bound:
        failures.append("loss_net")
    if method == "unsup":
        assert not np.any(tfu._np(tr.p.grads)[int(tr.p.offsets[2]):])
    # the step leaves the clipped gradients behind; a second trainer, forward_backward only, has the raw ones
    tr2 = tfu._cora_trainer(params)
    b = tr2.unsup_batch(ul, kind=unsup_loss, learn_method=method)
    tr2.forward_backward(b.nodes, field=tr2.field(b.nodes), unsup=b)
    torch.cuda.synchronize()
    assert float(tr2.loss_parts()[0]) == float(loss)
    for i, g in enumerate(refs[0]["grads"]):
        if method == "unsup" and i >= 2:
            continue
        try:
            check_rule(f"cora fast {unsup_loss} {method} d{tr2.p.names[i]}", tfu._np(tr2.p.view(i, grad=True)),
                       g.reshape(-1), refs[1]["grads"][i].reshape(-1))
        except AssertionError as e:
            failures.append(str(e))
    assert random.getstate() == state
    assert not failures, "\n".join(failures)
