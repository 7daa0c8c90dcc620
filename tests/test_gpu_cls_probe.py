"""The classifier probe on the GPU: the persistent kernel (hip_ops.cls_probe)
against the float64 torch restatement of the reference's loop
(tests/cls_probe_cases.py), its determinism and launch-cut independence,
train.ClassifierProbe, and train_classification(native=True) end to end
against the reference's own outputs (tests/golden/eval_utils.npz, tc__*).

Tolerance of the kernel, per case and per array (parameters, snapshots,
losses): with e32 the largest difference between the restatement run in fp32
on the CPU and in float64, the kernel's largest difference from float64 must
be at most 4 * e32 + one fp32 ulp of the array's largest magnitude.  e32
measures the reference's own arithmetic and does not depend on the kernel; the
4 is there because another summation order of the same length gives an error
of the same order, not the same value.  GS_CLS_PROBE_FIGURES=<path> writes the
measured ratios (kernel error / e32) as JSON.
"""
import importlib
import json
import os
import random
import types

import numpy as np
import pytest
import torch

from tests import cls_probe_cases as K
from tests import unsup_cases as C
from tests.golden.synth import uniform_features

pytestmark = pytest.mark.gpu

ops = importlib.import_module("graphsage-pytorch_amd.hip_ops")
models = importlib.import_module("graphsage-pytorch_amd.models")
utils = importlib.import_module("graphsage-pytorch_amd.utils")
train = importlib.import_module("graphsage-pytorch_amd.train")

G = os.path.join(os.path.dirname(__file__), "golden", "eval_utils.npz")
_FIGURES = {}


@pytest.fixture(scope="module", autouse=True)
def _write_figures():
    yield
    path = os.environ.get("GS_CLS_PROBE_FIGURES")
    if path and _FIGURES:
        with open(path, "w") as f:
            json.dump({"rule": "err <= 4 * e32 + ulp32(max |ref|); ratio = err / e32", "cases": _FIGURES,
                       "largest_ratio": max(v["ratio"] for c in _FIGURES.values() for v in c.values())}, f,
                      indent=1, sort_keys=True)


def _run(case, max_steps=0, snapshots=True, losses=True, shift=0):
    """The kernel on a case: (params, snapshots or None, losses or None) as float32 numpy.
    `shift`: the table sits that many columns into a table that much wider, so with an odd
    shift its rows start off a 16-byte boundary and the row stride is no multiple of 4."""
    c = K.case(*case)
    dev = torch.device("cuda", 0)
    table = torch.from_numpy(c.table).to(dev)
    if shift:
        wide = torch.full((table.shape[0], table.shape[1] + shift), float("nan"), device=dev)
        wide[:, shift:] = table
        table = wide[:, shift:]
    E = table[:, c.col0:c.col0 + c.D]
    labels = torch.from_numpy(c.labels.astype(np.int32)).to(dev)
    order = torch.from_numpy(c.order.astype(np.int32)).to(dev)
    params = torch.from_numpy(c.params).to(dev)
    P = params.numel()
    snaps = torch.full((c.epochs, P), float("nan"), device=dev) if snapshots else None
    ls = torch.full((c.epochs, c.steps), float("nan"), device=dev) if losses else None
    ops.cls_probe(E, labels, order, params, c.batch, K.LR, K.MAX_NORM, snaps, ls, max_steps_per_launch=max_steps)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(table.cpu().numpy(), c.table)  # the embeddings are read only
    return (params.cpu().numpy(), None if snaps is None else snaps.cpu().numpy(),
            None if ls is None else ls.cpu().numpy())


_full = {}


def _full_run(case):
    if case not in _full:
        _full[case] = _run(case)
    return _full[case]


def _check_rule(case, p, snaps, losses, tag):
    """The module docstring's rule on one run; the figures go to _FIGURES[tag]."""
    ref, r32 = K.reference(*case), K.reference(case[0], case[1], torch.float32)
    figs, fails = {}, []
    for what, got, want, w32 in (("params", p, ref.params, r32.params),
                                 ("snapshots", snaps, ref.snapshots, r32.snapshots),
                                 ("losses", losses, ref.losses, r32.losses)):
        assert np.all(np.isfinite(got)), what
        err = float(np.max(np.abs(got.astype(np.float64) - want)))
        e32 = float(np.max(np.abs(w32 - want)))
        bound = 4.0 * e32 + float(np.spacing(np.float32(np.max(np.abs(want)))))
        ratio = err / e32 if e32 > 0 else (0.0 if err == 0 else float("inf"))
        figs[what] = {"err": err, "e32": e32, "ratio": ratio, "bound": bound}
        print(f"{K.case_id(case)} {what}: err {err:.3e}, e32 {e32:.3e}, err/e32 {ratio:.2f}, bound {bound:.3e}")
        if err > bound:
            fails.append(what)
    _FIGURES[tag] = figs
    assert not fails, (fails, figs)
    np.testing.assert_array_equal(snaps[-1], p)  # the last snapshot is the returned parameters


@pytest.mark.parametrize("case", K.CASES, ids=K.case_id)
def test_kernel_matches_float64_restatement(case):
    _check_rule(case, *_full_run(case), K.case_id(case))


# shapes whose D is a multiple of 4: Cora's, the largest, and the column slice
_MISALIGNED = [c for c in K.CASES if c[0] in (0, 3, 4)]


@pytest.mark.parametrize("case", _MISALIGNED, ids=K.case_id)
def test_misaligned_rows_take_the_scalar_path(case):
    """D % 4 == 0 but the rows start one float off a 16-byte boundary and the
    row stride is odd: the launcher falls back to the scalar kernel with its own
    tile layout (rows of D | 1).  The same rule against float64, bitwise
    repeatable and independent of the launch cut."""
    c = K.case(*case)
    assert c.D % 4 == 0 and (c.col0 + 1) % 4 != 0  # float4 rows, were they aligned
    base = _run(case, shift=1)
    _check_rule(case, *base, K.case_id(case) + "-misaligned")
    for kw in (dict(), dict(max_steps=1), dict(max_steps=3)):
        got = _run(case, shift=1, **kw)
        for a, b in zip(base, got):
            np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32), err_msg=str(kw))


@pytest.mark.parametrize("case", K.CASES, ids=K.case_id)
def test_kernel_is_bitwise_repeatable_and_cut_independent(case):
    """The same call twice, then launches of 1 and of 3 steps: identical
    parameters, snapshots and losses; without snapshots and losses the
    parameters are the full call's."""
    base = _full_run(case)
    for kw in (dict(), dict(max_steps=1), dict(max_steps=3)):
        got = _run(case, **kw)
        for a, b in zip(base, got):
            np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32), err_msg=str(kw))
    p, s, l = _run(case, max_steps=3, snapshots=False, losses=False)
    assert s is None and l is None
    np.testing.assert_array_equal(base[0].view(np.uint32), p.view(np.uint32))
    p, s, l = _run(case, snapshots=False)
    np.testing.assert_array_equal(base[0].view(np.uint32), p.view(np.uint32))
    np.testing.assert_array_equal(base[2].view(np.uint32), l.view(np.uint32))


def test_kernel_treats_an_out_of_range_label_as_no_class():
    dev = torch.device("cuda", 0)
    rs = np.random.RandomState(4)
    E = rs.standard_normal((6, 4)).astype(np.float32)
    p0 = (rs.standard_normal(15) * 0.1).astype(np.float32)
    y = np.array([0, 1, 2, 7, -1, 1], np.int32)
    order = np.arange(6, dtype=np.int32)[None]
    want, _, wl = ops.cls_probe_host(E, y, order, p0, 6, 0.5, 5.0)
    params, losses = torch.from_numpy(p0).to(dev), torch.zeros(1, 1, device=dev)
    ops.cls_probe(torch.from_numpy(E).to(dev), torch.from_numpy(y).to(dev), torch.from_numpy(order).to(dev), params,
                  6, 0.5, 5.0, None, losses)
    np.testing.assert_allclose(params.cpu().numpy(), want, rtol=0, atol=1e-6)
    np.testing.assert_allclose(losses.cpu().numpy(), wl, rtol=0, atol=1e-6)


def test_wrapper_refuses_what_the_kernel_cannot_take():
    dev = torch.device("cuda", 0)
    E = torch.zeros(10, 8, device=dev)
    y = torch.zeros(10, dtype=torch.int32, device=dev)
    o = torch.zeros(1, 4, dtype=torch.int32, device=dev)
    p = torch.zeros(3 * 9, device=dev)
    with pytest.raises(ValueError):
        ops.cls_probe(E, y, o, p, 4, float("nan"), 5.0)
    with pytest.raises(ValueError):
        ops.cls_probe(E, y, o, p, 4, 0.5, 0.0)
    with pytest.raises(ValueError):
        ops.cls_probe(E, y, o, p[:-1], 4, 0.5, 5.0)
    with pytest.raises(ValueError):
        ops.cls_probe(E.t(), y, o, p, 4, 0.5, 5.0)
    with pytest.raises(TypeError):
        ops.cls_probe(E, y, o.long(), p, 4, 0.5, 5.0)
    with pytest.raises(RuntimeError):
        ops.cls_probe(E.cpu(), y, o, p, 4, 0.5, 5.0)


# ------------------------------------------------------------ train.ClassifierProbe
def test_classifier_probe_runs_and_predicts():
    case = (0, K.SCALES[0][1])
    c, base = K.case(*case), _full_run(case)
    dev = torch.device("cuda", 0)
    E = torch.from_numpy(np.ascontiguousarray(c.E)).to(dev)
    probe = train.ClassifierProbe(E, c.labels, c.C, weights=(torch.from_numpy(c.W), torch.from_numpy(c.b)),
                                  lr=K.LR, max_norm=K.MAX_NORM, batch=c.batch)
    assert sorted(probe.state_dict()) == ["layer.0.bias", "layer.0.weight"]
    losses, snaps = probe.run(c.order)
    assert losses.is_cuda and snaps.is_cuda
    assert tuple(losses.shape) == (c.epochs, c.steps) and tuple(snaps.shape) == (c.epochs, c.C * c.D + c.C)
    np.testing.assert_array_equal(snaps.cpu().numpy(), base[1])
    np.testing.assert_array_equal(losses.cpu().numpy(), base[2])
    sd = probe.state_dict()
    np.testing.assert_array_equal(sd["layer.0.weight"].cpu().numpy().reshape(-1), base[0][:c.C * c.D])
    np.testing.assert_array_equal(sd["layer.0.bias"].cpu().numpy(), base[0][c.C * c.D:])
    W, b = probe.weights()
    assert tuple(W.shape) == (c.C, c.D) and tuple(b.shape) == (c.C,)
    # predict: per epoch one by one (load_state_dict + predict) equals all epochs at once
    nodes = np.arange(len(c.E))
    allp = probe.predict(nodes, snaps).cpu().numpy()
    assert allp.shape == (c.epochs, len(nodes))
    for e in range(c.epochs):
        probe.load_state_dict({"layer.0.weight": snaps[e, :c.C * c.D].view(c.C, c.D),
                               "layer.0.bias": snaps[e, c.C * c.D:]})
        one = probe.predict(nodes).cpu().numpy()
        logits = c.E.astype(np.float64) @ base[1][e, :c.C * c.D].reshape(c.C, c.D).T.astype(np.float64) \
            + base[1][e, c.C * c.D:]
        top2 = np.sort(logits, 1)[:, -2:]
        sure = top2[:, 1] - top2[:, 0] > 1e-3  # rows whose argmax fp32 rounding cannot move
        np.testing.assert_array_equal(one[sure], logits.argmax(1)[sure])
        np.testing.assert_array_equal(allp[e][sure], one[sure])
    # a second object from the same start: torch tensors and int32 orders are accepted alike
    probe2 = train.ClassifierProbe(E, torch.from_numpy(c.labels), c.C,
                                   weights=(torch.from_numpy(c.W), torch.from_numpy(c.b)), batch=c.batch)
    _, snaps2 = probe2.run(torch.from_numpy(c.order.astype(np.int32)).to(dev))
    np.testing.assert_array_equal(snaps2.cpu().numpy(), base[1])


def test_classifier_probe_validates_once():
    dev = torch.device("cuda", 0)
    E = torch.zeros(20, 8, device=dev)
    y = np.arange(20) % 3
    with pytest.raises(ValueError):
        train.ClassifierProbe(E, y, 2)                      # a label >= n_classes
    with pytest.raises(ValueError):
        train.ClassifierProbe(E, -y, 3)                     # a negative label
    with pytest.raises(ValueError):
        train.ClassifierProbe(E.cpu(), y, 3)                # not on a HIP device
    with pytest.raises(ValueError):
        train.ClassifierProbe(E.double(), y, 3)             # not fp32
    with pytest.raises(ValueError):
        train.ClassifierProbe(torch.zeros(20, 8, 2, device=dev)[:, :, 0], y, 3)  # column stride != 1
    with pytest.raises(ValueError):
        train.ClassifierProbe(torch.zeros(20, 4096, device=dev), y, 16, batch=64)  # unsupported shape
    with pytest.raises(ValueError):
        train.ClassifierProbe(E, y, 3, batch=513)  # more rows than the workgroup has threads
    with pytest.raises(ValueError):
        ops.cls_probe(E, torch.zeros(20, dtype=torch.int32, device=dev), torch.zeros(1, 20, dtype=torch.int32, device=dev),
                      torch.zeros(3 * 9, device=dev), 1000, 0.5, 5.0)
    probe = train.ClassifierProbe(E, y, 3, batch=4)
    W, b = probe.weights()
    torch.manual_seed(824)
    ref = models.Classification(8, 3).layer[0]  # the reference's initialisation under the seed
    torch.testing.assert_close(W.cpu(), ref.weight.detach(), rtol=0, atol=0)
    torch.testing.assert_close(b.cpu(), ref.bias.detach(), rtol=0, atol=0)
    for bad in ([[0, 20]], [[-1, 3]]):
        with pytest.raises(IndexError):
            probe.run(np.array(bad))
        with pytest.raises(IndexError):
            probe.run(torch.tensor(bad, device=dev))
    with pytest.raises(ValueError):
        probe.run(np.arange(4))


# ------------------------------------------------------------ train_classification(native=True)
def _golden():
    return np.load(G)


def _setup(dev):
    """tests/test_eval_utils.py's setup: the golden's graph, split, features and trained weights."""
    A = _golden()
    n, F, H, Cn, seed = (int(x) for x in A["meta"])
    g = C.graphs()
    from collections import defaultdict
    adj = defaultdict(set)
    for a, b in zip(g["cora_src"].tolist(), g["cora_dst"].tolist()):
        adj[a].add(b)
        adj[b].add(a)
    np.random.seed(seed)
    perm = np.random.permutation(n)
    t, v = n // 3, n // 6
    test, val, tr = perm[:t], perm[t:t + v], perm[t + v:]
    labels = (np.arange(n) % Cn).astype(np.int64)
    dc = types.SimpleNamespace(g_test=test, g_val=val, g_train=tr, g_labels=labels)
    feats = torch.from_numpy(uniform_features(int(A["feat_seed"]), n, F)).to(dev)
    gsage = models.GraphSage(2, F, H, feats, adj, dev).to(dev)
    cls = models.Classification(H, Cn).to(dev)
    with torch.no_grad():
        for k, p in gsage.state_dict().items():
            p.copy_(torch.from_numpy(A[f"w__gs.{k}"]))
        for k, p in cls.state_dict().items():
            p.copy_(torch.from_numpy(A[f"w__cls.{k}"]))
    return A, dc, gsage, cls


def _state():
    return np.array(random.getstate()[1], np.int64)


def _np_state():
    s = np.random.get_state()
    return s[0], s[1].copy(), s[2:]


def _same_np_state(a, b):
    assert a[0] == b[0] and a[2] == b[2]
    np.testing.assert_array_equal(a[1], b[1])


def test_train_classification_native_matches_reference(tmp_path, monkeypatch, capsys):
    dev = torch.device("cuda", 0)
    A, dc, gsage, cls = _setup(dev)
    monkeypatch.chdir(tmp_path)
    random.seed(8)
    np.random.seed(8)
    cls2, m = utils.train_classification(dc, gsage, cls, "g", dev, 0.0, "golden", epochs=2, native=True)
    native_np = _np_state()
    native_out = capsys.readouterr().out
    native_saved = sorted(os.listdir(tmp_path / "models"))
    assert cls2 is cls
    assert m == float(A["tc__max"])
    np.testing.assert_array_equal(_state(), A["tc__state"])
    for k, v in cls.state_dict().items():
        np.testing.assert_allclose(v.cpu().numpy(), A[f"tc__cls.{k}"], atol=1e-4, rtol=1e-4, err_msg=k)
    assert all(p.requires_grad for p in cls.parameters())

    # the loop from the same seeds: numpy's stream ends in the same state, the same prints and checkpoints
    A, dc, gsage, cls = _setup(dev)
    (tmp_path / "loop").mkdir()
    monkeypatch.chdir(tmp_path / "loop")
    random.seed(8)
    np.random.seed(8)
    _, m_loop = utils.train_classification(dc, gsage, cls, "g", dev, 0.0, "golden", epochs=2)
    _same_np_state(native_np, _np_state())
    assert m_loop == m
    assert capsys.readouterr().out == native_out
    assert sorted(os.listdir(tmp_path / "loop" / "models")) == native_saved


def test_train_classification_frozen_evaluation(tmp_path, monkeypatch, capsys):
    dev = torch.device("cuda", 0)
    A, dc, gsage, cls = _setup(dev)
    monkeypatch.chdir(tmp_path)
    epochs = 4
    # the run by hand: the same embeddings, orders and probe, then the bookkeeping in plain Python
    random.seed(8)
    np.random.seed(8)
    feats = utils.get_gnn_embeddings(gsage, dc, "g")
    after_embed = random.getstate()
    from sklearn.utils import shuffle
    tr, order = dc.g_train, []
    for _ in range(epochs):
        tr = shuffle(tr)
        order.append(np.asarray(tr))
    lin = cls.layer[0]
    probe = train.ClassifierProbe(feats, dc.g_labels, lin.out_features,
                                  weights=(lin.weight.detach().clone(), lin.bias.detach().clone()))
    _, snaps = probe.run(np.stack(order))
    want_max, want_lines, want_files = 0.0, ["Training Classification ..."], []
    for e in range(epochs):
        probe.load_state_dict({"layer.0.weight": snaps[e, :lin.weight.numel()].view_as(lin.weight),
                               "layer.0.bias": snaps[e, lin.weight.numel():]})
        f1 = float(np.mean(probe.predict(dc.g_val).cpu().numpy() == dc.g_labels[dc.g_val]))
        want_lines.append(f"Validation F1: {f1}")
        if f1 > want_max:
            want_max = f1
            t1 = float(np.mean(probe.predict(dc.g_test).cpu().numpy() == dc.g_labels[dc.g_test]))
            want_lines.append(f"Test F1: {t1}")
            want_files.append("model_best_golden_ep{}_{:.4f}.torch".format(e, t1))
    capsys.readouterr()

    random.seed(8)
    np.random.seed(8)
    calls = []
    real_forward = type(gsage).forward
    monkeypatch.setattr(type(gsage), "forward", lambda self, nodes: calls.append(len(nodes)) or real_forward(self, nodes))
    cls2, m = utils.train_classification(dc, gsage, cls, "g", dev, 0.0, "golden", epochs=epochs, native=True,
                                         evaluate_on="frozen")
    assert cls2 is cls and m == want_max
    assert random.getstate() == after_embed  # nothing after the embeddings draws from `random`
    n = len(dc.g_labels)
    assert calls == [min(500, n - lo) for lo in range(0, n, 500)]  # get_gnn_embeddings' batches, no other forward
    assert capsys.readouterr().out.splitlines() == want_lines
    assert sorted(os.listdir(tmp_path / "models")) == sorted(want_files) if want_files else \
        not (tmp_path / "models").exists()
    np.testing.assert_array_equal(torch.cat([lin.weight.detach().reshape(-1), lin.bias.detach()]).cpu().numpy(),
                                  snaps[-1].cpu().numpy())  # the classifier ends with the last epoch's parameters
    for f in want_files:  # each checkpoint holds its own epoch's classifier
        e = int(f.split("_ep")[1].split("_")[0])
        saved = torch.load(tmp_path / "models" / f, weights_only=False)
        np.testing.assert_array_equal(saved[1].layer[0].bias.detach().cpu().numpy(),
                                      snaps[e, lin.weight.numel():].cpu().numpy())

    with pytest.raises(ValueError):
        utils.train_classification(dc, gsage, cls, "g", dev, 0.0, "golden", epochs=1, evaluate_on="frozen")
    with pytest.raises(ValueError):
        utils.train_classification(dc, gsage, cls, "g", dev, 0.0, "golden", epochs=1, native=True,
                                   evaluate_on="other")
