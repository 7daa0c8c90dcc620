"""The classifier probe without a GPU: the numpy mirror (hip_ops.cls_probe_host)
against the float64 torch restatement of the reference's loop
(tests/cls_probe_cases.py), the library's argument checks, the support
formula, accuracy == micro-F1, and the up-front shuffle chain of
train_classification(native=True).

Tolerance of the mirror: 1e-12 relative to the largest magnitude of the array
compared.  Both sides are float64 and every sum has at most 256 terms, so an
element's error is a few hundred float64 roundings of the magnitudes summed
(up to 1e-13 of the array's scale over the run, 1.8e-13 observed at most), not
of the element itself: a parameter that cancels to 1e-6 of the others, or the
loss of a memorised batch of one (1e-66), has no relative accuracy of its own
in either implementation.
"""
import ctypes
import importlib
import types

import numpy as np
import pytest
import torch

from tests import cls_probe_cases as K

ops = importlib.import_module("graphsage-pytorch_amd.hip_ops")
utils = importlib.import_module("graphsage-pytorch_amd.utils")
train = importlib.import_module("graphsage-pytorch_amd.train")
models = importlib.import_module("graphsage-pytorch_amd.models")
_lib = importlib.import_module("graphsage-pytorch_amd._lib")


def _close(got, ref, what):
    scale = np.max(np.abs(ref))
    err = np.max(np.abs(np.asarray(got, np.float64) - ref))
    assert err <= 1e-12 * scale, f"{what}: err {err:.3e} vs scale {scale:.3e}"


@pytest.mark.parametrize("case", K.CASES, ids=K.case_id)
def test_host_mirror_matches_float64_restatement(case):
    c, ref = K.case(*case), K.reference(*case)
    before = c.params.copy()
    p, snaps, losses = ops.cls_probe_host(c.E, c.labels, c.order, before, c.batch, K.LR, K.MAX_NORM,
                                          dtype=np.float64)
    np.testing.assert_array_equal(before, c.params)  # the caller's parameters are not modified
    assert p.dtype == snaps.dtype == losses.dtype == np.float64
    assert snaps.shape == (c.epochs, c.C * c.D + c.C) and losses.shape == (c.epochs, c.steps)
    _close(p, ref.params, "params")
    _close(snaps, ref.snapshots, "snapshots")
    _close(losses, ref.losses, "losses")
    np.testing.assert_array_equal(snaps[-1], p)


@pytest.mark.parametrize("shape", range(len(K.SHAPES)))
def test_scales_clip_some_steps_and_not_others(shape):
    """On the float64 restatement's recorded norms: no step clips at the
    small scale; at the large one at least one does and at least one does not."""
    small, large = K.SCALES[shape]
    assert not K.clipped(K.reference(shape, small).norms).any()
    cl = K.clipped(K.reference(shape, large).norms)
    assert cl.any() and not cl.all()


def test_absent_class_cases_have_one():
    for i, sh in enumerate(K.SHAPES):
        c = K.case(i, K.SCALES[i][0])
        if sh[5]:
            assert sh[1] - 1 not in set(c.labels.tolist())


def test_host_mirror_out_of_range_label_is_no_class():
    """A label outside [0, C) contributes the softmax term only: the same
    step as with the row's one-hot left out, and no loss from that row."""
    rs = np.random.RandomState(4)
    E = rs.standard_normal((6, 4))
    p0 = rs.standard_normal(3 * 4 + 3) * 0.1
    y = np.array([0, 1, 2, 7, -1, 1])
    order = np.arange(6)[None]
    p, _, loss = ops.cls_probe_host(E, y, order, p0, 6, 0.5, np.inf)
    W, b = p0[:12].reshape(3, 4), p0[12:]
    z = E @ W.T + b
    logp = z - z.max(1, keepdims=True)
    logp = logp - np.log(np.exp(logp).sum(1, keepdims=True))
    ok = (y >= 0) & (y < 3)
    G = np.exp(logp)
    G[ok, y[ok]] -= 1
    G /= 6
    want = np.concatenate([(W - 0.5 * G.T @ E).reshape(-1), b - 0.5 * G.sum(0)])
    np.testing.assert_allclose(p, want, rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(loss[0, 0], -logp[ok, y[ok]].sum() / 6, rtol=1e-13)


# ------------------------------------------------------------ the library's checks
def _supported_formula(D, C, batch):
    r4 = lambda x: (x + 3) // 4 * 4
    ld = D + 4 if D % 4 == 0 else D | 1
    fits = 2 * r4(C * D + C) + r4(batch * ld) + r4(batch * (C | 1)) + 4 * r4(batch) + 32 <= 160 * 1024 // 4
    return fits and batch <= 512


def test_supported_shapes():
    L = _lib.lib()
    assert L.gs_cls_probe_supported(128, 7, 50) == 1
    assert L.gs_cls_probe_supported(256, 16, 64) == 1
    for sh in K.SHAPES:
        assert L.gs_cls_probe_supported(*sh[:3]) == 1
    for D, C, batch in [(0, 7, 50), (128, 0, 50), (128, 7, 0), (-4, 7, 50), (4096, 16, 64), (128, 7, 1 << 40),
                        (1 << 40, 1 << 40, 1)]:
        assert L.gs_cls_probe_supported(D, C, batch) == 0
    for D in (1, 5, 64, 127, 128, 300, 512, 1024):  # the header's formula, either side of the limit
        for C in (1, 7, 16, 41, 100):
            for batch in (1, 50, 64, 128, 256, 511, 512, 513, 1000):
                assert L.gs_cls_probe_supported(D, C, batch) == int(_supported_formula(D, C, batch)), (D, C, batch)
    # one thread carries each row's id and label: a batch above the workgroup's 512 threads is
    # refused however little LDS it needs
    assert L.gs_cls_probe_supported(4, 2, 512) == 1
    assert L.gs_cls_probe_supported(4, 2, 513) == 0
    assert L.gs_cls_probe_supported(4, 2, 1000) == 0
    assert L.gs_cls_probe_supported(1, 1, 512) == 1 and L.gs_cls_probe_supported(1, 1, 513) == 0


@pytest.mark.parametrize("batch", [513, 1000])
def test_batch_above_the_workgroup_is_refused_by_the_run(batch):
    L = _lib.lib()
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    rc = L.gs_cls_probe_run(p, 4, 2000, 4, 2, p, p, 1500, batch, 1, p, 0.5, 5.0, None, None, None)
    assert rc == _lib.GS_EINVAL
    rc = L.gs_cls_probe_run_ex(p, 4, 2000, 4, 2, p, p, 1500, batch, 1, p, 0.5, 5.0, None, None, 7, None)
    assert rc == _lib.GS_EINVAL


_OK = dict(lde=128, n_rows=100, D=128, C=7, n_train=60, batch=50, n_epochs=2, lr=0.5, max_norm=5.0)
_BAD = [("E", None), ("labels", None), ("order", None), ("params", None),
        ("D", 0), ("C", 0), ("batch", 0), ("n_train", 0), ("n_epochs", 0), ("D", -1), ("batch", -3),
        ("lde", 127), ("lr", float("nan")), ("lr", float("inf")), ("lr", float("-inf")),
        ("max_norm", 0.0), ("max_norm", -1.0), ("max_norm", float("nan")),
        ("D", 4096), ("batch", 100000)]


@pytest.mark.parametrize("name,value", _BAD, ids=[f"{n}={v}" for n, v in _BAD])
@pytest.mark.parametrize("entry", ["gs_cls_probe_run", "gs_cls_probe_run_ex"])
def test_invalid_arguments_are_refused_before_any_device_work(entry, name, value):
    """Every GS_EINVAL case of the header, with no device: the pointers are
    host buffers the library must not touch (a launch would fail otherwise)."""
    L = _lib.lib()
    buf = np.zeros(64, np.float32)
    a = dict(_OK, E=buf.ctypes.data, labels=buf.ctypes.data, order=buf.ctypes.data, params=buf.ctypes.data)
    a[name] = value
    if name == "D" and value > a["lde"]:
        a["lde"] = value  # the unsupported shape itself, not lde < D
    args = [a["E"], a["lde"], a["n_rows"], a["D"], a["C"], a["labels"], a["order"], a["n_train"], a["batch"],
            a["n_epochs"], a["params"], a["lr"], a["max_norm"], None, None]
    if entry.endswith("_ex"):
        args.append(3)
    rc = getattr(L, entry)(*args, None)
    assert rc == _lib.GS_EINVAL
    assert L.gs_last_error()
    with pytest.raises(ValueError):
        _lib.check(rc)


# ------------------------------------------------------------ accuracy == micro-F1
def test_accuracy_is_micro_f1():
    """Single-label multi-class: every miss is one false positive and one
    false negative, so micro precision = recall = accuracy = x, and
    sklearn's F = 2·x·x / (x + x) is x up to the rounding of its own product
    and quotient (two roundings: 2 ulp)."""
    from sklearn.metrics import f1_score
    rs = np.random.RandomState(0)
    for n, C in [(1, 2), (7, 3), (451, 7), (902, 7), (1000, 41), (33, 2)]:
        for _ in range(4):
            y, p = rs.randint(0, C, n), rs.randint(0, C, n)
            if rs.rand() < 0.5:
                p[: n // 2] = y[: n // 2]
            acc, f1 = utils.micro_f1(y, p), f1_score(y, p, average="micro")
            assert acc == (y == p).mean()
            assert abs(acc - f1) <= 2 * np.spacing(acc), (n, C, acc, f1)
    assert utils.micro_f1([1, 2, 3], [1, 2, 3]) == 1.0 == f1_score([1, 2, 3], [1, 2, 3], average="micro")


# ------------------------------------------------------------ the shuffle chain
class _StubProbe:
    """Stands in for train.ClassifierProbe: records what run() is handed."""
    seen = None

    def __init__(self, embeddings, labels, n_classes, weights=None, lr=0.5, max_norm=5.0, batch=50, seed=824):
        self.P = weights[0].numel() + weights[1].numel()
        type(self).seen = dict(lr=lr, max_norm=max_norm, batch=batch, n_classes=n_classes)

    def run(self, order):
        type(self).seen["order"] = np.array(order)
        return None, torch.zeros(len(order), self.P)


def _loop_that_only_shuffles(train_nodes, epochs, b_sz=50):
    """train_classification's loop with everything but its randomness removed."""
    from sklearn.utils import shuffle
    import math
    chain = []
    for epoch in range(epochs):
        train_nodes = shuffle(train_nodes)
        for index in range(math.ceil(len(train_nodes) / b_sz)):
            train_nodes[index * b_sz:(index + 1) * b_sz]
        chain.append(np.array(train_nodes))
    return np.stack(chain)


def test_native_draws_the_loops_shuffles_up_front(monkeypatch, capsys):
    tr = np.random.RandomState(1).permutation(300)[:137]
    dc = types.SimpleNamespace(g_train=tr.copy(), g_val=np.arange(5), g_test=np.arange(5, 9),
                               g_labels=np.arange(300) % 7)
    np.random.seed(8)
    want = _loop_that_only_shuffles(tr.copy(), 5)
    state = np.random.get_state()

    calls = []
    monkeypatch.setattr(train, "ClassifierProbe", _StubProbe)
    monkeypatch.setattr(utils, "get_gnn_embeddings", lambda *a, **k: torch.zeros(300, 16))
    monkeypatch.setattr(utils, "evaluate", lambda dc_, ds, g, c, dev, m, name, epoch: calls.append(epoch) or m)
    cls = models.Classification(16, 7)
    np.random.seed(8)
    out, m = utils.train_classification(dc, None, cls, "g", "cpu", 0.25, "x", epochs=5, native=True)
    assert out is cls and m == 0.25 and calls == [0, 1, 2, 3, 4]
    np.testing.assert_array_equal(_StubProbe.seen["order"], want)
    got = np.random.get_state()
    assert got[0] == state[0] and got[2:] == state[2:]
    np.testing.assert_array_equal(got[1], state[1])
    assert (_StubProbe.seen["lr"], _StubProbe.seen["max_norm"], _StubProbe.seen["batch"]) == (0.5, 5.0, 50)
    np.testing.assert_array_equal(dc.g_train, tr)  # the data centre's own array is not shuffled in place
    assert capsys.readouterr().out.startswith("Training Classification ...")


def test_native_with_no_epochs_returns_as_the_loop_does(monkeypatch, capsys):
    """range(0) is empty in the loop: the embeddings are computed, then nothing.
    The native path builds no probe either (nothing to validate or refuse)."""
    class _NoProbe:
        def __init__(self, *a, **k):
            raise AssertionError("no probe for zero epochs")

    embedded = []
    monkeypatch.setattr(train, "ClassifierProbe", _NoProbe)
    monkeypatch.setattr(utils, "get_gnn_embeddings", lambda *a, **k: embedded.append(1) or torch.zeros(30, 4096))
    dc = types.SimpleNamespace(g_train=np.arange(20), g_val=np.arange(2), g_test=np.arange(2),
                               g_labels=np.arange(30) % 3)
    cls = models.Classification(4096, 3)
    np.random.seed(3)
    state = np.random.get_state()
    for kw in (dict(), dict(evaluate_on="frozen")):
        out, m = utils.train_classification(dc, None, cls, "g", "cpu", 0.5, "x", epochs=0, native=True, **kw)
        assert out is cls and m == 0.5
    assert embedded == [1, 1]
    np.testing.assert_array_equal(np.random.get_state()[1], state[1])
    assert capsys.readouterr().out == "Training Classification ...\n" * 2


def test_evaluate_on_is_validated_before_anything_runs():
    with pytest.raises(ValueError):
        utils.train_classification(None, None, None, "g", "cpu", 0.0, "x", evaluate_on="frozen")
    with pytest.raises(ValueError):
        utils.train_classification(None, None, None, "g", "cpu", 0.0, "x", native=True, evaluate_on="embeddings")


def test_probe_constructor_refuses_cpu_embeddings():
    with pytest.raises(ValueError):
        train.ClassifierProbe(torch.zeros(10, 8), np.zeros(10, np.int64), 3)
