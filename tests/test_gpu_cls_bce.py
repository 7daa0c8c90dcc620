"""The multi-label head on the GPU (hip_ops.cls_bce / cls_bce_eval,
gs_cls_bce_fwd_bwd / gs_cls_bce_eval) against float64 on every case of
tests/cls_bce_cases.py.

Tolerances.  loss, dE, dWc, dbc and the logits: adam_cases.check_rule, err <=
4 e_torch + 2^-23 max|ref|, with e_torch the error of fp32 torch on the CPU
against float64 for the same quantity, never measured from the kernel (the
loss's yardstick where fp32 torch happens to hit the float64 mean:
cls_bce_cases.loss_yardstick).  Predictions: a bit equals the float64 decision
wherever |z64| >= 8 e_torch(z) + 2^-22 max|z64|, and a case fails when more than
1 % of its elements fall below that margin.  The counts and n_exact are exactly
those of the device's own predictions, and where no element is below the margin
exactly the float64 reference's.  GS_CLS_BCE_FIGURES=<path> writes the observed
ratios err / e_torch as JSON.
"""
import importlib
import json
import os

import numpy as np
import pytest
import torch

from tests import cls_bce_cases as K
from tests.adam_cases import check_rule

pytestmark = pytest.mark.gpu

ops = importlib.import_module("graphsage-pytorch_amd.hip_ops")
_lib = importlib.import_module("graphsage-pytorch_amd._lib")
DEV = torch.device("cuda", 0)
_FIGURES = []
CASES = [c + ("",) for c in K.cases()]
SPECIAL = [((37, 128, 7), "rows", True, "x40"), ((50, 20, 17), "rows", True, "extreme"),
           ((257, 50, 33), "all", False, "extreme")]


def _id(case):
    return K.case_id(case[:3]) + ("-" + case[3] if case[3] else "")


@pytest.fixture(scope="module", autouse=True)
def _write_figures():
    yield
    path = os.environ.get("GS_CLS_BCE_FIGURES")
    if path and _FIGURES:
        with open(path, "w") as f:
            json.dump({"rule": "err <= 4 * e_torch + 2^-23 * max|ref|; ratio = err / e_torch",
                       "largest_ratio": max(r[3] for r in _FIGURES if np.isfinite(r[3])),
                       "figures": [{"what": w, "err": e, "e_torch": t, "ratio": r, "bound": b}
                                   for w, e, t, r, b in _FIGURES]}, f, indent=1)


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


class Inputs:
    """A Case on the device: E [B, D] with the table's row stride, the packed targets and roots of the training
    head, H / rows / targets of the evaluation head."""

    def __init__(self, c, garbage=False):
        table = _dev(c.table)
        words = ops.pack_multilabel(_dev(c.targets))
        if garbage and c.C % 32:      # ones in every bit at or above C
            words = words.clone()
            words[:, -1] |= torch.tensor(-1, dtype=torch.int32, device=DEV) << (c.C % 32)
        self.W, self.b = _dev(c.W), _dev(c.b)
        self.pw = None if c.pw is None else _dev(c.pw)
        if c.rows is not None:
            self.rows = _dev(c.rows, torch.int32)
            self.E = table.index_select(0, self.rows.long())[:, :c.D]      # keeps the row stride
            self.targets, self.roots = words, self.rows
            self.H, self.eval_targets = table[:, :c.D], words
        else:
            self.rows = self.roots = None
            self.E = self.H = table[:c.B, :c.D]
            self.targets = self.eval_targets = words[:c.B].contiguous()

    def train(self, mask):
        return ops.cls_bce(self.E, self.W, self.b, self.targets, roots=self.roots, pos_weight=self.pw,
                           mask_relu=mask)

    def evaluate(self, **kw):
        return ops.cls_bce_eval(self.H, self.eval_targets, self.W, self.b, rows=self.rows, pos_weight=self.pw, **kw)

    def tensors(self):
        return [t for t in (self.E, self.H, self.W, self.b, self.pw, self.targets, self.roots) if t is not None]


def _np(out):
    torch.cuda.synchronize()
    return [None if t is None else t.cpu().numpy() for t in out]


def _check_case(case):
    c = K.case(*case)
    ref, r32 = K.reference(*case), K.reference(*case, True)
    x = Inputs(c)
    before = [t.clone() for t in x.tensors()]
    tag = f"cls_bce {_id(case)}"
    for mask in (False, True):
        loss, dE, dW, db = _np(x.train(mask))
        assert dE.shape == (c.B, c.D) and dW.shape == (c.C, c.D) and db.shape == (c.C,) and loss.shape == ()
        m = "masked " if mask else ""
        check_rule(f"{tag} {m}loss", loss, np.array([ref.loss]), K.loss_yardstick(ref, r32), _FIGURES)
        check_rule(f"{tag} {m}dE", dE, (ref.dE_masked() if mask else ref.dE).reshape(-1),
                   (r32.dE_masked() if mask else r32.dE).reshape(-1), _FIGURES)
        check_rule(f"{tag} {m}dWc", dW, ref.dW.reshape(-1), r32.dW.reshape(-1), _FIGURES)
        check_rule(f"{tag} {m}dbc", db, ref.db, r32.db, _FIGURES)
        if mask:   # exactly zero, sign included
            assert (dE.view(np.uint32)[c.E <= 0] == 0).all()
    loss, counts, n_exact, pred, logits = _np(x.evaluate(want_logits=True))
    assert counts.dtype == np.int64 and counts.shape == (c.C, 3) and pred.dtype == np.int32
    assert pred.shape == (c.B, (c.C + 31) // 32) and logits.shape == (c.B, c.C)
    check_rule(f"{tag} eval loss", loss, np.array([ref.loss]), K.loss_yardstick(ref, r32), _FIGURES)
    check_rule(f"{tag} logits", logits, ref.z.reshape(-1), r32.z.reshape(-1), _FIGURES)
    bits = ops.unpack_multilabel(torch.from_numpy(pred), c.C).numpy()
    if c.C % 32:
        assert (pred.view(np.uint32)[:, -1] >> np.uint32(c.C % 32) == 0).all()
    keep = K.margin_rule(ref.z, r32.z)
    left_out = int((~keep).sum())
    print(f"{tag}: {left_out} of {keep.size} elements below the margin")
    assert left_out <= K.MARGIN_CAP * keep.size
    np.testing.assert_array_equal(bits[keep], ref.pred[keep])
    np.testing.assert_array_equal(bits, logits > 0)        # the device's own decision: z > 0, z == 0 predicts 0
    np.testing.assert_array_equal(counts, K.counts_of(bits, c.y))
    assert int(n_exact) == int((bits == c.y).all(1).sum())
    if keep.all():
        np.testing.assert_array_equal(counts, K.counts_of(ref.pred, c.y))
        assert int(n_exact) == int((ref.pred == c.y).all(1).sum())
    # without pred and logits: the same loss and counts, bit for bit
    l2, c2, n2, p2, g2 = x.evaluate(want_pred=False)
    assert p2 is None and g2 is None
    assert np.array_equal(_bits(l2.cpu().numpy()), _bits(loss)) and np.array_equal(c2.cpu().numpy(), counts)
    assert int(n2) == int(n_exact)
    for a, b in zip(before, x.tensors()):     # inputs and pos_weight unmodified
        assert np.array_equal(_bits(a.cpu().numpy()), _bits(b.cpu().numpy()))
    return c, x


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_operator_matches_float64(case):
    _check_case(case)


@pytest.mark.parametrize("case", SPECIAL, ids=_id)
def test_special_cases_match_float64(case):
    c, _x = _check_case(case)
    if case[3] == "extreme":
        assert (~c.y).all(1).any() and c.y.all(1).any()


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_operator_is_bitwise_repeatable(case):
    x = Inputs(K.case(*case))
    a = _np(x.train(True)) + _np(x.evaluate(want_logits=True))
    b = _np(x.train(True)) + _np(x.evaluate(want_logits=True))
    for u, v in zip(a, b):
        assert np.array_equal(_bits(u), _bits(v))


@pytest.mark.parametrize("shape", [(1, 4, 1), (50, 20, 17), (257, 50, 33), (4099, 128, 121)],
                         ids=lambda s: "x".join(map(str, s)))
def test_bits_at_or_above_c_are_ignored(shape):
    c = K.case(shape, "rows", True, "")
    clean, dirty = Inputs(c), Inputs(c, garbage=True)
    assert not torch.equal(clean.targets, dirty.targets)
    a = _np(clean.train(True)) + _np(clean.evaluate(want_logits=True))
    b = _np(dirty.train(True)) + _np(dirty.evaluate(want_logits=True))
    for u, v in zip(a, b):
        assert np.array_equal(_bits(u), _bits(v))


def test_a_zero_logit_predicts_zero():
    """Small integers: every product and sum is exact, many logits are exactly 0."""
    rs = np.random.RandomState(4)
    B, D, C = 300, 8, 21
    H = rs.randint(-2, 3, (B, D)).astype(np.float32)
    W = rs.randint(-1, 2, (C, D)).astype(np.float32)
    b = rs.randint(-1, 2, C).astype(np.float32)
    y = rs.uniform(0, 1, (B, C)) < 0.3
    z = H.astype(np.float64) @ W.T.astype(np.float64) + b
    assert (z == 0).sum() > 100
    loss, counts, n_exact, pred, logits = ops.cls_bce_eval(_dev(H), ops.pack_multilabel(_dev(y)), _dev(W), _dev(b),
                                                           want_logits=True)
    np.testing.assert_array_equal(logits.cpu().numpy(), z)
    bits = ops.unpack_multilabel(pred, C).cpu().numpy()
    np.testing.assert_array_equal(bits, z > 0)
    np.testing.assert_array_equal(counts.cpu().numpy(), K.counts_of(z > 0, y))
    assert int(n_exact) == int(((z > 0) == y).all(1).sum())


def test_the_shape_past_the_limit_is_refused():
    B, D, C = K.shapes()[-1]
    lib = _lib.lib()
    assert lib.gs_cls_bce_supported(D, C) == 1 and lib.gs_cls_bce_supported(D, C + 1) == 0
    c = K.Case((B, D, C + 1), "all", False)
    E, W, b = _dev(c.table[:B, :D]), _dev(c.W), _dev(c.b)
    t = ops.pack_multilabel(_dev(c.targets[:B]))
    with pytest.raises(ValueError):
        ops.cls_bce(E, W, b, t)
    with pytest.raises(ValueError):
        ops.cls_bce_eval(E, t, W, b)
    # the C ABI itself, with a workspace that would do for the shape below
    ws = torch.empty(int(lib.gs_cls_bce_ws_bytes(B, D, C)) + 65536, dtype=torch.uint8, device=DEV)
    out = torch.zeros(B * D + (C + 1) * D + C + 2, dtype=torch.float32, device=DEV)
    rc = lib.gs_cls_bce_fwd_bwd(B, D, C + 1, E.data_ptr(), D, W.data_ptr(), b.data_ptr(), t.data_ptr(), None, None, 0,
                                out.data_ptr(), out.data_ptr(), out.data_ptr(), out.data_ptr(), ws.data_ptr(),
                                ws.numel(), None)
    assert rc == _lib.GS_EINVAL
    torch.cuda.synchronize()
    assert not out.any()


def test_every_refusal_of_the_c_abi():
    lib = _lib.lib()
    B, D, C = 37, 20, 17
    c = K.Case((B, D, C), "all", True)
    E, W, b, pw = _dev(c.table[:B, :D]), _dev(c.W), _dev(c.b), _dev(c.pw)
    t = ops.pack_multilabel(_dev(c.targets[:B]))
    need = int(lib.gs_cls_bce_ws_bytes(B, D, C))
    eneed = int(lib.gs_cls_bce_eval_ws_bytes(B, D, C))
    assert need > 0 and eneed > 0
    ws = torch.empty(max(need, eneed) + 64, dtype=torch.uint8, device=DEV)
    wp = ws.data_ptr() + (-ws.data_ptr()) % 16
    loss = torch.zeros(1, dtype=torch.float32, device=DEV)
    dE, dW, db = torch.zeros(B, D, device=DEV), torch.zeros(C, D, device=DEV), torch.zeros(C, device=DEV)
    counts = torch.zeros(3 * C + 1, dtype=torch.int64, device=DEV)

    def train(**kw):
        a = dict(B=B, D=D, C=C, E=E.data_ptr(), lde=D, W=W.data_ptr(), b=b.data_ptr(), t=t.data_ptr(), roots=None,
                 pw=pw.data_ptr(), mask=1, loss=loss.data_ptr(), dE=dE.data_ptr(), dW=dW.data_ptr(),
                 db=db.data_ptr(), ws=wp, wsb=need)
        a.update(kw)
        return lib.gs_cls_bce_fwd_bwd(a["B"], a["D"], a["C"], a["E"], a["lde"], a["W"], a["b"], a["t"], a["roots"],
                                      a["pw"], a["mask"], a["loss"], a["dE"], a["dW"], a["db"], a["ws"], a["wsb"],
                                      None)

    def evaluate(**kw):
        a = dict(B=B, D=D, C=C, H=E.data_ptr(), ldh=D, rows=None, t=t.data_ptr(), W=W.data_ptr(), b=b.data_ptr(),
                 loss=loss.data_ptr(), counts=counts.data_ptr(), ws=wp, wsb=eneed)
        a.update(kw)
        return lib.gs_cls_bce_eval(a["B"], a["D"], a["C"], a["H"], a["ldh"], a["rows"], a["t"], 0, a["W"], a["b"],
                                   None, None, None, a["loss"], a["counts"], a["ws"], a["wsb"], None)

    assert train() == _lib.GS_OK and evaluate() == _lib.GS_OK
    torch.cuda.synchronize()
    for k in ("E", "W", "b", "t", "loss", "dE", "dW", "db", "ws"):
        assert train(**{k: None}) == _lib.GS_EINVAL, k
    for k in ("H", "W", "b", "t", "loss", "counts", "ws"):
        assert evaluate(**{k: None}) == _lib.GS_EINVAL, k
    for k in ("B", "D", "C"):
        assert train(**{k: 0}) == _lib.GS_EINVAL and evaluate(**{k: 0}) == _lib.GS_EINVAL, k
        assert train(**{k: -3}) == _lib.GS_EINVAL, k
    assert train(lde=D - 1) == _lib.GS_EINVAL and evaluate(ldh=D - 1) == _lib.GS_EINVAL
    assert train(wsb=need - 1) == _lib.GS_EINVAL and evaluate(wsb=eneed - 1) == _lib.GS_EINVAL
    assert train(ws=wp + 4) == _lib.GS_EINVAL and evaluate(ws=wp + 8) == _lib.GS_EINVAL
    assert train(B=1 << 31) == _lib.GS_EINVAL
    assert lib.gs_cls_bce_ws_bytes(0, D, C) < 0 and lib.gs_cls_bce_eval_ws_bytes(B, 0, C) < 0
    assert train(roots=None, pw=None) == _lib.GS_OK    # both nullable
    torch.cuda.synchronize()


def test_the_wrapper_checks_its_arguments():
    c = K.case((37, 128, 7), "all", True, "")
    x = Inputs(c)
    with pytest.raises(ValueError):
        ops.cls_bce(x.E, x.W[:, :64].contiguous(), x.b, x.targets)
    with pytest.raises(ValueError):
        ops.cls_bce(x.E, x.W, x.b[:3], x.targets)
    with pytest.raises(ValueError):
        ops.cls_bce(x.E, x.W, x.b, x.targets[:5])
    with pytest.raises(ValueError):
        ops.cls_bce(x.E, x.W, x.b, x.targets, pos_weight=x.pw[:2])
    with pytest.raises(TypeError):
        ops.cls_bce(x.E, x.W, x.b, x.targets.long())
    with pytest.raises(ValueError):
        ops.cls_bce(x.E.t(), x.W, x.b, x.targets)
    with pytest.raises(RuntimeError):
        ops.cls_bce(x.E.cpu(), x.W, x.b, x.targets)
    with pytest.raises(ValueError):
        ops.cls_bce_eval(x.H, x.targets[:5], x.W, x.b)
    with pytest.raises(ValueError):
        ops.cls_bce_eval(x.H, x.targets, x.W, x.b, rows=torch.zeros(0, dtype=torch.int32, device=DEV))
