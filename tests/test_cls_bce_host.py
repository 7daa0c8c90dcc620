"""The multi-label head on the CPU: hip_ops.cls_bce_host / cls_bce_eval_host (the
numpy mirrors of gs_cls_bce_fwd_bwd / gs_cls_bce_eval) against torch float64
autograd on every case of tests/cls_bce_cases.py, pack_multilabel and its
inverse, the margins the GPU test relies on, and train.MultiLabelEvalResult's
metrics against a direct restatement."""
import importlib

import numpy as np
import pytest
import torch

from tests import cls_bce_cases as K

ops = importlib.import_module("graphsage-pytorch_amd.hip_ops")
train = importlib.import_module("graphsage-pytorch_amd.train")

CASES = K.cases()
SPECIAL = [((37, 128, 7), "rows", True, "x40"), ((50, 20, 17), "rows", True, "extreme"),
           ((257, 50, 33), "all", False, "extreme")]


def _check_mirror(c, ref):
    for mask in (False, True):
        loss, dE, dW, db, z = ops.cls_bce_host(c.E, c.W, c.b, c.y, c.pw, mask_relu=mask)
        assert dE.dtype == np.float64 and dE.shape == (c.B, c.D) and dW.shape == (c.C, c.D) and db.shape == (c.C,)
        scale = max(1.0, float(np.abs(ref.z).max()))
        np.testing.assert_allclose(z, ref.z, rtol=0, atol=1e-12 * scale)
        np.testing.assert_allclose(loss, ref.loss, rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(dE, ref.dE_masked() if mask else ref.dE, rtol=0, atol=1e-13)
        np.testing.assert_allclose(dW, ref.dW, rtol=0, atol=1e-12)
        np.testing.assert_allclose(db, ref.db, rtol=0, atol=1e-13)
        if mask:
            assert (dE[c.E <= 0] == 0).all()
    table = c.table[:, :c.D]
    loss, counts, n_exact, pred, z = ops.cls_bce_eval_host(table if c.rows is not None else table[:c.B], c.y, c.W,
                                                           c.b, rows=c.rows, pos_weight=c.pw)
    np.testing.assert_allclose(loss, ref.loss, rtol=1e-12, atol=1e-13)
    sure = np.abs(ref.z) > 1e-9
    np.testing.assert_array_equal(pred[sure], ref.pred[sure])
    assert counts.dtype == np.int64 and counts.shape == (c.C, 3)
    np.testing.assert_array_equal(counts, K.counts_of(pred, c.y))
    assert n_exact == int((pred == c.y).all(1).sum())
    if sure.all():
        np.testing.assert_array_equal(counts, K.counts_of(ref.pred, c.y))


@pytest.mark.parametrize("case", CASES, ids=K.case_id)
def test_mirrors_match_torch_float64(case):
    c, ref = K.case(*case, ""), K.reference(*case, "")
    _check_mirror(c, ref)
    # the fp32 form is the same function in another dtype
    l32 = ops.cls_bce_host(c.E, c.W, c.b, c.y, c.pw, dtype=np.float32)
    assert l32[1].dtype == np.float32 and abs(float(l32[0]) - ref.loss) < 1e-4 * max(1.0, abs(ref.loss))


@pytest.mark.parametrize("case", SPECIAL, ids=lambda s: K.case_id(s[:3]) + "-" + s[3])
def test_mirrors_match_torch_float64_on_the_special_cases(case):
    c, ref = K.case(*case), K.reference(*case)
    _check_mirror(c, ref)
    if case[3] == "x40":
        assert np.abs(ref.z).max() > 50 and np.isfinite(ref.l).all()   # |z| in the tens to hundreds
    else:
        assert (~c.y).all(1).any() and c.y.all(1).any()


@pytest.mark.parametrize("case", CASES + SPECIAL,
                         ids=lambda s: K.case_id(s[:3]) + ("-" + s[3] if len(s) > 3 else ""))
def test_margins_stay_within_the_cap(case):
    """What the GPU test's prediction check leaves out: at most MARGIN_CAP of a case's (row, label) elements have
    |z64| below 8 e_torch + 2^-22 max|z64|, counted from the two CPU references alone."""
    variant = case[3] if len(case) > 3 else ""
    ref, r32 = K.reference(*case[:3], variant), K.reference(*case[:3], variant, True)
    keep = K.margin_rule(ref.z, r32.z)
    left_out = int((~keep).sum())
    print(f"{left_out} of {keep.size} elements below the margin, smallest |z| {np.abs(ref.z).min():.3e}, "
          f"e_torch {np.max(np.abs(r32.z - ref.z)):.3e}, std z {ref.z.std():.2f}")
    assert left_out <= K.MARGIN_CAP * keep.size


def test_the_last_shape_is_the_library_s_limit():
    B, D, C = K.shapes()[-1]
    lib = importlib.import_module("graphsage-pytorch_amd._lib").lib()
    assert D == 64 and lib.gs_cls_bce_supported(D, C) == 1 and lib.gs_cls_bce_supported(D, C + 1) == 0
    assert lib.gs_cls_bce_supported(128, 128) == 1 and lib.gs_cls_bce_supported(256, 128) == 1
    assert ops.cls_bce_supported(D, C) and not ops.cls_bce_supported(D, C + 1)
    assert lib.gs_cls_bce_ws_bytes(B, D, C + 1) < 0 and lib.gs_cls_bce_ws_bytes(B, D, C) > 0


@pytest.mark.parametrize("C", [1, 7, 31, 32, 33, 64, 121])
def test_pack_round_trip(C):
    rs = np.random.RandomState(C)
    y = rs.uniform(0, 1, (19, C)) < 0.4
    y[3] = True    # every bit of a word, the sign bit included
    y[4] = False
    words = ops.pack_multilabel(torch.from_numpy(y))
    nW = (C + 31) // 32
    assert words.dtype == torch.int32 and tuple(words.shape) == (19, nW) and words.is_contiguous()
    w = words.numpy().view(np.uint32)
    for c in range(C):
        np.testing.assert_array_equal((w[:, c // 32] >> np.uint32(c % 32)) & 1, y[:, c])
    if C % 32:
        assert (w[:, -1] >> np.uint32(C % 32) == 0).all()     # the bits at or above C are zero
    assert torch.equal(ops.unpack_multilabel(words, C), torch.from_numpy(y))
    for dt in (torch.uint8, torch.int64, torch.float32, torch.float64):
        assert torch.equal(ops.pack_multilabel(torch.from_numpy(y).to(dt)), words)
    garbage = words.clone()
    if C % 32:
        garbage[:, -1] |= torch.tensor(-1, dtype=torch.int32) << (C % 32)
        assert torch.equal(ops.unpack_multilabel(garbage, C), torch.from_numpy(y))


def test_pack_refusals():
    y = torch.zeros(4, 5)
    for bad in (y + 0.5, y - 1, y + 2, torch.full((4, 5), float("nan"))):
        with pytest.raises(ValueError):
            ops.pack_multilabel(bad)
    with pytest.raises(ValueError):
        ops.pack_multilabel(torch.zeros(5, dtype=torch.bool))
    with pytest.raises(ValueError):
        ops.pack_multilabel(torch.zeros(0, 5, dtype=torch.bool))
    with pytest.raises(ValueError):
        ops.pack_multilabel(np.zeros((4, 5), bool))
    with pytest.raises(ValueError):
        ops.unpack_multilabel(torch.zeros(4, 1, dtype=torch.int32), 33)
    with pytest.raises(ValueError):
        ops.unpack_multilabel(torch.zeros(4, 1, dtype=torch.int64), 5)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_eval_result_metrics_against_a_restatement(seed):
    rs = np.random.RandomState(seed)
    B, C = 211, 9
    y = rs.uniform(0, 1, (B, C)) < 0.3
    pred = np.where(rs.uniform(0, 1, (B, C)) < 0.7, y, ~y)
    y[:, 4] = False        # a label with no positive: recall 0 / 0, and under pred = False F1 0 / 0
    pred[:, 4] = False
    pred[:, 5] = False     # never predicted: precision 0 / 0
    y[:40] = pred[:40]     # some rows exactly right
    counts = torch.from_numpy(K.counts_of(pred, y))
    n_exact = torch.tensor(int((pred == y).all(1).sum()))
    words = ops.pack_multilabel(torch.from_numpy(pred))
    r = train.MultiLabelEvalResult(torch.tensor(0.5), counts, n_exact, words, None, B, C)
    want = K.f1_restated(pred, y)
    assert r.n_exact == int(n_exact) and r.n_exact >= 40
    for k in ("micro_f1", "macro_f1", "subset_accuracy"):
        assert abs(getattr(r, k) - want[k]) < 1e-14, k
    for k in ("precision", "recall", "f1"):
        np.testing.assert_allclose(r.per_label[k], want[k], rtol=0, atol=1e-14)
    assert r.per_label["f1"][4] == 0 and r.per_label["precision"][5] == 0 and r.per_label["recall"][4] == 0
    np.testing.assert_array_equal(r.per_label["support"], y.sum(0))
    assert torch.equal(r.pred, torch.from_numpy(pred))
    assert 0 < r.micro_f1 < 1 and r.micro_f1 != r.macro_f1
