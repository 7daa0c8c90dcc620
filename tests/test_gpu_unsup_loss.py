"""kernels/unsup.hip (pair_scores_kernel, loss_reduce_kernel, row_grad_kernel)
on the MI355X against the float64 reference of tests/unsup_loss_cases.py, on
synthetic plans at every width that reaches another template instance.

The rule of every numeric comparison is adam_cases.check_rule: with e_torch
the largest error of the reference's own fp32 run on the CPU against its
float64 run, the kernel stays within factor * e_torch + 2^-23 * max|ref|
(factor 4 unless unsup_loss_cases.FACTOR names the row).  The scalar loss is
never held to an e_torch of its own (one draw, 2e-10 to 2e-8 here): it is the
mean of the node scores, so it is bounded by their e_torch plus the rounding
of the reduce.  The margin cases have clear winners in float64
(test_unsup_loss_host.py), so which pairs carry a coefficient is compared
exactly.

The workspace is read back: {coef, cos, n1, n2} per pair, the P positive pairs
first, then the node scores at float offset 4 (P + N) -- the interface between
the forward and the backward entry point.
"""
import importlib

import numpy as np
import pytest
import torch

from tests import unsup_cases as UC
from tests import unsup_loss_cases as C
from tests.adam_cases import check_rule
from tests.test_unsup_native import _replay

pytestmark = pytest.mark.gpu

ops = importlib.import_module("graphsage-pytorch_amd.hip_ops")
unsup = importlib.import_module("graphsage-pytorch_amd.unsup")
DEV = torch.device("cuda", 0)
TENSORS = ("cos", "n1", "n2", "coef", "score", "dE")
_PLANS = {}


def _plan_dev(plan):
    key = plan.tobytes()
    if key not in _PLANS:
        _PLANS[key] = torch.from_numpy(plan.copy()).to(DEV)
    return _PLANS[key]


def _run(E, plan, dims, kind, margin, dloss=1.0, dE=None):
    """Forward + backward through the hip_ops wrappers.  E: a numpy array (copied to the device) or a device
    tensor taken as it is, strides included; dE: a device tensor to write, or None for a NaN-filled one."""
    Mn, P, N, Un = dims
    if not isinstance(E, torch.Tensor):
        E = torch.from_numpy(np.array(E)).to(DEV)
    if dE is None:
        dE = torch.full((Un, E.shape[1]), float("nan"), dtype=torch.float32, device=DEV)
    ws = ops.unsup_loss_workspace(Mn, P, N, DEV).fill_(float("nan"))
    pd = _plan_dev(plan)
    loss = ops.unsup_loss_fwd(C.KIND_ID[kind], E, pd, dims, C.Q, margin, ws)
    dl = torch.tensor([dloss], dtype=torch.float32, device=DEV)
    ops.unsup_loss_bwd(E, pd, dims, ws, dl, dE)
    torch.cuda.synchronize()
    used = ws[:4 * (P + N) + Mn].cpu().numpy()
    info = used[:4 * (P + N)].reshape(-1, 4)
    return {"coef": info[:, 0], "cos": info[:, 1], "n1": info[:, 2], "n2": info[:, 3], "score": used[4 * (P + N):],
            "loss": loss.cpu().numpy(), "dE": dE.cpu().numpy(), "ws": used}


def _compare(what, got, ref, tor, factor_of, failures):
    """check_rule on every tensor and the loss's bound; every figure is printed before anything is asserted."""
    for name in TENSORS:
        try:
            check_rule(f"{what} {name}", got[name], ref[name].reshape(-1), tor[name].reshape(-1),
                       factor=factor_of(name))
        except AssertionError as e:
            failures.append(str(e))
    e_score = float(np.max(np.abs(tor["score"] - ref["score"])))
    err = abs(float(got["loss"]) - ref["loss"])
    bound = 4.0 * e_score + 2.0 ** -23 * abs(ref["loss"])
    msg = f"{what} loss: err {err:.3e}, e_torch(score) {e_score:.3e}, bound {bound:.3e}"
    print(msg)
    if not err <= bound:
        failures.append(msg)


def _selection(what, got, ref, dims, failures):
    """Margin kinds: exactly the reference's selected pairs carry a coefficient; hinge off: nothing, score 0."""
    on = ref["h"] > 0
    want = np.sort(np.concatenate([ref["sel_pos"][on], dims[1] + ref["sel_neg"][on]]))
    nz = np.nonzero(got["coef"])[0]
    if not np.array_equal(nz, want):
        failures.append(f"{what}: pairs with a coefficient {sorted(set(nz) ^ set(want))} differ from the reference's")
    if not np.all(got["score"][~on] == 0.0):
        failures.append(f"{what}: a node with the hinge off scores {got['score'][~on]}")
    if not np.all(got["score"][on] > 0.0):
        failures.append(f"{what}: a node with the hinge on scores 0")


# ------------------------------------------------------------------ (a) matrix
@pytest.mark.parametrize("D", C.WIDTHS)
@pytest.mark.parametrize("kind", C.KINDS)
def test_matrix(D, kind):
    E, _lists, plan, dims = C.base(D)
    ref, tor = C.ref(D, kind), C.ref(D, kind, torch.float32)
    got = _run(E, plan, dims, kind, C.margin_of(D, kind))
    failures = []
    _compare(f"unsup {D} {kind}", got, ref, tor, lambda name: C.factor(D, kind, name), failures)
    if kind != "sage":
        _selection(f"unsup {D} {kind}", got, ref, dims, failures)
    # dE went in as NaN: every row is written, the rows in no pair with zeros
    assert np.all(np.isfinite(got["dE"]))
    assert np.all(got["dE"][-C.FREE_ROWS:] == 0.0)
    assert not failures, "\n".join(failures)


# ----------------------------------------------------------------- (b) strides
@pytest.mark.parametrize("D", [68, 260])
@pytest.mark.parametrize("kind", C.KINDS)
def test_strided_views_give_the_contiguous_bits(D, kind):
    E, _lists, plan, dims = C.base(D)
    margin = C.margin_of(D, kind)
    want = _run(E, plan, dims, kind, margin)
    for pad in (4, 12):
        buf = torch.full((C.U, D + pad), float("nan"), dtype=torch.float32, device=DEV)
        buf[:, :D] = torch.from_numpy(np.array(E)).to(DEV)
        dbuf = torch.full((C.U, D + 8), -7.0, dtype=torch.float32, device=DEV)
        view, dview = buf[:, :D], dbuf[:, :D]
        assert view.stride(0) == D + pad and dview.stride(0) == D + 8 and not view.is_contiguous()
        got = _run(view, plan, dims, kind, margin, dE=dview)
        assert got["ws"].tobytes() == want["ws"].tobytes()
        assert got["loss"].tobytes() == want["loss"].tobytes()
        assert got["dE"].tobytes() == want["dE"].tobytes()
        assert bool(torch.all(dbuf[:, D:] == -7.0))          # the padding is untouched
        assert bool(torch.all(torch.isnan(buf[:, D:])))


# -------------------------------------------------------------------- (c) ties
@pytest.mark.parametrize("D", C.TIE_WIDTHS)
def test_ties_select_the_first_index(D):
    E, _lists, plan, dims, sites = C.tie_case(D)
    ref, tor = C.tie_ref(D), C.tie_ref(D, torch.float32)
    got = _run(E, plan, dims, "margin", C.MARGIN)
    v = C.plan_views(plan, dims)
    for m, s, j, j2 in sites:
        g = (0 if s == "pos" else dims[1]) + v[f"{s}_ptr"][m]
        assert got["cos"][g + j].tobytes() == got["cos"][g + j2].tobytes()   # a tie in the kernel too
        assert got["coef"][g + j] != 0.0 and got["coef"][g + j2] == 0.0
    failures = []
    _selection(f"unsup ties {D}", got, ref, dims, failures)
    _compare(f"unsup ties {D}", got, ref, tor, lambda name: C.factor(D, "margin", name), failures)
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------- (d) determinism
@pytest.mark.parametrize("kind", ["sage", "split"])
def test_widest_instance_repeats_and_scales(kind):
    D = 1024
    E, _lists, plan, dims = C.base(D)
    a, b = (_run(E, plan, dims, kind, C.margin_of(D, kind)) for _ in range(2))
    for k in ("ws", "loss", "dE"):
        assert a[k].tobytes() == b[k].tobytes(), k
    c = _run(E, plan, dims, kind, C.margin_of(D, kind), dloss=2.5)
    assert c["ws"].tobytes() == a["ws"].tobytes()
    torch.testing.assert_close(torch.from_numpy(c["dE"]), torch.from_numpy(a["dE"]) * 2.5, rtol=1e-6, atol=0)


# ---------------------------------------------------------------- (e) refusals
def _refused(E, ws, match, dims, plan, dE=None):
    """Forward (and backward, with dE) raise GS_EINVAL's ValueError and launch nothing: ws and dE keep their fill."""
    pd = _plan_dev(plan)
    with pytest.raises(ValueError, match=match):
        ops.unsup_loss_fwd(0, E, pd, dims, C.Q, C.MARGIN, ws)
    if dE is not None:
        dl = torch.ones(1, dtype=torch.float32, device=DEV)
        with pytest.raises(ValueError, match=match):
            ops.unsup_loss_bwd(E, pd, dims, ws, dl, dE)
    torch.cuda.synchronize()
    assert bool(torch.all(ws == -3.0))
    assert dE is None or bool(torch.all(dE == -3.0))


def _filled(*shape):
    return torch.full(shape, -3.0, dtype=torch.float32, device=DEV)


def test_refusals():
    _E, _lists, plan, dims = C.base(64)
    Mn, P, N, Un = dims
    need = ops.unsup_loss_workspace(Mn, P, N, DEV).numel()
    for D in (2, 6, 1028):                                   # rows 16-byte aligned, so the width alone is refused
        ld = (D + 3) // 4 * 4
        E = torch.zeros(Un, ld, dtype=torch.float32, device=DEV)[:, :D]
        assert E.data_ptr() % 16 == 0 and E.stride(0) % 4 == 0
        _refused(E, _filled(need), "multiple of 4", dims, plan, dE=_filled(Un, ld)[:, :D])
    # lde % 4 != 0
    E = torch.zeros(Un, 66, dtype=torch.float32, device=DEV)[:, :64]
    _refused(E, _filled(need), "embedding rows must be 16-byte aligned", dims, plan, dE=_filled(Un, 64))
    # a base pointer 4 bytes off 16-byte alignment
    E = torch.zeros(Un * 64 + 1, dtype=torch.float32, device=DEV)[1:].view(Un, 64)
    assert E.data_ptr() % 16 == 4 and E.stride(0) == 64
    _refused(E, _filled(need), "embedding rows must be 16-byte aligned", dims, plan, dE=_filled(Un, 64))
    # the gradient's rows, with E in order
    E = torch.zeros(Un, 64, dtype=torch.float32, device=DEV)
    dl = torch.ones(1, dtype=torch.float32, device=DEV)
    for dE in (_filled(Un, 66)[:, :64], _filled(Un * 64 + 1)[1:].view(Un, 64)):
        with pytest.raises(ValueError, match="gradient rows must be 16-byte aligned"):
            ops.unsup_loss_bwd(E, _plan_dev(plan), dims, _filled(need), dl, dE)
        torch.cuda.synchronize()
        assert bool(torch.all(dE == -3.0))
    # a misaligned workspace
    ws = _filled(need + 4)[1:need + 1]
    assert ws.data_ptr() % 16 == 4
    _refused(E, ws, "workspace must be 16-byte aligned", dims, plan)


@pytest.mark.parametrize("kind", ["sage", "margin"])
def test_autograd_function_makes_a_misaligned_view_contiguous(kind):
    D = 64
    E, _lists, plan, dims = C.base(D)
    kid, pd = C.KIND_ID[kind], _plan_dev(plan)
    out = []
    src = torch.from_numpy(np.array(E)).to(DEV)
    off = torch.zeros(C.U * 66 + 1, dtype=torch.float32, device=DEV)[1:].view(C.U, 66)[:, :D]
    off.copy_(src)
    assert off.data_ptr() % 16 == 4 and off.stride(0) % 4 != 0
    for emb in (src, off):
        emb = emb.detach().requires_grad_(True)
        loss = unsup._UnsupLossFn.apply(emb, pd, dims, kid, C.Q, C.MARGIN)
        loss.backward()
        out.append((loss.detach().cpu().numpy().tobytes(), emb.grad.contiguous().cpu().numpy().tobytes()))
    assert out[0] == out[1]
    # and the bits are the wrappers' on the contiguous input
    want = _run(E, plan, dims, kind, C.MARGIN)
    assert out[0] == (want["loss"].tobytes(), want["dE"].tobytes())


# ------------------------------------------------------- (f) the class off 128
@pytest.mark.parametrize("D", sorted(C.CLASS_SEED))
@pytest.mark.parametrize("kind", ["sage", "margin"])
def test_class_losses_off_128(D, kind):
    ul = _replay(C.CLASS_TAG)
    pos_lists, neg_lists, n_rows = C.lists_of_object(ul)
    E = C.class_embedding(D, n_rows, UC.extend_file())
    ref = C.reference(E, (pos_lists, neg_lists), kind, float(ul.Q), float(ul.MARGIN), torch.float64)
    tor = C.reference(E, (pos_lists, neg_lists), kind, float(ul.Q), float(ul.MARGIN), torch.float32)
    emb = torch.from_numpy(np.array(E)).to(DEV).requires_grad_(True)
    loss = (ul.get_loss_sage if kind == "sage" else ul.get_loss_margin)(emb, np.asarray(ul.unique_nodes_batch))
    assert loss.shape == (() if kind == "sage" else (1,))
    loss.sum().backward()
    failures = []
    try:
        check_rule(f"class {D} {kind} dE", emb.grad.cpu().numpy(), ref["dE"].reshape(-1), tor["dE"].reshape(-1))
    except AssertionError as e:
        failures.append(str(e))
    e_score = float(np.max(np.abs(tor["score"] - ref["score"])))
    err = abs(float(loss.detach().reshape(-1)[0]) - ref["loss"])
    bound = 4.0 * e_score + 2.0 ** -23 * abs(ref["loss"])
    msg = f"class {D} {kind} loss: err {err:.3e}, e_torch(score) {e_score:.3e}, bound {bound:.3e}"
    print(msg)
    if not err <= bound:
        failures.append(msg)
    assert not failures, "\n".join(failures)
