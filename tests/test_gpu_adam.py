"""The fused clip + Adam/AdamW update on the MI355X: the operator on both
code paths (float4 and scalar), the trainer step by step, the bf16 W1 shadow,
the runner against the Python loop, two ranks, checkpoint / resume, and SGD
left as it was.

Tolerance of every numeric case (adam_cases.check_rule): the reference is
reference_adamw in float64 from the same fp32 inputs; with e_torch the largest
elementwise error of torch.optim.AdamW in fp32 on the CPU against it, the
kernel stays within 4 * e_torch + 2^-23 * max|x|, separately for p, m and v
(and the clipped gradient).  Hyper-parameters are rounded to fp32 first, the
precision the C ABI carries them in (adam_cases.f32).
"""
import importlib
import os

import numpy as np
import pytest
import torch

from tests.adam_cases import check_rule, f32, reference_adamw, torch_adamw
from tests.golden.synth import uniform_features

pytestmark = pytest.mark.gpu

models = importlib.import_module("graphsage-pytorch_amd.models")
train = importlib.import_module("graphsage-pytorch_amd.train")
ops = importlib.import_module("graphsage-pytorch_amd.hip_ops")
DEV = torch.device("cuda", 0)
G = os.path.join(os.path.dirname(__file__), "golden")
INF = float("inf")
LR, BETAS, EPS = f32(0.01), (f32(0.9), f32(0.999)), f32(1e-8)
WD = f32(0.01)
FAN, B, F, H = [25, 10], 48, 256, 128


# ------------------------------------------------------------------ operator
GOFF_VEC = [0, 262144, 524288, 600000]  # float4 path; 150000 quads > 512 blocks x 256 threads
GOFF_SCALAR = [0, 4097, 9001, 600001]   # scalar path; borders no multiple of 4 or 64
_DATA = {}


def _op_data(n):
    """Seeded fp32 state of n elements: parameters, a small gradient (every
    group's norm below 5), and moments of the gradient's scale."""
    if n not in _DATA:
        rs = np.random.RandomState(n % 1000)
        _DATA[n] = (rs.uniform(-1, 1, n).astype(np.float32), (rs.standard_normal(n) * 1e-3).astype(np.float32),
                    (rs.standard_normal(n) * 1e-3).astype(np.float32),
                    (rs.uniform(0, 1, n) * 1e-6).astype(np.float32))
    return _DATA[n]


def _op_state(n, step):
    p, g, m, v = _op_data(n)
    if step == 1:  # a first update starts from zero moments
        m, v = np.zeros_like(m), np.zeros_like(v)
    return p, g, m, v


def _run_op(goff, state, step, max_norm, wd, scale, shift=0):
    """hip_ops.clip_adam on device copies of `state`; shift = 1 places every
    buffer one float past a 16-byte boundary (forces the scalar kernel)."""
    n = goff[-1]
    bufs = []
    for x in state:
        t = torch.empty(n + shift, dtype=torch.float32, device=DEV)[shift:]
        t.copy_(torch.from_numpy(x))
        assert (t.data_ptr() % 16 == 0) == (shift == 0)
        bufs.append(t)
    p, g, m, v = bufs
    ws = torch.empty(64 * (len(goff) - 1), dtype=torch.float32, device=DEV)
    ops.clip_adam(goff, p, g, m, v, scale, max_norm, LR, BETAS, EPS, wd, step, ws)
    torch.cuda.synchronize()
    return p, g, m, v


CONFIGS = [(wd, scale, step) for wd in (0.0, WD) for scale in (1.0, 0.5) for step in (1, 2, 1000)]


@pytest.mark.parametrize("max_norm", [5.0, f32(1e-3), INF])
@pytest.mark.parametrize("goff", [GOFF_VEC, GOFF_SCALAR], ids=["float4", "scalar"])
def test_clip_adam_operator(gs, goff, max_norm):
    """Case 1 (a), (b): 3 groups of 600000 / 600001 elements, so the
    grid-stride loop runs; max_norm 5 (no clip), 1e-3 (clips) and inf; weight
    decay 0 and 0.01; grad_scale 1 and 0.5; updates 1, 2 and 1000."""
    n = goff[-1]
    worst = {}
    for wd, scale, step in CONFIGS:
        state = _op_state(n, step)
        got = _run_op(goff, state, step, max_norm, wd, scale)
        args = (step, LR, BETAS, EPS, wd, goff, scale, max_norm)
        ref = reference_adamw(*state, *args)
        tor = torch_adamw(*state, *args, torch.float32)
        if max_norm == f32(1e-3):  # it does clip: the gradient left behind is the clipped one
            assert np.max(np.abs(ref[1])) < 0.5 * scale * np.max(np.abs(state[1]))
        for name, a, r, t in zip("pgmv", got, ref, tor):
            ratio = check_rule(f"{name} wd={wd} scale={scale} step={step}", a.cpu().numpy(), r, t)
            worst[name] = max(worst.get(name, 0.0), ratio)
    print("worst err/e_torch:", {k: round(x, 2) for k, x in worst.items()})


@pytest.mark.parametrize("max_norm", [5.0, f32(1e-3), INF])
def test_clip_adam_scalar_equals_float4_bitwise(gs, max_norm):
    """Case 1 (c): the float4 case's data through buffers one float past a
    16-byte boundary takes the scalar kernel; p, m, v and g come out bitwise
    the same (one adam_elem, one fold of the norm partials)."""
    for wd, scale, step in CONFIGS:
        state = _op_state(GOFF_VEC[-1], step)
        a = _run_op(GOFF_VEC, state, step, max_norm, wd, scale)
        b = _run_op(GOFF_VEC, state, step, max_norm, wd, scale, shift=1)
        for name, x, y in zip("pgmv", a, b):
            assert torch.equal(x, y), (name, wd, scale, step)


@pytest.mark.parametrize("goff", [GOFF_VEC, GOFF_SCALAR], ids=["float4", "scalar"])
def test_clip_adam_zero_gradient(gs, goff):
    """Case 2: g = m = v = 0 at the first update: 0 / (0 + eps), p unchanged
    at weight_decay 0, nothing NaN or Inf."""
    n = goff[-1]
    p0 = _op_data(n)[0]
    z = np.zeros(n, np.float32)
    for max_norm in (5.0, INF):
        p, g, m, v = _run_op(goff, (p0, z, z, z), 1, max_norm, 0.0, 1.0)
        assert torch.equal(p.cpu(), torch.from_numpy(p0))
        for x in (g, m, v):
            assert torch.equal(x.cpu(), torch.from_numpy(z))
    p, g, m, v = _run_op(goff, (p0, z, z, z), 1, 5.0, WD, 1.0)  # decay alone
    decayed = torch.from_numpy(p0) * torch.tensor(np.float32(1.0 - LR * WD))
    assert torch.equal(p.cpu(), decayed) and bool(torch.isfinite(p).all())


# ------------------------------------------------------------------- trainer
@pytest.fixture(scope="module")
def wl(gs):
    """The tiny R-MAT workload of the other GPU tests (F = 256, B = 48,
    fanouts (25, 10)) with 8 batches sampled once on one stream."""
    g = np.load(os.path.join(G, "graphs.npz"))
    n = int(g["rmat_n"][0])
    graph = gs.CSRGraph.from_pairs(g["rmat_src"], g["rmat_dst"], n)
    X = torch.from_numpy(uniform_features(5, n, F)).to(DEV)
    batches = list(train.rank_batches(np.nonzero(graph.degrees())[0], B, 0, 1, 9))[:8]
    rng = train.make_rng(11)
    packs = [(models.DeviceSample(gs.sample(graph, rng, r, FAN), DEV), torch.from_numpy(r.astype(np.int32)).to(DEV))
             for r in batches]
    return {"graph": graph, "n": n, "X": X, "batches": batches, "packs": packs}


def _labels(wl, classes):
    return torch.from_numpy((np.arange(wl["n"]) % classes).astype(np.int32)).to(DEV)


def _trainer(wl, classes=16, X=None, max_norm=5.0, **kw):
    kw.setdefault("optimizer", "adam")
    if kw["optimizer"] == "adam":
        kw.setdefault("lr", LR)
        kw.setdefault("betas", BETAS)
        kw.setdefault("eps", EPS)
        kw.setdefault("weight_decay", WD)
    return train.NativeTrainer(wl["graph"], wl["X"] if X is None else X, _labels(wl, classes), classes, hidden=H,
                               fanouts=FAN, max_norm=max_norm, seed=824, **kw)


def _state(tr):
    return tuple(x.detach().cpu().numpy().copy() for x in (tr.p.params, tr.opt_m, tr.opt_v))


def _check_update(tag, tr, before, graw, t, scale, max_norm, wd=WD):
    """p, m, v and the clipped gradient of `tr` against the reference applied
    to (state before, raw gradient, update number t)."""
    args = (t, LR, BETAS, EPS, wd, tr.p.group_off, scale, max_norm)
    ref = reference_adamw(before[0], graw, before[1], before[2], *args)
    tor = torch_adamw(before[0], graw, before[1], before[2], *args, torch.float32)
    got = (tr.p.params, tr.p.grads, tr.opt_m, tr.opt_v)
    return [check_rule(f"{tag} {name}", a.detach().cpu().numpy(), r, x) for name, a, r, x in zip("pgmv", got, ref, tor)]


@pytest.mark.parametrize("max_norm", [5.0, f32(0.05)])
@pytest.mark.parametrize("classes", [16, 7], ids=["float4", "scalar"])
def test_trainer_adam_steps_teacher_forced(gs, wl, classes, max_norm):
    """Case 3: 6 steps, each checked on its own from the state read back
    before it and the raw gradient captured during it; the update count runs
    1..6 (the bias correction at t <= 6 moves the update by tens of percent,
    so a stuck or doubled counter fails the rule).  16 classes: every group
    offset a multiple of 4 (float4 kernel); 7: the total is not (scalar)."""
    tr = _trainer(wl, classes, max_norm=max_norm)
    assert (tr.p.params.numel() % 4 == 0) == (classes == 16)
    lib = gs._lib.lib()
    assert lib.gs_trainer_opt_step(tr._h) == 0
    _emb, graw = tr.capture(6, B)
    for i in range(6):
        before = _state(tr)
        ds, roots = wl["packs"][i]
        tr.step(ds, roots)
        torch.cuda.synchronize()
        assert tr.captured() == i + 1
        assert lib.gs_trainer_opt_step(tr._h) == i + 1
        _check_update(f"C={classes} step {i + 1}", tr, before, graw[i].cpu().numpy(), i + 1, 1.0, max_norm)
    assert tr.optimizer_state()["step"] == 6


def test_adam_keeps_bf16_shadow_current(gs, wl):
    """Case 4: bf16 features.  Inside a runner loop the Adam launch writes the
    bf16 W1 beside the update and the next forward reads it without a cast: two
    runner steps leave bitwise the Python loop's parameters (which casts W1
    before every forward), and a forward afterwards equals the forward of a
    fresh trainer built from the updated weights."""
    X = wl["X"].to(torch.bfloat16)
    a, b = _trainer(wl, X=X), _trainer(wl, X=X)
    for ds, roots in wl["packs"][:2]:
        a.step(ds, roots)
    runner = train.Runner(b, wl["graph"], wl["batches"][:2], [train.make_rng(11)], FAN, depth=2)
    runner.run(2)
    torch.cuda.synchronize()
    runner.close()
    assert torch.equal(a.p.params, b.p.params)
    assert torch.equal(a.opt_m, b.opt_m) and torch.equal(a.opt_v, b.opt_v)
    sd = b.state_dict()
    fresh = _trainer(wl, X=X, weights=([sd["sage_layer1.weight"], sd["sage_layer2.weight"]], sd["layer.0.weight"],
                                       sd["layer.0.bias"]))
    ds, _roots = wl["packs"][5]
    out_b = torch.empty(B, H, dtype=torch.float32, device=DEV)
    out_f = torch.empty_like(out_b)
    b.forward(ds, out_b)
    fresh.forward(ds, out_f)
    torch.cuda.synchronize()
    assert torch.equal(out_b, out_f)


@pytest.mark.parametrize("S", [1, 3])
def test_adam_runner_matches_python_loop(gs, wl, S):
    """Case 5: test_native_runner_matches_python_loop's construction (7
    batches, runs of 3 + 4, S sampler streams) under Adam: parameters, moments
    and loss bitwise, every step counted, and the runner finishes (the Adam
    launch stores the step's done flag)."""
    batches = wl["batches"][:7]
    a, b = _trainer(wl), _trainer(wl)
    pf = train.Prefetcher(wl["graph"], None, batches, FAN, False, DEV,
                          rngs=[train.make_rng(11, 0, w) for w in range(S)])
    for _ in batches:
        ds, roots_dev, _info = pf.next()
        a.step(ds, roots_dev)
    pf.close()
    runner = train.Runner(b, wl["graph"], batches, [train.make_rng(11, 0, w) for w in range(S)], FAN, depth=2)
    runner.run(3)
    runner.run(len(batches) - 3)
    torch.cuda.synchronize()
    assert runner.stats()["steps"] == 7
    runner.close()
    assert torch.equal(a.p.params, b.p.params)
    assert torch.equal(a.opt_m, b.opt_m) and torch.equal(a.opt_v, b.opt_v)
    assert float(a.loss) == float(b.loss)
    assert a.optimizer_state()["step"] == b.optimizer_state()["step"] == 7


def test_adam_never_defers(gs, wl):
    """Case 5, second half: defer(True) reports inactive under Adam and the
    update still applies at once."""
    tr = _trainer(wl)
    assert tr.defer(True) is False
    before = _state(tr)
    _emb, graw = tr.capture(1, B)
    ds, roots = wl["packs"][0]
    tr.forward_backward(ds, roots)
    tr.update(1.0)
    torch.cuda.synchronize()
    assert tr.optimizer_state()["step"] == 1
    assert not torch.equal(tr.p.params.cpu(), torch.from_numpy(before[0]))
    _check_update("no defer", tr, before, graw[0].cpu().numpy(), 1, 1.0, 5.0)
    tr.defer(False)


def test_adam_two_ranks_on_one_gpu(gs, wl):
    """Case 6: two trainers on disjoint batches, the gradients summed as the
    in-place all-reduce leaves them, update(0.5) on both: bitwise equal to
    each other, and within the rule of the reference on the summed gradient
    with scale 0.5 (two steps, each from the state before it)."""
    trs = [_trainer(wl), _trainer(wl)]
    assert not set(wl["batches"][0].tolist()) & set(wl["batches"][1].tolist())
    for i in range(2):
        before = _state(trs[0])
        for r, tr in enumerate(trs):
            ds, roots = wl["packs"][2 * i + r]
            tr.forward_backward(ds, roots)
        gsum = trs[0].p.grads + trs[1].p.grads
        for tr in trs:
            tr.p.grads.copy_(gsum)
            tr.update(0.5)
        torch.cuda.synchronize()
        for x, y in zip(_state(trs[0]), _state(trs[1])):
            assert np.array_equal(x, y)
        assert torch.equal(trs[0].p.grads, trs[1].p.grads)
        _check_update(f"two ranks step {i + 1}", trs[0], before, gsum.cpu().numpy(), i + 1, 0.5, 5.0)


def test_adam_checkpoint_resume_is_bitwise(gs, wl):
    """Case 7: 3 steps, state_dict + optimizer_state saved, a fresh trainer
    loads both and runs 3 more: bitwise the 6 uninterrupted steps."""
    full = _trainer(wl)
    for ds, roots in wl["packs"][:6]:
        full.step(ds, roots)
    first = _trainer(wl)
    for ds, roots in wl["packs"][:3]:
        first.step(ds, roots)
    torch.cuda.synchronize()
    sd, opt = first.state_dict(), first.optimizer_state()
    assert opt["step"] == 3 and opt["m"].data_ptr() != first.opt_m.data_ptr()
    del first
    second = _trainer(wl)
    second.load_state_dict(sd)
    second.load_optimizer_state(opt)
    assert second.optimizer_state()["step"] == 3
    for ds, roots in wl["packs"][3:6]:
        second.step(ds, roots)
    torch.cuda.synchronize()
    assert torch.equal(full.p.params, second.p.params)
    assert torch.equal(full.opt_m, second.opt_m) and torch.equal(full.opt_v, second.opt_v)
    assert second.optimizer_state()["step"] == 6


def test_set_optimizer_refused_while_deferring(gs, wl):
    """gs_trainer_set_option's rule: not while deferring."""
    tr = _trainer(wl, optimizer="sgd")
    assert tr.defer(True) is True
    with pytest.raises(ValueError):
        tr._set_optimizer(0)
    tr.defer(False)
    tr._set_optimizer(0)


def test_sgd_is_untouched(gs, wl):
    """Case 8: optimizer="sgd" and no optimiser argument are the same trainer
    (bitwise after 3 runner steps), and deferral still reports active."""
    out = []
    for kw in ({"optimizer": "sgd"}, {}):
        tr = train.NativeTrainer(wl["graph"], wl["X"], _labels(wl, 16), 16, hidden=H, fanouts=FAN, seed=824, **kw)
        assert tr.opt_m is None and tr.optimizer_state() == {"step": 0, "m": None, "v": None}
        runner = train.Runner(tr, wl["graph"], wl["batches"][:3], [train.make_rng(11)], FAN, depth=2)
        runner.run(3)
        torch.cuda.synchronize()
        runner.close()
        out.append((tr.p.params.clone(), float(tr.loss)))
        assert tr.defer(True) is True
        tr.defer(False)
    assert torch.equal(out[0][0], out[1][0]) and out[0][1] == out[1][1]
