"""The runner's pack path: every pinned slot has a device twin, the sampler
thread that finished a pack copies it there (hipMemcpyAsync on the runner's
copy stream, waited for by that thread before it offers the slot), the driver
gathers from the twin, and a slot goes back to its sampler when the step that
read the twin is done.

Nothing arithmetic depends on that path, so every check is bitwise: against
the Python loop over the same sampler streams, against an uninterrupted run,
and (Embedder) merge = 2 against merge = 1.  Shapes are the smallest the
runner tests use: the tiny R-MAT graph, F = 32, hidden 128, B = 16, fanouts
(5, 3), 2 layers, fp32 MEAN.  Step counts are 5 x streams x depth, so every
slot and its twin is reused five times; depth 1 leaves a sampler no free slot
while the driver waits for it (the recycle-while-blocked path)."""
import functools
import importlib
import os

import numpy as np
import pytest
import torch

from tests.golden.synth import uniform_features

pytestmark = pytest.mark.gpu

train = importlib.import_module("graphsage-pytorch_amd.train")
DEV = torch.device("cuda", 0)
G = os.path.join(os.path.dirname(__file__), "golden")
F, H, C, B, SEED, FAN = 32, 128, 5, 16, 824, [5, 3]


@functools.lru_cache(maxsize=None)
def _world():
    gs = importlib.import_module("graphsage-pytorch_amd")
    g = np.load(os.path.join(G, "graphs.npz"))
    n = int(g["rmat_n"][0])
    graph = gs.CSRGraph.from_pairs(g["rmat_src"], g["rmat_dst"], n)
    X = torch.from_numpy(uniform_features(3, n, F)).to(DEV)
    labels = torch.from_numpy((np.arange(n) % C).astype(np.int32)).to(DEV)
    cands = np.nonzero(graph.degrees() > 0)[0]
    return graph, X, labels, cands


def _batches(n_steps):
    """n_steps batches of B roots: permutations of the candidates, one after another."""
    cands = _world()[3]
    rs = np.random.RandomState(9)
    ids = np.concatenate([rs.permutation(cands) for _ in range(-(-n_steps * B // len(cands)))])
    return [ids[i * B:(i + 1) * B].astype(np.int64) for i in range(n_steps)]


def _trainer():
    graph, X, labels, _ = _world()
    return train.NativeTrainer(graph, X, labels, C, hidden=H, fanouts=FAN, seed=SEED)


def _rngs(S):
    return [train.make_rng(11, 0, w) for w in range(S)]


def _state(t):
    torch.cuda.synchronize()
    return t.p.params.clone(), t.p.grads.clone(), float(t.loss)


@functools.lru_cache(maxsize=None)
def _python_loop(S, n_steps):
    """(parameters, gradients, last loss) of the Python loop over S sampler streams."""
    graph = _world()[0]
    t = _trainer()
    pf = train.Prefetcher(graph, None, _batches(n_steps), FAN, False, DEV, rngs=_rngs(S))
    for _ in range(n_steps):
        ds, roots_dev, _info = pf.next()
        t.forward_backward(ds, roots_dev)
        t.apply_update()
    pf.close()
    return _state(t)


def _equal(got, want):
    assert torch.equal(got[0], want[0])  # parameters
    assert torch.equal(got[1], want[1])  # gradients
    assert got[2] == want[2]             # loss


@pytest.mark.parametrize("S,depth", [(1, 1), (1, 2), (3, 1), (3, 4)])
def test_runner_equals_python_loop(gs, S, depth):
    n_steps = 5 * S * depth
    t = _trainer()
    r = train.Runner(t, _world()[0], _batches(n_steps), _rngs(S), FAN, depth=depth)
    r.run(n_steps)
    got = _state(t)
    st = r.stats()
    r.close()
    assert st["steps"] == n_steps
    _equal(got, _python_loop(S, n_steps))


def test_hold_and_release_in_two_parts(gs):
    """hold=True, as the bench measures: release and run a first part, then the
    rest; the result is the uninterrupted run's."""
    S, depth, n_steps, first = 2, 2, 14, 5
    t = _trainer()
    r = train.Runner(t, _world()[0], _batches(n_steps), _rngs(S), FAN, depth=depth, hold=True)
    assert r.progress() == (0, 0)
    r.release(first)
    r.run(first)
    torch.cuda.synchronize()
    assert r.progress()[1] == first and r.progress()[0] <= first
    r.release(n_steps)
    r.run(n_steps - first)
    got = _state(t)
    r.close()
    u = _trainer()
    r = train.Runner(u, _world()[0], _batches(n_steps), _rngs(S), FAN, depth=depth)
    r.run(n_steps)
    want = _state(u)
    r.close()
    _equal(got, want)
    _equal(got, _python_loop(S, n_steps))


def test_several_run_calls_on_one_runner(gs):
    """1 + 2 + 4 steps: each call applies its last pending update and leaves
    its last steps' slots to be handed back by the next call."""
    S, depth = 2, 1
    t = _trainer()
    r = train.Runner(t, _world()[0], _batches(7), _rngs(S), FAN, depth=depth)
    for k in (1, 2, 4):
        r.run(k)
    got = _state(t)
    r.close()
    _equal(got, _python_loop(S, 7))


def test_embedder_merge_2_equals_merge_1(gs):
    """Forward-only steps of two batches in one pack (one copy per step, a twin
    of twice the size) against one batch per step, on one sampler stream."""
    graph, X, _, cands = _world()
    W = [w.to(DEV) for w in train.reference_init(2, F, H, C, False, SEED)[0]]
    nodes = np.concatenate(_batches(9))[:9 * B - 5]  # 8 full batches and a partial one
    out = []
    for merge in (1, 2):
        emb = train.Embedder(graph, X, W, FAN, depth=2, merge=merge).embed(nodes, B, [gs.RNG(7)])
        torch.cuda.synchronize()
        out.append(emb.clone())
    assert torch.isfinite(out[0]).all()
    assert torch.equal(out[0], out[1])


def test_sampling_error_is_reported_at_its_step(gs):
    """MAX with fail_empty: node 0 links only to itself, so the batch that
    holds it has an empty neighbourhood.  Its sampler thread copies nothing
    for it; the driver reports it at the step that reaches it, the steps
    before it ran, and the runner closes cleanly."""
    n = 24
    ring = np.arange(1, n)
    src = np.concatenate([[0], ring])
    dst = np.concatenate([[0], np.where(ring + 1 < n, ring + 1, 1)])
    graph = gs.CSRGraph.from_pairs(src.astype(np.int64), dst.astype(np.int64), n)
    X = torch.from_numpy(uniform_features(3, n, F)).to(DEV)
    labels = torch.from_numpy((np.arange(n) % C).astype(np.int32)).to(DEV)
    # the look-ahead takes batch i + 1 under step i, so the bad batch sits two past the first call's last step
    batches = [np.array(b, np.int64) for b in ([1, 2, 3, 4], [5, 6, 7, 8], [12, 13, 14, 15], [9, 0, 10, 11],
                                               [16, 17, 18, 19])]
    t = train.NativeTrainer(graph, X, labels, C, hidden=H, fanouts=FAN, agg_func="MAX", seed=SEED)
    r = train.Runner(t, graph, batches, [train.make_rng(11, 0, 0)], FAN, fail_empty=True, depth=2)
    r.run(2)
    torch.cuda.synchronize()
    assert r.stats()["steps"] == 2 and np.isfinite(float(t.loss))
    with pytest.raises(IndexError):
        r.run(2)  # at step 3, or already when step 2 looks ahead to it
    assert r.stats()["steps"] in (2, 3)
    r.close()
    torch.cuda.synchronize()
