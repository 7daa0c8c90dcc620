"""Counter-based (Philox) device sampler (graphsage-pytorch_amd/
csrc/kernels/fsample.hip) on the MI355X:

* every pack, its layout and sizes equal the host mirror's (fast_sample) bit
  for bit — the host mirror is itself held to a plain-Python statement of the
  rule in test_fast_sampler_host.py;
* the native forward / backward over such a pack against the dense-mask oracle
  over the hops decoded from that pack;
* the runner, the embedder and the GraphSage module in this mode."""
import ctypes
import importlib
import os
import random

import numpy as np
import pytest
import torch

import oracle
from tests import fast_cases as fc
from tests.golden.synth import uniform_features

pytestmark = pytest.mark.gpu

gs = importlib.import_module("graphsage-pytorch_amd")
S = importlib.import_module("graphsage-pytorch_amd.sampler")
L = importlib.import_module("graphsage-pytorch_amd._lib")
models = importlib.import_module("graphsage-pytorch_amd.models")
train = importlib.import_module("graphsage-pytorch_amd.train")
DEV = torch.device("cuda", 0)
GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def graph():
    return fc.special_graph()


@pytest.fixture(scope="module")
def rmat():
    g = np.load(os.path.join(GOLD, "graphs.npz"))
    n = int(g["rmat_n"][0])
    return gs.CSRGraph.from_pairs(g["rmat_src"], g["rmat_dst"], n), n


def assert_same(dev, host, n_roots, what=""):
    """Device run against host mirror: sizes, offsets, used, every field and the roots."""
    pack, dsz, doff, dused = dev
    ref, sizes, offs, used = host
    assert dused == used, what
    np.testing.assert_array_equal(dsz, sizes, err_msg=what)
    np.testing.assert_array_equal(doff, offs, err_msg=what)
    got, ref = pack[:used].cpu().numpy(), ref[:used].numpy()
    for fd, fh in zip(fc.fields(got, sizes, offs), fc.fields(ref, sizes, offs)):
        for name in fh:
            np.testing.assert_array_equal(fd[name], fh[name], err_msg=f"{what} {name}")
    np.testing.assert_array_equal(got[used - n_roots:], ref[used - n_roots:], err_msg=f"{what} roots")


@pytest.mark.parametrize("gcn", [False, True])
@pytest.mark.parametrize("fanouts", fc.FANOUT_SETS, ids=lambda f: "-".join(map(str, f)))
def test_device_matches_host(graph, fanouts, gcn):
    """Every case of the CPU structural list, on one handle: the batches run
    back to back, then the first one again (stale bitmap or cursor state)."""
    ds = S.FastDeviceSampler(graph, fanouts, 130, 824, gcn=gcn)
    order = [1, 7, 64, 130, 1, 7]
    for i, B in enumerate(order):
        roots = fc.roots_for(B)
        bi = 3 * B + len(fanouts)
        dev = ds.run(roots, bi)
        assert_same(dev, S.fast_sample(graph, 824, bi, roots, fanouts, gcn=gcn), B, f"run {i} B={B}")
    ds.set_seed(2 ** 40 + 5)  # high seed and batch-index words
    roots = fc.roots_for(64)
    assert_same(ds.run(roots, 2 ** 33 + 1), S.fast_sample(graph, 2 ** 40 + 5, 2 ** 33 + 1, roots, fanouts, gcn=gcn),
                64, "high words")


@pytest.mark.parametrize("gcn", [False, True])
def test_device_saturating_frontier(gcn):
    G = fc.dense_graph(40)
    roots = np.array([3, 17, 17, 39], np.int64)
    fanouts = [10, 10, 4]
    ds = S.FastDeviceSampler(G, fanouts, 4, 9, gcn=gcn)
    for _ in range(2):
        dev = ds.run(roots, 2)
        assert dev[1][1, 2] == 40
        assert_same(dev, S.fast_sample(G, 9, 2, roots, fanouts, gcn=gcn), 4)


def test_device_rmat_512(rmat):
    G, n = rmat
    cand = np.nonzero(G.degrees() > 0)[0]
    rs = np.random.RandomState(2)
    ds = S.FastDeviceSampler(G, [25, 10], 512, 11)
    for b in range(2):
        roots = rs.choice(cand, 512, replace=len(cand) < 512).astype(np.int64)
        assert_same(ds.run(roots, b), S.fast_sample(G, 11, b, roots, [25, 10]), 512, f"batch {b}")


def test_device_big_union_matches_host():
    """B = 4096, fanouts [10, 5] on a scale-16 R-MAT graph: a hop-1 frontier of
    tens of thousands of nodes (many scan blocks, many words of the bitmap)
    and transposed lists longer than a wave (hub sources: tlong_kernel)."""
    src, dst = gs.rmat_pairs(16, 1_000_000, seed=7, n_threads=8)
    G = gs.CSRGraph.from_pairs(src, dst, 1 << 16, n_threads=8)
    cand = np.nonzero(G.degrees() > 0)[0]
    roots = np.random.RandomState(3).choice(cand, 4096, replace=False).astype(np.int64)
    ds = S.FastDeviceSampler(G, [10, 5], 4096, 17)
    host = S.fast_sample(G, 17, 5, roots, [10, 5])
    sizes = host[1]
    # the size test_device_big_union_matches_host asks for (a union past one workgroup's LDS table); here
    # it is a dozen scan blocks of destinations and all 2048 words of the bitmap
    assert sizes[0, 2] > 6554
    f0 = fc.fields(host[0].numpy(), sizes, host[2])[0]
    assert np.diff(f0["tptr"]).max() > 64  # a long transposed list
    for _ in range(2):
        assert_same(ds.run(roots, 5), host, 4096)
    # three hops: the middle hop's bound (24576 destinations) is past the one-launch scan (15360 values),
    # so its neighbour-count scan takes the three-kernel form too, and F2 is most of the graph
    ds3 = S.FastDeviceSampler(G, [5, 4, 3], 4096, 17, gcn=True)
    host3 = S.fast_sample(G, 17, 6, roots, [5, 4, 3], gcn=True)
    assert host3[1][1, 0] > 6554
    assert_same(ds3.run(roots, 6), host3, 4096)


def test_fail_empty_and_bad_root(graph):
    ds = S.FastDeviceSampler(graph, [5, 4], 16, 0, fail_empty=True)
    with pytest.raises(IndexError):
        ds.run(np.array([fc.ISOLATED, 8], np.int64), 0)
    roots = np.array([8, 9], np.int64)
    assert_same(ds.run(roots, 0), S.fast_sample(graph, 0, 0, roots, [5, 4], fail_empty=True), 2)  # handle still good
    with pytest.raises(IndexError):
        ds.run(torch.tensor([fc.N, 3], dtype=torch.int32), 0)  # id outside the graph: reported, nothing read
    assert_same(ds.run(roots, 1), S.fast_sample(graph, 0, 1, roots, [5, 4], fail_empty=True), 2)


def test_capacity_and_arguments(graph):
    ds = S.FastDeviceSampler(graph, [25, 10], 16, 3)
    cap = ds.pack_bound(16)
    buf = torch.full((cap + 64,), -7, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError):
        ds.run(np.arange(17, dtype=np.int64), 0, pack=buf[:cap])  # 17 roots on a 16-root handle
    torch.cuda.synchronize()
    assert bool((buf == -7).all())  # nothing written, in or after the pack
    roots = fc.roots_for(16)
    pack, sizes, offs, used = ds.run(roots, 4, pack=buf[:cap])
    torch.cuda.synchronize()
    assert used <= cap and bool((buf[cap:] == -7).all())  # the words after cap untouched
    with pytest.raises(ValueError):
        ds.run(roots, 0, pack=buf[:cap - 8])  # below the bound
    with pytest.raises(ValueError):
        ds.run(roots, 0, pack=torch.zeros(cap, dtype=torch.int32))  # host memory
    # a fast handle has no MT19937 stream and no plain run
    lib = L.lib()
    mt = np.zeros(624, np.uint32)
    pos = ctypes.c_int64()
    r32 = torch.zeros(4, dtype=torch.int32, device=DEV)
    assert lib.gs_dsampler_set_rng(ds._h, mt.ctypes.data, 0, None) == L.GS_EINVAL
    assert lib.gs_dsampler_get_rng(ds._h, mt.ctypes.data, ctypes.byref(pos), None) == L.GS_EINVAL
    assert lib.gs_dsampler_words(ds._h, 4, mt.ctypes.data, None) == L.GS_EINVAL
    assert lib.gs_dsampler_run(ds._h, r32.data_ptr(), 4, buf.data_ptr(), cap, None) == L.GS_EINVAL
    # and a bit-exact handle has no seed
    plain = S.DeviceSampler(graph, [10], 8)
    assert lib.gs_dsampler_set_seed(plain._h, 1) == L.GS_EINVAL
    for bad in ([0, 5], [33], [None]):
        with pytest.raises(ValueError):
            S.FastDeviceSampler(graph, bad, 8, 0)


@pytest.mark.parametrize("gcn", [False, True])
@pytest.mark.parametrize("agg", ["MEAN", "MAX"])
@pytest.mark.parametrize("fanouts", [(5, 3), (25, 10)], ids=["5-3", "25-10"])
def test_forward_backward_vs_oracle(rmat, fanouts, agg, gcn):
    """NativeTrainer.forward and forward_backward over a fast pack (F = 32,
    H = 128, B = 16) against oracle.forward_dense + nll_loss autograd over the
    hops decoded from that pack: embeddings and the four gradients at 1e-5."""
    G, n = rmat
    F, H, C, B, seed, bi = 32, 128, 7, 16, 5, 3
    X = torch.from_numpy(uniform_features(5, n, F))
    labels = torch.from_numpy((np.arange(n) % C).astype(np.int32))
    roots = np.nonzero(G.degrees())[0][::5][:B].astype(np.int64)
    tr = train.NativeTrainer(G, X.to(DEV), labels.to(DEV), C, hidden=H, fanouts=fanouts, agg_func=agg, gcn=gcn,
                             seed=824)
    ds = S.FastDeviceSampler(G, list(fanouts), B, seed, gcn=gcn, fail_empty=agg == "MAX")
    pack, sizes, offs, used = ds.run(roots, bi)
    dsm = models.DeviceSample(train.SampleInfo(2, sizes.reshape(-1), offs, used, B), DEV, buf=pack[:used])
    emb = torch.empty(B, H, dtype=torch.float32, device=DEV)
    tr.forward(dsm, emb)
    loss = tr.forward_backward(dsm, pack[used - B:used])
    torch.cuda.synchronize()
    sage_w, cw, cb = train.reference_init(2, F, H, C, gcn, 824)
    W = [w.clone().requires_grad_(True) for w in sage_w]
    cw, cb = cw.clone().requires_grad_(True), cb.clone().requires_grad_(True)
    hops = fc.oracle_hops(G, pack[:used].cpu().numpy(), sizes, offs, roots, list(fanouts), seed, bi)
    ref = oracle.forward_dense(hops, X, W, agg, gcn)
    logp = torch.log_softmax(ref.mm(cw.t()) + cb, 1)
    ref_loss = oracle.nll_loss(logp, labels[torch.from_numpy(roots)].long())
    ref_loss.backward()
    torch.testing.assert_close(emb.cpu(), ref.detach(), atol=1e-5, rtol=1e-5)
    assert abs(float(loss) - float(ref_loss.detach())) < 1e-5
    g_ref = torch.cat([p.grad.reshape(-1) for p in W + [cw, cb]])
    g = tr.p.grads.cpu()
    assert g.numel() == g_ref.numel()
    torch.testing.assert_close(g, g_ref, atol=1e-5, rtol=1e-5)


def _runner_case(rmat, agg="MEAN", gcn=False):
    G, n = rmat
    X = torch.from_numpy(uniform_features(5, n, 256)).to(DEV)
    labels = torch.from_numpy((np.arange(n) % 16).astype(np.int32)).to(DEV)
    batches = list(train.rank_batches(np.nonzero(G.degrees())[0], 48, 0, 1, 9))[:6]
    mk = lambda: train.NativeTrainer(G, X, labels, 16, fanouts=(25, 10), agg_func=agg, gcn=gcn, seed=824)  # noqa: E731
    return G, batches, mk


@pytest.mark.parametrize("agg,gcn", [("MEAN", False), ("MAX", False), ("MEAN", True)])
def test_runner_matches_python_loop(rmat, agg, gcn):
    """Runner(sampler="device-fast") over 6 steps: bitwise the loss and
    parameters of a Python loop of FastDeviceSampler.run(roots_b, b) +
    trainer.step; S = 1 and S = 3 streams bitwise equal to each other."""
    G, batches, mk = _runner_case(rmat, agg, gcn)
    seed = 77
    a = mk()
    ds = S.FastDeviceSampler(G, [25, 10], 48, seed, gcn=gcn, fail_empty=agg == "MAX")
    for b, roots in enumerate(batches):
        pack, sizes, offs, used = ds.run(roots, b)
        dsm = models.DeviceSample(train.SampleInfo(2, sizes.reshape(-1), offs, used, 48), DEV, buf=pack[:used])
        a.step(dsm, pack[used - 48:used])
    torch.cuda.synchronize()
    rngs = [gs.RNG(1), gs.RNG(2), gs.RNG(3)]
    before = [r.getstate() for r in rngs]
    for streams in (1, rngs):
        t = mk()
        r = train.Runner(t, G, batches, streams, [25, 10], gcn=gcn, fail_empty=agg == "MAX", depth=2,
                         sampler="device-fast", seed=seed)
        r.run(2)
        r.run(len(batches) - 2)
        torch.cuda.synchronize()
        assert r.stats()["steps"] == len(batches)
        r.sync_rngs()  # a no-op in this mode
        r.close()
        assert torch.equal(a.p.params, t.p.params)
        assert float(a.loss) == float(t.loss)
    for r, (mt, pos) in zip(rngs, before):  # the rngs only counted the streams
        mt2, pos2 = r.getstate()
        assert pos2 == pos and np.array_equal(mt2, mt)
    with pytest.raises(ValueError):
        out = torch.zeros(len(batches) * 48, 128, device=DEV)
        train.Runner(mk(), G, batches, 1, [25, 10], sampler="device-fast", embed_out=out, merge=2)


def test_embedder_matches_per_batch_forward(rmat):
    G, n = rmat
    X = torch.from_numpy(uniform_features(5, n, 64)).to(DEV)
    W = [w.to(DEV) for w in train.reference_init(2, 64, 128, 4, False, 3)[0]]
    nodes = np.arange(0, 5 * 40 + 13, dtype=np.int64) * 7 % n  # 5 full batches and a partial one
    seed, fan = 21, [10, 5]
    emb = train.Embedder(G, X, W, fan, sampler="device-fast", seed=seed).embed(nodes, 40, 2)
    tr = train.NativeTrainer(G, X, torch.zeros(1, dtype=torch.int32), 1, hidden=128, fanouts=fan,
                             weights=(W, torch.zeros(1, 128, device=DEV), torch.zeros(1, device=DEV)))
    ds = S.FastDeviceSampler(G, fan, 40, seed)
    for i, lo in enumerate(range(0, len(nodes), 40)):
        roots = nodes[lo:lo + 40]
        pack, sizes, offs, used = ds.run(roots, i)
        dsm = models.DeviceSample(train.SampleInfo(2, sizes.reshape(-1), offs, used, len(roots)), DEV,
                                  buf=pack[:used])
        ref = torch.empty(len(roots), 128, device=DEV)
        tr.forward(dsm, ref)
        assert torch.equal(emb[lo:lo + len(roots)], ref), i


@pytest.mark.parametrize("agg", ["MEAN", "MAX"])
def test_graphsage_module_fast(rmat, agg):
    G, n = rmat
    fan, seed = [25, 10], 9
    X = torch.from_numpy(uniform_features(3, n, 64))
    torch.manual_seed(1)
    m = models.GraphSage(2, 64, 128, X.to(DEV), G, DEV, agg_func=agg, fanouts=fan, device_sampler="fast",
                         sampler_seed=seed).to(DEV)
    roots = np.nonzero(G.degrees())[0][::3][:100].tolist()
    random.seed(4)
    state = random.getstate()
    e0 = m(roots)
    e1 = m(roots)       # batch index 1: another sample
    assert m.batch_index == 2
    m.batch_index = 0
    e2 = m(roots)       # the same seed and index: the same output
    assert random.getstate() == state  # the global stream is neither read nor advanced
    assert torch.equal(e0, e2) and not torch.equal(e0, e1)
    host = S.fast_sample(G, seed, 0, roots, fan)
    hops = fc.oracle_hops(G, host[0].numpy(), host[1], host[2], roots, fan, seed, 0)
    W = [getattr(m, f"sage_layer{i}").weight.detach().cpu() for i in (1, 2)]
    ref = oracle.forward_dense(hops, X, W, agg, False)
    torch.testing.assert_close(e0.detach().cpu(), ref, atol=1e-5, rtol=1e-5)
    with pytest.raises(ValueError):
        models.GraphSage(2, 64, 128, X.to(DEV), G, DEV, fanouts=[25, None], device_sampler="fast")
