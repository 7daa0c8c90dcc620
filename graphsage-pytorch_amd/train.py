"""Native supervised training step — the reference's per-batch loop
(utils.py:144-191: forward, log_softmax + NLL mean, backward, clip_grad_norm_(5)
per model, SGD lr=0.7) as one stream of HIP kernels over flat parameter and
gradient buffers, fed by a sampler thread, data-parallel over RCCL.

Parameter layout (one flat fp32 buffer, one all-reduce per step):
    [sage_layer1.weight | ... | sage_layerL.weight | layer.0.weight | layer.0.bias]
    groups for clipping: GraphSage = all SageLayer weights, Classification = rest
    (utils.py:185-186 clip each model separately).
Initialisation reproduces the reference modules' init under torch.manual_seed
(SageLayer xavier_uniform_ per layer, then Linear + xavier on its weight).
"""
import ctypes
import os
import queue
import threading
import time

import numpy as np
import torch
import torch.distributed as dist

from . import _lib
from . import hip_ops as ops
from ._lib import check, lib
from .models import Classification, DeviceSample, SageLayer
from .sampler import RNG, sample


def reference_init(num_layers, input_size, hidden, n_classes, gcn=False, seed=824):
    """Weights exactly as main.py:41-58 would create them after torch.manual_seed(seed)."""
    torch.manual_seed(seed)
    layers = [SageLayer(input_size if i == 1 else hidden, hidden, gcn=gcn) for i in range(1, num_layers + 1)]
    cls = Classification(hidden, n_classes)
    return [l.weight.detach().clone() for l in layers], cls.layer[0].weight.detach().clone(), \
        cls.layer[0].bias.detach().clone()


class FlatParams:
    """Contiguous parameter + gradient buffers with named views."""

    def __init__(self, tensors, names, groups, device):
        sizes = [t.numel() for t in tensors]
        self.offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        self.params = torch.empty(int(self.offsets[-1]), dtype=torch.float32, device=device)
        self.grads = torch.zeros_like(self.params)
        self.names = names
        self.shapes = [tuple(t.shape) for t in tensors]
        for i, t in enumerate(tensors):
            self.view(i).copy_(t.to(device=device, dtype=torch.float32))
        self.group_off = np.array([self.offsets[g] for g in groups] + [self.offsets[-1]], np.int64)

    def view(self, i, grad=False):
        buf = self.grads if grad else self.params
        return buf[int(self.offsets[i]):int(self.offsets[i + 1])].view(self.shapes[i])

    def state_dict(self):
        return {n: self.view(i).detach().clone() for i, n in enumerate(self.names)}


_OPTIMIZERS = {"sgd": _lib.GS_OPT_SGD, "adam": _lib.GS_OPT_ADAM}


def optimizer_kind(name):
    """GS_OPT_* of an optimiser name ("sgd" or "adam"); ValueError otherwise."""
    try:
        return _OPTIMIZERS[name]
    except (KeyError, TypeError):
        raise ValueError(f"optimizer must be one of {sorted(_OPTIMIZERS)}, got {name!r}") from None


class NativeTrainer:
    """Fused supervised GraphSAGE step on one GPU (one rank of data parallel).

    `optimizer`: "sgd" (the reference's clip_grad_norm_(max_norm) + SGD(lr)) or
    "adam": the same clip, then torch.optim.AdamW's update with `betas`, `eps`
    and `weight_decay` (Adam at weight_decay = 0) on flat moment buffers beside
    the parameters.  max_norm = float("inf") disables the clip.  Adam updates
    are never deferred into the next step: each is a launch of its own."""

    def __init__(self, graph, features, labels, n_classes, num_layers=2, hidden=128, fanouts=(10, 10),
                 agg_func="MEAN", gcn=False, lr=0.7, max_norm=5.0, seed=824, weights=None, optimizer="sgd",
                 betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        self.optimizer = optimizer
        self._opt_kind = optimizer_kind(optimizer)
        self.betas, self.eps, self.weight_decay = (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)
        if not features.is_cuda:
            raise RuntimeError("NativeTrainer runs on a HIP device")
        self.device = features.device
        self.graph, self.X = graph, features
        self.labels = labels.to(device=self.device, dtype=torch.int32)
        self.L, self.H, self.C = num_layers, hidden, n_classes
        self.fanouts = list(fanouts)
        self.agg, self.gcn, self.lr, self.max_norm = agg_func, gcn, lr, max_norm
        if weights is None:
            weights = reference_init(num_layers, features.shape[1], hidden, n_classes, gcn, seed)
        sage_w, cls_w, cls_b = weights
        names = [f"sage_layer{i}.weight" for i in range(1, num_layers + 1)] + ["layer.0.weight", "layer.0.bias"]
        self.p = FlatParams(list(sage_w) + [cls_w, cls_b], names, [0, num_layers], self.device)
        self.row_ptr, self.col = graph.device_csr(self.device)
        self.loss = torch.zeros(1, dtype=torch.float32, device=self.device)
        self.clip_ws = torch.empty(65 * 2, dtype=torch.float32, device=self.device)
        X = self.X
        cfg = _lib.TrainerConfig(
            n_layers=num_layers, hidden=hidden, n_classes=n_classes, agg=ops.agg_op(agg_func), gcn=int(gcn),
            feat_dtype=_lib.GS_BF16 if X.dtype == torch.bfloat16 else _lib.GS_F32,
            feat_dim=X.shape[1], feat_ld=X.stride(0), X=X.data_ptr(), row_ptr=self.row_ptr.data_ptr(),
            col=self.col.data_ptr(), labels=self.labels.data_ptr(), params=self.p.params.data_ptr(),
            grads=self.p.grads.data_ptr(), lr=lr, max_norm=max_norm)
        h = ctypes.c_void_p()
        check(lib().gs_trainer_create(ctypes.byref(cfg), ctypes.byref(h)))
        self._h = h
        if lib().gs_trainer_n_params(h) != self.p.params.numel():
            raise RuntimeError("flat parameter layout mismatch")
        self._ws = torch.empty(0, dtype=torch.uint8, device=self.device)
        self.opt_m = self.opt_v = None
        if self._opt_kind == _lib.GS_OPT_ADAM:
            self.opt_m = torch.zeros_like(self.p.params)
            self.opt_v = torch.zeros_like(self.p.params)
            self._set_optimizer(0)

    def _set_optimizer(self, step):
        oc = _lib.OptimizerConfig(kind=self._opt_kind, beta1=self.betas[0], beta2=self.betas[1], eps=self.eps,
                                  weight_decay=self.weight_decay, m=_lib.ptr(self.opt_m),
                                  v=_lib.ptr(self.opt_v), step=int(step))
        check(lib().gs_trainer_set_optimizer(self._h, ctypes.byref(oc)))

    def optimizer_state(self):
        """{"step", "m", "v"}: the updates applied so far and clones of the
        flat Adam moments (None under SGD, which keeps no state)."""
        return {"step": int(lib().gs_trainer_opt_step(self._h)),
                "m": None if self.opt_m is None else self.opt_m.detach().clone(),
                "v": None if self.opt_v is None else self.opt_v.detach().clone()}

    def load_optimizer_state(self, state):
        """Restore optimizer_state() of a trainer with the same optimiser and
        parameter layout: with the parameters restored too, training continues
        bit for bit."""
        if self.opt_m is not None:
            if state["m"] is None or state["v"] is None:
                raise ValueError("load_optimizer_state: the state holds no Adam moments")
            if state["m"].numel() != self.opt_m.numel() or state["v"].numel() != self.opt_v.numel():
                raise ValueError("load_optimizer_state: moment size != parameter count")
            self.opt_m.copy_(state["m"].reshape(-1))
            self.opt_v.copy_(state["v"].reshape(-1))
        self._set_optimizer(state["step"])

    def load_state_dict(self, sd):
        """Copy the named parameters of state_dict() back into the flat buffer."""
        for i, n in enumerate(self.p.names):
            self.p.view(i).copy_(sd[n])

    def state_dict(self):
        return self.p.state_dict()

    def weights(self):
        return [self.p.view(i) for i in range(self.L)]

    def forward_backward(self, ds, roots_dev):
        """Loss (device scalar) and gradients into self.p.grads for one batch:
        one native call that issues every kernel of the step on the stream."""
        sizes, offs = ds.native_sizes()
        self._reserve_ws(sizes)
        check(lib().gs_trainer_forward_backward(
            self._h, ds.buf.data_ptr(), sizes.ctypes.data, offs.ctypes.data, roots_dev.data_ptr(),
            roots_dev.numel(), self._ws.data_ptr(), self._ws.numel(), self.loss.data_ptr(),
            _lib.stream_ptr(self.device)))
        return self.loss

    def _reserve_ws(self, sizes):
        need = int(lib().gs_trainer_ws_bytes(self._h, sizes.ctypes.data))
        if need < 0:
            check(_lib.GS_EINVAL)
        if self._ws.numel() < need:
            self._ws = torch.empty(int(need * 1.25) + (1 << 20), dtype=torch.uint8, device=self.device)

    def forward(self, ds, out):
        """GraphSage forward alone (models.py:241-269): the batch's embeddings
        into `out` ([n_roots, hidden] fp32, contiguous); no loss or backward."""
        if not (out.is_contiguous() and out.dtype == torch.float32 and out.shape[1] == self.H):
            raise ValueError("out must be a contiguous fp32 [n_roots, hidden] tensor")
        sizes, offs = ds.native_sizes()
        if out.shape[0] != sizes[0]:
            raise ValueError("out rows != batch roots")
        self._reserve_ws(sizes)
        check(lib().gs_trainer_forward(self._h, ds.buf.data_ptr(), sizes.ctypes.data, offs.ctypes.data,
                                       self._ws.data_ptr(), self._ws.numel(), out.data_ptr(),
                                       _lib.stream_ptr(self.device)))
        return out

    _OPTIONS = {"fused_bwd": _lib.GS_TOPT_FUSED_BWD, "top_launch": _lib.GS_TOPT_TOP_LAUNCH,
                "self_rows": _lib.GS_TOPT_SELF_ROWS, "defer_update": _lib.GS_TOPT_DEFER_UPDATE}

    def set_option(self, name, value):
        """gs_trainer_set_option: switch an alternative of the step (fused_bwd,
        top_launch, self_rows, defer_update; default all on).
        self_rows and defer_update are bitwise the default, and so is
        fused_bwd wherever the top launch does not run; top_launch matches it
        within fp32 rounding of its split-K order, and at the top launch's
        shape (two layers, hidden 128, at most 32 classes, no gcn) fused_bwd
        off turns the top launch off with it, so there it matches the default
        within that rounding too."""
        check(lib().gs_trainer_set_option(self._h, self._OPTIONS[name], int(bool(value))))
        return self

    def capture(self, n_steps, batch):
        """Parity capture (tests): the next n_steps training steps' root
        embeddings [n_steps, batch, hidden] and flat gradients before their
        clip + SGD [n_steps, n_params] (gs_trainer_capture); returns both
        tensors, filled in stream order as the steps run."""
        emb = torch.zeros(n_steps, batch, self.H, dtype=torch.float32, device=self.device)
        grads = torch.zeros(n_steps, self.p.params.numel(), dtype=torch.float32, device=self.device)
        self._cap = (emb, grads)  # kept alive while the trainer may write them
        check(lib().gs_trainer_capture(self._h, emb.data_ptr(), batch * self.H, grads.data_ptr(), n_steps))
        return emb, grads

    def captured(self):
        return int(lib().gs_trainer_captured(self._h))

    def update(self, grad_scale=1.0):
        """gs_trainer_update: grads *= grad_scale, clip per model, SGD — what
        every rank runs after the gradient all-reduce (grad_scale = 1/world)."""
        check(lib().gs_trainer_update(self._h, float(grad_scale), self.clip_ws.data_ptr(),
                                      _lib.stream_ptr(self.device)))

    def defer(self, on):
        """gs_trainer_defer: from now on each update(1/W) after the gradient
        all-reduce is left pending and applied by the next forward (the
        runner's communicator path); defer(False) applies a pending update.
        Returns whether deferring took effect for this step shape."""
        active = ctypes.c_int32(0)
        check(lib().gs_trainer_defer(self._h, int(bool(on)), ctypes.byref(active), _lib.stream_ptr(self.device)))
        return bool(active.value)

    def apply_update(self, world_size=1, group=None):
        """All-reduce (sum) the flat gradients over ranks, then clip + SGD with 1/world."""
        if world_size > 1:
            dist.all_reduce(self.p.grads, group=group)
            check(lib().gs_trainer_update(self._h, 1.0 / world_size, self.clip_ws.data_ptr(),
                                          _lib.stream_ptr(self.device)))
        else:
            check(lib().gs_trainer_update_local(self._h, _lib.stream_ptr(self.device)))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and getattr(_lib, "_lib", None) is not None:  # _lib is None at interpreter exit
            _lib._lib.gs_trainer_destroy(h)
            self._h = None

    def step(self, ds, roots_dev, world_size=1, group=None):
        loss = self.forward_backward(ds, roots_dev)
        self.apply_update(world_size, group)
        return loss


# ------------------------------------------------------------ data pipeline
def rank_batches(candidates, batch_size, rank, world_size, seed, epoch=0):
    """Shuffle candidate roots (numpy, like sklearn.shuffle at utils.py:127) and
    deal batch i*world+rank to this rank: disjoint across ranks, B per rank."""
    perm = np.random.RandomState(seed + epoch).permutation(np.asarray(candidates, np.int64))
    n_steps = len(perm) // (batch_size * world_size)
    for i in range(n_steps):
        b = i * world_size + rank
        yield perm[b * batch_size:(b + 1) * batch_size]


def rank_seed(seed, rank, stream=0):
    """Sampler stream (rank, stream): random.seed(seed + rank + 64 * stream);
    rank 0 stream 0 is exactly the reference's random.seed(seed) stream."""
    return seed + rank + 64 * stream


class SampleInfo:
    """Sizes / pack offsets of one packed batch (what DeviceSample needs)."""

    def __init__(self, n_hops, sizes, offsets, used, n_roots):
        self.n_hops = n_hops
        self._sizes = [tuple(int(x) for x in sizes[4 * j:4 * j + 4]) for j in range(n_hops)]
        self.offsets = offsets.reshape(_lib.GS_MAX_HOPS, _lib.GS_PK_NFIELDS)[:n_hops].tolist()
        self.pack_total = int(used) - n_roots
        self.n_roots = n_roots

    def sizes(self, j):
        return self._sizes[j - 1]


class _SamplerWorker:
    """One RNG stream: samples its batches in order on a host thread (the GIL
    is released for the whole native sample+pack call) into a ring of pinned
    buffers; the consumer copies each to the device and recycles the slot."""

    def __init__(self, graph, rng, batches, fanouts, flags, depth):
        self.graph, self.rng, self.batches, self.flags = graph, rng, batches, flags
        self.fan = np.array([(-1 if k is None else int(k)) for k in fanouts], np.int32)
        self.q = queue.Queue(maxsize=depth)
        self.slots = [None] * (depth + 1)
        self.events = [None] * (depth + 1)
        self.free = queue.Queue()
        for i in range(depth + 1):
            self.free.put(i)
        self.sample_s = []
        self.stop = False
        self.t = threading.Thread(target=self._run, daemon=True)
        self.t.start()

    def _run(self):
        L = len(self.fan)
        try:
            for roots in self.batches:
                if self.stop:
                    break
                roots = np.ascontiguousarray(roots, dtype=np.int64)
                bound = int(lib().gs_sample_pack_bound(self.graph.handle, len(roots), self.fan.ctypes.data, L))
                slot = self.free.get()
                ev = self.events[slot]
                if ev is not None:
                    ev.synchronize()  # the previous H2D copy out of this slot is done
                buf = self.slots[slot]
                if buf is None or buf.numel() < bound:
                    buf = self.slots[slot] = torch.empty(bound, dtype=torch.int32, pin_memory=True)
                sizes = np.empty(4 * L, np.int64)
                offs = np.empty(_lib.GS_MAX_HOPS * _lib.GS_PK_NFIELDS, np.int64)
                used = ctypes.c_int64()
                t0 = time.perf_counter()
                check(lib().gs_sample_pack_run(self.graph.handle, self.rng._h, roots.ctypes.data, len(roots),
                                               self.fan.ctypes.data, L, self.flags, buf.data_ptr(), buf.numel(),
                                               sizes.ctypes.data, offs.ctypes.data, ctypes.byref(used)))
                self.sample_s.append(time.perf_counter() - t0)
                self.q.put((slot, SampleInfo(L, sizes, offs, used.value, len(roots)), offs, sizes))
        except BaseException as e:  # surface sampler errors in the consumer
            self.q.put(e)
        self.q.put(None)


class Prefetcher:
    """Host sampling pipelined with the GPU.  With one RNG (the default) the
    batches are sampled in order from that single stream — exactly the
    reference's sequence.  With `rngs` = S streams, stream w samples batches
    w, w+S, ... (each stream individually bit-exact with the reference seeded
    the same way, like S data-parallel ranks sharing this GPU); batches are
    still consumed in order."""

    def __init__(self, graph, rng, batches, fanouts, gcn, device, depth=3, rngs=None, fail_empty=False):
        self.device = torch.device(device)
        rngs = list(rngs) if rngs is not None else [rng]
        S = len(rngs)
        batches = list(batches)
        flags = (_lib.GS_SAMPLE_GCN if gcn else 0) | (4 if fail_empty else 0)
        self.workers = [_SamplerWorker(graph, rngs[w], batches[w::S], fanouts, flags, depth) for w in range(S)]
        self.i = 0

    @property
    def sample_s(self):
        return [t for w in self.workers for t in w.sample_s]

    def next(self):
        w = self.workers[self.i % len(self.workers)]
        item = w.q.get()
        if item is None:
            raise StopIteration
        if isinstance(item, BaseException):
            raise item
        self.i += 1
        slot, info, offs, sizes = item
        used = info.pack_total + info.n_roots
        dev = w.slots[slot][:used].to(self.device, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        w.events[slot] = ev
        w.free.put(slot)
        ds = DeviceSample(info, self.device, buf=dev)
        ds._native = (sizes, offs)
        return ds, dev[info.pack_total:used], info

    def __iter__(self):
        return self

    def __next__(self):
        return self.next()

    def close(self):
        for w in self.workers:
            w.stop = True


def init_distributed():
    """torch.distributed from torchrun env (RCCL on HIP devices); (rank, world)."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    if world > 1 and not dist.is_initialized():
        backend = "nccl" if torch.cuda.is_available() else "gloo"
        if backend == "nccl":
            torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
        dist.init_process_group(backend=backend)
    return rank, world


def make_rng(seed, rank=0, stream=0):
    return RNG(rank_seed(seed, rank, stream))


# ------------------------------------------------------------ native runner
class Communicator:
    """Native RCCL communicator for the runner's gradient all-reduce; the
    128-byte id is created on rank 0 and broadcast over torch.distributed."""

    def __init__(self, rank, world, device):
        self.world = world
        uid = torch.zeros(128, dtype=torch.uint8)
        if rank == 0:
            check(lib().gs_comm_unique_id(uid.numpy().ctypes.data))
        if world > 1:
            t = uid.to(device)
            dist.broadcast(t, 0)
            uid = t.cpu().contiguous()
        h = ctypes.c_void_p()
        check(lib().gs_comm_create(uid.numpy().ctypes.data, world, rank, ctypes.byref(h)))
        self._h = h

    def close(self):
        if self._h is not None and self._h.value:
            lib().gs_comm_destroy(self._h)
        self._h = None


class Runner:
    """The training loop as one native pipeline (gs_runner): S sampler
    threads, pinned pack rings whose slots each have a device twin (the sampler
    thread copies a finished pack there), the next batch's layer-1
    gather on a high-priority side stream, and the fused
    step, all without Python per step.  `batches`: iterable of equal-size
    int64 root arrays consumed in order; `rngs`: one RNG per sampler stream
    (stream w samples batches w, w+S, ...).  Forward-only (`embed_out`) with
    `merge` = m > 1: each step is m consecutive batches in one pack and one
    forward; step u (batches u·m .. u·m+m-1) is sampled by stream u % S.
    `hold`: no batch is sampled before `release(mark)` allows it (measurement:
    proves a timed region sampled its own batches).  `ar_buckets=2` (with a
    communicator): the upper layers' + classifier gradients are all-reduced on
    a comm stream under the layer-1 weight-gradient GEMM, W1's after it.
    `helpers`: helper threads per sampler stream (gs_team; same draws, lower
    per-batch latency).  `warm`: every sampler thread samples one throwaway
    batch (its last, from a copy of its rng) before the constructor returns,
    so measured batches never pay a cold sampling context.
    `sampler="device"`: the streams sample on the GPU instead (SURVEY §8 f-4,
    gs_dsampler: one per stream, each on its own HIP stream), writing every
    pack straight into the device ring — no host sampler threads; the same
    packs and stream consumption as the host sampler.  The rngs are updated
    at ``sync_rngs()`` and ``close()``.
    `sampler="device-fast"`: the counter-based sampler on the GPU (DESIGN §5d,
    sampler.FastDeviceSampler) under `seed`: batch b is sampled with
    batch_index = b, so the packs depend on neither the stream count nor any
    ``random`` stream.  `rngs` only gives the number of device streams (an
    int, or a sequence whose items are ignored and left untouched)."""

    def __init__(self, trainer, graph, batches, rngs, fanouts, gcn=False, fail_empty=False, depth=4,
                 comm=None, embed_out=None, merge=1, hold=False, ar_buckets=1, helpers=0, warm=False,
                 sampler="host", seed=0):
        if sampler not in ("host", "device", "device-fast"):
            raise ValueError("sampler must be 'host', 'device' or 'device-fast'")
        self.sampler = sampler
        self.trainer, self.graph = trainer, graph
        self.embed_out = embed_out
        fast = sampler == "device-fast"
        if fast:
            n_streams = int(rngs) if isinstance(rngs, int) else len(list(rngs))
            rngs = []
        self.rngs = list(rngs)
        self.batches = np.ascontiguousarray(np.stack([np.asarray(b, np.int64) for b in batches]))
        # None (the reference's num_sample=None, the whole neighbourhood) is -1 natively, as in sample()
        self.fanouts = np.array([(-1 if k is None else int(k)) for k in fanouts], np.int32)
        self._rng_ptrs = (ctypes.c_void_p * len(self.rngs))(*[r._h.value for r in self.rngs])
        self.comm = comm
        flags = (_lib.GS_SAMPLE_GCN if gcn else 0) | (4 if fail_empty else 0)
        cfg = _lib.RunnerConfig(
            graph=graph._h.value, trainer=trainer._h.value, batches=self.batches.ctypes.data,
            n_batches=self.batches.shape[0], batch=self.batches.shape[1], fanouts=self.fanouts.ctypes.data,
            n_hops=len(self.fanouts), flags=flags, n_streams=n_streams if fast else len(self.rngs),
            rngs=None if fast else ctypes.cast(self._rng_ptrs, ctypes.c_void_p), depth=depth,
            comm=comm._h.value if comm is not None else None, world=comm.world if comm is not None else 1,
            hold=int(bool(hold)), ar_buckets=int(ar_buckets), helpers=int(helpers), warm=int(bool(warm)),
            device_sampler=2 if fast else int(sampler == "device"), sampler_seed=int(seed) & (2 ** 64 - 1))
        if embed_out is not None:
            n_rows = self.batches.shape[0] * self.batches.shape[1]
            if not (embed_out.is_contiguous() and embed_out.dtype == torch.float32
                    and embed_out.device == trainer.device and embed_out.dim() == 2
                    and embed_out.shape[0] >= n_rows and embed_out.shape[1] == trainer.H):
                raise ValueError("embed_out must be a contiguous fp32 [n_batches * batch, hidden] device tensor")
            cfg.embed_out = embed_out.data_ptr()
            cfg.embed_ld = trainer.H
            cfg.merge = max(1, int(merge))
        elif merge > 1:
            raise ValueError("merge > 1 needs embed_out (forward-only)")
        self.merge = max(1, int(merge)) if embed_out is not None else 1
        h = ctypes.c_void_p()
        check(lib().gs_runner_create(ctypes.byref(cfg), ctypes.byref(h)))
        self._h = h

    def run(self, n_steps):
        """Issue the next n_steps steps (asynchronous on the device): training
        steps, or forward-only steps (of `merge` batches each) into embed_out."""
        check(lib().gs_runner_run(self._h, int(n_steps), self.trainer.loss.data_ptr(),
                                  _lib.stream_ptr(self.trainer.device)))
        return self.embed_out if self.embed_out is not None else self.trainer.loss

    def sync_rngs(self):
        """sampler="device": copy the device streams' states back into the rngs
        (every batch sampled so far, consumed or not)."""
        check(lib().gs_runner_sync_rngs(self._h))

    def release(self, mark):
        """hold=True runners: let the sampler threads start batches < mark."""
        check(lib().gs_runner_release(self._h, int(mark)))

    def progress(self):
        """(batches sampled so far, steps issued so far)."""
        a, b = ctypes.c_int64(), ctypes.c_int64()
        check(lib().gs_runner_progress(self._h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def stats(self, reset=False):
        st = _lib.RunnerStats()
        check(lib().gs_runner_stats_get(self._h, ctypes.byref(st)))
        if reset:
            lib().gs_runner_stats_reset(self._h)
        sizes = np.array(st.hop_sizes[:], dtype=np.float64).reshape(_lib.GS_MAX_HOPS, 4)
        return {"steps": st.steps, "wait_s": st.wait_s, "issue_s": st.issue_s, "sample_s": st.sample_s,
                "wait_sample_s": st.wait_sample_s, "wait_ring_s": st.wait_ring_s,
                "wait_gather_s": st.wait_gather_s, "fwd_bwd_s": st.fwd_bwd_s, "update_s": st.update_s,
                "max_step_s": st.max_step_s, "lookahead_misses": st.lookahead_misses, "hop_sizes_sum": sizes}

    def close(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and getattr(_lib, "_lib", None) is not None:  # _lib is None at interpreter exit
            _lib._lib.gs_runner_destroy(h)
        self._h = None

    def __del__(self):
        self.close()


# ------------------------------------------------------- full-graph inference
class Embedder:
    """get_gnn_embeddings (utils.py:59-78) as one native pipeline: the
    training runner in forward-only mode (gs_runner_config.embed_out) over
    batches of `batch` ids, S sampler streams, the next batch's layer-1
    gather under the current forward, embeddings written in place.

    `merge` = m consecutive batches share one pack and one forward launch
    sequence (each still sampled on its own, so each row equals its own
    batch's forward): the runner is host-issue bound at one 500-id batch per
    launch.  Stream w of `rngs` samples the groups w, w+S, ... (batch i on
    stream (i // m) % S); a trailing partial batch is sampled afterwards by
    the stream whose turn it is and run through NativeTrainer.forward.  With
    one stream that is exactly the reference's sequence of GraphSage calls on
    one `random` stream, for any m."""

    def __init__(self, graph, features, weights, fanouts, agg_func="MEAN", gcn=False, depth=4, merge=2, helpers=0,
                 sampler="host", seed=0):
        if sampler not in ("host", "device-fast"):
            raise ValueError("Embedder: sampler must be 'host' or 'device-fast'")
        # "device-fast": the counter-based device sampler under `seed` (DESIGN
        # §5d), one batch per launch; batch i of an embed() call is sampled
        # with batch_index = i (the trailing partial batch included)
        self.sampler, self.seed = sampler, int(seed)
        weights = [w.detach() for w in weights]
        H = weights[0].shape[0]
        dev = features.device
        dummy_cls = (torch.zeros(1, H, device=dev), torch.zeros(1, device=dev))
        self.trainer = NativeTrainer(graph, features, torch.zeros(1, dtype=torch.int32), 1,
                                     num_layers=len(weights), hidden=H, fanouts=fanouts, agg_func=agg_func,
                                     gcn=gcn, weights=(weights, *dummy_cls))
        self.graph, self.fanouts, self.gcn, self.agg = graph, list(fanouts), gcn, agg_func
        self.depth = depth
        self.merge = max(1, int(merge))
        self.helpers = int(helpers)  # gs_team helper threads per sampler stream (same draws)
        self.last_stats = None

    def embed(self, nodes, batch, rngs):
        """[len(nodes), hidden] fp32 embeddings on the device, row i = nodes[i]."""
        nodes = np.ascontiguousarray(nodes, dtype=np.int64).reshape(-1)
        rngs = [None] * rngs if isinstance(rngs, int) else list(rngs)
        n_full = len(nodes) // batch
        out = torch.empty(len(nodes), self.trainer.H, dtype=torch.float32, device=self.trainer.device)
        fast = self.sampler == "device-fast"
        merge = 1 if fast else self.merge
        if n_full:
            r = Runner(self.trainer, self.graph, nodes[:n_full * batch].reshape(n_full, batch),
                       len(rngs) if fast else rngs, self.fanouts,
                       gcn=self.gcn, fail_empty=self.agg == "MAX", depth=self.depth, embed_out=out,
                       merge=merge, helpers=self.helpers, sampler=self.sampler, seed=self.seed)
            try:
                r.run(-(-n_full // merge))
                self.last_stats = r.stats()
            finally:
                r.close()  # joins the sampler threads: every rng has advanced past its batches
        rest = nodes[n_full * batch:]
        if len(rest) and fast:
            from .sampler import FastDeviceSampler
            fds = FastDeviceSampler(self.graph, self.fanouts, len(rest), self.seed, gcn=self.gcn,
                                    fail_empty=self.agg == "MAX", device=self.trainer.device)
            pack, hs, offs, used = fds.run(rest, n_full)
            L = len(self.fanouts)
            info = SampleInfo(L, hs.reshape(-1), offs, used, len(rest))
            ds = DeviceSample(info, self.trainer.device, buf=pack[:used])
            self.trainer.forward(ds, out[n_full * batch:])
        elif len(rest):
            s = sample(self.graph, rngs[(n_full // self.merge) % len(rngs)], rest, self.fanouts, gcn=self.gcn)
            if self.agg == "MAX" and any(s.n_empty(j) for j in range(1, s.n_hops + 1)):
                raise IndexError("MAX aggregation over an empty neighbourhood (reference: models.py:321-325)")
            self.trainer.forward(DeviceSample(s, self.trainer.device), out[n_full * batch:])
        return out


class FullEmbedder:
    """Exact embeddings over full neighbourhoods: the reference's
    num_sample=None branch (models.py:280-289) for every node, computed layer
    by layer over the device CSR (gs_infer_full) -- H_1 for all N nodes from
    the features, H_2 from H_1, ... -- with no sampler, no pack and no
    `random` stream.  The result does not depend on a batch size, and it is
    bitwise the same for every `chunk_rows` and from run to run.

    `weights`: the SageLayer weights, layer 1 first.  bf16 features: layer 1
    runs in bf16 (its aggregate rounded to bf16, W1 cast to bf16), the layers
    above in fp32.  MEAN gives a node without neighbours a NaN aggregate, as
    the reference's 0/0; MAX raises IndexError here, at construction, when any
    node's neighbourhood is empty (as Embedder does when it samples one).
    `seg_len` / `chunk_rows`: None takes the measured defaults
    (hip_ops.FULL_SEG_LEN, FULL_CHUNK_ROWS).  `edge_weight`, `edge_norm`,
    `self_weight`: per-edge weights, as FullTrainer takes them (MEAN only; not
    a reference feature).  Single GPU, inference only."""

    def __init__(self, graph, features, weights, agg_func="MEAN", gcn=False, seg_len=None, chunk_rows=None,
                 edge_weight=None, edge_norm="mean", self_weight=1.0):
        self.agg, self.gcn = agg_func, bool(gcn)
        op = ops.agg_op(agg_func)
        self.plan = ops.agg_full_plan(graph, gcn=gcn, seg_len=seg_len)
        if agg_func == "MAX" and self.plan.n_empty:
            raise IndexError(f"MAX aggregation over an empty neighbourhood ({self.plan.n_empty} nodes have none; "
                             "reference: models.py:321-325)")
        self.edge_weights = _edge_weights("FullEmbedder", self.plan, agg_func, edge_weight, edge_norm, self_weight)
        if not features.is_cuda:
            raise RuntimeError("FullEmbedder runs on a HIP device")
        if features.dim() != 2 or features.stride(1) != 1 or features.shape[0] != graph.n_nodes or \
                features.dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("features must be [n_nodes, F] fp32 or bf16 with unit column stride")
        self.graph, self.X, self.device = graph, features, features.device
        self.W = [w.detach().to(device=self.device, dtype=torch.float32).contiguous() for w in weights]
        self.L, self.H, F = len(self.W), int(self.W[0].shape[0]), features.shape[1]
        m = 1 if gcn else 2
        for l, w in enumerate(self.W):
            if tuple(w.shape) != (self.H, m * (F if l == 0 else self.H)):
                raise ValueError(f"weights[{l}] must be [{self.H}, {m * (F if l == 0 else self.H)}]")
        self.chunk_rows = ops.FULL_CHUNK_ROWS if chunk_rows is None else int(chunk_rows)
        self._dev, self.row_ptr, self.col = self.plan.device(self.device)
        if self.edge_weights is not None:
            self._dev = self.edge_weights.device(self.device)
        self.cfg = _lib.InferFullConfig(
            n_layers=self.L, hidden=self.H, agg=op,
            feat_dtype=_lib.GS_BF16 if features.dtype == torch.bfloat16 else _lib.GS_F32, feat_dim=F,
            feat_ld=features.stride(0), X=features.data_ptr(), row_ptr=self.row_ptr.data_ptr(),
            col=self.col.data_ptr(), chunk_rows=self.chunk_rows)
        for l, w in enumerate(self.W):
            self.cfg.W[l] = w.data_ptr()
        need = int(lib().gs_infer_full_ws_bytes(self.plan.handle, ctypes.byref(self.cfg)))
        if need < 0:
            check(_lib.GS_EINVAL)
        self._ws = torch.empty(need + 256, dtype=torch.uint8, device=self.device)
        self._ws_off = (-self._ws.data_ptr()) % 256
        self._ws_bytes = need

    def embed(self, nodes=None):
        """[N, hidden] fp32 embeddings on the device (row v = node v), or the
        rows `nodes` of them."""
        out = torch.empty(self.graph.n_nodes, self.H, dtype=torch.float32, device=self.device)
        check(lib().gs_infer_full(self.plan.handle, ctypes.byref(self._dev), ctypes.byref(self.cfg), out.data_ptr(),
                                  out.stride(0), self._ws.data_ptr() + self._ws_off, self._ws_bytes,
                                  _lib.stream_ptr(self.device)))
        if nodes is None:
            return out
        idx = torch.from_numpy(np.ascontiguousarray(nodes, dtype=np.int64).reshape(-1)).to(self.device)
        return out.index_select(0, idx)


def _edge_weights(who, plan, agg_func, edge_weight, edge_norm, self_weight):
    """The hip_ops.EdgeWeights of an exact embedder or trainer (None: unweighted), every refusal at construction:
    `edge_weight` is None, per-entry values (numpy or torch, the CSR's col order), "sym" (hip_ops.sym_norm_weights
    with norm="sum") or an EdgeWeights of this very plan."""
    if edge_weight is None:
        return None
    if agg_func == "MAX":
        raise ValueError(f"{who}: edge weights go with agg_func='MEAN'; MAX selects and has no weighted form")
    if isinstance(edge_weight, ops.EdgeWeights):
        if edge_weight.plan is not plan:
            raise ValueError(f"{who}: the edge weights were made for another plan (graph, gcn or seg_len)")
        ew = edge_weight
    elif isinstance(edge_weight, str):
        if edge_weight != "sym":
            raise ValueError(f"{who}: edge_weight must be per-entry values, an EdgeWeights or 'sym'")
        w, sw = ops.sym_norm_weights(plan)
        ew = ops.EdgeWeights(plan, w, norm="sum", self_weight=sw)
    else:
        ew = ops.EdgeWeights(plan, edge_weight, norm=edge_norm, self_weight=self_weight)
    if ew.norm == "mean":
        bad = ew.bad_rows()
        if len(bad):
            raise ValueError(f"{who}: under edge_norm='mean' {len(bad)} rows have a weight sum that is not finite and "
                             f"> 0 (the first: node {int(bad[0])}), whose mean is a NaN or infinite row; use "
                             "edge_norm='sum' or other weights")
    return ew


# ------------------------------------------------------- full-batch training
ReceptiveField = ops.ReceptiveField
_FULL_AGG1 = "full"   # FullTrainer._agg1 after an unrestricted forward (no field's build_id)


class UnsupBatch:
    """One extended batch of the unsupervised losses on the exact path
    (FullTrainer.unsup_batch): the device `nodes` (int32, the plan's row
    order), the native descriptor `desc` (a _lib.TrainFullUnsup over `plan`)
    and the head's buffer `uws` (uws_ptr: 256-byte aligned, uws_bytes)."""

    def __init__(self, nodes, plan, dims, kind, learn_method, q, margin, uws, uws_bytes):
        self.nodes, self.plan, self.dims = nodes, plan, dims
        self.kind, self.learn_method, self.with_sup = kind, learn_method, learn_method == "plus_unsup"
        M, P, N, _U = dims
        self.desc = _lib.TrainFullUnsup(kind=0 if kind == "normal" else 1, with_sup=int(self.with_sup), M=M, P=P,
                                        N=N, plan=plan.data_ptr(), q=q, margin=margin)
        self.uws = uws
        self.uws_off = (-uws.data_ptr()) % 256
        self.uws_ptr, self.uws_bytes = uws.data_ptr() + self.uws_off, int(uws_bytes)

    def pair_state(self):
        """[P + N, 4] {coef, cos, n1, n2} per pair as the last head left them (positive pairs first)."""
        _M, P, N, _U = self.dims
        return self.uws[self.uws_off:self.uws_off + 16 * (P + N)].view(torch.float32).view(P + N, 4)

    def d_embeddings(self, hidden):
        """[U, hidden] dE of the pair loss as the last head left it."""
        M, P, N, U = self.dims
        off = self.uws_off + -(-4 * int(lib().gs_unsup_loss_ws_floats(M, P, N)) // 256) * 256
        return self.uws[off:off + 4 * U * hidden].view(torch.float32).view(U, hidden)


class EvalResult:
    """What hip_ops.cls_eval left on the device -- `loss` (the mean NLL over
    the counted rows), `counts` ([C·C + 2] int64: the confusion matrix, then
    n_counted and n_bad), `pred` ([B] int32) and `logp` ([B, C], or None) --
    and the metrics of the confusion matrix, computed on first use in float64
    from one download of `counts`:

        confusion [C, C] int64 (row = true class), n, n_bad,
        accuracy, micro_f1 (equal to the accuracy: utils.micro_f1's docstring),
        macro_f1 (the plain mean over all C classes),
        per_class: {"precision", "recall", "f1", "support"} arrays of C.

    A class with no true and no predicted row scores 0 (sklearn's
    zero_division=0); with no counted row the accuracy is NaN.  A result over
    several parameter sets (ClassifierProbe.evaluate with snapshots) carries a
    leading dimension on every tensor and every metric."""

    def __init__(self, loss, counts, pred, logp):
        self.loss, self.counts, self.pred, self.logp = loss, counts, pred, logp
        self._m = None

    def _metrics(self):
        if self._m is None:
            c = self.counts.cpu().numpy().astype(np.int64)   # the one download
            C = int(round(np.sqrt(c.shape[-1] - 2)))
            lead = c.shape[:-1]
            conf = c[..., :C * C].reshape(lead + (C, C))
            n, n_bad = c[..., C * C], c[..., C * C + 1]
            tp = np.diagonal(conf, axis1=-2, axis2=-1).astype(np.float64)
            support, predicted = conf.sum(-1), conf.sum(-2)

            def ratio(num, den):
                den = np.asarray(den, np.float64)
                return np.divide(num, den, out=np.zeros_like(den), where=den > 0)

            acc = np.divide(tp.sum(-1), n, out=np.full(lead, np.nan), where=n > 0)
            f1 = ratio(2.0 * tp, support + predicted)
            scalar = (lambda x: x.item()) if not lead else (lambda x: x)
            self._m = {"confusion": conf, "n": scalar(n), "n_bad": scalar(n_bad), "accuracy": scalar(acc),
                       "macro_f1": scalar(f1.mean(-1)),
                       "per_class": {"precision": ratio(tp, predicted), "recall": ratio(tp, support), "f1": f1,
                                     "support": support}}
        return self._m

    confusion = property(lambda self: self._metrics()["confusion"])
    n = property(lambda self: self._metrics()["n"])
    n_bad = property(lambda self: self._metrics()["n_bad"])
    accuracy = property(lambda self: self._metrics()["accuracy"])
    micro_f1 = property(lambda self: self._metrics()["accuracy"])
    macro_f1 = property(lambda self: self._metrics()["macro_f1"])
    per_class = property(lambda self: self._metrics()["per_class"])


class MultiLabelEvalResult:
    """What hip_ops.cls_bce_eval left on the device -- `loss` (the BCE mean
    over rows x labels), `counts` ([C, 3] int64: true positives, false
    positives, false negatives per label), `n_exact_dev` (the rows whose every
    label is right), `pred_words` ([B, ceil(C / 32)] packed int32, z > 0) and
    `logits` ([B, C], or None) -- and the metrics, computed on first use in
    float64 from one download of the counts:

        n_exact, subset_accuracy (n_exact / rows),
        micro_f1 (2 TP / (2 TP + FP + FN) over all labels' sums),
        macro_f1 (the plain mean of the per-label F1 over all C labels),
        per_label: {"precision", "recall", "f1", "support"} arrays of C.

    0 / 0 counts as 0 (sklearn's zero_division=0), as EvalResult does for an
    absent class.  `pred` unpacks the predictions to bool [B, C] on request."""

    def __init__(self, loss, counts, n_exact, pred_words, logits, n_rows, n_classes):
        self.loss, self.counts, self.n_exact_dev = loss, counts, n_exact
        self.pred_words, self.logits = pred_words, logits
        self.n_rows, self.n_classes = int(n_rows), int(n_classes)
        self._m = None

    @staticmethod
    def metrics_of(counts, n_exact, n_rows):
        """The metrics from host counts [C, 3] (tp, fp, fn), n_exact and the row count."""
        c = np.asarray(counts, np.int64)
        tp, fp, fn = (c[:, k].astype(np.float64) for k in range(3))

        def ratio(num, den):
            den = np.asarray(den, np.float64)
            return np.divide(num, den, out=np.zeros_like(den), where=den > 0)

        f1 = ratio(2.0 * tp, 2.0 * tp + fp + fn)
        micro = ratio(2.0 * tp.sum(), 2.0 * tp.sum() + fp.sum() + fn.sum())
        return {"n_exact": int(n_exact), "subset_accuracy": float(n_exact) / float(n_rows),
                "micro_f1": float(micro), "macro_f1": float(f1.mean()),
                "per_label": {"precision": ratio(tp, tp + fp), "recall": ratio(tp, tp + fn), "f1": f1,
                              "support": (c[:, 0] + c[:, 2])}}

    def _metrics(self):
        if self._m is None:
            flat = torch.cat([self.counts.reshape(-1), self.n_exact_dev.reshape(1)]).cpu().numpy()  # the one download
            self._m = self.metrics_of(flat[:-1].reshape(-1, 3), flat[-1], self.n_rows)
        return self._m

    @property
    def pred(self):
        return None if self.pred_words is None else ops.unpack_multilabel(self.pred_words, self.n_classes)

    n_exact = property(lambda self: self._metrics()["n_exact"])
    subset_accuracy = property(lambda self: self._metrics()["subset_accuracy"])
    micro_f1 = property(lambda self: self._metrics()["micro_f1"])
    macro_f1 = property(lambda self: self._metrics()["macro_f1"])
    per_label = property(lambda self: self._metrics()["per_label"])


class FullTrainer:
    """Exact full-batch training over full neighbourhoods: the reference's
    num_sample=None branch (models.py:280-289) put through loss.backward(),
    layer by layer over the device CSR for all N nodes (gs_train_full_*) --
    no sampler, no pack and no `random` stream, bitwise repeatable.

    One step: A_l = agg_full(H_{l-1}) and H_l = relu(W_l [H_{l-1} | A_l]) for
    every node (H_L is bitwise FullEmbedder's), log_softmax + NLL mean over
    the rows `nodes`, the backward through every layer (agg_full_bwd over the
    transposed plan), then NativeTrainer's update: clip_grad_norm_(max_norm)
    per model and SGD(lr), or `optimizer="adam"` (AdamW with `betas`, `eps`,
    `weight_decay`).  The parameter layout, names and optimiser state are
    NativeTrainer's, so a model moves between the two, FullEmbedder and the
    GraphSage module through state_dict / weights.

    bf16 features: layer 1 runs in bf16 (its aggregate rounded to bf16, W1
    cast to bf16 each step), the layers above in fp32.  `cache_agg1`: layer
    1's aggregate does not depend on the weights, so it is computed on the
    first step and reused (the gradients are bitwise the same with it off);
    call invalidate_cache() after changing the feature table in place.
    `seg_len`: None takes the measured defaults, hip_ops.FULL_SEG_LEN for the
    forward plan and FULL_BWD_SEG_LEN for the transposed one; a value holds
    for both.

    A node with an empty effective neighbourhood is refused here, at
    construction (its NaN row would poison every loss): IndexError under MAX,
    as FullEmbedder; ValueError under MEAN -- use gcn=True, or train on a
    subgraph in which every node has a neighbour.

    Memory: every A_l and H_l is kept for the backward.  With N nodes, F
    features of e bytes (4, or 2 for bf16), H hidden, L layers, B = len(nodes)
    and the split rows' partial slots S (S_t transposed), ws_bytes is about
        N (F e + 4 H)                          A_1, H_1
      + (L - 1) N 4 H (2, or 3 under MAX)      A_l, H_l (and argmax_l), l >= 2
      + 4 N H (1 if L == 1 else 4, 3 with gcn) dH ping-pong, dSelf, dA
      + ceil(N / 2048) 4 K H                   dW row slabs (K = the widest layer input)
      + 4 max(S max(F, H), S_t H) + O(B H)     partials, loss head
    -- about 12 N H bytes per layer above the first: 8.7 GB on a 2.1 M-node
    graph at H = 128, L = 2, F = 128.  The graph's entry count enters only
    through the plans and the two device CSRs (12 bytes per entry each).

    Mini-batches: without a field every step computes all N rows, whatever
    len(nodes) is.  field(nodes) finds the L-hop receptive field of the batch
    on the device (hip_ops.ReceptiveField), and forward_backward / step /
    embed with `field=` then work on its rows only -- the same function (every
    row outside the field has a gradient of exactly zero), at a cost that
    follows the field instead of N.  The workspace keeps its size.

    The unsupervised losses (reference learn_method "unsup" and "plus_unsup",
    utils.py:159-181): unsup_batch(source, kind, learn_method) describes one
    extended batch -- an unsup.UnsupervisedLoss after extend_nodes, whose pair
    plan and unique_nodes_batch it takes -- and forward_backward / step /
    embed with `unsup=` then run the same forward and backward with another
    head (gs_train_full_unsup_forward_backward): get_loss_sage ("normal") or
    get_loss_margin ("margin") over H_L[nodes], plus the NLL mean over the
    same rows under "plus_unsup".  loss_parts() holds (total, loss_sup,
    loss_net).  Under "unsup" the classifier has no gradient in the reference
    and its optimisers skip it: apply_update after such a step updates the
    sage group only and leaves the classifier's parameters and Adam moments
    bitwise unchanged (no weight decay either).  The trainer keeps ONE step
    counter, which still advances, so the classifier's next Adam update is
    bias-corrected with the trainer's step, not with a count of its own
    updates as torch.optim would.  unsup_step(unsupervised_loss, batch_ids,
    ...) is one apply_model batch: extend, plan, field, step; nothing on this
    path draws from a `random` stream but extend_nodes itself.

    head="multilabel": C independent sigmoid outputs per node under
    binary_cross_entropy_with_logits (mean over nodes x labels, optional
    `pos_weight` [C]) in place of log_softmax + NLL (gs_cls_bce_fwd_bwd).
    `labels` is then a [N, C] multi-hot tensor of hard 0 / 1 targets (C ==
    n_classes), packed at construction (hip_ops.pack_multilabel).  The
    classifier keeps its shape, names and place in the flat buffer, so
    state_dict, optimizer_state, apply_update, field, embed and cache_agg1
    are untouched, step / forward_backward work full, with `field=` and with
    `unsup=` ("plus_unsup" adds the BCE mean), and evaluate returns a
    MultiLabelEvalResult.  head="nll" (the default) is the single-label head.
    Out of scope for the multi-label head: the sampled path (NativeTrainer,
    Runner, the GraphSage / Classification modules), ClassifierProbe, soft
    targets.

    Per-edge weights (not a reference feature; MEAN only, ValueError under
    MAX): `edge_weight` is float32 [n_entries] in the CSR's col order
    (hip_ops.edge_weights_from_pairs maps (dst, src, w) triples onto it), a
    hip_ops.EdgeWeights of this trainer's plan, or "sym" -- Kipf-Welling's
    1 / sqrt(c_v c_u) with edge_norm="sum", under gcn D^-1/2 (A + I) D^-1/2.
    edge_norm="mean" divides a row's weighted sum by the sum of its weights,
    "sum" leaves it; `self_weight` (a scalar or [N]) weighs the self row gcn
    appends.  Every aggregate of the step, forward and backward, full, with
    `field=` and with `unsup=`, in embed and in evaluate, then runs weighted;
    with unit weights the step is bitwise the unweighted one.  The weights are
    data and take no gradient.  Under "mean" a row whose weight sum is not
    finite and > 0 is refused at construction, as an empty row is.
    set_edge_weight swaps the weight set between steps.

    Single GPU.  Out of scope: data parallel."""

    def __init__(self, graph, features, labels, n_classes, num_layers=2, hidden=128, agg_func="MEAN", gcn=False,
                 lr=0.7, max_norm=5.0, seed=824, weights=None, optimizer="sgd", betas=(0.9, 0.999), eps=1e-8,
                 weight_decay=0.0, seg_len=None, cache_agg1=True, head="nll", pos_weight=None, edge_weight=None,
                 edge_norm="mean", self_weight=1.0):
        if head not in ("nll", "multilabel"):
            raise ValueError("FullTrainer: head must be 'nll' or 'multilabel'")
        self.head = head
        self.optimizer = optimizer
        self._opt_kind = optimizer_kind(optimizer)
        self.betas, self.eps, self.weight_decay = (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)
        self.agg, self.gcn, self.lr, self.max_norm = agg_func, bool(gcn), float(lr), float(max_norm)
        op = ops.agg_op(agg_func)
        self.plan = ops.agg_full_plan(graph, gcn=gcn, seg_len=seg_len)
        if self.plan.n_empty:
            if agg_func == "MAX":
                raise IndexError(f"MAX aggregation over an empty neighbourhood ({self.plan.n_empty} nodes have none; "
                                 "reference: models.py:321-325)")
            raise ValueError(f"FullTrainer: {self.plan.n_empty} nodes have an empty neighbourhood, whose MEAN is a "
                             "NaN row in every loss; use gcn=True or train on a self-contained subgraph")
        self.edge_weights = _edge_weights("FullTrainer", self.plan, agg_func, edge_weight, edge_norm, self_weight)
        if not features.is_cuda:
            raise RuntimeError("FullTrainer runs on a HIP device")
        if features.dim() != 2 or features.stride(1) != 1 or features.shape[0] != graph.n_nodes or \
                features.dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("features must be [n_nodes, F] fp32 or bf16 with unit column stride")
        self.graph, self.X, self.device = graph, features, features.device
        self.L, self.H, self.C, F = int(num_layers), int(hidden), int(n_classes), features.shape[1]
        if head == "multilabel":
            if not isinstance(labels, torch.Tensor) or labels.dim() != 2 or \
                    tuple(labels.shape) != (graph.n_nodes, self.C):
                raise ValueError("FullTrainer: with head='multilabel', labels must be a [n_nodes, n_classes] "
                                 "multi-hot tensor")
            if not ops.cls_bce_supported(self.H, self.C):
                raise ValueError(f"FullTrainer: (hidden, n_classes) = ({self.H}, {self.C}) does not fit the "
                                 "multi-label head (gs_cls_bce_supported)")
        elif labels.dim() > 1 and labels.numel() != max(labels.shape):
            raise ValueError("labels must hold one class per node (a [N, C] multi-hot tensor goes with "
                             "head='multilabel')")
        elif labels.numel() != graph.n_nodes:
            raise ValueError("labels must hold one class per node")
        if pos_weight is not None and head != "multilabel":
            raise ValueError("FullTrainer: pos_weight goes with head='multilabel'")
        if weights is None:
            weights = reference_init(self.L, F, self.H, self.C, gcn, seed)
        sage_w, cls_w, cls_b = weights
        m = 1 if gcn else 2
        shapes = [(self.H, m * (F if l == 0 else self.H)) for l in range(self.L)] + [(self.C, self.H), (self.C,)]
        tensors = list(sage_w) + [cls_w, cls_b]
        if len(tensors) != len(shapes):
            raise ValueError(f"weights: {self.L} SageLayer weights, the classifier's weight and its bias expected")
        for i, (t, want) in enumerate(zip(tensors, shapes)):
            if tuple(t.shape) != want:
                raise ValueError(f"weights[{i}] must be {list(want)}, got {list(t.shape)}")
        self.pos_weight = None
        if head == "multilabel":
            self.labels = ops.pack_multilabel(labels.to(self.device))  # [N, ceil(C / 32)] packed words
            if pos_weight is not None:
                pw = torch.as_tensor(pos_weight, dtype=torch.float32).reshape(-1)
                if pw.numel() != self.C:
                    raise ValueError("FullTrainer: pos_weight must hold n_classes values")
                self.pos_weight = pw.to(self.device).contiguous()
        else:
            self.labels = labels.reshape(-1).to(device=self.device, dtype=torch.int32)
        names = [f"sage_layer{i}.weight" for i in range(1, self.L + 1)] + ["layer.0.weight", "layer.0.bias"]
        self.p = FlatParams(tensors, names, [0, self.L], self.device)
        self.tplan = self.plan.transposed(ops.FULL_BWD_SEG_LEN if seg_len is None else seg_len)
        self._dev, self.row_ptr, self.col = self.plan.device(self.device)
        self._tdev, self.t_row_ptr, self.t_col = self.tplan.device(self.device)
        if self.edge_weights is not None:
            self._dev = self.edge_weights.device(self.device)
            self._tdev = self.edge_weights.t_device(self.tplan, self.device)
        self._loss3 = torch.zeros(3, dtype=torch.float32, device=self.device)  # total, loss_sup, loss_net
        self.loss = self._loss3[:1]
        self._uws = None           # the unsupervised head's buffer: grows on demand, kept between batches
        self._cls_frozen = False   # the last head was 'unsup': the classifier takes no update
        self._unsup_field = None   # unsup_step's field, rebuilt in place
        self.clip_ws = torch.empty(65 * 2, dtype=torch.float32, device=self.device)
        self.cfg = _lib.TrainFullConfig(
            n_layers=self.L, hidden=self.H, n_classes=self.C, agg=op,
            feat_dtype=_lib.GS_BF16 if features.dtype == torch.bfloat16 else _lib.GS_F32, feat_dim=F,
            feat_ld=features.stride(0), max_nodes=graph.n_nodes, X=features.data_ptr(),
            row_ptr=self.row_ptr.data_ptr(), col=self.col.data_ptr(), t_row_ptr=self.t_row_ptr.data_ptr(),
            t_col=self.t_col.data_ptr(), labels=self.labels.data_ptr(), params=self.p.params.data_ptr(),
            grads=self.p.grads.data_ptr(), head=1 if head == "multilabel" else 0,
            pos_weight=None if self.pos_weight is None else self.pos_weight.data_ptr())
        need = int(lib().gs_train_full_ws_bytes(self.plan.handle, self.tplan.handle, ctypes.byref(self.cfg)))
        if need < 0:
            check(_lib.GS_EINVAL)
        self.ws_bytes = need
        self._ws = torch.empty(need + 256, dtype=torch.uint8, device=self.device)
        self._ws_off = (-self._ws.data_ptr()) % 256
        self.cache_agg1 = bool(cache_agg1)
        self._agg1 = None      # whose A_1 the buffer holds: None, _FULL_AGG1 (all N rows), or a field's build_id
        self._opt_step = 0
        self.opt_m = self.opt_v = None
        if self._opt_kind == _lib.GS_OPT_ADAM:
            self.opt_m = torch.zeros_like(self.p.params)
            self.opt_v = torch.zeros_like(self.p.params)
        self._embedder = None

    # -- parameters and optimiser state: NativeTrainer's names and layout
    def state_dict(self):
        return self.p.state_dict()

    def load_state_dict(self, sd):
        """Copy the named parameters of state_dict() back into the flat buffer."""
        for i, n in enumerate(self.p.names):
            self.p.view(i).copy_(sd[n])

    def weights(self):
        return [self.p.view(i) for i in range(self.L)]

    def optimizer_state(self):
        """{"step", "m", "v"}, as NativeTrainer.optimizer_state()."""
        return {"step": self._opt_step,
                "m": None if self.opt_m is None else self.opt_m.detach().clone(),
                "v": None if self.opt_v is None else self.opt_v.detach().clone()}

    def load_optimizer_state(self, state):
        if self.opt_m is not None:
            if state["m"] is None or state["v"] is None:
                raise ValueError("load_optimizer_state: the state holds no Adam moments")
            if state["m"].numel() != self.opt_m.numel() or state["v"].numel() != self.opt_v.numel():
                raise ValueError("load_optimizer_state: moment size != parameter count")
            self.opt_m.copy_(state["m"].reshape(-1))
            self.opt_v.copy_(state["v"].reshape(-1))
        self._opt_step = int(state["step"])

    def invalidate_cache(self):
        """Recompute layer 1's aggregate on the next step, full or restricted (the feature table changed in
        place)."""
        self._agg1 = None

    def set_edge_weight(self, edge_weight, edge_norm="mean", self_weight=1.0):
        """Replace the weight set (the constructor's three arguments; None: back to unweighted) between steps.
        No plan is rebuilt; layer 1's cached aggregate and embed()'s embedder are dropped, so the next step,
        embed and evaluate are those of a trainer constructed with these weights.  The launches already issued
        keep the old set, which stays alive until the next call."""
        ew = _edge_weights("FullTrainer", self.plan, self.agg, edge_weight, edge_norm, self_weight)
        self._old_edge_weights, self.edge_weights = self.edge_weights, ew
        if ew is None:
            self._dev, self._tdev = self.plan.device(self.device)[0], self.tplan.device(self.device)[0]
        else:
            self._dev, self._tdev = ew.device(self.device), ew.t_device(self.tplan, self.device)
        self._agg1 = None
        self._embedder = None

    def _embedder_weights(self):
        """The weight arguments of embed()'s FullEmbedder: this trainer's set, by value (its plan is looked up
        again there)."""
        ew = self.edge_weights
        return {} if ew is None else {"edge_weight": ew.w, "edge_norm": ew.norm, "self_weight": ew.self_weight}

    def field(self, nodes, out=None):
        """The receptive field of `nodes` under this trainer's plans and depth
        (a hip_ops.ReceptiveField): pass it as `field=` to forward_backward,
        step or embed together with the same `nodes`.  It holds for any number
        of steps (it depends on the graph and `nodes` only); `out`: an earlier
        field of this trainer to rebuild in place for the next mini-batch,
        which costs a few dozen small launches and one synchronisation."""
        nodes = self._nodes(nodes)
        if out is None:
            out = ops.ReceptiveField(self.plan, self.tplan, self.L, self.device)
        elif not isinstance(out, ops.ReceptiveField) or out.plan is not self.plan or out.tplan is not self.tplan or \
                out.n_layers != self.L:
            raise ValueError("FullTrainer.field: `out` was made for another plan or depth")
        return out.build(nodes)

    def _check_field(self, field, nodes):
        """Every refusal of a field, before any launch."""
        if not isinstance(field, ops.ReceptiveField) or not field.build_id:
            raise TypeError("FullTrainer: field must be a built ReceptiveField (FullTrainer.field(nodes))")
        if field.plan is not self.plan or field.tplan is not self.tplan:
            raise ValueError("FullTrainer: the field was built for another plan (graph, gcn or seg_len)")
        if field.n_layers != self.L:
            raise ValueError(f"FullTrainer: the field was built for {field.n_layers} layers, the model has {self.L}")
        if not field.covers(nodes):
            raise ValueError("FullTrainer: the field was built for other nodes than those passed")

    def _nodes(self, nodes):
        """`nodes` as a device int32 vector of unique ids in [0, N); every check before any launch of the step."""
        n = self.graph.n_nodes
        if isinstance(nodes, torch.Tensor):
            if not nodes.is_cuda:
                raise RuntimeError("FullTrainer: nodes must be a device tensor (or a host array / list of ids)")
            if nodes.dtype != torch.int32 or nodes.dim() != 1 or not nodes.is_contiguous():
                raise TypeError("FullTrainer: nodes must be a contiguous 1-D int32 tensor")
            if nodes.numel() < 1 or nodes.numel() > n:
                raise ValueError("FullTrainer: nodes must hold 1 to n_nodes ids")
            key = (nodes.data_ptr(), nodes.numel(), nodes._version)
            if getattr(self, "_nodes_ok", None) != key:
                lo, hi = int(nodes.min()), int(nodes.max())
                if lo < 0 or hi >= n:
                    raise IndexError("FullTrainer: node id out of range")
                if int(torch.unique(nodes).numel()) != nodes.numel():
                    raise ValueError("FullTrainer: duplicate ids in nodes")
                self._nodes_ok = key
            return nodes
        a = np.asarray(nodes)
        if a.ndim != 1 or a.size < 1 or a.dtype.kind not in "iu":
            raise TypeError("FullTrainer: nodes must be a 1-D array of integer ids")
        if a.min() < 0 or a.max() >= n:
            raise IndexError("FullTrainer: node id out of range")
        if len(np.unique(a)) != a.size:
            raise ValueError("FullTrainer: duplicate ids in nodes")
        t = torch.from_numpy(a.astype(np.int32)).to(self.device)
        self._nodes_ok = (t.data_ptr(), t.numel(), t._version)  # checked above, on the host
        return t

    def unsup_batch(self, source, kind="normal", learn_method="unsup", q=None, margin=None):
        """One extended batch of the unsupervised losses, for `unsup=`.

        `source`: an unsup.UnsupervisedLoss after extend_nodes / extend_nodes_array
        (its pair plan and unique_nodes_batch are taken; q and margin default to
        its Q and MARGIN), or a raw (plan int32 device tensor, (M, P, N, U), nodes)
        triple laid out as gs_unsup_loss_plan, rows = positions in `nodes` (q and
        margin then default to the reference's 10 and 3).  kind: "normal"
        (get_loss_sage) or "margin" (get_loss_margin); learn_method: "unsup" or
        "plus_unsup".  No scored node (M == 0) raises the ValueError the
        reference's torch.cat raises."""
        if kind not in ("normal", "margin"):
            raise ValueError("FullTrainer.unsup_batch: kind must be 'normal' or 'margin'")
        if learn_method not in ("unsup", "plus_unsup"):
            raise ValueError("FullTrainer.unsup_batch: learn_method must be 'unsup' or 'plus_unsup'")
        if isinstance(source, (tuple, list)):
            plan, dims, nodes = source
            dq, dm = 10.0, 3.0
        else:
            nodes = source._unique_array()
            plan, dims = source._device_plan(self.device)
            dq, dm = float(source.Q), float(source.MARGIN)
        M, P, N, U = (int(x) for x in tuple(dims)[:4])
        if M == 0:
            raise ValueError("torch.cat(): expected a non-empty list of Tensors")
        nodes = self._nodes(nodes)
        if nodes.numel() != U:
            raise ValueError(f"FullTrainer.unsup_batch: the plan has {U} rows, nodes holds {nodes.numel()} ids")
        if M < 1 or P < M or N < M:
            raise ValueError("FullTrainer.unsup_batch: every scored node owns a positive and a negative pair")
        if not isinstance(plan, torch.Tensor) or plan.device != self.device or plan.dtype != torch.int32 or \
                plan.dim() != 1 or not plan.is_contiguous() or plan.numel() < 2 * (M + 1) + 4 * (P + N) + U + 1:
            raise ValueError("FullTrainer.unsup_batch: plan must be a contiguous int32 tensor on the trainer's "
                             "device, as long as its dims say")
        need = int(lib().gs_train_full_unsup_ws_bytes(self.H, U, M, P, N))
        if need < 0:
            raise ValueError("FullTrainer.unsup_batch: bad plan sizes")
        if self._uws is None or self._uws.numel() < need + 256:
            self._uws = torch.empty(need + need // 4 + 256, dtype=torch.uint8, device=self.device)
        return UnsupBatch(nodes, plan, (M, P, N, U), kind, learn_method, dq if q is None else float(q),
                          dm if margin is None else float(margin), self._uws, need)

    def loss_parts(self):
        """(total, loss_sup, loss_net) of the last step with `unsup=`, as device scalars (loss_sup is 0 under
        "unsup")."""
        return self._loss3[0], self._loss3[1], self._loss3[2]

    def _check_unsup(self, unsup, nodes):
        """`nodes` of a call with `unsup=`: the batch's own, checked before any launch."""
        if not isinstance(unsup, UnsupBatch):
            raise TypeError("FullTrainer: unsup must come from FullTrainer.unsup_batch")
        if nodes is unsup.nodes:
            return nodes
        nodes = self._nodes(nodes)
        if nodes.numel() != unsup.nodes.numel() or not torch.equal(nodes, unsup.nodes):
            raise ValueError("FullTrainer: with unsup=, nodes must be the batch's own nodes (unsup.nodes)")
        return unsup.nodes

    def forward_backward(self, nodes, stages=_lib.GS_TF_ALL, field=None, unsup=None):
        """Loss (device scalar, the NLL mean over `nodes`) and the raw,
        unclipped gradients into self.p.grads: one native call that issues
        every launch of the step on the current stream.  `nodes`: unique ids,
        a device int32 vector or a host array.  `stages`: a _lib.GS_TF_* subset,
        for measurement only.  `field`: field(nodes), to work on the batch's
        receptive field only (gs_train_full_field_forward_backward); hidden()
        then holds valid rows on R_l only.  `unsup`: unsup_batch(...), whose
        loss replaces (or, "plus_unsup", joins) the NLL mean; `nodes` must then
        be unsup.nodes, the loss is the total and loss_parts() its terms."""
        if unsup is not None:
            return self._forward_backward(self._check_unsup(unsup, nodes), stages, field, unsup)
        return self._forward_backward(self._nodes(nodes), stages, field)

    def _forward_backward(self, nodes, stages, field, unsup=None):
        """Every path's native call.  Layer 1's aggregate is reused only while the buffer holds this path's own
        (all N rows, or this very build of the field); a forward stage makes the buffer this path's."""
        head = (self.plan.handle, ctypes.byref(self._dev), self.tplan.handle, ctypes.byref(self._tdev),
                ctypes.byref(self.cfg))
        if field is None:
            mine, fn = _FULL_AGG1, lib().gs_train_full_forward_backward
        else:
            self._check_field(field, nodes)
            mine, fn, head = field.build_id, lib().gs_train_full_field_forward_backward, head + (field.ref,)
        tail = ()
        if unsup is not None:
            fn = lib().gs_train_full_unsup_forward_backward
            if field is None:
                head = head + (None,)
            tail = (ctypes.byref(unsup.desc), unsup.uws_ptr, unsup.uws_bytes)
        reuse = self.cache_agg1 and self._agg1 == mine
        if stages & _lib.GS_TF_FORWARD and not reuse:
            self._agg1 = None  # this path's A_1 overwrites whatever the buffer held
        check(fn(*head, nodes.data_ptr(), nodes.numel(), *tail, int(reuse), int(stages), self._loss3.data_ptr(),
                 self._ws.data_ptr() + self._ws_off, self.ws_bytes, _lib.stream_ptr(self.device)))
        if stages & _lib.GS_TF_FORWARD:
            self._agg1 = mine
        if stages & _lib.GS_TF_HEAD:
            self._cls_frozen = unsup is not None and not unsup.with_sup
        self._last_nodes = nodes  # alive until the stream has run the step
        self._last_unsup = unsup
        if field is not None:
            self._last_field = field
        return self.loss

    def apply_update(self):
        """clip per model + SGD, or + AdamW (gs_clip_sgd / gs_clip_adam) on the flat buffers.  After an 'unsup'
        head the classifier's group is left out of the call: its parameters and moments are not touched."""
        self._opt_step += 1
        goff = self.p.group_off[:2] if self._cls_frozen else self.p.group_off
        if self._opt_kind == _lib.GS_OPT_ADAM:
            ops.clip_adam(goff, self.p.params, self.p.grads, self.opt_m, self.opt_v, 1.0, self.max_norm,
                          self.lr, self.betas, self.eps, self.weight_decay, self._opt_step, self.clip_ws)
        else:
            ops.clip_sgd(goff, self.p.params, self.p.grads, 1.0, self.max_norm, self.lr, self.clip_ws)

    def step(self, nodes, field=None, unsup=None):
        loss = self.forward_backward(nodes, field=field, unsup=unsup)
        self.apply_update()
        return loss

    def unsup_step(self, unsupervised_loss, batch_ids, unsup_loss="normal", learn_method="unsup", num_neg=None,
                   use_field=True):
        """One apply_model batch (utils.py:113-193) on the exact path:
        extend_nodes(batch_ids, num_neg) on `unsupervised_loss`, its pair plan,
        the receptive field of the extended batch (use_field) and one step.
        num_neg: None takes the reference's 100 ("normal") or 6 ("margin").
        Returns (loss, extended nodes as an int64 array); the only host
        synchronisation is the field's."""
        defaults = {"normal": 100, "margin": 6}
        if unsup_loss not in defaults:
            raise ValueError("FullTrainer.unsup_step: unsup_loss must be 'normal' or 'margin'")
        if learn_method not in ("unsup", "plus_unsup"):
            raise ValueError("FullTrainer.unsup_step: learn_method must be 'unsup' or 'plus_unsup'")
        nodes = unsupervised_loss.extend_nodes_array(batch_ids, num_neg=defaults[unsup_loss] if num_neg is None
                                                     else int(num_neg))
        batch = self.unsup_batch(unsupervised_loss, kind=unsup_loss, learn_method=learn_method)
        field = None
        if use_field:
            field = self._unsup_field = self.field(batch.nodes, out=self._unsup_field)
        return self.step(batch.nodes, field=field, unsup=batch), nodes

    def hidden(self, layer=None, which=0):
        """A view of H_layer (which=0) or A_layer (which=1) as the last
        forward left it in the workspace ([N, width]; layer None: the last).
        After a field step H_layer holds valid rows on R_layer only, and
        A_layer's first n_layer rows are the compact aggregate in R_layer order.
        which=2: the buffer of dH_layer (dZ_layer, masked by relu'), valid
        until the backward of layer - 1 reuses it for dH_{layer-2} (two
        buffers ping-pong): dZ_L is there after the head stage, and still
        after the whole step when L <= 2; row v is node v, or after a field
        step row i is R_layer[i] and only the first n_layer rows are written."""
        layer = self.L if layer is None else int(layer)
        off = int(lib().gs_train_full_ws_offset(self.plan.handle, self.tplan.handle, ctypes.byref(self.cfg), which,
                                                layer))
        if off < 0:
            check(_lib.GS_EINVAL)
        n = self.graph.n_nodes
        if which == 1 and layer == 1:
            w, dt = self.X.shape[1], self.X.dtype
        else:
            w, dt = self.H, torch.float32
        nbytes = n * w * (2 if dt == torch.bfloat16 else 4)
        raw = self._ws[self._ws_off + off:self._ws_off + off + nbytes]
        return raw.view(dt).view(n, w)

    def embed(self, nodes=None, field=None, unsup=None):
        """[N, hidden] exact embeddings under the current weights (or the rows
        `nodes`): FullEmbedder over this trainer's parameter views, bitwise
        FullEmbedder(graph, X, tr.weights(), ...).embed().  `field`:
        field(nodes) -- the field path's forward stage alone, then the rows
        `nodes` of H_L (in the order of `nodes`); it overwrites the step's
        activations in the workspace.  Restricted inference without a trainer
        is out of scope: FullEmbedder always computes all N rows.  `unsup`:
        unsup_batch(...) -- the forward stage of the unsupervised step's own
        entry point, then the rows of its nodes."""
        if field is not None or unsup is not None:
            if nodes is None:
                raise ValueError("FullTrainer.embed: a field or an unsup batch goes with its nodes")
            nodes = self._check_unsup(unsup, nodes) if unsup is not None else self._nodes(nodes)
            self._forward_backward(nodes, _lib.GS_TF_FORWARD, field, unsup)
            return self.hidden().index_select(0, nodes.long())
        if self._embedder is None:
            self._embedder = FullEmbedder(self.graph, self.X, self.weights(), agg_func=self.agg, gcn=self.gcn,
                                          seg_len=self.plan.seg_len, **self._embedder_weights())
        for dst, src in zip(self._embedder.W, self.weights()):
            dst.copy_(src)
        return self._embedder.embed(nodes)

    def evaluate(self, nodes, field=None, want_logp=False):
        """The model on `nodes` (unique ids, as forward_backward takes them)
        under the current parameters, as an EvalResult: the forward stage
        alone (embed(nodes, field=)'s call, with or without field(nodes)),
        then the forward-only head hip_ops.cls_eval over H_L[nodes] and this
        trainer's labels -- the NLL mean, the predictions (row i is nodes[i]),
        the confusion matrix, and with want_logp the log-probabilities.  It
        overwrites the step's activations in the workspace and nothing else:
        parameters, gradients, optimiser state and the step counter stay as
        they were, and nothing waits for the device until a metric is read.
        The trainer does not range-check its labels; a row whose label lies
        outside [0, n_classes) is left out and counted in n_bad."""
        nodes = self._nodes(nodes)
        self._forward_backward(nodes, _lib.GS_TF_FORWARD, field)
        if self.head == "multilabel":
            # the BCE mean, the packed predictions z > 0, the per-label counts: a MultiLabelEvalResult
            # (want_logp: the logits)
            loss, counts, n_exact, pred, logits = ops.cls_bce_eval(
                self.hidden(), self.labels, self.p.view(self.L), self.p.view(self.L + 1), rows=nodes,
                pos_weight=self.pos_weight, want_logits=want_logp)
            return MultiLabelEvalResult(loss, counts, n_exact, pred, logits, nodes.numel(), self.C)
        head = self.p.params[int(self.p.offsets[self.L]):]   # [Wc | bc], the tail of the flat buffer
        loss, counts, pred, logp = ops.cls_eval(self.hidden(), self.labels, head, self.C, rows=nodes,
                                                want_logp=want_logp)
        return EvalResult(loss[0], counts[0], pred[0], None if logp is None else logp[0])


class ClassifierProbe:
    """The linear probe of train_classification (utils.py:80-111) on frozen
    embeddings: every batch-`batch` SGD step of every epoch inside the
    persistent single-workgroup kernel (hip_ops.cls_probe), with one
    clip_grad_norm_(max_norm) over weight and bias together and SGD(lr).
    Parameters are named as Classification names them (layer.0.weight [C, D],
    layer.0.bias [C]) and live in one flat buffer, W row-major then b.
    `weights`: (W, b), or None for the reference's initialisation of
    Classification(D, n_classes) under torch.manual_seed(seed).

    Everything is validated here, once (ValueError): labels in [0, n_classes),
    `embeddings` fp32 2-D with unit column stride on a HIP device, and a shape
    the kernel supports (gs_cls_probe_supported).  There is no other path."""

    def __init__(self, embeddings, labels, n_classes, weights=None, lr=0.5, max_norm=5.0, batch=50, seed=824):
        E = embeddings
        if not isinstance(E, torch.Tensor) or not E.is_cuda:
            raise ValueError("ClassifierProbe: embeddings must be a tensor on a HIP device")
        if E.dtype != torch.float32 or E.dim() != 2 or E.stride(1) != 1 or E.shape[0] < 1 or E.shape[1] < 1:
            raise ValueError("ClassifierProbe: embeddings must be float32 [N, D] with unit column stride")
        self.E = E.detach()
        self.device = E.device
        self.N, self.D = int(E.shape[0]), int(E.shape[1])
        self.C, self.batch = int(n_classes), int(batch)
        self.lr, self.max_norm = float(lr), float(max_norm)
        if self.C < 1 or self.batch < 1:
            raise ValueError("ClassifierProbe: n_classes and batch must be >= 1")
        if not ops.cls_probe_supported(self.D, self.C, self.batch):
            raise ValueError(f"ClassifierProbe: (D, C, batch) = ({self.D}, {self.C}, {self.batch}) does not fit "
                             "the probe kernel's LDS (gs_cls_probe_supported)")
        y = np.asarray(labels.cpu() if isinstance(labels, torch.Tensor) else labels).reshape(-1)
        if len(y) != self.N or not np.issubdtype(y.dtype, np.integer):
            raise ValueError("ClassifierProbe: labels must be N integers")
        if y.min() < 0 or y.max() >= self.C:
            raise ValueError("ClassifierProbe: labels must lie in [0, n_classes)")
        self.labels = torch.from_numpy(y.astype(np.int32)).to(self.device)
        if weights is None:
            torch.manual_seed(seed)
            lin = Classification(self.D, self.C).layer[0]
            weights = (lin.weight.detach(), lin.bias.detach())
        W, b = weights
        if tuple(W.shape) != (self.C, self.D) or tuple(b.shape) != (self.C,):
            raise ValueError(f"ClassifierProbe: weights must be ([{self.C}, {self.D}], [{self.C}])")
        self.p = FlatParams([W, b], ["layer.0.weight", "layer.0.bias"], [0], self.device)

    def state_dict(self):
        return self.p.state_dict()

    def load_state_dict(self, sd):
        """Copy the named parameters of state_dict() (or of a Classification) into the flat buffer."""
        for i, n in enumerate(self.p.names):
            self.p.view(i).copy_(sd[n])

    def weights(self):
        """Views of the flat buffer: (layer.0.weight, layer.0.bias)."""
        return self.p.view(0), self.p.view(1)

    def steps_per_epoch(self, n_train):
        return -(-int(n_train) // self.batch)

    def _order(self, order):
        """`order` as a device int32 [n_epochs, n_train], its ids checked against [0, N): on the host for an array
        or a CPU tensor; a device tensor is checked on the device, which waits for it."""
        if isinstance(order, torch.Tensor) and order.is_cuda:
            if order.dim() != 2 or order.numel() == 0 or order.dtype not in (torch.int32, torch.int64):
                raise ValueError("ClassifierProbe.run: order must be an integer [n_epochs, n_train]")
            if bool(((order < 0) | (order >= self.N)).any()):
                raise IndexError("ClassifierProbe.run: row id out of range")
            return order.to(device=self.device, dtype=torch.int32).contiguous()
        o = np.asarray(order.numpy() if isinstance(order, torch.Tensor) else order)
        if o.ndim != 2 or o.size == 0 or not np.issubdtype(o.dtype, np.integer):
            raise ValueError("ClassifierProbe.run: order must be an integer [n_epochs, n_train]")
        if o.min() < 0 or o.max() >= self.N:
            raise IndexError("ClassifierProbe.run: row id out of range")
        return torch.from_numpy(np.ascontiguousarray(o, dtype=np.int32)).to(self.device)

    def run(self, order, *, max_steps_per_launch=0):
        """Train over order [n_epochs, n_train] (row e: epoch e's shuffled
        ids, batches in that order).  Returns (losses [n_epochs, steps],
        snapshots [n_epochs, P]) on the device: every step's loss and the flat
        parameters after each epoch; the parameters themselves end in this
        object.  Nothing here waits for the device."""
        o = self._order(order)
        n_epochs, n_train = o.shape
        P = self.p.params.numel()
        losses = torch.empty(n_epochs, self.steps_per_epoch(n_train), dtype=torch.float32, device=self.device)
        snaps = torch.empty(n_epochs, P, dtype=torch.float32, device=self.device)
        ops.cls_probe(self.E, self.labels, o, self.p.params, self.batch, self.lr, self.max_norm, snaps, losses,
                      max_steps_per_launch=max_steps_per_launch)
        return losses, snaps

    def predict(self, nodes, snapshots=None):
        """argmax class of the frozen rows `nodes` under the current
        parameters ([n]), or under every row of `snapshots` at once
        ([n_epochs, n]: one batched torch.matmul)."""
        ids = torch.as_tensor(np.asarray(nodes), device=self.device).long()
        X = self.E.index_select(0, ids)
        C, D = self.C, self.D
        if snapshots is None:
            W, b = self.weights()
            return (X @ W.t() + b).argmax(1)
        S = snapshots.reshape(-1, C * D + C)
        W = S[:, :C * D].reshape(-1, C, D)
        return (torch.matmul(X, W.transpose(1, 2)) + S[:, None, C * D:]).argmax(2)

    def evaluate(self, nodes, snapshots=None):
        """hip_ops.cls_eval over the frozen rows `nodes` (ids in [0, N),
        checked here) and their labels, as an EvalResult: under the current
        parameters, or under every row of `snapshots` ([n_epochs, P], as run()
        returns them) in one call -- every field then carries a leading epoch
        dimension.  Where two logits tie, pred is the lower class.  Ids given
        as a host array or list are checked on the host and nothing waits for
        the device; a device tensor of ids is range-checked on the device,
        which waits for it (as run() does for a device `order`)."""
        if isinstance(nodes, torch.Tensor) and nodes.is_cuda:
            ids = nodes.reshape(-1)
            if ids.numel() < 1 or ids.dtype not in (torch.int32, torch.int64):
                raise ValueError("ClassifierProbe.evaluate: nodes must hold at least one integer id")
            if bool(((ids < 0) | (ids >= self.N)).any()):
                raise IndexError("ClassifierProbe.evaluate: row id out of range")
            ids = ids.to(device=self.device, dtype=torch.int32).contiguous()
        else:
            a = np.asarray(nodes.numpy() if isinstance(nodes, torch.Tensor) else nodes).reshape(-1)
            if a.size < 1 or not np.issubdtype(a.dtype, np.integer):
                raise ValueError("ClassifierProbe.evaluate: nodes must hold at least one integer id")
            if a.min() < 0 or a.max() >= self.N:
                raise IndexError("ClassifierProbe.evaluate: row id out of range")
            ids = torch.from_numpy(a.astype(np.int32)).to(self.device)
        P = self.p.params.numel()
        if snapshots is None:
            out = ops.cls_eval(self.E, self.labels, self.p.params, self.C, rows=ids)
            return EvalResult(*(None if t is None else t[0] for t in out))
        if not isinstance(snapshots, torch.Tensor) or snapshots.device != self.device or \
                snapshots.dtype != torch.float32 or snapshots.numel() < P or snapshots.numel() % P:
            raise ValueError("ClassifierProbe.evaluate: snapshots must be float32 [n_epochs, C*D + C] on the "
                             "probe's device")
        S = snapshots.reshape(-1, P).contiguous()
        return EvalResult(*ops.cls_eval(self.E, self.labels, S.reshape(-1), self.C, rows=ids, n_sets=S.shape[0]))
