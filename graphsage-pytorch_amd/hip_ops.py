"""torch-tensor front-end of the gfx950 kernels (C-ABI in include/graphsage_amd.h).

Every function checks shapes/dtypes/devices, then launches on torch's current
stream of the tensors' device.  There is deliberately no CPU path: tensors
that are not on a HIP device raise.
"""
import torch

from . import _lib
from ._lib import check, lib, ptr

_DT = {torch.float32: _lib.GS_F32, torch.bfloat16: _lib.GS_BF16}
_AGG = {"MEAN": _lib.GS_AGG_MEAN, "MAX": _lib.GS_AGG_MAX}


def _dev(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("graphsage_amd kernels run on a HIP device; got a CPU tensor "
                               "(move raw_features / the model to cuda)")


def _stream(t):
    return _lib.stream_ptr(t.device)


def _i32(t):
    if t is not None and t.dtype != torch.int32:
        raise TypeError("index tensors must be int32")
    return t


def agg_op(agg_func):
    try:
        return _AGG[agg_func]
    except KeyError:
        raise ValueError(f"agg_func must be 'MEAN' or 'MAX', got {agg_func!r}") from None


def agg_fwd(agg_func, X, ptr_, idx, out, *, row_ptr=None, col=None, dst_ids=None, gcn=False,
            argmax=None):
    """Segmented mean/max of rows of X (models.py:291-330); see gs_agg_fwd."""
    _dev(X, ptr_, idx, out)
    if X.dtype not in _DT or out.dtype != X.dtype:
        raise TypeError("X/out must share dtype float32 or bfloat16")
    n_dst = ptr_.numel() - 1
    F = X.shape[1]
    if out.shape[0] < n_dst or out.shape[1] < F:
        raise ValueError("out too small")
    check(lib().gs_agg_fwd(agg_op(agg_func), _DT[X.dtype], ptr(X), X.stride(0), F, n_dst,
                           ptr(_i32(ptr_)), ptr(_i32(idx)), ptr(row_ptr), ptr(_i32(col)),
                           ptr(_i32(dst_ids)), int(bool(gcn)), ptr(out), _DT[out.dtype],
                           out.stride(0), ptr(_i32(argmax)), _stream(X)))
    return out


# Defaults of the full-neighbourhood path, the fastest measured on rmat2m
# (profiles/full_infer_bench.json, DESIGN §4 "Exact full-neighbourhood
# inference"): rows longer than 256 entries are reduced in segments, and the
# driver works in chunks of 2 Mi rows (rmat2m as one chunk: smaller chunks
# were slower, larger graphs keep the chunk buffer at this size).
FULL_SEG_LEN = 256
FULL_CHUNK_ROWS = 1 << 21
# seg_len of the backward aggregate's transposed plan, the fastest measured on rmat2m at width 128
# (profiles/full_train_bench.json, DESIGN §4 "Exact full-batch training"): the MEAN backward pays a division
# per element and wants more items per hub row than the forward (5.0 ms at 64 against 6.4 at 256); the MAX
# backward is flat from 64 to 256 (5.15-5.27 ms).
FULL_BWD_SEG_LEN = 64


class FullPlan:
    """The work plan of agg_full (gs_full_plan): built on the host once per
    graph, gcn flag and seg_len (None: FULL_SEG_LEN; <= 0: no row is split).
    `graph` is a CSRGraph or a (row_ptr int64, col int32) pair of numpy arrays.
    The host arrays are readable without a GPU (array()); device() uploads the
    ones the kernels read, once per device."""

    _DTYPES = {_lib.GS_FP_ITEMS: "int32", _lib.GS_FP_ITEM_PTR: "int64", _lib.GS_FP_SLOT_PTR: "int64",
               _lib.GS_FP_SPLIT_PTR: "int64", _lib.GS_FP_SPLIT_ROWS: "int32", _lib.GS_FP_COUNT: "int32",
               _lib.GS_FP_SELF_LOOP: "uint8", _lib.GS_FP_EMPTY_ROWS: "int32", _lib.GS_FP_T_ROW_PTR: "int64",
               _lib.GS_FP_T_COL: "int32", _lib.GS_FP_T_SRC: "int64"}
    is_transposed = False

    def __init__(self, graph, gcn=False, seg_len=None):
        import ctypes

        import numpy as np
        self._t = {}
        if isinstance(graph, tuple):
            row_ptr, col = graph
            self.graph = None
        else:
            row_ptr, col = graph.row_ptr(), graph.col()
            self.graph = graph
        self.row_ptr = np.ascontiguousarray(row_ptr, dtype=np.int64)
        self.col = np.ascontiguousarray(col, dtype=np.int32)
        if self.row_ptr.ndim != 1 or len(self.row_ptr) < 1 or self.col.ndim != 1 or \
                len(self.col) < int(self.row_ptr[-1]):
            raise ValueError("FullPlan: row_ptr [n + 1] and col [row_ptr[n]] expected")
        seg_len = FULL_SEG_LEN if seg_len is None else int(seg_len)
        h = ctypes.c_void_p()
        check(lib().gs_full_plan_create(ptr(self.row_ptr), ptr(self.col), len(self.row_ptr) - 1, int(bool(gcn)),
                                        seg_len, ctypes.byref(h)))
        self._h = h
        self._read_dims()

    def _read_dims(self):
        import numpy as np
        h = self._h
        dims = np.zeros(_lib.GS_FP_NDIMS, np.int64)
        check(lib().gs_full_plan_dims(h, ptr(dims)))
        self.n_nodes, self.n_items, self.n_slots, self.n_split, self.n_empty, self.seg_len = \
            (int(dims[i]) for i in (_lib.GS_FP_N_NODES, _lib.GS_FP_N_ITEMS, _lib.GS_FP_N_SLOTS, _lib.GS_FP_N_SPLIT,
                                    _lib.GS_FP_N_EMPTY, _lib.GS_FP_SEG_LEN))
        self.gcn = bool(dims[_lib.GS_FP_GCN])
        self.n_entries = int(dims[_lib.GS_FP_N_ENTRIES])
        self._dev = {}

    def transposed(self, seg_len=None):
        """The plan of agg_full_bwd (gs_full_plan_transpose), built once per
        seg_len (None: this plan's; <= 0: no row is split): a FullPlan over the
        transposed CSR -- row u lists the destinations whose effective
        neighbourhood (this plan's gcn rule) holds u, ascending -- cut into
        segments of its own.  Its row_ptr / col are that CSR, and its
        COUNT array is this plan's (the MEAN divisor of every destination).
        Its T_SRC array names, for every transposed entry, the entry of this
        plan's col it came from (-1: the self entry gcn added), which is how
        EdgeWeights carries per-edge weights over.
        Correct for directed input: symmetry is never assumed."""
        import ctypes
        import weakref
        if self.is_transposed:
            raise ValueError("FullPlan.transposed: the plan is already a transposed one")
        seg_len = self.seg_len if seg_len is None else int(seg_len)
        if seg_len not in self._t:
            h = ctypes.c_void_p()
            check(lib().gs_full_plan_transpose(self._h, ptr(self.row_ptr), ptr(self.col), seg_len, ctypes.byref(h)))
            t = FullPlan.__new__(FullPlan)
            t._h, t._t, t.graph, t.is_transposed = h, {}, None, True
            t._fwd = weakref.ref(self)
            t._read_dims()
            t.row_ptr = t.array(_lib.GS_FP_T_ROW_PTR)
            t.col = t.array(_lib.GS_FP_T_COL)
            self._t[seg_len] = t
        return self._t[seg_len]

    def array(self, which):
        """A copy of one of the plan's host arrays (a _lib.GS_FP_* array id)."""
        import ctypes

        import numpy as np
        n = {_lib.GS_FP_ITEMS: 2 * self.n_items, _lib.GS_FP_ITEM_PTR: self.n_nodes + 1,
             _lib.GS_FP_SLOT_PTR: self.n_nodes + 1, _lib.GS_FP_SPLIT_PTR: self.n_nodes + 1,
             _lib.GS_FP_SPLIT_ROWS: self.n_split, _lib.GS_FP_COUNT: self.n_nodes,
             _lib.GS_FP_SELF_LOOP: self.n_nodes, _lib.GS_FP_EMPTY_ROWS: self.n_empty,
             _lib.GS_FP_T_ROW_PTR: self.n_nodes + 1, _lib.GS_FP_T_COL: self.n_entries,
             _lib.GS_FP_T_SRC: self.n_entries}[which]
        dt = np.dtype(self._DTYPES[which])
        if n == 0:
            return np.zeros(0, dt)
        p = lib().gs_full_plan_array(self._h, which)
        if not p:
            raise ValueError("FullPlan.array: only a transposed plan owns a CSR")
        buf = (ctypes.c_char * (n * dt.itemsize)).from_address(p)
        a = np.frombuffer(buf, dtype=dt).copy()
        return a.reshape(-1, 2) if which == _lib.GS_FP_ITEMS else a

    def device(self, device):
        """(gs_full_plan_dev, row_ptr, col) on `device`; the tensors stay alive with the plan."""
        key = str(torch.device(device))
        if key not in self._dev:
            ts = {w: torch.from_numpy(self.array(w).reshape(-1)).to(device)
                  for w in (_lib.GS_FP_ITEMS, _lib.GS_FP_SLOT_PTR, _lib.GS_FP_SPLIT_ROWS, _lib.GS_FP_COUNT,
                            _lib.GS_FP_SELF_LOOP)}
            if self.graph is not None:
                rp, cl = self.graph.device_csr(device)
            else:
                rp = torch.from_numpy(self.row_ptr).to(device)
                cl = torch.from_numpy(self.col).to(device)
                if cl.numel() == 0:
                    cl = torch.zeros(1, dtype=torch.int32, device=device)
            d = _lib.FullPlanDev(items=ptr(ts[_lib.GS_FP_ITEMS]), slot_ptr=ptr(ts[_lib.GS_FP_SLOT_PTR]),
                                 split_rows=ptr(ts[_lib.GS_FP_SPLIT_ROWS]) if self.n_split else None,
                                 count=ptr(ts[_lib.GS_FP_COUNT]), self_loop=ptr(ts[_lib.GS_FP_SELF_LOOP]))
            self._dev[key] = (d, rp, cl, ts)
        return self._dev[key][:3]

    @property
    def handle(self):
        return self._h

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and getattr(_lib, "_lib", None) is not None:
            _lib._lib.gs_full_plan_destroy(h)
            self._h = None


def agg_full(agg_func, X, graph, out=None, *, gcn=False, seg_len=None, row0=0, n_rows=None, ws=None, argmax=None,
             field=None, layer=None, edge_weight=None):
    """Full-neighbourhood mean/max of rows of X over the device CSR for the
    destination rows [row0, row0 + n_rows) (gs_agg_full): adj[v] without v, or
    with v exactly once under gcn; rows longer than `seg_len` entries are
    reduced in segments (None: FULL_SEG_LEN; <= 0: never).  `graph` is a
    CSRGraph (its plan for (gcn, seg_len) is built once and kept on it) or a
    FullPlan, whose own gcn and seg_len then hold.  out: [n_rows, F] in X's
    dtype.  MEAN of an empty neighbourhood is a NaN row; MAX over a window
    that holds one raises IndexError before any launch.  `argmax` (MAX over
    fp32 rows only; an int32 [n_rows, F] tensor): also filled with the id of
    each element's first maximal source in the kernel's visiting order (CSR
    row order, gcn's missing self row last), which agg_full_bwd routes the
    gradient to; `out` is bitwise the same with and without it.
    `field`, `layer` (a ReceptiveField of this plan, 1 <= layer <= its depth):
    only the rows of R_layer, row v as row field.pos(layer)[v] of a compact
    [n_layer, F] out (and argmax, which still holds global source ids); every
    row is bitwise the unrestricted call's (gs_agg_full_field).
    `edge_weight` (an EdgeWeights of this plan, MEAN only): the weighted mean
    or sum it describes, with a window and with a field alike; with unit
    weights and norm="mean" the result is bitwise the unweighted one."""
    _dev(X, out, ws, argmax)
    import ctypes
    plan = graph if isinstance(graph, FullPlan) else agg_full_plan(graph, gcn=gcn, seg_len=seg_len)
    _check_edge_weight("agg_full", edge_weight, plan, agg_func)
    if field is not None:
        if field.plan is not plan or not field.build_id:
            raise ValueError("agg_full: the field was built for another plan (or not built)")
        if layer is None or not 1 <= int(layer) <= field.n_layers:
            raise ValueError("agg_full: layer must lie in 1 .. field.n_layers")
        if row0 != 0 or n_rows is not None:
            raise ValueError("agg_full: a field takes no row window")
        n_rows = field.size(int(layer))
    elif layer is not None:
        raise ValueError("agg_full: layer goes with a field")
    if X.dtype not in _DT:
        raise TypeError("X must be float32 or bfloat16")
    if argmax is not None and (agg_op(agg_func) != _lib.GS_AGG_MAX or X.dtype != torch.float32):
        raise ValueError("agg_full: argmax is recorded for MAX over float32 rows only "
                         "(a bf16 feature table's aggregate has no backward)")
    if X.dim() != 2 or X.stride(1) != 1 or X.shape[0] < plan.n_nodes:
        raise ValueError("X must be [n_nodes, F] with unit column stride")
    n_rows = plan.n_nodes - row0 if n_rows is None else int(n_rows)
    row0 = int(row0)
    F = X.shape[1]
    ws_fn = lib().gs_agg_full_ws_bytes if argmax is None else lib().gs_agg_full_argmax_ws_bytes
    need = int(ws_fn(plan.handle, F, row0, n_rows if field is None else plan.n_nodes))
    if need < 0:
        check(_lib.GS_EINVAL)
    if out is None:
        out = torch.empty(n_rows, F, dtype=X.dtype, device=X.device)
    if out.dtype != X.dtype or out.dim() != 2 or out.stride(1) != 1 or out.shape[0] < n_rows or out.shape[1] < F:
        raise ValueError("out must be [n_rows, F] in X's dtype")
    if ws is None:
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=X.device)
    d, rp, cl = plan.device(X.device)
    if edge_weight is not None:
        d = edge_weight.device(X.device)
    if argmax is not None:
        if argmax.dtype != torch.int32 or argmax.dim() != 2 or argmax.stride(1) != 1 or argmax.shape[0] < n_rows or \
                argmax.shape[1] < F:
            raise ValueError("argmax must be int32 [n_rows, F]")
    if field is not None:
        check(lib().gs_agg_full_field(plan.handle, ctypes.byref(d), field.tplan.handle, field.ref, int(layer),
                                      agg_op(agg_func), _DT[X.dtype], ptr(X), X.stride(0), F, ptr(rp), ptr(cl),
                                      ptr(out), out.stride(0), ptr(argmax),
                                      argmax.stride(0) if argmax is not None else 0, ptr(ws),
                                      ws.numel() * ws.element_size(), _stream(X)))
        return out
    if argmax is not None:
        check(lib().gs_agg_full_argmax(plan.handle, ctypes.byref(d), _DT[X.dtype], ptr(X), X.stride(0), F, ptr(rp),
                                       ptr(cl), row0, n_rows, ptr(out), out.stride(0), ptr(argmax), argmax.stride(0),
                                       ptr(ws), ws.numel() * ws.element_size(), _stream(X)))
        return out
    check(lib().gs_agg_full(plan.handle, ctypes.byref(d), agg_op(agg_func), _DT[X.dtype], ptr(X), X.stride(0), F,
                            ptr(rp), ptr(cl), row0, n_rows, ptr(out), out.stride(0), ptr(ws),
                            ws.numel() * ws.element_size(), _stream(X)))
    return out


def agg_full_plan(graph, *, gcn=False, seg_len=None):
    """The FullPlan of a CSRGraph for (gcn, seg_len), built once per graph."""
    key = (bool(gcn), FULL_SEG_LEN if seg_len is None else int(seg_len))
    plans = graph.__dict__.setdefault("_full_plans", {})
    if key not in plans:
        plans[key] = FullPlan(graph, gcn=key[0], seg_len=key[1])
    return plans[key]


def agg_full_bwd_plan(graph, *, gcn=False, seg_len=None):
    """The transposed FullPlan of a CSRGraph for (gcn, seg_len) (seg_len None:
    FULL_BWD_SEG_LEN), built once per graph and kept on its forward plan."""
    seg_len = FULL_BWD_SEG_LEN if seg_len is None else int(seg_len)
    return agg_full_plan(graph, gcn=gcn).transposed(seg_len)


def agg_full_bwd(agg_func, dA, graph, dH=None, *, gcn=False, seg_len=None, dSelf=None, argmax=None, Hprev=None,
                 ws=None, field=None, layer=None, edge_weight=None):
    """Backward of agg_full over all rows (gs_agg_full_bwd), fp32:
    dH[u] = sum over the destinations v that read u of dA[v] / count[v] (MEAN)
    or of dA[v] where argmax[v] == u (MAX; `argmax` from agg_full), plus
    dSelf[u], zeroed where Hprev[u] <= 0 (both optional).  `graph` is a
    CSRGraph (its transposed plan for (gcn, seg_len) is built once and kept)
    or a FullPlan, forward or transposed.  No atomics: bitwise repeatable.
    `field`, `layer` (a ReceptiveField over this transposed plan): the
    backward of layer `layer` into the rows u of R_{layer-1} only
    (gs_agg_full_bwd_field).  dA, dSelf and argmax are then compact in R_layer
    order ([n_layer, F]; destinations outside R_layer are skipped, dSelf is
    added only where u is in R_layer), Hprev stays the [n_nodes, F] table,
    and dH is compact in R_{layer-1} order ([n_{layer-1}, F]).
    `edge_weight` (the EdgeWeights the forward ran with, MEAN only):
    dH[u] = sum of w_vu dA[v] / den[v] (norm="mean") or of w_vu dA[v]
    (norm="sum"); the weights themselves take no gradient."""
    _dev(dA, dH, dSelf, argmax, Hprev, ws)
    import ctypes
    if field is not None:
        tplan = field.tplan
        if isinstance(graph, FullPlan) and graph is not tplan and graph is not field.plan:
            raise ValueError("agg_full_bwd: the field was built for another plan")
        if not field.build_id or layer is None or not 1 <= int(layer) <= field.n_layers:
            raise ValueError("agg_full_bwd: a built field and a layer in 1 .. field.n_layers expected")
        layer = int(layer)
        # rows of dA / dSelf / argmax, of Hprev and of dH, and their names in the messages
        na, nh, nd, ra, rd = field.size(layer), tplan.n_nodes, field.size(layer - 1), "n_layer", "n_{layer-1}"
    else:
        if layer is not None:
            raise ValueError("agg_full_bwd: layer goes with a field")
        if isinstance(graph, FullPlan):
            tplan = graph if graph.is_transposed else graph.transposed()
        else:
            tplan = agg_full_bwd_plan(graph, gcn=gcn, seg_len=seg_len)
        na = nh = nd = tplan.n_nodes
        ra = rd = "n_nodes"
    op = agg_op(agg_func)
    _check_edge_weight("agg_full_bwd", edge_weight, tplan._fwd(), agg_func)

    def ok(t, rows, width=0, dtype=torch.float32):
        return t.dtype == dtype and t.dim() == 2 and t.stride(1) == 1 and t.shape[0] == rows and t.shape[1] >= width

    if not ok(dA, na):
        raise ValueError(f"dA must be float32 [{ra}, F] with unit column stride")
    F = dA.shape[1]
    if dH is None:
        dH = torch.empty(nd, F, dtype=torch.float32, device=dA.device)
    if not ok(dH, nd, F):
        raise ValueError(f"dH must be float32 [{rd}, F] with unit column stride")
    if dSelf is not None and (not ok(dSelf, na, F) or dSelf.stride(0) != dA.stride(0)):
        raise ValueError(f"dSelf must be float32 [{ra}, F] and share dA's leading dimension")
    # without a field Hprev and dH are both [n_nodes, F] and the native call takes one leading dimension for the two
    if Hprev is not None and (not ok(Hprev, nh, F) or (field is None and Hprev.stride(0) != dH.stride(0))):
        raise ValueError("Hprev must be float32 [n_nodes, F]" + (" and share dH's leading dimension" if field is None
                                                                 else ""))
    if op == _lib.GS_AGG_MAX and (argmax is None or not ok(argmax, na, F, torch.int32)):
        raise ValueError(f"MAX needs the forward's argmax: int32 [{ra}, F]")
    need = int(lib().gs_agg_full_bwd_ws_bytes(tplan.handle, F))
    if need < 0:
        check(_lib.GS_EINVAL)
    if ws is None:
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dA.device)
    d, rp, cl = tplan.device(dA.device)
    if edge_weight is not None:
        d = edge_weight.t_device(tplan, dA.device)
    lda = argmax.stride(0) if argmax is not None else 0
    if field is None:
        check(lib().gs_agg_full_bwd(tplan.handle, ctypes.byref(d), op, F, ptr(rp), ptr(cl), ptr(dA), ptr(dSelf),
                                    dA.stride(0), ptr(argmax), lda, ptr(Hprev), ptr(dH), dH.stride(0), ptr(ws),
                                    ws.numel() * ws.element_size(), _stream(dA)))
    else:
        check(lib().gs_agg_full_bwd_field(field.plan.handle, tplan.handle, ctypes.byref(d), field.ref, layer, op, F,
                                          ptr(rp), ptr(cl), ptr(dA), ptr(dSelf), dA.stride(0), ptr(argmax), lda,
                                          ptr(Hprev), Hprev.stride(0) if Hprev is not None else 0, ptr(dH),
                                          dH.stride(0), ptr(ws), ws.numel() * ws.element_size(), _stream(dA)))
    return dH


# ------------------------------------------------- per-edge weights of the exact path
def _check_edge_weight(who, ew, plan, agg_func):
    """Every refusal of an `edge_weight=` argument, before any launch."""
    if ew is None:
        return
    if not isinstance(ew, EdgeWeights):
        raise TypeError(f"{who}: edge_weight must be a hip_ops.EdgeWeights")
    if ew.plan is not plan:
        raise ValueError(f"{who}: the edge weights were made for another plan (graph, gcn or seg_len)")
    if agg_op(agg_func) == _lib.GS_AGG_MAX:
        raise ValueError(f"{who}: edge weights go with MEAN; MAX selects and has no weighted form")


class EdgeWeights:
    """Per-edge weights of a forward FullPlan, for `edge_weight=` of agg_full /
    agg_full_bwd and for FullEmbedder / FullTrainer.

    `w`: float32 [n_entries], aligned with the plan's CSR `col` (entry e of
    row v weighs X[col[e]] in out[v]; edge_weights_from_pairs maps (dst, src,
    w) triples onto that order).  The effective entries of a row are the
    unweighted kernel's: without gcn an entry equal to the row's own id is
    skipped and its weight ignored; with gcn every entry counts with its own
    weight and a row without a self entry gets one last, weighing
    `self_weight[v]` (a scalar or [n_nodes]).
        S[v] = sum over eff(v) of fmaf(w_e, X[col_e], acc)   fp32, the unweighted visiting order
        norm="sum":  out[v] = S[v]
        norm="mean": out[v] = S[v] / den[v],  den[v] = sum over eff(v) of w_e
    den is computed here, once per weight set, on the host: summed in float64
    per row in entry order and rounded to fp32 (no floating-point atomics), so
    with unit weights it is float(count[v]) and the weighted mean is bitwise
    the unweighted one.  Weights must be finite; negative and zero weights are
    allowed (a zero-weight edge is still an edge of the receptive field), and
    a row whose den is 0 gets what IEEE gives.  The weights are data: there is
    no gradient with respect to them.

    The backward reads the weights in the transposed plan's entry order: w is
    permuted through the transposed plan's T_SRC array (-1, the self entry gcn
    added, takes self_weight), once -- the transposed CSR's entry order does
    not depend on its seg_len.  device() / t_device() hand out weighted COPIES
    of the plans' device structs; the plans' own (unweighted, shared per
    graph) structs are never touched.  host(): (w, den, w_t) as numpy."""

    def __init__(self, plan, w, norm="mean", self_weight=1.0):
        import numpy as np
        if not isinstance(plan, FullPlan) or plan.is_transposed:
            raise ValueError("EdgeWeights: a forward FullPlan expected")
        if norm not in ("mean", "sum"):
            raise ValueError("EdgeWeights: norm must be 'mean' or 'sum'")
        self.plan, self.norm = plan, norm
        self.w = self._values(w, plan.n_entries, "w must hold one weight per CSR entry (n_entries)")
        sw = self_weight.detach().cpu().numpy() if isinstance(self_weight, torch.Tensor) else np.asarray(self_weight)
        if sw.ndim == 0:
            sw = np.full(plan.n_nodes, float(sw), np.float32)
        self.self_weight = self._values(sw, plan.n_nodes, "self_weight must be a scalar or hold n_nodes values")
        self.den = np.zeros(plan.n_nodes, np.float32)
        if plan.n_nodes:
            check(lib().gs_full_plan_edge_denom(plan.handle, ptr(plan.row_ptr), ptr(plan.col), ptr(self.w),
                                                ptr(self.self_weight), ptr(self.den)))
        self._w_t = None
        self._dev = {}

    @staticmethod
    def _values(a, n, msg):
        import numpy as np
        if isinstance(a, torch.Tensor):
            a = a.detach().cpu().numpy()
        a = np.ascontiguousarray(a, dtype=np.float32)
        if a.ndim != 1 or len(a) != n:
            raise ValueError("EdgeWeights: " + msg)
        if not np.isfinite(a).all():
            raise ValueError("EdgeWeights: weights must be finite")
        return a

    def bad_rows(self):
        """Rows whose den is not finite and > 0: what norm="mean" cannot divide by."""
        import numpy as np
        return np.nonzero(~(np.isfinite(self.den) & (self.den > 0)))[0]

    def transposed_weights(self):
        """w in the transposed CSR's entry order (float32 [t_entries])."""
        import numpy as np
        if self._w_t is None:
            ts = self.plan._t
            t = next(iter(ts.values())) if ts else self.plan.transposed()
            src = t.array(_lib.GS_FP_T_SRC)
            w_t = np.empty(len(src), np.float32)
            fwd = src >= 0
            w_t[fwd] = self.w[src[fwd]]
            w_t[~fwd] = self.self_weight[t.col[~fwd]]  # gcn's added self entry: row u's own, t_col == u
            self._w_t = w_t
        return self._w_t

    def host(self):
        """(w, den, w_t) as numpy arrays: forward order, per destination, transposed order."""
        return self.w, self.den, self.transposed_weights()

    def _tensors(self, device):
        key = str(torch.device(device))
        if key not in self._dev:
            def up(a):  # an empty array still gets an address
                return torch.from_numpy(a).to(device) if len(a) else torch.zeros(1, device=device)

            self._dev[key] ={"w": up(self.w), "den": up(self.den), "sw": up(self.self_weight), "structs": {}}
        return self._dev[key]

    def _struct(self, plan, device, weight, self_weight):
        ts = self._tensors(device)
        if id(plan) not in ts["structs"]:
            base = plan.device(device)[0]
            d = _lib.FullPlanDev(items=base.items, slot_ptr=base.slot_ptr, split_rows=base.split_rows,
                                 count=base.count, self_loop=base.self_loop, weight=ptr(weight),
                                 denom=ptr(ts["den"]) if self.norm == "mean" else None,
                                 self_weight=ptr(self_weight) if self_weight is not None else None)
            ts["structs"][id(plan)] = (d, plan)
        return ts["structs"][id(plan)][0]

    def device(self, device):
        """The forward plan's gs_full_plan_dev with this weight set; the tensors stay alive with this object."""
        ts = self._tensors(device)
        return self._struct(self.plan, device, ts["w"], ts["sw"])

    def t_device(self, tplan, device):
        """A transposed plan's gs_full_plan_dev with this weight set (weights in its entry order)."""
        if not isinstance(tplan, FullPlan) or not tplan.is_transposed or tplan._fwd() is not self.plan:
            raise ValueError("EdgeWeights: a transposed plan of this weight set's forward plan expected")
        ts = self._tensors(device)
        if "w_t" not in ts:
            w_t = self.transposed_weights()
            ts["w_t"] = torch.from_numpy(w_t).to(device) if len(w_t) else torch.zeros(1, device=device)
        return self._struct(tplan, device, ts["w_t"], None)


def edge_weights_from_pairs(row_ptr, col, dst, src, w, symmetric=False, default=None):
    """float32 [n_entries] weights in the CSR's entry order from weighted edge
    triples: entry e of row v with col[e] == u takes the weight of the triple
    (dst = v, src = u), looked up by the key dst * n + src (a CSRGraph's rows
    are in CPython-set order, which no caller can guess).  `symmetric`: every
    triple also stands for (src, dst).  A CSR entry without a triple raises
    KeyError unless `default` is given; a triple given twice (after
    `symmetric` mirrored them) raises ValueError; a triple without a CSR entry
    is ignored."""
    import numpy as np
    row_ptr = np.asarray(row_ptr, np.int64)
    col = np.asarray(col, np.int64)
    n = len(row_ptr) - 1
    dst = np.asarray(dst, np.int64).reshape(-1)
    src = np.asarray(src, np.int64).reshape(-1)
    w = np.asarray(w, np.float32).reshape(-1)
    if not (len(dst) == len(src) == len(w)):
        raise ValueError("edge_weights_from_pairs: dst, src and w must have one length")
    if len(dst) and (min(dst.min(), src.min()) < 0 or max(dst.max(), src.max()) >= n):
        raise IndexError("edge_weights_from_pairs: node id out of range")
    if symmetric:
        off = dst != src
        dst, src, w = np.concatenate([dst, src[off]]), np.concatenate([src, dst[off]]), np.concatenate([w, w[off]])
    keys = dst * n + src
    order = np.argsort(keys, kind="stable")
    keys, w = keys[order], w[order]
    if len(keys) > 1 and (keys[1:] == keys[:-1]).any():
        k = int(keys[1:][keys[1:] == keys[:-1]][0])
        raise ValueError(f"edge_weights_from_pairs: the edge (dst {k // n}, src {k % n}) is given twice")
    n_entries = int(row_ptr[-1])
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(row_ptr))
    want = rows * n + col[:n_entries]
    at = np.searchsorted(keys, want)
    hit = at < len(keys)
    hit[hit] = keys[at[hit]] == want[hit]
    if default is None and not hit.all():
        k = int(want[~hit][0])
        raise KeyError(f"edge_weights_from_pairs: no weight for the CSR entry (dst {k // n}, src {k % n})")
    out = np.full(n_entries, 0.0 if default is None else default, np.float32)
    out[hit] = w[at[hit]]
    return out


def sym_norm_weights(plan):
    """(w float32 [n_entries], self_weight float32 [n_nodes]) of the Kipf-Welling
    symmetric normalisation over a forward FullPlan: w_e = 1 / sqrt(c_v c_u)
    for entry e = (v reads u) and self_weight[v] = 1 / c_v, with c the plan's
    effective counts.  They go with norm="sum"; under gcn that aggregate is
    D^-1/2 (A + I) D^-1/2 X.  A node that is read but has no effective entry
    of its own (c = 0) gives an infinite weight, which EdgeWeights refuses."""
    import numpy as np
    if not isinstance(plan, FullPlan) or plan.is_transposed:
        raise ValueError("sym_norm_weights: a forward FullPlan expected")
    c = plan.array(_lib.GS_FP_COUNT).astype(np.float64)
    rows = np.repeat(np.arange(plan.n_nodes, dtype=np.int64), np.diff(plan.row_ptr))
    with np.errstate(divide="ignore"):
        w = 1.0 / np.sqrt(c[rows] * c[plan.col[:plan.n_entries]])
        sw = 1.0 / c
    return w.astype(np.float32), sw.astype(np.float32)


# ------------------------------------------------- the receptive field of a batch
class HostField:
    """full_field_host's result: rows(l) (ascending int32 ids of R_l), pos(l)
    (int32 [N]: id -> index in rows(l), -1 outside) and sizes (n_L .. n_0)."""

    def __init__(self, rows, n):
        import numpy as np
        self._rows = rows
        self._pos = []
        for r in rows:
            p = np.full(n, -1, np.int32)
            p[r] = np.arange(len(r), dtype=np.int32)
            self._pos.append(p)
        self.n_layers = len(rows) - 1
        self.sizes = tuple(len(rows[l]) for l in range(self.n_layers, -1, -1))

    def rows(self, l):
        return self._rows[l]

    def pos(self, l):
        return self._pos[l]


def full_field_host(row_ptr, col, nodes, n_layers, gcn=False):
    """The L-hop receptive field of `nodes` in plain numpy, the CPU reference
    of full_field (as sampler.fast_sample is of the Philox sampler):
        R_L = nodes,  R_{l-1} = R_l U N_eff(R_l)
    with N_eff(v) the plan's effective neighbourhood: v's CSR row without v's
    own id.  Under `gcn` the row itself joins its neighbourhood, which changes
    nothing here: it is in R_l already."""
    import numpy as np
    row_ptr = np.asarray(row_ptr, np.int64)
    col = np.asarray(col, np.int64)
    n = len(row_ptr) - 1
    nodes = np.asarray(nodes, np.int64).reshape(-1)
    if nodes.size < 1 or nodes.min() < 0 or nodes.max() >= n:
        raise IndexError("full_field_host: node id out of range")
    if len(np.unique(nodes)) != nodes.size:
        raise ValueError("full_field_host: duplicate ids in nodes")
    L = int(n_layers)
    member = np.zeros(n, bool)
    member[nodes] = True
    rows = [None] * (L + 1)
    for l in range(L, -1, -1):
        rows[l] = np.nonzero(member)[0].astype(np.int32)
        if l == 0:
            break
        for v in rows[l]:
            nb = col[row_ptr[v]:row_ptr[v + 1]]
            member[nb[nb != v]] = True
    return HostField(rows, n)


_field_builds = 0


class ReceptiveField:
    """The receptive field of a mini-batch on the device (gs_full_field_*):
    owns the buffer the build fills for one (forward plan, transposed plan,
    n_layers).  build(nodes) finds the field of `nodes` -- every launch on the
    current stream, one host synchronisation at the end for the counts -- and
    may be called again for the next mini-batch: the maps are then reset by
    walking the old rows.  rows(l) / pos(l): R_l ascending and its inverse
    map; items(l) / split(l) / t_items(l) / t_split(l): the plans' work items
    and split rows restricted to R_l (transposed: to R_{l-1}); sizes: (n_L,
    .., n_0).  `build_id` changes with every build."""

    def __init__(self, plan, tplan, n_layers, device):
        import ctypes
        if not isinstance(plan, FullPlan) or plan.is_transposed or not isinstance(tplan, FullPlan) or \
                not tplan.is_transposed:
            raise ValueError("ReceptiveField: a forward FullPlan and its transposed plan expected")
        self.plan, self.tplan, self.n_layers, self.device = plan, tplan, int(n_layers), torch.device(device)
        need = int(lib().gs_full_field_bytes(plan.handle, tplan.handle, self.n_layers))
        if need < 0:
            check(_lib.GS_EINVAL)
        self._buf = torch.empty(need + 256, dtype=torch.uint8, device=self.device)
        self._off = (-self._buf.data_ptr()) % 256
        self._f = _lib.FullField(n_layers=self.n_layers, buf=self._buf.data_ptr() + self._off, buf_bytes=need)
        self._built = False
        self.build_id = 0
        self.nodes = None
        self.sizes = ()
        self._ref = ctypes.byref(self._f)

    def build(self, nodes):
        """`nodes`: a device int32 vector of unique ids in [0, N) (checked by the caller)."""
        import ctypes
        global _field_builds
        if self._buf is None:
            raise RuntimeError("ReceptiveField: released")
        _dev(nodes)
        if nodes.dtype != torch.int32 or nodes.dim() != 1 or not nodes.is_contiguous() or nodes.numel() < 1:
            raise TypeError("ReceptiveField: nodes must be a contiguous 1-D int32 device tensor")
        d, rp, cl = self.plan.device(self.device)
        td, _trp, _tcl = self.tplan.device(self.device)
        st = _lib.stream_ptr(self.device)
        check(lib().gs_full_field_build(self.plan.handle, ctypes.byref(d), self.tplan.handle, ctypes.byref(td),
                                        ptr(rp), ptr(cl), ptr(nodes), nodes.numel(), int(self._built), self._ref, st))
        self._built = True
        check(lib().gs_full_field_counts(self.plan.handle, self.tplan.handle, self._ref, st))
        _field_builds += 1
        self.build_id = _field_builds
        self.nodes, self._nodes_version = nodes, nodes._version
        self.sizes = tuple(int(self._f.counts[l]) for l in range(self.n_layers, -1, -1))
        return self

    def size(self, l):
        return int(self._f.counts[l])

    def layer_counts(self, l):
        """(items, split rows, transposed items, transposed split rows) of layer l."""
        c0 = _lib.GS_FF_LAYER0 + 4 * (l - 1)
        return tuple(int(self._f.counts[c0 + k]) for k in range(4))

    def _view(self, which, level, count, width=1):
        if not self.build_id:
            raise RuntimeError("ReceptiveField: not built")
        off = int(lib().gs_full_field_offset(self.plan.handle, self.tplan.handle, self.n_layers, which, level))
        if off < 0:
            raise ValueError("ReceptiveField: level outside the field")
        raw = self._buf[self._off + off:self._off + off + 4 * count * width].view(torch.int32)
        return raw.view(count, width) if width > 1 else raw

    def rows(self, l):
        return self._view(_lib.GS_FF_ROWS, l, self.size(l))

    def pos(self, l):
        return self._view(_lib.GS_FF_POS, l, self.plan.n_nodes)

    def items(self, l):
        return self._view(_lib.GS_FF_ITEMS, l, self.layer_counts(l)[0], 2)

    def split(self, l):
        return self._view(_lib.GS_FF_SPLIT, l, self.layer_counts(l)[1])

    def t_items(self, l):
        return self._view(_lib.GS_FF_T_ITEMS, l, self.layer_counts(l)[2], 2)

    def t_split(self, l):
        return self._view(_lib.GS_FF_T_SPLIT, l, self.layer_counts(l)[3])

    def covers(self, nodes):
        """True when `nodes` (a device int32 vector of unique ids) is the set this field was built for."""
        if nodes is self.nodes and nodes._version == self._nodes_version:
            return True
        if nodes.numel() != self.size(self.n_layers):
            return False
        return bool(torch.equal(torch.sort(nodes).values, self.rows(self.n_layers)))

    def release(self):
        """Free the buffer (the maps go with it); the object cannot be built again."""
        self._buf = None
        self.build_id = 0
        self.nodes = None

    @property
    def ref(self):
        return self._ref


def _field_nodes(nodes, n, device):
    """`nodes` as a device int32 vector of unique ids in [0, n), checked before any launch."""
    import numpy as np
    if isinstance(nodes, torch.Tensor) and nodes.is_cuda:
        if nodes.dtype != torch.int32 or nodes.dim() != 1 or not nodes.is_contiguous() or nodes.numel() < 1:
            raise TypeError("full_field: nodes must be a contiguous 1-D int32 tensor")
        if int(nodes.min()) < 0 or int(nodes.max()) >= n:
            raise IndexError("full_field: node id out of range")
        if int(torch.unique(nodes).numel()) != nodes.numel():
            raise ValueError("full_field: duplicate ids in nodes")
        return nodes
    a = np.asarray(nodes.cpu() if isinstance(nodes, torch.Tensor) else nodes)
    if a.ndim != 1 or a.size < 1 or a.dtype.kind not in "iu":
        raise TypeError("full_field: nodes must be a 1-D array of integer ids")
    if a.min() < 0 or a.max() >= n:
        raise IndexError("full_field: node id out of range")
    if len(np.unique(a)) != a.size:
        raise ValueError("full_field: duplicate ids in nodes")
    return torch.from_numpy(a.astype(np.int32)).to(device)


def full_field(plan, tplan, nodes, n_layers, device=None, out=None):
    """The receptive field of `nodes` over `n_layers` layers, found on the
    device (gs_full_field_build): a ReceptiveField that owns its buffers.
    `nodes`: unique ids, a device int32 vector or a host array (then `device`
    says where to build; default cuda).  `out`: a ReceptiveField of the same
    plans and depth to rebuild in place.  full_field_host is the CPU mirror."""
    if device is None:
        device = nodes.device if isinstance(nodes, torch.Tensor) and nodes.is_cuda else torch.device("cuda")
    nodes = _field_nodes(nodes, plan.n_nodes, device)
    if out is None:
        out = ReceptiveField(plan, tplan, n_layers, device)
    elif out.plan is not plan or out.tplan is not tplan or out.n_layers != int(n_layers):
        raise ValueError("full_field: `out` was made for other plans or another depth")
    return out.build(nodes)


def sage_linear_fwd(A, Wd, out, *, Xs=None, sidx=None, relu=True):
    """relu([Xs[sidx] | A] · Wᵀ) (models.py:209-220); Xs=None is the gcn form."""
    _dev(A, Wd, out, Xs)
    n, F = A.shape
    H = Wd.shape[0]
    K = 2 * F if Xs is not None else F
    if Wd.shape[1] != K or Wd.dtype != A.dtype or (Xs is not None and Xs.dtype != A.dtype):
        raise ValueError(f"weight must be [{H}, {K}] in the activation dtype")
    if out.dtype != torch.float32 or out.shape[0] < n or out.shape[1] < H:
        raise ValueError("out must be fp32 [n, H]")
    check(lib().gs_sage_linear_fwd(_DT[A.dtype], n, F, H, ptr(Xs), Xs.stride(0) if Xs is not None else 0,
                                   ptr(_i32(sidx)), ptr(A), A.stride(0), ptr(Wd), ptr(out),
                                   out.stride(0), int(bool(relu)), _stream(A)))
    return out


def sage1_supported(dtype, F, H, gcn):
    return bool(lib().gs_sage1_fwd_supported(_DT[dtype], F, H, int(bool(gcn))))


def sage1_fwd(agg_func, X, ptr_, ent, col, dst_ids, W, agg_out, out, *, gcn=False, relu=True):
    """Fused layer 1 (gs_sage1_fwd): gather-aggregate over absolute CSR
    entries + relu([X[dst] | agg] · Wᵀ); fills agg_out and out."""
    _dev(X, ptr_, ent, col, dst_ids, W, agg_out, out)  # col None: explicit lists (layers >= 2)
    n_dst = ptr_.numel() - 1
    F = X.shape[1]
    H = W.shape[0]
    if W.dtype != X.dtype or agg_out.dtype != X.dtype or out.dtype != torch.float32:
        raise TypeError("W / agg_out must share X's dtype; out is fp32")
    check(lib().gs_sage1_fwd(agg_op(agg_func), _DT[X.dtype], ptr(X), X.stride(0), F, H, n_dst, ptr(_i32(ptr_)),
                             ptr(_i32(ent)), ptr(_i32(col)), ptr(_i32(dst_ids)), int(bool(gcn)), ptr(W),
                             ptr(agg_out), agg_out.stride(0), ptr(out), out.stride(0), int(bool(relu)),
                             _stream(X)))
    return out


def linear_dw_workspace(n, K, H, device):
    nbytes = int(lib().gs_sage_linear_bwd_weight_ws(n, K, H))
    return torch.empty(max(nbytes // 4, 1), dtype=torch.float32, device=device), nbytes


def sage_linear_bwd_weight(A, dout, out, dW, *, Xs=None, sidx=None, relu=True, ws=None):
    """dW = (dOut ⊙ relu')ᵀ · [Xs[sidx] | A]."""
    _dev(A, dout, out, dW, Xs)
    n, F = A.shape
    H = dW.shape[0]
    K = 2 * F if Xs is not None else F
    if dW.shape[1] != K or dW.dtype != torch.float32:
        raise ValueError("dW must be fp32 [H, K]")
    if ws is None:
        ws, nbytes = linear_dw_workspace(n, K, H, A.device)
    else:
        ws, nbytes = ws
    check(lib().gs_sage_linear_bwd_weight(_DT[A.dtype], n, F, H, ptr(Xs),
                                          Xs.stride(0) if Xs is not None else 0, ptr(_i32(sidx)),
                                          ptr(A), A.stride(0), ptr(dout), ptr(out), out.stride(0),
                                          int(bool(relu)), ptr(dW), ptr(ws), nbytes, _stream(A)))
    return dW


def sage_linear_bwd_input(dout, out, W, dA, *, dSelf=None, relu=True):
    """[dSelf | dA] = (dOut ⊙ relu') · W."""
    _dev(dout, out, W, dA, dSelf)
    n, H = dout.shape
    F = dA.shape[1]
    if dSelf is not None and dSelf.stride(0) != dA.stride(0):
        raise ValueError("dSelf and dA must share a leading dimension")
    check(lib().gs_sage_linear_bwd_input(n, F, H, ptr(dout), ptr(out), out.stride(0), int(bool(relu)),
                                         ptr(W), ptr(dSelf), ptr(dA), dA.stride(0), _stream(dout)))


def agg_bwd(agg_func, tptr, tidx, ptr_, dA, dH, *, dSelf=None, argmax=None, Hprev=None):
    """Transposed gather of the aggregate / self-row gradients (+ relu mask)."""
    _dev(tptr, tidx, ptr_, dA, dH, dSelf, argmax, Hprev)
    n_src = tptr.numel() - 1
    F = dA.shape[1]
    ldh = dH.stride(0)
    if Hprev is not None and Hprev.stride(0) != ldh:
        raise ValueError("Hprev and dH must share a leading dimension")
    check(lib().gs_agg_bwd(agg_op(agg_func), n_src, F, ptr(_i32(tptr)), ptr(_i32(tidx)),
                           ptr(_i32(ptr_)), ptr(dA), ptr(dSelf), dA.stride(0), ptr(_i32(argmax)),
                           ptr(Hprev), ldh, ptr(dH), _stream(dA)))
    return dH


def cls_nll_workspace(B, D, C, device):
    return torch.empty(int(lib().gs_cls_nll_ws_floats(B, D, C)), dtype=torch.float32, device=device)


def cls_nll_fwd_bwd(E, Wc, bc, labels, loss, dE, dWc, dbc, ws, roots=None, mask_relu=False):
    """Classification + NLL forward/backward; labels[roots[i]] is row i's label
    (labels[i] without roots).  mask_relu zeroes dE where E <= 0."""
    _dev(E, Wc, bc, labels, loss, dE, dWc, dbc, ws, roots)
    B, D = E.shape
    C = Wc.shape[0]
    check(lib().gs_cls_nll_fwd_bwd(B, D, C, ptr(E), ptr(Wc), ptr(bc), ptr(_i32(labels)), ptr(_i32(roots)),
                                   int(bool(mask_relu)), ptr(loss),
                                   ptr(dE), ptr(dWc), ptr(dbc), ptr(ws), _stream(E)))


def cls_probe_supported(D, C, batch):
    """gs_cls_probe_supported: the probe kernel's LDS image fits (no device work)."""
    return bool(lib().gs_cls_probe_supported(int(D), int(C), int(batch)))


def cls_probe(E, labels, order, params, batch, lr, max_norm, snapshots=None, losses=None, *,
              max_steps_per_launch=0):
    """train_classification's loop over frozen embeddings (gs_cls_probe_run):
    E [N, D] fp32 with unit column stride, labels [N] int32, order
    [n_epochs, n_train] int32 row ids, params [C*D + C] (W row-major then b,
    updated in place), snapshots [n_epochs, C*D + C] and losses
    [n_epochs, steps] optional.  Ids and labels are not checked here
    (train.ClassifierProbe does).  max_steps_per_launch: a smaller launch cut
    than the library's (the result does not depend on it)."""
    _dev(E, labels, order, params, snapshots, losses)
    if E.dtype != torch.float32 or E.dim() != 2 or E.stride(1) != 1:
        raise ValueError("embeddings must be float32 [N, D] with unit column stride")
    if _i32(order).dim() != 2 or not order.is_contiguous():
        raise ValueError("order must be a contiguous int32 [n_epochs, n_train]")
    if _i32(labels).dim() != 1 or not labels.is_contiguous() or labels.numel() != E.shape[0]:
        raise ValueError("labels must be a contiguous int32 [N]")
    N, D = E.shape
    n_epochs, n_train = order.shape
    P = params.numel()
    if params.dtype != torch.float32 or not params.is_contiguous() or P % (D + 1) != 0 or P == 0:
        raise ValueError("params must be a contiguous float32 [C*D + C]")
    C = P // (D + 1)
    steps = -(-n_train // int(batch)) if int(batch) >= 1 else 0
    for t, shape, what in ((snapshots, n_epochs * P, "snapshots [n_epochs, C*D + C]"),
                           (losses, n_epochs * steps, "losses [n_epochs, steps]")):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != shape):
            raise ValueError(f"{what} must be contiguous float32")
    check(lib().gs_cls_probe_run_ex(ptr(E), E.stride(0), N, D, C, ptr(labels), ptr(order), n_train, int(batch),
                                    n_epochs, ptr(params), float(lr), float(max_norm), ptr(snapshots), ptr(losses),
                                    int(max_steps_per_launch), _stream(E)))
    return params


def cls_probe_host(E, labels, order, params, batch, lr, max_norm, dtype=None):
    """cls_probe in plain numpy, its CPU reference (as full_field_host is of
    full_field): the same step in `dtype` (float64 by default) with numpy's own
    summation order.  Nothing is modified; returns (params, snapshots
    [n_epochs, P], losses [n_epochs, steps])."""
    import numpy as np
    dt = np.dtype(np.float64 if dtype is None else dtype).type
    E = np.asarray(E, dt)
    labels = np.asarray(labels, np.int64).reshape(-1)
    order = np.asarray(order, np.int64)
    if E.ndim != 2 or order.ndim != 2 or len(labels) != len(E):
        raise ValueError("cls_probe_host: E [N, D], labels [N], order [n_epochs, n_train]")
    if order.size and (order.min() < 0 or order.max() >= len(E)):
        raise IndexError("cls_probe_host: row id out of range")
    N, D = E.shape
    p = np.array(params, dt).reshape(-1)
    if p.size == 0 or p.size % (D + 1):
        raise ValueError("cls_probe_host: params must hold C*D + C values")
    C = p.size // (D + 1)
    batch = int(batch)
    if batch < 1 or order.shape[0] < 1 or order.shape[1] < 1:
        raise ValueError("cls_probe_host: batch, n_epochs and n_train must be >= 1")
    n_epochs, n_train = order.shape
    steps = -(-n_train // batch)
    lr, max_norm, eps = dt(lr), dt(max_norm), dt(1e-6)
    W, b = p[:C * D].reshape(C, D), p[C * D:]
    snaps = np.empty((n_epochs, p.size), dt)
    losses = np.empty((n_epochs, steps), dt)
    for e in range(n_epochs):
        for s in range(steps):
            rows = order[e, s * batch:(s + 1) * batch]
            n = len(rows)
            X, y = E[rows], labels[rows]
            z = X @ W.T + b
            z = z - z.max(1, keepdims=True)
            logp = z - np.log(np.exp(z).sum(1, keepdims=True))
            has = (y >= 0) & (y < C)  # outside [0, C): no class
            losses[e, s] = -logp[np.nonzero(has)[0], y[has]].sum() / dt(n)
            G = np.exp(logp)
            G[np.nonzero(has)[0], y[has]] -= dt(1)
            G = G / dt(n)
            dW, db = G.T @ X, G.sum(0)
            norm = np.sqrt((dW * dW).sum() + (db * db).sum())
            coef = min(dt(1), max_norm / (norm + eps))
            W -= lr * (dW * coef)  # views of p
            b -= lr * (db * coef)
        snaps[e] = p
    return p.copy(), snaps, losses


def cls_eval(H, labels, params, C, rows=None, labels_by_row=True, n_sets=1, set_stride=None, want_pred=True,
             want_logp=False):
    """The classifier head forward only (gs_cls_eval): log_softmax(H[rows]·Wcᵀ
    + bc), its argmax (the lowest index among the maxima), the mean NLL and the
    confusion matrix, for n_sets parameter sets at once.

    H [*, D] fp32 with unit column stride; rows: None (every row of H) or [B]
    int32 ids into H (not checked here: the caller guarantees them); labels
    int32, row i's label labels[rows[i]] (labels_by_row, with rows) or
    labels[i]; params: a contiguous fp32 vector whose set s starts at
    s·set_stride (default C·D + C) and holds Wc [C, D] row-major, then bc [C].
    A label outside [0, C) leaves its row out of the loss and the matrix and
    counts it in n_bad.  Returns (loss [n_sets], counts [n_sets, C·C + 2] int64
    -- counts[y·C + pred], then n_counted and n_bad --, pred [n_sets, B] int32
    or None, logp [n_sets, B, C] or None) on the device; nothing here waits
    for the device."""
    _dev(H, labels, params, rows)
    if H.dtype != torch.float32 or H.dim() != 2 or H.stride(1) != 1 or H.shape[0] < 1 or H.shape[1] < 1:
        raise ValueError("H must be float32 [N, D] with unit column stride")
    D, C, n_sets = int(H.shape[1]), int(C), int(n_sets)
    if C < 1 or n_sets < 1:
        raise ValueError("C and n_sets must be >= 1")
    if rows is not None and (_i32(rows).dim() != 1 or not rows.is_contiguous() or rows.numel() < 1):
        raise ValueError("rows must be a contiguous int32 vector of at least one id")
    B = int(H.shape[0] if rows is None else rows.numel())
    by_row = bool(labels_by_row) and rows is not None
    if _i32(labels).dim() != 1 or not labels.is_contiguous() or labels.numel() < (H.shape[0] if by_row else B):
        raise ValueError("labels must be a contiguous int32 vector, one per row of H (labels_by_row) or per "
                         "evaluated row")
    stride = C * D + C if set_stride is None else int(set_stride)
    if params.dtype != torch.float32 or params.dim() != 1 or not params.is_contiguous():
        raise ValueError("params must be a contiguous float32 vector")
    if stride < C * D + C or params.numel() < (n_sets - 1) * stride + C * D + C:
        raise ValueError("params must hold n_sets sets of C*D + C values, set_stride >= C*D + C apart")
    dev = H.device
    need = int(lib().gs_cls_eval_ws_bytes(B, D, C, n_sets))
    if need < 0:
        check(_lib.GS_EINVAL)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    loss = torch.empty(n_sets, dtype=torch.float32, device=dev)
    counts = torch.empty(n_sets, C * C + 2, dtype=torch.int64, device=dev)
    pred = torch.empty(n_sets, B, dtype=torch.int32, device=dev) if want_pred else None
    logp = torch.empty(n_sets, B, C, dtype=torch.float32, device=dev) if want_logp else None
    check(lib().gs_cls_eval(B, D, C, ptr(H), H.stride(0), ptr(rows), ptr(labels), int(by_row), ptr(params), n_sets,
                            stride, ptr(pred), ptr(logp), ptr(loss), ptr(counts), ptr(ws), need, _stream(H)))
    return loss, counts, pred, logp


def cls_eval_host(H, labels, params, C, rows=None, labels_by_row=True, n_sets=1, set_stride=None, dtype=None):
    """cls_eval in plain numpy, its CPU reference: the same function in
    `dtype` (float64 by default) with numpy's own summation order, the same tie
    rule (np.argmax: the lowest index among the maxima, a NaN is maximal and
    the first NaN wins) and the same bad-label rule.  Returns (loss [n_sets],
    counts [n_sets, C·C + 2] int64, pred [n_sets, B] int32, logp
    [n_sets, B, C])."""
    import numpy as np
    dt = np.dtype(np.float64 if dtype is None else dtype).type
    H = np.asarray(H)
    if H.ndim != 2 or H.shape[0] < 1 or H.shape[1] < 1:
        raise ValueError("cls_eval_host: H [N, D]")
    D, C, n_sets = H.shape[1], int(C), int(n_sets)
    if C < 1 or n_sets < 1:
        raise ValueError("cls_eval_host: C and n_sets must be >= 1")
    labels = np.asarray(labels, np.int64).reshape(-1)
    if rows is None:
        X, y = H.astype(dt), labels[:H.shape[0]]
    else:
        rows = np.asarray(rows, np.int64).reshape(-1)
        if rows.size < 1 or rows.min() < 0 or rows.max() >= H.shape[0]:
            raise IndexError("cls_eval_host: row id out of range")
        X, y = H[rows].astype(dt), labels[rows] if labels_by_row else labels[:rows.size]
    B = X.shape[0]
    if len(y) != B:
        raise ValueError("cls_eval_host: too few labels")
    stride = C * D + C if set_stride is None else int(set_stride)
    p = np.asarray(params).reshape(-1)
    if stride < C * D + C or p.size < (n_sets - 1) * stride + C * D + C:
        raise ValueError("cls_eval_host: params must hold n_sets sets of C*D + C values")
    has = (y >= 0) & (y < C)  # outside [0, C): not counted
    idx, yh = np.nonzero(has)[0], y[has]
    loss = np.empty(n_sets, dt)
    counts = np.zeros((n_sets, C * C + 2), np.int64)
    pred = np.empty((n_sets, B), np.int32)
    logp = np.empty((n_sets, B, C), dt)
    with np.errstate(invalid="ignore", divide="ignore"):
        for s in range(n_sets):
            W = p[s * stride:s * stride + C * D].reshape(C, D).astype(dt)
            b = p[s * stride + C * D:s * stride + C * D + C].astype(dt)
            z = X @ W.T + b
            pred[s] = np.argmax(z, 1)
            zs = z - z.max(1, keepdims=True)
            logp[s] = zs - np.log(np.exp(zs).sum(1, keepdims=True))
            loss[s] = -logp[s][idx, yh].sum(dtype=dt) / dt(len(idx)) if len(idx) else dt(np.nan)
            counts[s, :C * C] = np.bincount(yh * C + pred[s][has], minlength=C * C)
            counts[s, C * C], counts[s, C * C + 1] = len(idx), B - len(idx)
    return loss, counts, pred, logp


def multilabel_words(C):
    """int32 words per node of packed multi-label targets: ceil(C / 32)."""
    return (int(C) + 31) // 32


def pack_multilabel(y):
    """[N, C] hard multi-label targets (bool, uint8, or a 0/1 integer or float
    tensor) as the packed int32 words [N, ceil(C / 32)] the multi-label head
    reads: label c is bit c % 32 of word c // 32, the bits at or above C are
    zero.  Torch ops on y's own device.  Anything other than 0 or 1 raises
    ValueError (soft targets are out of scope)."""
    if not isinstance(y, torch.Tensor) or y.dim() != 2 or y.shape[0] < 1 or y.shape[1] < 1:
        raise ValueError("pack_multilabel: y must be a tensor [N, C] with N, C >= 1")
    if y.dtype != torch.bool:
        if y.dtype.is_complex or not bool(((y == 0) | (y == 1)).all()):
            raise ValueError("pack_multilabel: targets must be 0 or 1 (soft targets are not supported)")
        y = y != 0
    N, C = y.shape
    nW = multilabel_words(C)
    bits = torch.zeros(N, nW * 32, dtype=torch.int64, device=y.device)
    bits[:, :C] = y
    shifts = torch.arange(32, dtype=torch.int64, device=y.device)
    words = (bits.view(N, nW, 32) << shifts).sum(-1)           # in [0, 2^32)
    words = torch.where(words >= 2 ** 31, words - 2 ** 32, words)  # the bit pattern as an int32
    return words.to(torch.int32).contiguous()


def unpack_multilabel(words, C):
    """pack_multilabel's inverse: int32 [N, ceil(C / 32)] to bool [N, C] (bits at or above C are dropped)."""
    C = int(C)
    if not isinstance(words, torch.Tensor) or words.dtype != torch.int32 or words.dim() != 2 or C < 1 or \
            words.shape[1] != multilabel_words(C):
        raise ValueError("unpack_multilabel: words must be int32 [N, ceil(C / 32)]")
    shifts = torch.arange(32, dtype=torch.int64, device=words.device)
    bits = (words.to(torch.int64).unsqueeze(-1) >> shifts) & 1
    return bits.reshape(words.shape[0], -1)[:, :C].bool()


def cls_bce_supported(D, C):
    """gs_cls_bce_supported: the multi-label head's LDS image and accumulators fit (no device work)."""
    return bool(lib().gs_cls_bce_supported(int(D), int(C)))


def _bce_params(name, Wc, bc, pos_weight, D):
    if Wc.dtype != torch.float32 or Wc.dim() != 2 or not Wc.is_contiguous() or Wc.shape[1] != D or Wc.shape[0] < 1:
        raise ValueError(f"{name}: Wc must be a contiguous float32 [C, D]")
    C = int(Wc.shape[0])
    if bc.dtype != torch.float32 or bc.dim() != 1 or not bc.is_contiguous() or bc.numel() != C:
        raise ValueError(f"{name}: bc must be a contiguous float32 [C]")
    if pos_weight is not None and (pos_weight.dtype != torch.float32 or pos_weight.dim() != 1 or
                                   not pos_weight.is_contiguous() or pos_weight.numel() != C):
        raise ValueError(f"{name}: pos_weight must be a contiguous float32 [C]")
    if not cls_bce_supported(D, C):
        raise ValueError(f"{name}: (D, C) = ({D}, {C}) does not fit the multi-label head (gs_cls_bce_supported)")
    return C


def _bce_targets(name, targets, C, n_min):
    if _i32(targets).dim() != 2 or not targets.is_contiguous() or targets.shape[1] != multilabel_words(C) or \
            targets.shape[0] < n_min:
        raise ValueError(f"{name}: targets must be contiguous int32 [n, ceil(C / 32)] packed words "
                         "(pack_multilabel), one row per node")


def cls_bce(E, Wc, bc, targets, roots=None, pos_weight=None, mask_relu=False):
    """The multi-label head, forward + backward (gs_cls_bce_fwd_bwd):
    binary_cross_entropy_with_logits(E·Wcᵀ + bc, y, pos_weight=, reduction=
    "mean") and its gradients.  E [B, D] fp32 with unit column stride (any row
    stride); targets: packed int32 words (pack_multilabel), row i's are node
    roots[i]'s (roots: [B] int32 ids, not checked here) or node i's;
    mask_relu zeroes dE where E <= 0.  Returns (loss 0-d, dE [B, D], dWc
    [C, D], dbc [C]) on the device; nothing waits for it."""
    _dev(E, Wc, bc, targets, roots, pos_weight)
    if E.dtype != torch.float32 or E.dim() != 2 or E.stride(1) != 1 or E.shape[0] < 1 or E.shape[1] < 1:
        raise ValueError("cls_bce: E must be float32 [B, D] with unit column stride")
    B, D = int(E.shape[0]), int(E.shape[1])
    C = _bce_params("cls_bce", Wc, bc, pos_weight, D)
    if roots is not None and (_i32(roots).dim() != 1 or not roots.is_contiguous() or roots.numel() != B):
        raise ValueError("cls_bce: roots must be a contiguous int32 [B]")
    _bce_targets("cls_bce", targets, C, 1 if roots is not None else B)
    dev = E.device
    need = int(lib().gs_cls_bce_ws_bytes(B, D, C))
    if need < 0:
        check(_lib.GS_EINVAL)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    dE = torch.empty(B, D, dtype=torch.float32, device=dev)
    dWc = torch.empty(C, D, dtype=torch.float32, device=dev)
    dbc = torch.empty(C, dtype=torch.float32, device=dev)
    check(lib().gs_cls_bce_fwd_bwd(B, D, C, ptr(E), E.stride(0), ptr(Wc), ptr(bc), ptr(targets), ptr(roots),
                                   ptr(pos_weight), int(bool(mask_relu)), ptr(loss), ptr(dE), ptr(dWc), ptr(dbc),
                                   ptr(ws), need, _stream(E)))
    return loss, dE, dWc, dbc


def cls_bce_eval(H, targets, Wc, bc, rows=None, targets_by_row=True, pos_weight=None, want_pred=True,
                 want_logits=False):
    """The multi-label head forward only (gs_cls_bce_eval) over H[rows] (rows:
    None, or [B] int32 ids into H, not checked here): the BCE mean, the
    predictions z > 0 as packed words in the targets' layout, the per-label
    counts and the number of rows with every label right.  Row i's targets are
    node rows[i]'s (targets_by_row, with rows) or node i's.  Returns (loss
    0-d, counts [C, 3] int64 -- true positives, false positives, false
    negatives --, n_exact 0-d int64, pred [B, ceil(C / 32)] int32 or None,
    logits [B, C] or None) on the device; counts and n_exact are views of one
    buffer."""
    _dev(H, targets, Wc, bc, rows, pos_weight)
    if H.dtype != torch.float32 or H.dim() != 2 or H.stride(1) != 1 or H.shape[0] < 1 or H.shape[1] < 1:
        raise ValueError("cls_bce_eval: H must be float32 [N, D] with unit column stride")
    D = int(H.shape[1])
    C = _bce_params("cls_bce_eval", Wc, bc, pos_weight, D)
    if rows is not None and (_i32(rows).dim() != 1 or not rows.is_contiguous() or rows.numel() < 1):
        raise ValueError("cls_bce_eval: rows must be a contiguous int32 vector of at least one id")
    B = int(H.shape[0] if rows is None else rows.numel())
    by_row = bool(targets_by_row) and rows is not None
    _bce_targets("cls_bce_eval", targets, C, H.shape[0] if by_row else B)
    dev = H.device
    need = int(lib().gs_cls_bce_eval_ws_bytes(B, D, C))
    if need < 0:
        check(_lib.GS_EINVAL)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    counts = torch.empty(3 * C + 1, dtype=torch.int64, device=dev)
    pred = torch.empty(B, multilabel_words(C), dtype=torch.int32, device=dev) if want_pred else None
    logits = torch.empty(B, C, dtype=torch.float32, device=dev) if want_logits else None
    check(lib().gs_cls_bce_eval(B, D, C, ptr(H), H.stride(0), ptr(rows), ptr(targets), int(by_row), ptr(Wc), ptr(bc),
                                ptr(pos_weight), ptr(pred), ptr(logits), ptr(loss), ptr(counts), ptr(ws), need,
                                _stream(H)))
    return loss, counts[:3 * C].view(C, 3), counts[3 * C], pred, logits


def _bce_host_args(name, X, Wc, bc, y, pos_weight, dt):
    import numpy as np
    X, Wc, bc = np.asarray(X, dt), np.asarray(Wc, dt), np.asarray(bc, dt).reshape(-1)
    if X.ndim != 2 or Wc.ndim != 2 or Wc.shape[1] != X.shape[1] or bc.size != Wc.shape[0] or X.shape[0] < 1:
        raise ValueError(f"{name}: E [B, D], Wc [C, D], bc [C]")
    y = np.asarray(y)
    if y.shape != (X.shape[0], Wc.shape[0]) or not np.isin(y, (0, 1)).all():
        raise ValueError(f"{name}: y must be [B, C] of 0 / 1")
    pw = np.ones(Wc.shape[0], dt) if pos_weight is None else np.asarray(pos_weight, dt).reshape(-1)
    if pw.size != Wc.shape[0]:
        raise ValueError(f"{name}: pos_weight [C]")
    return X, Wc, bc, y.astype(dt), pw


def _bce_host_terms(z, y, pw):
    import numpy as np
    w = 1.0 + (pw - 1.0) * y
    e = np.exp(-np.abs(z))
    l = (1.0 - y) * z + w * (np.log1p(e) + np.maximum(-z, 0.0))
    sig = np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    return l, sig, w


def cls_bce_host(E, Wc, bc, y, pos_weight=None, mask_relu=False, dtype=None):
    """cls_bce in plain numpy, its CPU reference: the same function in `dtype`
    (float64 by default) over unpacked targets y [B, C] of 0 / 1 (row i's own:
    gather by roots before the call).  Returns (loss, dE, dWc, dbc, z)."""
    import numpy as np
    dt = np.dtype(np.float64 if dtype is None else dtype).type
    X, Wc, bc, y, pw = _bce_host_args("cls_bce_host", E, Wc, bc, y, pos_weight, dt)
    z = X @ Wc.T + bc
    l, sig, w = _bce_host_terms(z, y, pw)
    n = dt(z.size)
    dz = (sig * w - pw * y) / n
    dE = dz @ Wc
    if mask_relu:
        dE = np.where(X <= 0, dt(0), dE)
    return l.sum(dtype=dt) / n, dE, dz.T @ X, dz.sum(0), z


def cls_bce_eval_host(H, y, Wc, bc, rows=None, pos_weight=None, dtype=None):
    """cls_bce_eval in plain numpy, its CPU reference: y [B, C] of 0 / 1 are the
    evaluated rows' own targets.  Returns (loss, counts [C, 3] int64, n_exact,
    pred bool [B, C], z [B, C])."""
    import numpy as np
    dt = np.dtype(np.float64 if dtype is None else dtype).type
    H = np.asarray(H)
    if rows is not None:
        rows = np.asarray(rows, np.int64).reshape(-1)
        if rows.size < 1 or rows.min() < 0 or rows.max() >= H.shape[0]:
            raise IndexError("cls_bce_eval_host: row id out of range")
        H = H[rows]
    X, Wc, bc, y, pw = _bce_host_args("cls_bce_eval_host", H, Wc, bc, y, pos_weight, dt)
    z = X @ Wc.T + bc
    l, _sig, _w = _bce_host_terms(z, y, pw)
    pred = z > 0
    yb = y > 0
    counts = np.stack([(pred & yb).sum(0), (pred & ~yb).sum(0), (~pred & yb).sum(0)], 1).astype(np.int64)
    return l.sum(dtype=dt) / dt(z.size), counts, int((pred == yb).all(1).sum()), pred, z


def unsup_loss_workspace(M, P, N, device):
    """The buffer unsup_loss_fwd leaves for unsup_loss_bwd: {coef, cos, n1, n2} per pair (the P positive
    pairs, then the N negative ones), then the M node scores at float offset 4 (P + N)."""
    return torch.empty(int(lib().gs_unsup_loss_ws_floats(M, P, N)), dtype=torch.float32, device=device)


def _unsup_args(E, plan, dims, ws):
    M, P, N, U = (int(x) for x in dims)
    if E.dtype != torch.float32 or E.dim() != 2 or E.stride(1) != 1 or E.shape[0] < U:
        raise ValueError("embeddings must be float32 [U, D] with unit column stride")
    if _i32(plan).dim() != 1 or not plan.is_contiguous() or plan.numel() < 2 * (M + 1) + 4 * (P + N) + U + 1:
        raise ValueError("plan is shorter than its dims say")
    if ws.dtype != torch.float32 or ws.dim() != 1 or not ws.is_contiguous() or ws.numel() < 4 * (P + N) + M:
        raise ValueError("workspace must hold unsup_loss_workspace(M, P, N) floats")
    return M, P, N, U


def unsup_loss_fwd(kind, E, plan, dims, q, margin, ws):
    """get_loss_sage (kind 0) / get_loss_margin (kind 1) over a device copy of gs_unsup_loss_plan
    (gs_unsup_loss_fwd); dims = (M, P, N, U).  E is read as given, with its row stride; rows that are
    not 16-byte aligned are refused (ValueError).  Fills ws, returns the loss (a 0-d tensor)."""
    _dev(E, plan, ws)
    M, P, N, U = _unsup_args(E, plan, dims, ws)
    loss = torch.empty((), dtype=torch.float32, device=E.device)
    check(lib().gs_unsup_loss_fwd(int(kind), M, P, N, U, E.shape[1], ptr(E), E.stride(0), ptr(plan), float(q),
                                  float(margin), ptr(loss), ptr(ws), _stream(E)))
    return loss


def unsup_loss_bwd(E, plan, dims, ws, dloss, dE):
    """dE = dloss * d loss / d E from the ws of unsup_loss_fwd on the same E and plan (gs_unsup_loss_bwd);
    dloss: one float32 on the device.  Writes the rows [0, U) of dE over E's width, with dE's own stride."""
    _dev(E, plan, ws, dloss, dE)
    M, P, N, U = _unsup_args(E, plan, dims, ws)
    if dE.dtype != torch.float32 or dE.dim() != 2 or dE.stride(1) != 1 or dE.shape[0] < U or \
            dE.shape[1] != E.shape[1]:
        raise ValueError("dE must be float32 [U, D] with unit column stride")
    if dloss.dtype != torch.float32 or dloss.numel() != 1:
        raise ValueError("dloss must be one float32")
    check(lib().gs_unsup_loss_bwd(M, P, N, U, E.shape[1], ptr(E), E.stride(0), ptr(plan), ptr(ws), ptr(dloss),
                                  ptr(dE), dE.stride(0), _stream(E)))
    return dE


def clip_sgd(goff, params, grads, grad_scale, max_norm, lr, ws):
    import numpy as np
    _dev(params, grads, ws)
    go = np.ascontiguousarray(goff, dtype=np.int64)
    check(lib().gs_clip_sgd(len(go) - 1, ptr(go), ptr(params), ptr(grads), float(grad_scale),
                            float(max_norm), float(lr), ptr(ws), _stream(params)))


def clip_adam(goff, params, grads, m, v, grad_scale, max_norm, lr, betas, eps, weight_decay, step, ws):
    """gs_clip_adam: clip per group (the clipped gradient stays in `grads`),
    then one AdamW update of `params` and the moments `m`, `v` in place;
    `step` >= 1 numbers the update being applied."""
    import numpy as np
    _dev(params, grads, m, v, ws)
    go = np.ascontiguousarray(goff, dtype=np.int64)
    check(lib().gs_clip_adam(len(go) - 1, ptr(go), ptr(params), ptr(grads), ptr(m), ptr(v), float(grad_scale),
                             float(max_norm), float(lr), float(betas[0]), float(betas[1]), float(eps),
                             float(weight_decay), int(step), ptr(ws), _stream(params)))


def fill_uniform(X, seed):
    _dev(X)
    check(lib().gs_fill_uniform(ptr(X), _DT[X.dtype], X.shape[0], X.shape[1], X.stride(0),
                                int(seed) & 0xFFFFFFFFFFFFFFFF, _stream(X)))
    return X


def cast_bf16(src, dst):
    _dev(src, dst)
    if src.numel() != dst.numel() or dst.dtype != torch.bfloat16 or src.dtype != torch.float32:
        raise ValueError("cast_bf16: fp32 -> bf16 of equal size")
    check(lib().gs_cast_f32_bf16(ptr(src), ptr(dst), src.numel(), _stream(src)))
    return dst
