"""The shape matrix of the native step's float64 comparison (no tests here).

Each row names the smallest shape that still reaches the kernel path its
"reaches" entry claims; test_step_ref_host.py evaluates the predicates below
(the dispatch rules of step.hip, bwd.hip, linear.hip and step_update.hip
restated in Python) on every row and checks the claim, and
test_gpu_step_matrix.py runs the rows on the device.

Graphs come from tests/golden/graphs.npz: the tiny R-MAT (436 nodes), or
Pubmed's for the `slabs` row.  Features are uniform_features, labels
arange % C.  Batch i of a row is the first B entries of a permutation of the
nodes with degree > 0 under seed SEED + i (`dup`: 32 of them, then the first 8
again); the sampler stream is RNG(SEED).  Under these seeds no destination of
any hop has an empty neighbourhood (checked on the CPU), so no row needs a
skip.

bf16 rows use MAX on purpose: MAX selects, so the reference's bf16 rounding
points are the kernel's.  A bf16 MEAN rounds an fp32 sum, and a float64
reference differs by a whole bf16 ulp wherever the two sums straddle a
rounding boundary; bf16 MEAN stays with the bitwise tests.

FACTOR: check_rule's factor (err <= factor * e_torch + 2^-23 * max|ref|) is
the Adam work's 4 unless a row says otherwise here, with its reason.
"""
import importlib
import os

import numpy as np

from tests.golden.synth import uniform_features

G = os.path.join(os.path.dirname(__file__), "golden")
SEED = 824
N_BATCHES = 4      # the runner tests' batches; the step tests use the first 2
LR = 0.7
MAX_NORMS = (5.0, 0.05)   # step 1: the reference's; step 2: small enough to clip both groups


def _row(id, L, fanouts, F, H, C, agg, gcn, feat, B, reaches, graph="rmat", dup=0):
    return {"id": id, "L": L, "fanouts": list(fanouts), "F": F, "H": H, "C": C, "agg": agg, "gcn": gcn,
            "bf16": feat == "bf16", "B": B, "reaches": reaches, "graph": graph, "dup": dup}


# reaches: predicate name -> the value it must take (a (lo, hi) pair: a range, None = open)
CASES = [
    # control: top launch, float4 update
    _row("bench", 2, (25, 10), 256, 128, 16, "MEAN", False, "f32", 48,
         {"top": True, "update": "float4", "vload": True, "group": 32, "defer": True}),
    # no top launch; fused bwd G = 16; K chunk of 100; scalar update
    _row("h64", 2, (25, 10), 100, 64, 7, "MEAN", False, "f32", 97,
         {"top": False, "fused": True, "group": 16, "vload": True, "update": "scalar", "defer": False}),
    # smallest H and F; ragged 16-row tiles
    _row("tiny", 2, (5, 3), 8, 16, 3, "MAX", False, "f32", 33,
         {"top": False, "group": 16, "col_tiles": 1, "partial_tile": True, "ragged_rows": True, "defer": False}),
    # rows not 16-B aligned: scalar-load forward, dW, gather; partial 64-column tile
    _row("unal", 2, (10, 5), 50, 48, 5, "MEAN", True, "f32", 64,
         {"vload": False, "partial_tile": True, "col_tiles": 1, "top": False, "defer": False}),
    # G = 32 partly filled; 2 layer-2 dW slabs; argmax backward
    _row("h80", 2, (15, 5), 36, 80, 19, "MAX", False, "f32", 130,
         {"group": 32, "group_lanes": 20, "dw_slabs_2": 2, "col_tiles": 2, "partial_tile": True, "top": False,
          "defer": False}),
    # G = 64; 4 column tiles; K2 = 512; general head
    _row("h256", 2, (10, 5), 64, 256, 33, "MEAN", False, "f32", 40,
         {"group": 64, "col_tiles": 4, "K_2": 512, "top": False, "defer": False}),
    # H = 128 but one class past the top launch
    _row("c33", 2, (25, 10), 256, 128, 33, "MEAN", False, "f32", 97,
         {"top": False, "group": 32, "fused": True, "defer": False}),
    # gcn at more than one slab (K = F, no self half)
    _row("gcn", 2, (25, 10), 256, 128, 16, "MAX", True, "f32", 96,
         {"top": False, "K_1": 256, "K_2": 128, "dw_slabs_1": (2, None), "defer": False}),
    # one layer: backward_unfused, roots are layer 1's rows
    _row("l1", 1, (10,), 256, 128, 16, "MEAN", False, "f32", 97,
         {"fused": False, "top": False, "rows_1": 97, "defer": False}),
    # one layer, Cora's width
    _row("l1g", 1, (10,), 1433, 32, 7, "MAX", True, "f32", 37,
         {"fused": False, "vload": False, "K_1": 1433, "rows_1": 37, "defer": False}),
    # two fused upper layers, dbuf ping-pong
    _row("l3", 3, (10, 5, 5), 256, 128, 16, "MEAN", False, "f32", 48,
         {"fused": True, "fused_layers": 2, "top": False, "group": 32, "defer": False}),
    # the same, off 128, MAX, gcn
    _row("l3m", 3, (5, 5, 3), 64, 64, 5, "MAX", True, "f32", 32,
         {"fused": True, "fused_layers": 2, "top": False, "group": 16, "defer": False}),
    # bf16 on the top path (cast W1)
    _row("bfm", 2, (25, 10), 256, 128, 16, "MAX", False, "bf16", 48,
         {"top": True, "vload": True, "update": "float4", "defer": True}),
    # bf16 with F % 8 != 0: scalar bf16 loads
    _row("bfu", 2, (10, 5), 100, 64, 7, "MAX", False, "bf16", 64,
         {"vload": False, "top": False, "group": 16, "defer": False}),
    # 8 of the 40 roots repeated: several destinations per source in the transposed lists
    _row("dup", 2, (25, 10), 256, 128, 16, "MEAN", False, "f32", 40,
         {"top": True, "defer": True, "repeated_roots": 8}, dup=8),
    # Pubmed graph: > 8 layer-2 slabs (grouped sum) off H = 128; several row tiles per workgroup
    _row("slabs", 2, (25, 10), 256, 64, 3, "MEAN", False, "f32", 1100,
         {"dw_slabs_2": (9, None), "group": 16, "top": False, "fwd_row_tiles": (2, None), "defer": False},
         graph="pubmed"),
]
BY_ID = {c["id"]: c for c in CASES}
IDS = [c["id"] for c in CASES]

# check_rule factors above 4, {row id: {tensor name: (factor, reason)}}: twice the ratio observed on
# the MI355X, rounded up to a power of two, never above 16 (DESIGN §4 holds every observed ratio)
_SERIAL_K = ("F = 1433 fails the 16-byte rule, so layer 1 runs linear_fwd_kernel, whose one fp32 accumulator per "
             "output takes all K = 1433 products in a single serial MFMA chain (359 x 16x16x4); the CPU GEMM of "
             "the fp32 yardstick blocks and vectorises its sums.  A serial fp32 FMA chain over the same operands "
             "on the CPU has the kernel's error to 1 % (1.02e-5 against 1.03e-5 at step 2), so the order is "
             "valid; observed err / e_torch 7.04, factor 16")
FACTOR = {"l1g": {"emb_fwd": (16.0, _SERIAL_K), "emb": (16.0, _SERIAL_K)}}


def factor(case_id, tensor):
    return FACTOR.get(case_id, {}).get(tensor, (4.0, ""))[0]


# ------------------------------------------------------------- the workload
_GRAPHS = {}


def graph_of(name):
    """(CSRGraph, n_nodes, row_ptr, col) of a golden graph; built once."""
    if name not in _GRAPHS:
        gs = importlib.import_module("graphsage-pytorch_amd")
        g = np.load(os.path.join(G, "graphs.npz"))
        n = int(g[f"{name}_n"][0])
        graph = gs.CSRGraph.from_pairs(g[f"{name}_src"], g[f"{name}_dst"], n)
        _GRAPHS[name] = (graph, n, graph.row_ptr(), graph.col())
    return _GRAPHS[name]


def adjacency_of(name):
    """The oracle's adjacency of the same graph."""
    import oracle
    g = np.load(os.path.join(G, "graphs.npz"))
    return oracle.Adjacency(g[f"{name}_src"], g[f"{name}_dst"], int(g[f"{name}_n"][0]))


def features_of(case):
    """The row's feature table as numpy fp32 (bf16 rows: bf16-representable values)."""
    _graph, n, _rp, _col = graph_of(case["graph"])
    X = uniform_features(5, n, case["F"])
    if case["bf16"]:
        import torch
        X = torch.from_numpy(X).to(torch.bfloat16).float().numpy()
    return X


def labels_of(case):
    return (np.arange(graph_of(case["graph"])[1]) % case["C"]).astype(np.int32)


def batches_of(case, n=N_BATCHES):
    graph = graph_of(case["graph"])[0]
    cands = np.nonzero(graph.degrees())[0].astype(np.int64)
    out = []
    for i in range(n):
        perm = np.random.RandomState(SEED + i).permutation(cands)
        base = perm[:case["B"] - case["dup"]]
        out.append(np.concatenate([base, base[:case["dup"]]]))
    return out


def samples_of(case, n=N_BATCHES):
    """The row's first n batches sampled on one host stream RNG(SEED): [(roots, Sample)]."""
    gs = importlib.import_module("graphsage-pytorch_amd")
    graph = graph_of(case["graph"])[0]
    rng = gs.RNG(SEED)
    return [(roots, gs.sample(graph, rng, roots, case["fanouts"], gcn=case["gcn"])) for roots in batches_of(case, n)]


# ------------------------------------------- the dispatch rules, restated
def pick_group(H, vec=4):
    """agg_dev.hpp pick_group: lanes of the fused backward's aggregate group."""
    lanes = (H + vec - 1) // vec
    g = 16
    while g < lanes and g < 64:
        g <<= 1
    return g


def dw_splits(n, K, H, phases=1):
    """linear_dev.hpp dw_splits: row slabs of a weight gradient over n rows."""
    tiles = ((K + 63) // 64) * ((H + 63) // 64)
    want = max(1, (512 // phases + tiles - 1) // tiles)
    cap = max(1, n // 64)
    S = max(min(want, cap), (n + 2047) // 2048)
    rows = (n + S - 1) // S
    rps = min(2048, max(16, (rows + 15) // 16 * 16))
    return max(1, (n + rps - 1) // rps)


def total_params(case):
    L, F, H, C = case["L"], case["F"], case["H"], case["C"]
    m = 1 if case["gcn"] else 2
    return sum(H * m * (F if l == 1 else H) for l in range(1, L + 1)) + C * H + C


def predicates(case, sample, roots):
    """What one step of `case` on `sample` dispatches to."""
    L, F, H, C, gcn = case["L"], case["F"], case["H"], case["C"], case["gcn"]
    epv = 8 if case["bf16"] else 4
    m = 1 if gcn else 2
    total = total_params(case)
    top = H == 128 and C <= 32 and not gcn and L == 2
    rows = {l: sample.sizes(L - l + 1)[0] for l in range(1, L + 1)}
    K = {l: m * (F if l == 1 else H) for l in range(1, L + 1)}
    # linear_fwd_launch's wide form: 16-row tiles balanced over one workgroup per CU (256) and column tile
    tiles, groups = (rows[1] + 15) // 16, max(1, 256 // ((H + 63) // 64))
    per = (tiles + groups - 1) // groups
    if per > 4:
        per = (tiles + groups * ((per + 3) // 4) - 1) // (groups * ((per + 3) // 4))
    out = {
        "top": top,
        "fwd_row_tiles": per if F % epv == 0 else 1,   # row tiles per workgroup of the layer-1 forward
        "fused": L >= 2,                   # backward_unfused otherwise
        "fused_layers": L - 1,
        "group": pick_group(H),
        "group_lanes": (H + 3) // 4,
        "vload": F % epv == 0,             # fwd_vload / linear_dw_slabs' vload (the rows are 16-B aligned)
        "col_tiles": (H + 63) // 64,
        "partial_tile": H % 64 != 0,
        "ragged_rows": any(r % 16 != 0 for r in rows.values()),
        "update": "float4" if total % 4 == 0 and (H * sum(K.values())) % 4 == 0 else "scalar",
        # trainer_defer_update: SGD, two layers, no gcn, the switches on, 16-B rows, every offset a multiple of 4
        "defer": L == 2 and not gcn and F % epv == 0 and (H * K[1]) % 4 == 0 and total % 4 == 0
        and (H * (K[1] + K.get(2, 0))) % 4 == 0,
        "repeated_roots": len(roots) - len(set(int(x) for x in roots)),
    }
    for l in range(1, L + 1):
        out[f"rows_{l}"] = rows[l]
        out[f"K_{l}"] = K[l]
        # layer 1 in two row phases (kDw1Phases), the layers above in one
        out[f"dw_slabs_{l}"] = dw_splits(rows[l], K[l], H, 2 if l == 1 else 1)
    return out


def claim_holds(want, got):
    if isinstance(want, tuple):
        lo, hi = want
        return (lo is None or got >= lo) and (hi is None or got <= hi)
    return type(want) is type(got) and want == got
