"""Inputs of the receptive-field tests (no tests here).

The graphs, features, parameters and labels are those of tests/full_cases.py
and tests/full_train_cases.py; what this module adds is the mini-batches
(FIELD_CASES), a brute-force statement of the field with Python sets, a numpy
filter of a plan's host arrays, and a graph object for the directed CSR that
train.FullTrainer accepts (it only asks a graph for n_nodes, row_ptr(), col()
and device_csr()).

FIELD_CASES, with the sizes n_L .. n_0 that test_full_field_host.py recounts:

* hub_four   hub_max [2, 4, 125, 7], L = 2: 4, 90, 213.  A four-segment row and
  the rows whose self loop sits in the first and the last segment; split rows
  at both layers.
* hub_one    hub_max [3], L = 2: 1, 2, 5.  One root of degree 1: fewer rows
  than one GEMM tile, a grid of one, no split row.
* hub_seg    hub_max [0], L = 3: 1, 9, 34, 126.  One full segment at the root.
* rmat5      rmat RandomState(13).permutation(436)[:5], L = 2: 5, 73, 402
  (three layers reach 435 of the 436 rows).
* directed   nodes_of(48, 3) + DIRECTED_NO_READER, L = 2: 4, 14, 33.  A root
  whose transposed row is empty; hubs 0 .. 3 whose transposed rows split.

FACTOR: check_rule's factor is the project's 4 unless a row says otherwise
here, with its reason.  Three rows do, all for outputs of the loss head on a
batch of one or five roots (see _ONE_DRAW); DESIGN §4 has the observed ratios.
"""
import numpy as np

from tests import full_cases as fc
from tests import full_train_cases as tc

SEG_LEN = fc.SEG_LEN
# A factor of PROPAGATED is computed by propagated_head_factor from the two reference runs alone.
PROPAGATED = "propagated"
_ONE_DRAW = ("the loss of a batch of %d is one fp32 scalar, so its e_torch is one draw of the reference's rounding "
             "error, not a maximum over many elements, and it depends on the CPU the reference runs on: for these "
             "inputs it was seen anywhere from 0.035 to 3 ulp of the loss, mostly below the half ulp no fp32 result "
             "is expected to beat.  The device loss is bitwise the full path's on these nodes (DESIGN §4), and H_L "
             "passes at factor 4; the loss may then differ by what the H_L error the rule admits propagates to: "
             "propagated_head_factor")
_HEAD = ("with one root the classifier's gradients are 7 and 7 x 80 numbers computed from one row of H_L, and their "
         "e_torch is as much a matter of a few draws as the loss's; the same propagation: propagated_head_factor")
FACTOR = {               # {(test, case id): (factor, reason)}
    ("step_loss", "hub_seg-max_l3"): (PROPAGATED, _ONE_DRAW % 1),
    ("step_loss", "rmat5-max"): (PROPAGATED, _ONE_DRAW % 5),
    ("step_head", "hub_seg-max_l3"): (PROPAGATED, _HEAD),
}


def factor(test, case_id):
    return FACTOR.get((test, case_id), (4.0, ""))[0]


def propagated_head_factor(what, h64, h32, nodes, labels, Wc, bc, ref, tor, base=4.0):
    """check_rule's factor for a quantity of the loss head where FACTOR says
    PROPAGATED, from the float64 and fp32 reference runs alone (ref, tor: the
    quantity in both).  The rule admits an error of
        b_H = base * e_torch(H_L) + 2^-23 * max|H_L|
    in every element of H_L, and a bound on a head quantity below what b_H
    propagates to (first order) would contradict the bound on H_L.  With E =
    H_L[nodes], p_i = softmax(Wc E_i + bc), y_i the one-hot label, W1 the
    largest 1-norm of a row of Wc:
      loss            moves by at most  sum_i |Wc^T (p_i - y_i)|_1 / B * b_H
      layer.0.bias    = mean_i (p_i - y_i): a logit moves by at most W1 b_H and
                      |dp_c| <= 2 p_c (1 - p_c) max|dz| <= W1 b_H / 2
      layer.0.weight  = mean_i (p_i - y_i) E_i^T: at most (W1 max|E| / 2 + 1) b_H
    Returned: base + that / e_torch(quantity)."""
    nodes = np.asarray(nodes, np.int64)
    Wc = np.asarray(Wc, np.float64)
    E = np.asarray(h64, np.float64)[nodes]
    b_H = base * float(np.abs(np.asarray(h32) - h64).max()) + 2.0 ** -23 * float(np.abs(h64).max())
    W1 = float(np.abs(Wc).sum(1).max())
    if what == "loss":
        z = E @ Wc.T + np.asarray(bc, np.float64)
        p = np.exp(z - z.max(1, keepdims=True))
        p /= p.sum(1, keepdims=True)
        p[np.arange(len(nodes)), np.asarray(labels, np.int64)[nodes]] -= 1.0
        add = float(np.abs(p @ Wc).sum() / len(nodes)) * b_H
    elif what == "layer.0.bias":
        add = 0.5 * W1 * b_H
    elif what == "layer.0.weight":
        add = (0.5 * W1 * float(np.abs(E).max()) + 1.0) * b_H
    else:
        raise KeyError(what)
    e_torch = float(np.abs(np.asarray(tor, np.float64) - np.asarray(ref, np.float64)).max())
    return base + add / e_torch


def _case(id, graph, nodes, L, sizes, split_at_r1=True):
    return {"id": id, "graph": graph, "nodes": np.asarray(nodes, np.int64), "L": L, "sizes": sizes,
            "split_at_r1": split_at_r1}


FIELD_CASES = [
    _case("hub_four", "hub_max", [2, 4, 125, 7], 2, (4, 90, 213)),
    _case("hub_one", "hub_max", [3], 2, (1, 2, 5), split_at_r1=False),
    _case("hub_seg", "hub_max", [0], 3, (1, 9, 34, 126)),
    _case("rmat5", "rmat", np.random.RandomState(13).permutation(436)[:5], 2, (5, 73, 402)),
    _case("directed", "directed", list(tc.nodes_of(tc.DIRECTED_N, 3)) + [tc.DIRECTED_NO_READER], 2, (4, 14, 33)),
]
FIELD_BY_ID = {c["id"]: c for c in FIELD_CASES}
FIELD_IDS = [c["id"] for c in FIELD_CASES]


class CsrOnlyGraph:
    """A graph given as a bare CSR, with the four things FullTrainer and
    FullPlan ask of a CSRGraph."""

    def __init__(self, row_ptr, col):
        self._rp = np.ascontiguousarray(row_ptr, np.int64)
        self._col = np.ascontiguousarray(col, np.int32)
        self.n_nodes = len(self._rp) - 1
        self._dev = {}

    def row_ptr(self):
        return self._rp.copy()

    def col(self):
        return self._col.copy()

    def device_csr(self, device):
        import torch
        key = str(torch.device(device))
        if key not in self._dev:
            self._dev[key] = (torch.from_numpy(self._rp).to(device), torch.from_numpy(self._col).to(device))
        return self._dev[key]


_GRAPHS = {}


def graph_of(name):
    """(graph for FullTrainer / agg_full_plan, n, row_ptr, col); "directed" as a CsrOnlyGraph."""
    if name == "directed":
        if name not in _GRAPHS:
            rp, col, n = tc.directed_csr()
            _GRAPHS[name] = (CsrOnlyGraph(rp, col), n, rp, col)
        return _GRAPHS[name]
    return fc.graph_of(name)


def brute_field(row_ptr, col, nodes, L):
    """[R_0, .., R_L] as Python sets: the fixed point of the definition, level by level."""
    adj = [set(int(u) for u in col[row_ptr[v]:row_ptr[v + 1]]) - {v} for v in range(len(row_ptr) - 1)]
    levels = [None] * (L + 1)
    levels[L] = set(int(v) for v in nodes)
    for l in range(L, 0, -1):
        levels[l - 1] = set(levels[l])
        for v in levels[l]:
            levels[l - 1] |= adj[v]
    return levels


def filter_plan(plan, pos):
    """(items, split rows) of a FullPlan's host arrays whose row has pos >= 0, in plan order."""
    _lib = __import__("importlib").import_module("graphsage-pytorch_amd._lib")
    items = plan.array(_lib.GS_FP_ITEMS).reshape(-1, 2)
    split = plan.array(_lib.GS_FP_SPLIT_ROWS)
    return items[pos[items[:, 0]] >= 0], split[pos[split] >= 0]
