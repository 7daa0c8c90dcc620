"""Graphs and case tables of the full-batch training tests (no tests here).

The graphs are those of tests/full_cases.py plus "directed": a small CSR
given as (row_ptr, col), not symmetric -- most edges have no reverse, node 5
holds a self loop beside other entries, node 11 a self loop beside one
neighbour, nodes 0 .. 3 are hubs that about 40 nodes read (so their transposed
rows are split at SEG_LEN) and node DIRECTED_NO_READER is nobody's source: no row names it,
so its transposed row is empty.  Every row has at least one entry that is not
its own id, so MEAN and MAX both run without gcn.

STEP_CASES mirrors full_cases.PIPE_CASES without its chunking: L = 1, 2, 3,
(F, H) in {(256, 128), (64, 80), (50, 16)}, gcn, MAX, MAX + gcn, and bf16
features with MAX (the reason full_cases.py gives).  `nodes` is a strict
subset of the ids of a size off every block multiple (37), labels are random
in C = 3 or 7 classes.

FACTOR: check_rule's factor is the project's 4 unless a row says otherwise
here, with its reason (none does: DESIGN §4 has the observed ratios).
"""
import numpy as np

from tests import full_cases as fc

SEG_LEN = fc.SEG_LEN
DIRECTED_N = 48
DIRECTED_NO_READER = 47
FACTOR = {}              # {(test, case id): (factor, reason)}
N_NODES_SUBSET = 37


def factor(test, case_id):
    return FACTOR.get((test, case_id), (4.0, ""))[0]


def directed_csr():
    """(row_ptr int64, col int32, n) of the directed graph above."""
    n = DIRECTED_N
    rs = np.random.RandomState(23)
    rows = []
    for v in range(n):
        if v == DIRECTED_NO_READER:
            row = [0, 3]
        elif v == 0:
            row = [1, 2]
        else:
            k = 1 + int(rs.randint(0, 5))
            cand = np.setdiff1d(np.arange(4, n - 1), [v])
            row = sorted(rs.choice(cand, k, replace=False).tolist())
            if v <= 40:                  # ~40 readers of each of the nodes 0 .. 3: their transposed rows split
                row = [u for u in range(4) if u != v] + row
        if v == 5:
            row = sorted(row + [5])      # a self loop among other entries
        if v == 11:
            row = [11, 12]               # a self loop first, one neighbour
        rows.append(row)
    row_ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    col = np.concatenate(rows).astype(np.int32)
    return row_ptr, col, n


_CSR = {}


def csr_of(name):
    """(graph for FullPlan / agg_full_plan, n, row_ptr, col): a CSRGraph for
    the symmetric graphs, the (row_ptr, col) tuple for "directed"."""
    if name == "directed":
        if name not in _CSR:
            rp, col, n = directed_csr()
            _CSR[name] = ((rp, col), n, rp, col)
        return _CSR[name]
    return fc.graph_of(name)


def _case(id, L, F, H, C, agg, gcn, bf16=False, seg_len=SEG_LEN):
    return {"id": id, "L": L, "F": F, "H": H, "C": C, "agg": agg, "gcn": gcn, "bf16": bf16, "seg_len": seg_len}


STEP_CASES = [
    _case("l1", 1, 256, 128, 3, "MEAN", False),
    _case("l2", 2, 256, 128, 7, "MEAN", False),
    _case("l2_default", 2, 256, 128, 3, "MEAN", False, seg_len=None),
    _case("l3_h80", 3, 64, 80, 7, "MEAN", False),
    _case("h16_f50", 2, 50, 16, 3, "MEAN", False),
    _case("gcn", 2, 128, 128, 7, "MEAN", True),
    _case("max", 2, 128, 80, 3, "MAX", False),
    _case("max_l3", 3, 64, 80, 7, "MAX", False),
    _case("max_gcn", 2, 50, 16, 7, "MAX", True),
    _case("bf16_max", 2, 256, 128, 3, "MAX", False, bf16=True),
    _case("bf16_f100", 2, 100, 16, 7, "MAX", True, bf16=True),
]
STEP_BY_ID = {c["id"]: c for c in STEP_CASES}
STEP_IDS = [c["id"] for c in STEP_CASES]


def labels_of(n, C, seed=7):
    return np.random.RandomState(seed + C).randint(0, C, n).astype(np.int64)


def nodes_of(n, k=N_NODES_SUBSET, seed=13):
    """k unique ids, unsorted, a strict subset of range(n)."""
    assert k < n
    return np.random.RandomState(seed).permutation(n)[:k].astype(np.int64)


def params_of(case, seed=824):
    """[W_1 .. W_L, Wc, bc] as fp32 numpy: full_cases.weights and a xavier classifier."""
    import torch
    W = fc.weights(case["L"], case["F"], case["H"], case["gcn"], seed)
    g = torch.Generator().manual_seed(seed + 1)
    C, H = case["C"], case["H"]
    bound = float(np.sqrt(6.0 / (C + H)))
    Wc = ((torch.rand(C, H, generator=g) * 2 - 1) * bound).numpy()
    bc = ((torch.rand(C, generator=g) * 2 - 1) * 0.1).numpy()
    return W + [Wc, bc]


def names_of(L):
    return [f"sage_layer{i}.weight" for i in range(1, L + 1)] + ["layer.0.weight", "layer.0.bias"]
