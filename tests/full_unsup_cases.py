"""Case table of the exact step under the unsupervised losses (no tests here;
numpy and CPU torch only).

Graphs: full_cases' "hub" without its rows of no neighbour ("hub_max", 297
nodes: FullTrainer refuses an empty neighbourhood) and "bounded" (300 nodes),
and full_train_cases' "directed" (48 nodes).  The extended batch `nodes` is a
strict subset of the ids, unsorted: U = 96 rows on the large graphs, 40 on the
directed one.

Shapes (SHAPES): the smallest that reach each branch of the step -- L = 1, 2,
3; MEAN and MAX; gcn; bf16 features (with MAX, for full_cases' reason); hidden
16, 80, 128 and 256, the only hidden width that reaches the loss kernels'
NC = 4 instance (the others run NC = 2).  CASES pairs every shape with one
graph in turn and adds two more pairs so that each graph sees MEAN and MAX.

Pair lists are synthetic, laid out by unsup_loss_cases.build_plan: M scored
nodes (node m sits in row 1 + m), positive counts cycling through POS_COUNTS
(1, 2, 15, 16, 17, 40) and negative counts through NEG_COUNTS (1, 6, 16, 33,
70), partners drawn from the rows 1 .. U - 4 without replacement where the
list is shorter than the candidates and with replacement where it is not (the
directed case; extend_nodes' walks repeat pairs too).  Row 0 owns nothing and
is a partner in every list; the last FREE_ROWS rows are in no pair.

KINDS: sage (q = 10), margin (3.0) and split: the margin at the fp32-rounded
negative median of max log s(cos-) - min log s(cos+) over the nodes on the
float64 embeddings, so about half the hinges are off.

The margin loss selects, and fp32 cannot tell candidates apart that float64
can; SEED pins, per case, the first seed of the lists' generator at which
margin and split have clear winners (test_full_unsup_host.py measures the
fp32 reference's own error per case and asserts the conditions).

FACTOR: check_rule's factor is 4 unless a row says otherwise here, with its
reason (twice the ratio observed on the MI355X, rounded up to a power of two).
"""
import functools

import numpy as np
import torch

from tests import full_cases as fc
from tests import full_field_cases as ffc
from tests import full_train_cases as tc
from tests import full_unsup_ref as uref
from tests import unsup_loss_cases as ulc

POS_COUNTS, NEG_COUNTS = ulc.POS_COUNTS, ulc.NEG_COUNTS
FREE_ROWS = 3
KINDS = ("sage", "margin", "split")
METHODS = ("unsup", "plus_unsup")
Q, MARGIN = ulc.Q, ulc.MARGIN
GRAPH_U_M = {"hub_max": (96, 40), "bounded": (96, 40), "directed": (40, 30)}   # graph -> (U, M)

# {(case id, method, kind, path, tensor): (factor, reason)}
FACTOR = {}


def factor(case_id, method, kind, path, tensor):
    return FACTOR.get((case_id, method, kind, path, tensor), (4.0, ""))[0]


def _shape(id, L, F, H, agg, gcn=False, bf16=False, C=3):
    return {"id": id, "L": L, "F": F, "H": H, "C": C, "agg": agg, "gcn": gcn, "bf16": bf16, "seg_len": tc.SEG_LEN}


SHAPES = [
    _shape("l2_h16", 2, 64, 16, "MEAN"),
    _shape("max_h80", 2, 128, 80, "MAX", C=7),
    _shape("l1_f50", 1, 50, 16, "MEAN"),
    _shape("l3_h80", 3, 64, 80, "MEAN", C=7),
    _shape("gcn_h128", 2, 128, 128, "MEAN", gcn=True),
    _shape("bf16_max", 2, 100, 16, "MAX", bf16=True, C=7),
    _shape("h256", 2, 64, 256, "MEAN"),
]
_GRAPHS = ("hub_max", "bounded", "directed")
CASES = [dict(s, graph=_GRAPHS[i % 3], id=f"{s['id']}-{_GRAPHS[i % 3]}") for i, s in enumerate(SHAPES)]
CASES += [dict(SHAPES[1], graph="directed", id="max_h80-directed"),
          dict(SHAPES[0], graph="bounded", id="l2_h16-bounded")]
BY_ID = {c["id"]: c for c in CASES}
IDS = [c["id"] for c in CASES]
FD_CASE = "l1_f50-directed"     # the 48-node case of the finite-difference check

# case id -> seed of the pair lists: the first of 0, 1, 2, .. at which `margin` and `split` meet the conditions
SEED = {c["id"]: 0 for c in CASES}
SEED["max_h80-bounded"] = 1     # seed 0: a positive gap of 5.2e-6 under the case's 1.1e-5


def make_lists(rs, U, M):
    pos_lists, neg_lists = [], []
    for m in range(M):
        c = 1 + m
        cand = np.array([r for r in range(1, U - FREE_ROWS) if r != c])
        for counts, lists in ((POS_COUNTS, pos_lists), (NEG_COUNTS, neg_lists)):
            k = counts[m % len(counts)]
            partners = np.concatenate([[0], rs.choice(cand, k - 1, replace=k - 1 > len(cand))])
            rs.shuffle(partners)
            lists.append([(c, int(p)) for p in partners])
    return pos_lists, neg_lists


@functools.lru_cache(maxsize=None)
def setup(case_id, seed=None):
    """Everything a step of the case reads, built once and read-only: a dict of the case's fields plus
    n, rp, col, X (fp32 numpy, bf16 values when bf16), labels, params, nodes (int64 [U]), lists, plan, dims."""
    case = BY_ID[case_id]
    graph, n, rp, col = ffc.graph_of(case["graph"])
    U, M = GRAPH_U_M[case["graph"]]
    rs = np.random.RandomState(1000 * IDS.index(case_id) + (SEED[case_id] if seed is None else seed))
    lists = make_lists(rs, U, M)
    plan, dims = ulc.build_plan(lists[0], lists[1], U)
    plan.flags.writeable = False
    nodes = tc.nodes_of(n, k=U, seed=17)
    out = dict(case, graph_obj=graph, n=n, rp=rp, col=col, X=fc.features(n, case["F"], case["bf16"]),
               labels=tc.labels_of(n, case["C"]), params=tc.params_of(case), nodes=nodes, lists=lists, plan=plan,
               dims=dims, U=U, M=M)
    assert U < n and len(np.unique(nodes)) == U
    return out


def _run(s, kind, margin, with_sup, dtype):
    return uref.step_reference(s["rp"], s["col"], s["X"], s["labels"], s["nodes"], s["params"], s["agg"], s["gcn"],
                               lists=s["lists"], kind=kind, q=Q, margin=margin, with_sup=with_sup, bf16=s["bf16"],
                               dtype=dtype)


@functools.lru_cache(maxsize=None)
def margin_of(case_id, kind, seed=None):
    """The margin of (case, kind) as an fp32 value: the C ABI carries it in fp32."""
    if kind != "split":
        return MARGIN
    r = _run(setup(case_id, seed), "margin", MARGIN, False, torch.float64)
    return float(np.float32(-np.median(r["ext_neg"] - r["ext_pos"])))


@functools.lru_cache(maxsize=None)
def ref(case_id, method, kind, dtype=torch.float64, seed=None):
    """step_reference of (case, method, kind), computed once and read-only."""
    return _run(setup(case_id, seed), kind, margin_of(case_id, kind, seed), method == "plus_unsup", dtype)


def conditions(r, lists, gap_min, h_min):
    """unsup_loss_cases.conditions with the case's own thresholds: the list of conditions the float64
    reference `r` of a margin kind fails.  Copies of the winning pair in one list are one candidate
    (whichever is selected, loss and dE are the same; the kernels and torch both take the first)."""
    bad = []
    for k, side in enumerate(("pos", "neg")):
        gap = r[f"gap_{side}"].copy()
        for m, tied in enumerate(r[f"ties_{side}"]):
            if len({lists[k][m][j] for j in tied}) == 1:
                gap[m] = r[f"gap2_{side}"][m]
        if gap.min() < gap_min:
            bad.append(f"{side} gap {gap.min():.3e} at node {int(gap.argmin())} < {gap_min:.3e}")
    if np.abs(r["h"]).min() < h_min:
        bad.append(f"|h| {np.abs(r['h']).min():.3e} at node {int(np.abs(r['h']).argmin())} < {h_min:.3e}")
    return bad


def thresholds(case_id, kind, seed=None):
    """(gap_min, h_min): 100 times the fp32 reference's own error in the selected extremes and in h."""
    r64, r32 = ref(case_id, "unsup", kind, torch.float64, seed), ref(case_id, "unsup", kind, torch.float32, seed)
    e_ext = max(np.abs(r32["ext_pos"] - r64["ext_pos"]).max(), np.abs(r32["ext_neg"] - r64["ext_neg"]).max())
    e_h = np.abs(r32["h"] - r64["h"]).max()
    return 100.0 * float(e_ext), 100.0 * float(e_h)


def failures(case_id, seed=None):
    """Every condition the case fails at `seed` (empty: the seed may be pinned)."""
    bad = []
    lists = setup(case_id, seed)["lists"]
    for kind in ("margin", "split"):
        r = ref(case_id, "unsup", kind, torch.float64, seed)
        bad += [f"{kind}: {b}" for b in conditions(r, lists, *thresholds(case_id, kind, seed))]
    on = float(np.mean(ref(case_id, "unsup", "split", torch.float64, seed)["h"] > 0))
    if not 0.25 <= on <= 0.75:
        bad.append(f"split: {on:.2f} of the hinges on")
    return bad
