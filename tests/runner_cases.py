"""The shape tables of the forward-only runner (train.Embedder) and of the
whole-neighbourhood hops (a `None` fanout, the reference's num_sample=None),
with their float64 yardstick (no tests here).

WHOLE: five rows on the tiny R-MAT (436 nodes, maximum degree 236) in
step_cases' row format, each with a `None` hop.  A `None` last hop makes
gs_trainer_gather's k_ids 0, the only way into its second and third branch;
a `None` first hop gives the top launch hop-1 lists longer than its 31 padded
slots, so it walks the lists.  test_runner_cases_host.py checks every claim
under `predicates` below; test_gpu_whole_hop.py runs the rows on the device.

EMBED: the rows of test_gpu_embedder_matrix.py.  A row names a shape (a
step_cases id or a WHOLE id), the batch size, the number of ids, `merge`, the
stream count S, `helpers` and `depth`.  Ids are the first n of
np.random.RandomState(SEED).permutation(nodes with degree > 0), except the
`repeat` row: pool[np.arange(n) * 7 % 40] over a pool of the first 40 of that
permutation, with n = 203 > 40 and batch 48, so every batch holds 8 nodes
twice and every node sits in both batches of a merged pack.

embed_reference restates the stream order train.Embedder documents: batch i
(the trailing partial one as i = n_full) is sampled by stream
(i // merge) % S with the row's own, unclamped merge, every stream takes its
batches in ascending order, and the streams are train.make_rng(SEED, 0, w).
Each batch is sampled with gs.sample and evaluated by
step_ref.step_reference (dummy labels; only the embeddings are taken).

FACTOR: check_rule's factor is 4 unless step_cases.FACTOR (rows taken from
there) or FACTOR below says otherwise, with the reason next to it, by
step_cases.FACTOR's convention.
"""
import importlib

import numpy as np
import torch

from tests import step_cases as sc
from tests import step_ref
from tests.step_cases import SEED, _row, batches_of, claim_holds, features_of, graph_of, labels_of  # noqa: F401

INIT_SEED = 824   # train.reference_init's seed for every row's weights
POOL = 40         # the `repeat` row's id pool

WHOLE = [
    # last hop whole: the gather writes the aggregate half of a [self | agg] slot only; rows of 65+ entries
    _row("fl2", 2, (10, None), 36, 48, 5, "MEAN", False, "f32", 40,
         {"gather": "self_half", "layer1_list_max": (65, None), "top": False, "defer": False}),
    # the same under gcn: a plain gather into the slot; rows not 16-byte aligned
    _row("fl2g", 2, (5, None), 50, 80, 5, "MAX", True, "f32", 33,
         {"gather": "plain", "vload": False, "top": False, "defer": False}),
    # first hop whole: the id gather, and the top launch walking hop-1 lists past its 31 slots
    _row("fh1", 2, (None, 5), 256, 128, 16, "MEAN", False, "f32", 24,
         {"gather": "ids", "top": True, "top_list_max": (32, None), "defer": True}),
    # one whole hop: unfused backward over a [self | agg] slot without its self half; scalar bf16 loads
    _row("fl1", 1, (None,), 100, 64, 7, "MAX", False, "bf16", 37,
         {"gather": "self_half", "fused": False, "vload": False, "defer": False}),
    # three hops, the last whole: two fused upper layers
    _row("fl3", 3, (5, 3, None), 64, 64, 5, "MEAN", False, "f32", 16,
         {"gather": "self_half", "fused": True, "fused_layers": 2, "defer": False}),
]
WHOLE_BY_ID = {c["id"]: c for c in WHOLE}
WHOLE_IDS = [c["id"] for c in WHOLE]
WHOLE_DEFERS = ("fh1",)

# {row id: {tensor name: (factor, reason)}}; empty: every WHOLE row stays within 4 (DESIGN §4 holds the ratios)
FACTOR = {}


def shape_of(shape_id):
    """The step_cases or WHOLE row of that id."""
    return WHOLE_BY_ID[shape_id] if shape_id in WHOLE_BY_ID else sc.BY_ID[shape_id]


def factor(shape_id, tensor):
    if shape_id in FACTOR:
        return FACTOR[shape_id].get(tensor, (4.0, ""))[0]
    return sc.factor(shape_id, tensor)


def predicates(case, sample, roots):
    """step_cases.predicates, plus what gs_trainer_gather takes for the
    sample when a runner gathers it and how long the top launch's lists get."""
    out = sc.predicates(case, sample, roots)
    L, k = case["L"], case["fanouts"][-1]
    n_dst, n_pos = sample.sizes(L)[:2]
    # gs_trainer_gather: k_ids is the last fanout (0 when it is None); then self_rows (never under gcn)
    if k is not None and k > 0 and n_pos <= n_dst * k:
        out["gather"] = "ids"
    else:
        out["gather"] = "plain" if case["gcn"] else "self_half"
    last = sample.hop(L)
    out["layer1_list_max"] = int(np.diff(last.pos_ptr).max())
    # the top launch's hop-1 lists (run_step: two layers only; trainer_reserve_top pads to at most 31)
    first = sample.hop(1)
    out["top_list_max"] = int(np.diff(first.nbr_ptr if first.materialised else first.pos_ptr).max())
    return out


# ------------------------------------------------------------ the embedder table
def _emb(id, shape, batch, n_ids, merge, S=1, helpers=0, depth=4, ids="perm"):
    return {"id": id, "shape": shape, "batch": batch, "n_ids": n_ids, "merge": merge, "S": S, "helpers": helpers,
            "depth": depth, "ids": ids}


EMBED = [
    _emb("bench", "bench", 16, 5 * 16 + 9, 2),              # the control; its last unit holds one batch
    _emb("h64", "h64", 24, 3 * 24 + 7, 4, S=2),             # merge clamped to 3; the partial batch's stream is not
    _emb("tiny", "tiny", 33, 4 * 33 + 5, 2, S=2),
    _emb("unal", "unal", 32, 7 * 32 + 3, 3, S=2),           # units of 3, 3 and 1 batches
    _emb("h80", "h80", 48, 4 * 48 + 10, 1, S=3, helpers=2),
    _emb("h256", "h256", 40, 3 * 40 + 6, 2, depth=1),
    _emb("l1g", "l1g", 37, 3 * 37 + 5, 2),                  # a merged pack of one hop
    _emb("l3", "l3", 16, 4 * 16 + 3, 3),                    # a merged pack of three hops
    _emb("l3m", "l3m", 32, 3 * 32 + 4, 2),
    _emb("bfm", "bfm", 48, 2 * 48 + 5, 2),
    _emb("bfu", "bfu", 32, 3 * 32 + 9, 2, S=2),
    _emb("fl2", "fl2", 40, 3 * 40 + 7, 2),
    _emb("fl2g", "fl2g", 33, 3 * 33 + 6, 2),
    _emb("fh1", "fh1", 24, 3 * 24 + 5, 2),
    _emb("fl1", "fl1", 37, 3 * 37 + 4, 2),
    _emb("fl3", "fl3", 16, 3 * 16 + 3, 2),
    # edges, all on `tiny`
    _emb("exact", "tiny", 16, 4 * 16, 2),                   # no partial batch
    _emb("short", "tiny", 16, 11, 2),                       # no full batch: no runner at all
    _emb("repeat", "tiny", 48, 203, 2, ids="repeat"),       # a node twice in a batch and in both batches of a pack
]
EMBED_BY_ID = {r["id"]: r for r in EMBED}
EMBED_IDS = [r["id"] for r in EMBED]


def ids_of(row):
    """The row's id list (int64)."""
    case = shape_of(row["shape"])
    graph = graph_of(case["graph"])[0]
    cands = np.nonzero(graph.degrees())[0].astype(np.int64)
    perm = np.random.RandomState(SEED).permutation(cands)
    if row["ids"] == "repeat":
        assert row["n_ids"] > POOL
        return perm[:POOL][np.arange(row["n_ids"]) * 7 % POOL]
    assert row["ids"] == "perm" and row["n_ids"] <= len(perm)
    return perm[:row["n_ids"]]


def batch_slices(row):
    """[(i, lo, hi)] of the row's batches, the trailing partial one included."""
    n, b = row["n_ids"], row["batch"]
    return [(i, lo, min(lo + b, n)) for i, lo in enumerate(range(0, n, b))]


def stream_of(row, i):
    """The stream that samples batch i."""
    return (i // row["merge"]) % row["S"]


def make_rngs(row):
    train = importlib.import_module("graphsage-pytorch_amd.train")
    return [train.make_rng(SEED, 0, w) for w in range(row["S"])]


def rng_state(rng):
    mt, pos = rng.getstate()
    return np.asarray(mt).tolist(), int(pos)


def weights_of(case):
    """(sage weights, Wc, bc) of the shape from train.reference_init (CPU tensors)."""
    train = importlib.import_module("graphsage-pytorch_amd.train")
    return train.reference_init(case["L"], case["F"], case["H"], case["C"], case["gcn"], INIT_SEED)


def trajectory_reference(case, n_steps, dtype=torch.float64, max_norm=5.0):
    """(parameters, last loss) after n_steps steps of clip + SGD on the row's
    batches (step_cases.samples_of: one stream RNG(SEED)) from
    train.reference_init's weights, as float64 numpy: step_ref's step and
    clip_sgd in float64, or the step in fp32 with torch's fp32 clip + SGD
    (check_rule's yardstick for a whole trajectory)."""
    from tests.adam_cases import f32
    _graph, _n, row_ptr, col = graph_of(case["graph"])
    X, labels = features_of(case), labels_of(case)
    L, F, H, C = case["L"], case["F"], case["H"], case["C"]
    offs = step_ref.param_offsets(L, F, H, C, case["gcn"])
    goff = [0, int(offs[L]), int(offs[-1])]
    sage_w, cw, cb = weights_of(case)
    p = np.concatenate([t.detach().numpy().reshape(-1) for t in list(sage_w) + [cw, cb]]).astype(np.float64)
    loss = None
    for roots, s in sc.samples_of(case, n_steps):
        _e, loss, g = step_ref.step_reference(s, row_ptr, col, X, labels, roots, p, L, H, C, case["agg"], case["gcn"],
                                              bf16=case["bf16"], dtype=dtype)
        if dtype == torch.float64:
            p = step_ref.clip_sgd(p, g, goff, f32(sc.LR), f32(max_norm))[0]
        else:
            p = step_ref.clip_sgd_torch_fp32(p, g, goff, f32(sc.LR), f32(max_norm))[0]
    return p, loss


_SAMPLES = {}


def embed_samples(row):
    """([(i, lo, hi, Sample)] in batch order, [final state of every stream])
    under the stream order of the module docstring; sampled once."""
    if row["id"] not in _SAMPLES:
        gs = importlib.import_module("graphsage-pytorch_amd")
        case = shape_of(row["shape"])
        graph = graph_of(case["graph"])[0]
        ids, rngs = ids_of(row), make_rngs(row)
        out = [(i, lo, hi, gs.sample(graph, rngs[stream_of(row, i)], ids[lo:hi], case["fanouts"], gcn=case["gcn"]))
               for i, lo, hi in batch_slices(row)]
        _SAMPLES[row["id"]] = (out, [rng_state(r) for r in rngs])
    return _SAMPLES[row["id"]]


_REFERENCE = {}


def embed_reference(row, dtype=torch.float64):
    """(embeddings of the row's ids [len(ids), H] as float64 numpy, computed
    at `dtype`; the final state of every stream).  Computed once per dtype."""
    key = (row["id"], dtype)
    if key not in _REFERENCE:
        case = shape_of(row["shape"])
        _graph, _n, row_ptr, col = graph_of(case["graph"])
        X, ids = features_of(case), ids_of(row)
        sage_w, cw, cb = weights_of(case)
        params = np.concatenate([t.detach().numpy().reshape(-1) for t in list(sage_w) + [cw, cb]])
        labels = np.zeros(X.shape[0], np.int32)  # dummy: only the embeddings are taken
        samples, states = embed_samples(row)
        out = np.full((len(ids), case["H"]), np.nan)
        for _i, lo, hi, s in samples:
            out[lo:hi] = step_ref.step_reference(s, row_ptr, col, X, labels, ids[lo:hi], params, case["L"], case["H"],
                                                 case["C"], case["agg"], case["gcn"], bf16=case["bf16"],
                                                 dtype=dtype)[0]
        _REFERENCE[key] = (out, states)
    return _REFERENCE[key]
