"""The forward-only runner (train.Embedder) off the benchmark's shape:
tests/runner_cases.EMBED (hidden 16 .. 256, 1 to 3 layers, gcn, MAX over
bf16, feature widths that fail the 16-byte rule, whole-neighbourhood hops,
units shorter than `merge`, `merge` above the number of full batches, no
partial batch, no full batch, repeated ids).

Per row, from one set of weights (train.reference_init):
1. Embedder.embed against runner_cases.embed_reference in float64, under
   adam_cases.check_rule: err <= factor * e_torch + 2^-23 * max|ref| with
   e_torch the error of the reference's own fp32 run on the CPU; the factor
   is 4 (`l1g`: step_cases.FACTOR's 16, the same kernel and reason);
2. bitwise against NativeTrainer.forward(DeviceSample(s)) batch by batch on
   the same samples ("each row equals its own batch's forward");
3. bitwise across the pipeline's knobs the row sets: merge m against 1 (rows
   with one stream: with more, merge decides which stream samples a batch),
   helpers against 0, depth against 4, and self_rows off against the default;
4. every sampler stream ends in the state the reference's streams end in;
5. Runner(embed_out=buf, merge=m) on a buffer two rows longer than the full
   batches: the extra rows stay NaN, the rows inside equal the Embedder's,
   the feature table is unchanged.

GS_RUNNER_MATRIX_FIGURES=<path> writes every observed err / e_torch of this
file and of test_gpu_whole_hop.py as JSON (DESIGN §4 quotes them).
"""
import importlib
import json
import os

import pytest
import torch

from tests import runner_cases as rc
from tests import step_cases as sc
from tests.adam_cases import check_rule

pytestmark = pytest.mark.gpu

models = importlib.import_module("graphsage-pytorch_amd.models")
train = importlib.import_module("graphsage-pytorch_amd.train")
DEV = torch.device("cuda", 0)
FIGURES = {}   # {group: {tag: {"err", "e_torch", "ratio", "bound"}}}; test_gpu_whole_hop.py adds its own
_STATE = {}


def record(group, figures):
    """check_rule's figure tuples into FIGURES[group]."""
    for what, err, e_torch, ratio, bound in figures:
        FIGURES.setdefault(group, {})[what] = {"err": err, "e_torch": e_torch, "ratio": ratio, "bound": bound}


def write_figures():
    path = os.environ.get("GS_RUNNER_MATRIX_FIGURES")
    if not (path and FIGURES):
        return
    with open(path, "w") as f:  # each file of the pair rewrites it with everything gathered so far
        json.dump({"rule": "err <= factor * e_torch + 2^-23 * max|ref|; ratio = err / e_torch", "groups": FIGURES,
                   "largest_ratio": {g: max(v["ratio"] for v in t.values()) for g, t in FIGURES.items()}}, f,
                  indent=1, sort_keys=True)


@pytest.fixture(scope="module", autouse=True)
def _write_figures():
    yield
    write_figures()


def _world(row):
    """The row's graph, feature table and weights on the device; built once per shape."""
    case = rc.shape_of(row["shape"])
    key = ("world", case["id"])
    if key not in _STATE:
        graph = sc.graph_of(case["graph"])[0]
        X = sc.features_of(case)
        Xd = torch.from_numpy(X).to(DEV)
        if case["bf16"]:
            Xd = Xd.to(torch.bfloat16)
            assert torch.equal(Xd.float().cpu(), torch.from_numpy(X))
        W = [w.to(DEV) for w in rc.weights_of(case)[0]]
        _STATE[key] = (graph, Xd, Xd.clone(), W)
    return _STATE[key]


def _embedder(row, **over):
    case = rc.shape_of(row["shape"])
    graph, Xd, _keep, W = _world(row)
    knobs = {"depth": row["depth"], "merge": row["merge"], "helpers": row["helpers"], **over}
    return train.Embedder(graph, Xd, W, case["fanouts"], agg_func=case["agg"], gcn=case["gcn"], **knobs)


def _embed(row, self_rows=True, **over):
    """(embeddings, the streams' final states) of one Embedder run on fresh streams."""
    e = _embedder(row, **over)
    if not self_rows:
        e.trainer.set_option("self_rows", False)
    rngs = rc.make_rngs(row)
    out = e.embed(rc.ids_of(row), row["batch"], rngs)
    torch.cuda.synchronize()
    assert out.shape == (row["n_ids"], rc.shape_of(row["shape"])["H"])
    return out.clone(), [rc.rng_state(r) for r in rngs]


def _default(row):
    key = ("default", row["id"])
    if key not in _STATE:
        _STATE[key] = _embed(row)
    return _STATE[key]


@pytest.mark.parametrize("row_id", rc.EMBED_IDS)
def test_embedder_matches_float64_reference(gs, row_id):
    """1 and 4: the embeddings under check_rule, and the streams' final states."""
    row = rc.EMBED_BY_ID[row_id]
    got, states = _default(row)
    e64, want_states = rc.embed_reference(row)
    e32, _ = rc.embed_reference(row, torch.float32)
    figures = []
    try:
        check_rule(f"{row_id} emb", got.cpu().numpy(), e64.reshape(-1), e32.reshape(-1), figures=figures,
                   factor=rc.factor(row["shape"], "emb"))
    finally:
        record("embedder", figures)
    assert states == want_states


@pytest.mark.parametrize("row_id", rc.EMBED_IDS)
def test_embedder_rows_equal_their_own_batch_forward(gs, row_id):
    """2: the same samples through the Python path, one batch per forward."""
    row = rc.EMBED_BY_ID[row_id]
    case = rc.shape_of(row["shape"])
    graph, Xd, _keep, W = _world(row)
    got, _states = _default(row)
    H = case["H"]
    tr = train.NativeTrainer(graph, Xd, torch.zeros(1, dtype=torch.int32), 1, num_layers=case["L"], hidden=H,
                             fanouts=case["fanouts"], agg_func=case["agg"], gcn=case["gcn"],
                             weights=(W, torch.zeros(1, H, device=DEV), torch.zeros(1, device=DEV)))
    samples, _ = rc.embed_samples(row)
    for i, lo, hi, s in samples:
        ref = torch.full((hi - lo, H), float("nan"), device=DEV)
        tr.forward(models.DeviceSample(s, DEV), ref)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(ref).all())
        assert torch.equal(got[lo:hi], ref), (row_id, i)


def _knobs(row):
    out = []
    # merge decides which stream samples which batch, so only one stream gives merge 1 the same samples
    if row["merge"] > 1 and row["S"] == 1:
        out.append(("merge", {"merge": 1}))
    if row["helpers"]:
        out.append(("helpers", {"helpers": 0}))
    if row["depth"] != 4:
        out.append(("depth", {"depth": 4}))
    if not rc.shape_of(row["shape"])["gcn"]:  # under gcn there is no self half to leave out
        out.append(("self_rows", {"self_rows": False}))
    return out


@pytest.mark.parametrize("row_id,knob", [(r["id"], k[0]) for r in rc.EMBED for k in _knobs(r)])
def test_embedder_is_bitwise_across_the_pipelines_knobs(gs, row_id, knob):
    """3: the knob at its other value leaves the same bits and the same streams."""
    row = rc.EMBED_BY_ID[row_id]
    got, states = _default(row)
    other, other_states = _embed(row, **dict(_knobs(row))[knob])
    assert bool(torch.isfinite(other).all())
    assert torch.equal(got, other)
    assert states == other_states


@pytest.mark.parametrize("row_id", [r["id"] for r in rc.EMBED if r["n_ids"] >= r["batch"]])
def test_runner_writes_its_own_rows_only(gs, row_id):
    """5: the runner itself on a NaN-filled buffer two rows too long."""
    row = rc.EMBED_BY_ID[row_id]
    case = rc.shape_of(row["shape"])
    graph, Xd, keep, _W = _world(row)
    got, _states = _default(row)
    ids, batch, m = rc.ids_of(row), row["batch"], row["merge"]
    n_full = row["n_ids"] // batch
    rows = n_full * batch
    tr = _embedder(row).trainer
    buf = torch.full((rows + 2, case["H"]), float("nan"), device=DEV)
    r = train.Runner(tr, graph, ids[:rows].reshape(n_full, batch), rc.make_rngs(row), case["fanouts"],
                     gcn=case["gcn"], fail_empty=case["agg"] == "MAX", depth=row["depth"], embed_out=buf, merge=m,
                     helpers=row["helpers"])
    try:
        r.run(-(-n_full // min(m, n_full)))
        torch.cuda.synchronize()
        assert r.stats()["steps"] == -(-n_full // min(m, n_full))
    finally:
        r.close()
    assert bool(torch.isnan(buf[rows:]).all())
    assert bool(torch.isfinite(buf[:rows]).all())
    assert torch.equal(buf[:rows], got[:rows])
    assert torch.equal(Xd, keep)
