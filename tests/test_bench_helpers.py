"""bench.py's lookups of the committed profiles (CPU): the rocprofv3 summary,
PMC traffic and MFMA busy of the layer-1 kernels are found under the names the
bench launches them with (parameter lists and the deferred-update flag of the
forward's template stripped)."""
import os

import numpy as np
import torch

import bench


FWD = "void gs::linear_fwd_wide_kernel<float, 48, true, true, true>(int, int, int, int, float const*, long)"
DW = "void gs::linear_dw_xcd_kernel<float, true, false, true, true>(int, int, int)"


def test_kernel_key_drops_params_and_pending_flag():
    assert bench.kernel_key(FWD) == "void gs::linear_fwd_wide_kernel<float, 48, true, true>"
    assert bench.kernel_key(FWD.replace("true, true, true>", "true, true, false>")) == bench.kernel_key(FWD)
    assert bench.kernel_key(DW) == "void gs::linear_dw_xcd_kernel<float, true, false, true, true>"


def test_dump_outputs_are_float32_bounded_and_repeatable(tmp_path, monkeypatch):
    """--dump-outputs: fp32 copies taken at the call, small arrays whole, a
    large one as the same sorted row sample every time, DUMP_LIMIT in all."""
    monkeypatch.setattr(bench, "DUMP_LIMIT", 3 * 4096)  # 4096 bytes per array
    w = torch.arange(35, dtype=torch.float64).reshape(7, 5)
    big = torch.arange(1000 * 8, dtype=torch.bfloat16).reshape(1000, 8)  # 32 bytes per fp32 row: 128 rows fit
    tensors = {"loss": torch.tensor(1.5), "layer.0.weight": w, "big": big}
    a = bench.snapshot_outputs(tensors, seed=824)
    w += 1.0  # a later step: the snapshot holds the earlier values
    assert all(v.dtype == np.float32 and v.flags["C_CONTIGUOUS"] for v in a.values())
    assert a["loss"].shape == (1,) and a["loss"][0] == 1.5
    assert np.array_equal(a["layer.0.weight"], np.arange(35, dtype=np.float32).reshape(7, 5))
    assert a["big"].shape == (128, 8) and sum(v.nbytes for v in a.values()) <= bench.DUMP_LIMIT
    rows = np.sort(np.random.RandomState(824).choice(1000, 128, replace=False))
    assert np.array_equal(a["big"], big.float().numpy()[rows])
    assert np.array_equal(bench.snapshot_outputs(tensors, seed=824)["big"], a["big"])
    out = tmp_path / "not" / "there" / "yet"
    bench.write_outputs(str(out), a)
    assert sorted(os.listdir(out)) == ["big.npy", "layer_0_weight.npy", "loss.npy"]
    assert all(np.array_equal(np.load(out / (k.replace(".", "_") + ".npy")), v) for k, v in a.items())


def test_committed_profiles_resolve():
    for cfg in ("rmat2m", "rmat2m-max-bf16"):
        rel = bench.rocprof_stats_file(cfg, 512)
        assert rel is not None and os.path.exists(os.path.join(bench.ROOT, rel))
    tr = bench.load_traffic("rmat2m", 512, FWD)
    assert tr is not None and tr["hbm_bytes"] > 0
    for k in (FWD, DW):
        mb = bench.load_mfma_busy("rmat2m", k)
        assert mb is not None and 0.0 < mb["mfma_util"] < 1.0
    assert bench.load_mfma_busy("no-such-config", FWD) is None


def test_plain_run_is_the_default():
    """--full and --dump-outputs are off unless given; --full is not taken for --full-graph."""
    args = bench.build_parser().parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (args.steps, args.warmup, args.full, args.dump_outputs, args.full_graph) == (7, 2, False, None, False)
    args = bench.build_parser().parse_args(["--full", "--dump-outputs", "d"])
    assert args.full and args.dump_outputs == "d" and not args.full_graph
