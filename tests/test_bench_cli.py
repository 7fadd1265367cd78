"""CPU: bench.py's command line - a plain run's result line, `--full`, and `--dump-outputs` on the step's own code path
(the tensors on the CPU, the convolution on the explicit backend with an oracle-built map, as in test_dist_gloo.py)."""
import numpy as np
import pytest
import torch

NAMES = ("out_features", "out_coords", "grad_features", "grad_weight", "grad_bias")


def test_plain_run_is_the_default_and_steps_must_be_positive():
    import bench

    args = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert not args.full and args.dump_outputs is None and args.steps == 7 and args.warmup == 2
    args = bench.parse_args(["--full", "--dump-outputs", "d", "--no-secondary"])
    assert args.full and args.dump_outputs == "d" and args.no_secondary
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])


def test_headline_line_carries_the_headline_fields():
    import bench

    args = bench.parse_args(["--steps", "4"])
    line = bench.headline(args, 1, 1000, 12.5, 0.08, {"value": 13.0})
    for key, want in (("value", 12.5), ("unit", "M voxels/s"), ("higher_is_better", True), ("dtype", "bf16"),
                      ("ms_per_step", 0.08), ("steps", 4)):
        assert line[key] == want, key
    assert line["metric"].startswith("M active voxels/sec fwd+bwd")


def _run_and_dump(out_dir, steps):
    import bench
    from tests.test_host_api import _attach_oracle_map

    torch.set_num_threads(1)
    args = bench.parse_args(["--steps", str(steps), "--warmup", "1", "--voxels", "600"])
    dev = torch.device("cpu")
    kw = dict(fwd_algo="explicit_gemm", dgrad_algo="explicit_gemm", wgrad_algo="explicit_gemm")
    coords, feats, grad_out, offsets, conv, params = bench.build_workload(args, dev, 0, conv_kwargs=kw)
    keep = {}
    step, _ = bench.make_step(dev, 1, coords, feats, grad_out, offsets, conv, params, attach=_attach_oracle_map, keep=keep)
    bench.timed_loop(step, args, dev, 1)
    y = keep["y"]
    bench.dump_outputs(str(out_dir), y, feats, conv, rows=500)
    return y, feats, conv


def test_dump_outputs_writes_the_last_step_and_repeats(tmp_path):
    y, feats, conv = _run_and_dump(tmp_path / "a", 2)
    got = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in NAMES}
    assert all(a.dtype == np.float32 for a in got.values())
    n = y.batched_features.batched_tensor.shape[0]
    assert got["out_features"].shape == (500, 128) and got["grad_features"].shape == (500, 64)
    assert got["out_coords"].shape == (500, 3) and got["grad_weight"].shape == (27, 64, 128) and got["grad_bias"].shape == (128,)
    pick = np.sort(np.random.default_rng(0).choice(n, size=500, replace=False))
    np.testing.assert_array_equal(got["out_features"], y.batched_features.batched_tensor.detach().numpy()[pick])
    np.testing.assert_array_equal(got["grad_features"], feats.grad.numpy()[pick])
    np.testing.assert_array_equal(got["grad_weight"], conv.weight.grad.numpy())
    np.testing.assert_array_equal(got["grad_bias"], conv.bias.grad.numpy())
    # the same arguments give the same inputs, so a second process-like run dumps the same arrays
    _run_and_dump(tmp_path / "b", 2)
    for name in NAMES:
        np.testing.assert_array_equal(np.load(tmp_path / "b" / f"{name}.npy"), got[name])
