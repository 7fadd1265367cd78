"""CPU: the status every BatchNorm entry point of include/wcn.h returns for arguments it must refuse (or accept as empty)
BEFORE any launch.  The pointers are addresses inside a host buffer and are never dereferenced: every row of the table is a call
that returns from the argument checks.  Combinations that would launch (a layer entry whose only fault is a NULL `y` / `dx`: the
first pass runs before the second one looks at it) are left out on purpose.

The expected statuses were taken from the library as it was before the host half of csrc/norm.hip was rewritten around one
pass description (that library is the yardstick): -5 (WCN_ERROR_INVALID_PARAMETERS) everywhere, except that the apply-type
passes check shape / dtype (and the relu_scale / relu_shift pairing) first, then take n = 0 as success, then look at pointers.
Since then: `channels` above wcn_bn_max_channels() is -4 (WCN_ERROR_UNSUPPORTED_CONFIG) in every `wcn_bn_*` entry, looked at first.
include/wcn.h declares thirteen `wcn_bn_*` entries (one of them the workspace size) and the two `wcn_conv_bn_backward*`."""
import ctypes

import pytest

INVALID = -5
UNSUPPORTED = -4
C, N = 8, 4
_BUF = (ctypes.c_char * 256)()
P = (ctypes.addressof(_BUF) + 15) & ~15  # "a pointer": 16-B aligned, valid-looking, never read or written
BF16, F32 = 2, 0

_RED_TAIL = [("sum_dy", P), ("sum_dy_xhat", P), ("workspace", P), ("workspace_bytes", "WS"), ("stream", None)]
_SHAPE = [("n", N), ("channels", C), ("dtype", BF16)]
_TRAIN_BWD = [("x", P), ("z", None), ("relu", 1)] + _SHAPE + [("stats", P), ("gamma", P), ("training", 1), ("sums", P), ("dx", P),
                                                             ("dres", None), ("workspace", P), ("workspace_bytes", "WS"), ("stream", None)]
_CONV_BWD = [("x", P), ("y", P), ("z", None), ("relu", 1), ("stats", P), ("gamma", P), ("training", 1), ("sums", P), ("dy_conv", P),
             ("dres", None), ("w_packed_dgrad", P), ("rev_nbr", P), ("rev_mask", P), ("rev_perm", P), ("flip", 0), ("dx", P),
             ("in_maps", P), ("out_maps", P), ("offsets", P), ("dw", P), ("wgrad_workspace", P), ("wgrad_workspace_bytes", 1 << 20),
             ("n_in", N), ("n", N), ("cin", 64), ("channels", 64), ("num_offsets", 27), ("dtype", BF16), ("workspace", P),
             ("workspace_bytes", "WS"), ("stream", None)]

# entry -> (arguments in ABI order with a value that passes every check, the pointers the entry requires)
ENTRIES = {
    "wcn_bn_stats": ([("x", P)] + _SHAPE + [("mean", P), ("var", P), ("workspace", P), ("workspace_bytes", "WS"), ("stream", None)],
                     ["x", "mean", "var", "workspace"]),
    "wcn_bn_stats_fold": ([("x", P)] + _SHAPE + [("gamma", P), ("beta", P), ("running_mean", P), ("running_var", P), ("momentum", 0.1),
                                                 ("eps", 1e-5), ("mean", P), ("var", P), ("rstd", P), ("scale", P), ("shift", P),
                                                 ("num_batches_tracked", P), ("workspace", P), ("workspace_bytes", "WS"), ("stream", None)],
                          ["x", "mean", "var", "rstd", "scale", "shift", "workspace"]),
    "wcn_bn_fold": ([("running_mean", P), ("running_var", P), ("gamma", P), ("beta", P), ("eps", 1e-5), ("channels", C), ("mean", P),
                     ("rstd", P), ("scale", P), ("shift", P), ("stream", None)],
                    ["running_mean", "running_var", "mean", "rstd", "scale", "shift"]),
    "wcn_bn_apply": ([("x", P)] + _SHAPE + [("scale", P), ("shift", P), ("relu", 1), ("y", P), ("stream", None)],
                     ["x", "scale", "shift", "y"]),
    "wcn_bn_apply_residual": ([("x", P), ("residual", P)] + _SHAPE + [("scale", P), ("shift", P), ("relu", 1), ("y", P), ("stream", None)],
                              ["x", "residual", "scale", "shift", "y"]),
    "wcn_bn_backward_reduce": ([("dy", P), ("x", P), ("relu_scale", P), ("relu_shift", P)] + _SHAPE + [("mean", P), ("rstd", P)] + _RED_TAIL,
                               ["dy", "x", "mean", "rstd", "sum_dy", "sum_dy_xhat", "workspace"]),
    "wcn_bn_backward_reduce_masked": ([("dy", P), ("x", P), ("z", P)] + _SHAPE + [("mean", P), ("rstd", P)] + _RED_TAIL,
                                      ["dy", "x", "z", "mean", "rstd", "sum_dy", "sum_dy_xhat", "workspace"]),
    "wcn_bn_backward_apply": ([("dy", P), ("x", P), ("relu_scale", P), ("relu_shift", P)] + _SHAPE +
                              [("mean", P), ("rstd", P), ("gamma", P), ("sum_dy", P), ("sum_dy_xhat", P), ("dx", P), ("stream", None)],
                              ["dy", "x", "mean", "rstd", "sum_dy", "sum_dy_xhat", "dx"]),
    "wcn_bn_backward_apply_masked": ([("dy", P), ("x", P), ("z", P)] + _SHAPE +
                                     [("mean", P), ("rstd", P), ("gamma", P), ("sum_dy", P), ("sum_dy_xhat", P), ("dx", P), ("dres", P),
                                      ("stream", None)],
                                     ["dy", "x", "z", "mean", "rstd", "sum_dy", "sum_dy_xhat", "dx"]),
    # layer entries: only what the FIRST pass (statistics / reduce) refuses - `y` and `dx` are looked at after it has launched
    "wcn_bn_train_forward": ([("x", P), ("residual", None)] + _SHAPE +
                             [("gamma", P), ("beta", P), ("running_mean", P), ("running_var", P), ("momentum", 0.1), ("eps", 1e-5),
                              ("num_batches_tracked", P), ("relu", 1), ("stats", P), ("y", P), ("workspace", P), ("workspace_bytes", "WS"),
                              ("stream", None)],
                             ["x", "stats", "workspace"]),
    "wcn_bn_train_backward": ([("dy", P)] + _TRAIN_BWD, ["dy", "x", "stats", "sums", "workspace"]),
    "wcn_bn_train_backward_ld": ([("dy", P), ("dy_ld", 0)] + _TRAIN_BWD, ["dy", "x", "stats", "sums", "workspace"]),
    "wcn_conv_bn_backward": ([("dy", P)] + _CONV_BWD, ["dy", "y", "stats", "sums", "dy_conv", "workspace"]),
    "wcn_conv_bn_backward_ld": ([("dy", P), ("dy_ld", 0)] + _CONV_BWD, ["dy", "y", "stats", "sums", "dy_conv", "workspace"]),
}
# n = 0 is an empty tensor and a success for these (after the shape / dtype checks, before the pointer checks)
EMPTY_OK = ("wcn_bn_apply", "wcn_bn_apply_residual", "wcn_bn_backward_apply", "wcn_bn_backward_apply_masked")


def _rows(name):
    """-> [(what, overrides, expected status)] for one entry."""
    args, required = ENTRIES[name]
    has = {k for k, _ in args}
    rows = [(f"{p} NULL", {p: None}, INVALID) for p in required]
    if "n" in has:
        rows += [("n = 0", {"n": 0}, 0 if name in EMPTY_OK else INVALID), ("n = -1", {"n": -1}, INVALID)]
    rows += [("channels = 0", {"channels": 0}, INVALID)]
    if name.startswith("wcn_bn_"):  # wider than wcn_bn_max_channels(): refused first, forward and backward alike
        rows += [("channels = limit + 1", {"channels": "LIMIT+1"}, UNSUPPORTED)]
        if "n" in has:
            rows += [("channels = limit + 1, n = 0", {"channels": "LIMIT+1", "n": 0}, UNSUPPORTED)]
    if "dtype" in has:
        rows += [("dtype 3", {"dtype": 3}, INVALID)]
    if name in EMPTY_OK:  # the order of the checks: shape / dtype -> n == 0 is success -> pointers
        rows += [("n = 0, every pointer NULL", {"n": 0, **{p: None for p in required}}, 0),
                 ("n = 0, channels = 0", {"n": 0, "channels": 0}, INVALID), ("n = 0, dtype 3", {"n": 0, "dtype": 3}, INVALID)]
    if "workspace_bytes" in has:
        rows += [("workspace one byte short", {"workspace_bytes": "WS-1"}, INVALID)]
    if "relu_scale" in has:
        rows += [("relu_scale without relu_shift", {"relu_shift": None}, INVALID),
                 ("relu_shift without relu_scale", {"relu_scale": None}, INVALID)]
        if name in EMPTY_OK:  # (the pairing belongs to the shape checks: refused on an empty tensor too)
            rows += [("n = 0, relu_scale without relu_shift", {"n": 0, "relu_shift": None}, INVALID)]
    if "running_mean" in has and name != "wcn_bn_fold":
        rows += [("running_mean without running_var", {"running_var": None}, INVALID),
                 ("running_var without running_mean", {"running_mean": None}, INVALID)]
    if "dy_ld" in has:
        rows += [("dy_ld = channels - 1", {"dy_ld": dict(args)["channels"] - 1}, INVALID)]
    if "z" in has and "relu" in has:  # layer entries: the same refusals on the masked passes of a residual tail
        rows += [(f"residual tail, {what}", {"z": P, **over}, want) for what, over, want in list(rows)]
    if name.startswith("wcn_conv_bn"):
        rows += [("fp32 (the convolution's kernels are 16-bit)", {"dtype": F32}, INVALID)]
    return rows


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_bn_entry_refuses_before_any_launch(hip_lib, name):
    fn = getattr(hip_lib, name)
    args, _ = ENTRIES[name]
    got = []
    for what, over, want in _rows(name):
        vals = dict(args)
        vals.update(over)
        ws = hip_lib.wcn_bn_workspace(dict(args)["channels"])
        named = {"WS": ws, "WS-1": ws - 1, "LIMIT+1": hip_lib.wcn_bn_max_channels() + 1}
        call = [named.get(vals[k], vals[k]) if isinstance(vals[k], str) else vals[k] for k, _ in args]
        rc = fn(*call)
        if rc != want:
            got.append(f"{what}: {rc}, expected {want}")
    assert len(_rows(name)) >= 5 and not got, f"{name}: " + "; ".join(got)


def test_bn_workspace_size(hip_lib):
    assert hip_lib.wcn_bn_workspace(0) == 0 and hip_lib.wcn_bn_workspace(-1) == 0
    assert hip_lib.wcn_bn_workspace(C) > 0 and hip_lib.wcn_bn_workspace(2 * C) == 2 * hip_lib.wcn_bn_workspace(C)


def test_bn_channel_limit_is_the_backward_applys_lds(hip_lib):
    """Five fp32 coefficients per channel in the 64 KB of dynamic LDS a launch gets without raising the kernel's limit."""
    limit = hip_lib.wcn_bn_max_channels()
    assert limit == 3276 and 5 * 4 * limit <= 65536 < 5 * 4 * (limit + 1)
