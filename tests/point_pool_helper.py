"""Shared by test_point_pool_api.py / test_gpu_point_pool.py / test_gpu_voxelize.py: the golden fixture, an fp64 segment
reference and the derived error bounds."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "point_pool.npz")
U_OUT = {torch.float64: 2.0 ** -53, torch.float32: 2.0 ** -24, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
# half the spacing of the subnormals: the absolute rounding error of a result that underflows (the relative model stops there)
UNDERFLOW = {torch.float64: 2.0 ** -1075, torch.float32: 2.0 ** -150, torch.float16: 2.0 ** -25, torch.bfloat16: 2.0 ** -134}
_CACHE = {}


def golden():
    if "z" not in _CACHE:
        _CACHE["z"] = np.load(GOLDEN)
    return _CACHE["z"]


def golden_case(name):
    z = golden()
    return {k.split(".", 1)[1]: z[k] for k in z.files if k.startswith(name + ".")}


def golden_names():
    return [str(n) for n in golden()["names"]]


def first_point_rule(to_orig, m):
    """Smallest row of every voxel, recomputed from the inverse map."""
    first = np.full(m, len(to_orig), np.int64)
    np.minimum.at(first, to_orig, np.arange(len(to_orig)))
    return first


def segment_reference(x64: torch.Tensor, csr_indices: torch.Tensor, csr_offsets: torch.Tensor):
    """fp64, CPU: per segment the sum, the sum of magnitudes, max / min with the FIRST extremum's original row, the length.
    Scatter reductions over the flat list: nothing is padded to the longest segment."""
    idx, off = csr_indices.cpu().long(), csr_offsets.cpu().long()
    m, c, nnz = off.numel() - 1, x64.shape[1], idx.numel()
    length = off[1:] - off[:-1]
    seg = torch.repeat_interleave(torch.arange(m), length)
    g = x64[idx]
    out = {"len": length, "sum": torch.zeros((m, c), dtype=torch.float64).index_add_(0, seg, g),
           "abs": torch.zeros((m, c), dtype=torch.float64).index_add_(0, seg, g.abs())}
    segc, empty = seg[:, None].expand(nnz, c), (length == 0)[:, None]
    for name, fill, red in (("max", float("-inf"), "amax"), ("min", float("inf"), "amin")):
        val = torch.full((m, c), fill, dtype=torch.float64).scatter_reduce_(0, segc, g, red)
        at = torch.where(g == val[seg], torch.arange(nnz)[:, None].expand(nnz, c), torch.full((nnz, c), nnz))
        first = torch.full((m, c), nnz, dtype=torch.long).scatter_reduce_(0, segc, at, "amin")  # first position of the extremum
        out[name] = torch.where(empty, torch.zeros_like(val), val)
        out["arg" + name] = torch.where(empty, torch.full_like(first, -1), idx[first.clamp_max(max(nnz - 1, 0))] if nnz else first)
    return out


def assert_sum_like(got: torch.Tensor, ref: dict, op: str, dtype, what="", underflow=False):
    """|got - ref| <= L * 2^-24 * sum|x| + u_out * |ref| (mean: twice the first term for its division, then / L).
    ``underflow``: for inputs that hold subnormals (coordinates one ulp from zero) the absolute rounding error of a subnormal
    result is added - the relative model stops there."""
    L = ref["len"].double().clamp_min(1)[:, None]
    want = ref["sum"] / L if op == "mean" else ref["sum"]
    acc = 2.0 ** -53 if dtype == torch.float64 else 2.0 ** -24
    first = L * acc * ref["abs"]
    bound = (2 * first / L if op == "mean" else first) + U_OUT[dtype] * want.abs() + (UNDERFLOW[dtype] if underflow else 0.0)
    err = (got.detach().double().cpu() - want).abs()
    worst = (err - bound).max().item() if err.numel() else 0.0
    print(f"{what} {op} {dtype}: max err {err.max().item() if err.numel() else 0:.3e}, max bound {bound.max().item() if err.numel() else 0:.3e}")
    assert worst <= 0, f"{what} {op} {dtype}: error exceeds the bound by {worst:.3e}"
