"""CPU checks of the 16-bit PointConv edge path (csrc/pointconv16.hip): the C declarations, the support predicate at its limits
and the rounding contract the kernels implement."""
import os

import pytest
import torch

from tests import pointconv_bounds as pb
from tests.test_gpu_pointconv16 import CASES, build, run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("supported", "packed_bytes", "pack", "edge_forward", "edge_backward", "backward_workspace", "grad_floats")


def test_symbols_declared_and_bound():
    from warpconvnet_amd import _lib

    header = open(os.path.join(ROOT, "include", "wcn.h")).read()
    for s in SYMBOLS:
        assert f"wcn_pointconv16_{s}(" in header and f"wcn_pointconv16_{s}" in _lib.SIGNATURES, s


@pytest.mark.parametrize("args,want", [
    ((32, 32, 0, 128, 64, 16, 0, 2), 1), ((32, 29, 3, 128, 64, 32, 0, 1), 1), ((16, 0, 0, 32, 24, 1, 1, 2), 1),
    ((32, 32, 3, 128, 64, 16, 1, 2), 0),   # edge-in 67
    ((32, 32, 0, 129, 64, 16, 0, 2), 0), ((32, 32, 0, 128, 65, 16, 1, 2), 0),
    ((32, 32, 0, 128, 64, 64, 0, 2), 0), ((32, 32, 0, 128, 64, 3, 0, 2), 0),   # k above 32, k no power of two
    ((32, 32, 0, 128, 48, 16, 0, 2), 0),   # identity shortcut with other widths
    ((32, 32, 0, 128, 64, 16, 0, 0), 0),   # fp32 is the other family
])
def test_supported_limits(args, want):
    from warpconvnet_amd import _lib

    assert _lib.lib().wcn_pointconv16_supported(*args) == want


@pytest.mark.parametrize("name", list(CASES))
def test_rounding_contract(name):
    """The operand roundings of the kernels that can be applied from outside - the fp64 chain on bf16-rounded feature rows and
    weights (not the relative positions or the hidden activation, which are rounded inside the chain) - move the forward result
    no further from the plain fp64 chain than the composed CPU-autocast evaluation is, and the composed run has the fp64 ReLU
    mask: what the GPU parity test compares is well defined.  bf16, forward."""
    case, ids, ref = build(name)
    r64 = pb.chain(ref, torch.float64)
    comp, mask = run(case, ids, ref, torch.bfloat16, torch.device("cpu"), fused=False)
    assert torch.equal(mask, r64["z1"] > 0)
    bf = lambda t: None if t is None else t.bfloat16().float()
    rounded = pb.make_case(name, tiefree=True, **CASES[name])
    rounded.feats, rounded.qfeats = bf(case.feats), bf(case.qfeats)
    rounded.nbr, rounded.counts = ref.nbr, ref.counts
    with torch.no_grad():
        for lin in (rounded.mlp.block[0], rounded.mlp.block[3], rounded.mlp.shortcut):
            if isinstance(lin, torch.nn.Linear):
                lin.weight.copy_(bf(lin.weight))
    r16 = pb.chain(rounded, torch.float64, backward=False)
    assert (r16["out"] - r64["out"]).abs().max() <= pb.LANE_ORDER * (comp["out"] - r64["out"]).abs().max()
