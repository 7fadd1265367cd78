"""The grid caps and tile sizes that the shapes of tests/test_gpu_grid_caps.py are derived from, read from the sources.  Those
tests exist to run the second and later trips of the capped, striding kernels; a cap raised (or a tile widened) later would
silently turn them back into single-trip tests, so a change here must come with new shapes there."""
import os
import re

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "warpconvnet_amd", "csrc")
WHY = "tests/test_gpu_grid_caps.py derives its shapes from this value: re-derive them there (and here) with the new one"

CONSTANTS = [
    ("ada_row.h", "kAdaThreads", 256),
    ("ada_row.h", "kAdaFwdBlocks", 4096),
    ("row_lists.h", "kRowThreads", 256),
    ("row_lists.h", "kRunPer", 8),
    ("row_lists.h", "kRowMaxGrid", 4096),
    ("row_lists.h", "kRowChunk", 256),
    ("attn_varlen.hip", "kAttnMaxGrid", 1 << 22),
    ("attn_varlen.hip", "kAttnBlock", 32),
    ("norm.hip", "WCN_NORM_BLOCKS", 512),
    ("norm.hip", "WCN_NORM_ROWS", 8),
    ("norm.hip", "kNormApplyBlocks", 2048),
    ("norm.hip", "kNormBwdApplyBlocks", 4096),
    ("pointconv.hip", "kPcMaxGrid", 256),
]
# the BatchNorm layouts and apply grids belong to another file
BN_WHY = ("tests/test_gpu_bn_bounds.py takes its shapes from tests/bn_bounds.py, which restates the layout with this value: change it "
          "there, and tests/test_bn_bounds_api.py says which cases no longer reach their second trips")
PC_WHY = ("tests/test_gpu_pointconv_bounds.py runs tests/pointconv_bounds.py's large cases past this cap (backward: one 32-edge "
          "tile a workgroup and trip; forward: eight): change BWD_GRID_CAP / FWD_WAVE_CAP there and the edge counts follow")
WHY_OF = {"WCN_NORM_ROWS": BN_WHY, "kNormApplyBlocks": BN_WHY, "kNormBwdApplyBlocks": BN_WHY, "kPcMaxGrid": PC_WHY}


def _value(text, name):
    """The integer a source gives ``name``: ``constexpr <type> name = <expr>;`` or ``#define name <expr>``."""
    found = re.findall(rf"constexpr\s+\w+\s+{name}\s*=\s*([^;]+);", text) + re.findall(rf"#define\s+{name}\s+(.+)", text)
    assert len(found) == 1, f"{name}: {len(found)} definitions found. {WHY}"
    expr = found[0].split("//")[0].strip()
    assert re.fullmatch(r"[0-9 <>*+()]+", expr), f"{name} = {expr!r} is no longer a plain integer expression. {WHY}"
    return eval(expr)  # digits, shifts, products and sums only (checked above)


@pytest.mark.parametrize("source,name,want", CONSTANTS, ids=[c[1] for c in CONSTANTS])
def test_constant_is_what_the_grid_cap_tests_assume(source, name, want):
    with open(os.path.join(CSRC, source)) as f:
        got = _value(f.read(), name)
    assert got == want, f"{source}: {name} = {got}, the grid-cap tests assume {want}. {WHY_OF.get(name, WHY)}"


def test_the_tests_use_the_same_values():
    from tests import test_gpu_grid_caps as caps

    want = {name: value for _, name, value in CONSTANTS}
    assert (caps.ADA_THREADS, caps.ADA_FWD_BLOCKS) == (want["kAdaThreads"], want["kAdaFwdBlocks"]), WHY
    assert (caps.VX_THREADS, caps.VX_PER, caps.VX_MAX_GRID) == (want["kRowThreads"], want["kRunPer"], want["kRowMaxGrid"]), WHY
    assert caps.CG_CHUNK == want["kRowChunk"] and (caps.ATTN_MAX_GRID, caps.ATTN_BLOCK) == (want["kAttnMaxGrid"], want["kAttnBlock"]), WHY
    from tests import bn_bounds as bb

    assert (bb.NORM_BLOCKS, bb.NORM_ROWS, bb.APPLY_BLOCKS, bb.BWD_APPLY_BLOCKS) == (
        want["WCN_NORM_BLOCKS"], want["WCN_NORM_ROWS"], want["kNormApplyBlocks"], want["kNormBwdApplyBlocks"]), BN_WHY
    from tests import pointconv_bounds as pb

    assert (pb.BWD_GRID_CAP, pb.FWD_WAVE_CAP) == (want["kPcMaxGrid"], 8 * want["kPcMaxGrid"]), PC_WHY


def test_chunk_rows_of_the_library(hip_lib):
    assert hip_lib.wcn_csr_chunk_rows() == 256, f"wcn_csr_chunk_rows() (kRowChunk). {WHY}"
