"""The constants that the shapes of tests/test_gpu_fps.py are derived from (tests/fps_caps.py), read from the source and from
the library: a cap raised or a workgroup resized later would silently turn the edge cases into plain ones."""
import os
import re

import pytest

from tests import fps_caps as caps

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "warpconvnet_amd", "csrc")
WHY = "tests/fps_caps.py derives the shapes of tests/test_gpu_fps.py from this value: re-derive them with the new one"

CONSTANTS = [
    ("kFpsThreads", caps.FPS_THREADS),
    ("kFpsMaxP", caps.FPS_MAX_P),
    ("kFpsBlocksPerSeg", caps.FPS_BLOCKS_PER_SEG),
    ("kFpsMaxGrid", caps.FPS_MAX_GRID),
]


@pytest.mark.parametrize("name,want", CONSTANTS, ids=[c[0] for c in CONSTANTS])
def test_constant_is_what_the_fps_tests_assume(name, want):
    with open(os.path.join(CSRC, "fps.hip")) as f:
        found = re.findall(rf"constexpr\s+int\s+{name}\s*=\s*([0-9]+)\s*;", f.read())
    assert len(found) == 1, f"{name}: {len(found)} plain integer definitions found. {WHY}"
    assert int(found[0]) == want, f"fps.hip: {name} = {found[0]}, the tests assume {want}. {WHY}"


def test_the_resident_instantiations_are_the_ones_the_tests_walk():
    with open(os.path.join(CSRC, "fps.hip")) as f:
        found = sorted(int(p) for p in set(re.findall(r"fps_resident_launch<(\d+)>\(a, s\)", f.read())))
    assert tuple(found) == caps.FPS_INSTANTIATIONS, WHY


def test_the_library_exports_the_same_values(hip_lib):
    assert hip_lib.wcn_abi_version() >= 17
    assert hip_lib.wcn_fps_resident_max_points() == caps.R, WHY
    assert hip_lib.wcn_fps_block_threads() == caps.T, WHY
    assert hip_lib.wcn_fps_blocks_per_segment() == caps.G, WHY
    assert hip_lib.wcn_fps_max_grid() == caps.FPS_MAX_GRID, WHY


def test_the_length_sets_cross_what_they_are_meant_to_cross():
    t, g, r = caps.T, caps.G, caps.R
    assert {0, 1, 63, 64, 65, t - 1, t, t + 1, r - 1, r}.issubset(caps.RESIDENT) and max(caps.RESIDENT) == r
    # every instantiation is launched for a full segment and for the shortest one that needs it
    assert {caps.instantiation(n) for n in caps.PER_INSTANTIATION} | {caps.instantiation(r)} == set(caps.FPS_INSTANTIATIONS)
    for p in caps.FPS_INSTANTIATIONS[:-1]:
        assert p * t in caps.PER_INSTANTIATION and p * t + 1 in caps.PER_INSTANTIATION
    assert len(caps.MANY) > caps.FPS_MAX_GRID and set(caps.MANY) == {0, 1, 2}
    assert max(caps.STREAMED) > g * t > sorted(caps.STREAMED)[-2] and t + 1 in caps.STREAMED  # second trip of the stride
    assert caps.NATURAL == (r + 1,)
    assert max(caps.MIXED) > r and r in caps.MIXED and 0 in caps.MIXED
    assert max(caps.SHORT) == 7 and min(caps.SHORT) < 7
