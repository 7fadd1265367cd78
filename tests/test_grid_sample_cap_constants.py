"""The grid cap, chunk and tile sizes of csrc/row_lists.h and csrc/grid.hip that the second-trip shapes of tests/test_gpu_grid_sample.py are derived
from, read from the sources.  Those shapes exist to run the second trip of every capped, striding kernel and the chunked cells
of the backward; a constant changed later would silently turn them into single-trip tests, so a change here must come with
new shapes there."""
import os

import pytest

from tests.test_grid_cap_constants import CSRC, _value

WHY = "tests/grid_sample_caps.py derives the second-trip shapes from this value: re-derive them there (and here) with the new one"
CONSTANTS = [("kRowThreads", 256), ("kRowMaxGrid", 4096), ("kRowChunk", 256), ("kGsPlanarCh", 8)]
SOURCE = {"kGsPlanarCh": "grid.hip"}  # the rest: row_lists.h, shared with voxelize.hip and lattice.hip


@pytest.mark.parametrize("name,want", CONSTANTS, ids=[c[0] for c in CONSTANTS])
def test_constant_is_what_the_second_trip_shapes_assume(name, want):
    source = SOURCE.get(name, "row_lists.h")
    with open(os.path.join(CSRC, source)) as f:
        got = _value(f.read(), name)
    assert got == want, f"{source}: {name} = {got}, the tests assume {want}. {WHY}"


def test_the_tests_use_the_same_values():
    from tests import grid_sample_caps as caps

    want = dict(CONSTANTS)
    assert (caps.GS_THREADS, caps.GS_MAX_GRID, caps.GS_CHUNK, caps.GS_PLANAR_CH) == (
        want["kRowThreads"], want["kRowMaxGrid"], want["kRowChunk"], want["kGsPlanarCh"]), WHY
    # one thread per point (keys), one lane per point (rows, C = 1), one item per point (planar, C = 1)
    assert caps.POINTS_SECOND_TRIP_KEYS == caps.POINTS_SECOND_TRIP_ROWS == caps.POINTS_SECOND_TRIP_PLANAR == 4096 * 256 + 1
    # one workgroup per tile of 256 sorted positions; one lane per vertex at C = 1
    assert caps.POINTS_SECOND_TRIP_CHUNKS == 4096 * 256 + 1 and caps.VERTICES_SECOND_TRIP == 4096 * 256 + 1


def test_constants_of_the_library(hip_lib):
    assert hip_lib.wcn_grid_max_grid() == 4096, f"wcn_grid_max_grid() (kRowMaxGrid). {WHY}"
    assert hip_lib.wcn_grid_chunk_points() == 256, f"wcn_grid_chunk_points() (kRowChunk). {WHY}"
