"""The constants of csrc/row_lists.h and csrc/lattice.hip that the second-trip shapes of tests/test_gpu_bilateral_solver.py are derived from, read
from the sources and from the library.  A constant changed later would silently turn those into single-trip tests, so a change
here must come with new shapes there."""
import os

import pytest

from tests.test_grid_cap_constants import CSRC, _value

WHY = "tests/bilateral_caps.py derives the second-trip shapes from this value: re-derive them there (and here) with the new one"
CONSTANTS = [("kRowThreads", 256), ("kRowMaxGrid", 4096), ("kPcgWords", 8)]
SOURCE = {"kPcgWords": "lattice.hip"}  # the rest: row_lists.h


@pytest.mark.parametrize("name,want", CONSTANTS, ids=[c[0] for c in CONSTANTS])
def test_constant_is_what_the_second_trip_shapes_assume(name, want):
    source = SOURCE.get(name, "row_lists.h")
    with open(os.path.join(CSRC, source)) as f:
        got = _value(f.read(), name)
    assert got == want, f"{source}: {name} = {got}, the tests assume {want}. {WHY}"


def test_the_tests_use_the_same_values():
    from tests import bilateral_caps as caps

    want = dict(CONSTANTS)
    assert (caps.LT_THREADS, caps.LT_MAX_GRID) == (want["kRowThreads"], want["kRowMaxGrid"]), WHY
    assert caps.WIDE_CHANNELS == 253 and caps.WIDE_PITCH == 256 and caps.ROWS_PER_WORKGROUP == 4
    assert caps.VERTICES_SECOND_TRIP == 4096 * 4 + 1
    assert caps.LATTICE_VERTICES == 131 * 131 and caps.LATTICE_VERTICES >= caps.VERTICES_SECOND_TRIP
    assert caps.QUERIES_SECOND_TRIP == 4096 * 256 + 1


def test_grid_rule_of_the_library(hip_lib):
    """The row kernels' grid = the number of partials of a scalar: lanes per row from the pitch, capped."""
    from tests import bilateral_caps as caps

    assert hip_lib.wcn_abi_version() >= 14
    assert hip_lib.wcn_lattice_max_grid() == caps.LT_MAX_GRID, WHY
    assert hip_lib.wcn_lattice_row_grid(100, caps.WIDE_PITCH) == 25  # four rows per workgroup
    assert hip_lib.wcn_lattice_row_grid(caps.VERTICES_SECOND_TRIP - 1, caps.WIDE_PITCH) == caps.LT_MAX_GRID
    assert hip_lib.wcn_lattice_row_grid(caps.VERTICES_SECOND_TRIP, caps.WIDE_PITCH) == caps.LT_MAX_GRID  # strides from here on
    assert hip_lib.wcn_lattice_row_grid(1000, 4) == 4 and hip_lib.wcn_lattice_row_grid(1000, 8) == 8  # 256 / 128 rows
    assert hip_lib.wcn_lattice_row_grid(1, 4) == 1 and hip_lib.wcn_lattice_row_grid(0, 4) == 1
    assert hip_lib.wcn_lattice_row_grid(10, 6) == 0  # not a pitch
    # argument checks come back as status codes before any launch
    assert hip_lib.wcn_bilateral_pcg(None, 2, 4, 4, 0.5, 1.0, 0.5, None, None, None, 1.0, None, None, None, None, None, 1, 0.0, None) == -5
    assert hip_lib.wcn_bilateral_matvec(None, 2, 4, 4, 0.5, 1.0, 0.5, None, None, 1.0, None, None, None, None, None) == -5
    assert hip_lib.wcn_bilateral_knn_weights(None, None, None, None, None, 4, 4, 0, 3, 3, 1.0, 1.0, None, None) == -5
    assert hip_lib.wcn_bilateral_knn_weights(None, None, None, None, None, 4, 0, 1, 3, 3, 1.0, 1.0, None, None) == 0
