"""The grid cap, tile and chunk sizes of csrc/row_lists.h and csrc/lattice.hip that the shapes of tests/test_gpu_lattice_filter.py and
tests/test_gpu_hash128.py are derived from, read from the sources.  Those shapes exist to run the second trip of every capped,
striding kernel and the chunked rows of the splat; a constant changed later would silently turn them into single-trip tests, so
a change here must come with new shapes there."""
import pytest

from tests.test_grid_cap_constants import CSRC, _value
import os

WHY = "tests/lattice_caps.py derives the second-trip shapes from this value: re-derive them there (and here) with the new one"
CONSTANTS = [("kRowThreads", 256), ("kRunPer", 8), ("kRowMaxGrid", 4096), ("kRowChunk", 256), ("kLtSearchMax", 32)]
SOURCE = {"kLtSearchMax": "lattice.hip"}  # the rest: row_lists.h, shared with voxelize.hip


@pytest.mark.parametrize("name,want", CONSTANTS, ids=[c[0] for c in CONSTANTS])
def test_constant_is_what_the_second_trip_shapes_assume(name, want):
    source = SOURCE.get(name, "row_lists.h")
    with open(os.path.join(CSRC, source)) as f:
        got = _value(f.read(), name)
    assert got == want, f"{source}: {name} = {got}, the tests assume {want}. {WHY}"


def test_the_tests_use_the_same_values():
    from tests import lattice_caps as caps

    want = dict(CONSTANTS)
    assert (caps.LT_THREADS, caps.LT_PER, caps.LT_MAX_GRID, caps.LT_CHUNK) == (want["kRowThreads"], want["kRunPer"],
                                                                             want["kRowMaxGrid"], want["kRowChunk"]), WHY
    # one thread per point / key: the first count that takes a second trip
    assert caps.POINTS_SECOND_TRIP == 4096 * 256 + 1
    # one scan tile of 2048 sorted entries per workgroup
    assert caps.ENTRIES_SECOND_TRIP == 4096 * 2048 + 1
    # 64 lanes per row at the widest rows: four rows per workgroup
    assert caps.WIDE_CHANNELS == 253 and caps.WIDE_ROWS_SECOND_TRIP == 4096 * 4 + 1
    # longest_row_kernel / row_list_collect_kernel: a thread per vertex row; lt_splat_kernel<true> / lt_combine_kernel: a lane group per item / long row
    assert caps.VERTICES_SECOND_TRIP == 4096 * 256 + 1 and caps.LONG_ROWS_SECOND_TRIP == 4096 * 4 + 1


def test_chunk_rows_of_the_library(hip_lib):
    assert hip_lib.wcn_lattice_chunk_rows() == 256, f"wcn_lattice_chunk_rows() (kRowChunk). {WHY}"
