"""The constants that the shapes of tests/test_gpu_segmented.py are derived from (tests/segmented_caps.py), read from the
sources: a chunk widened or a cap raised later would silently turn the chunk-boundary and second-trip cases into plain ones."""
import os
import re

import pytest

from tests import segmented_caps as caps

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "warpconvnet_amd", "csrc")
WHY = "tests/segmented_caps.py derives the shapes of tests/test_gpu_segmented.py from this value: re-derive them with the new one"

CONSTANTS = [
    ("segmented.hip", "kSegThreads", caps.SEG_THREADS),
    ("segmented.hip", "kSegChunk", caps.SEG_CHUNK),
    ("segmented.hip", "kSegMergeCols", caps.SEG_MERGE_COLS),
    ("segmented.hip", "kSegMergeSlices", caps.SEG_MERGE_SLICES),
    ("row_lists.h", "kRowMaxGrid", caps.SEG_MAX_GRID),
]


@pytest.mark.parametrize("source,name,want", CONSTANTS, ids=[c[1] for c in CONSTANTS])
def test_constant_is_what_the_segmented_tests_assume(source, name, want):
    with open(os.path.join(CSRC, source)) as f:
        found = re.findall(rf"constexpr\s+int\s+{name}\s*=\s*([0-9]+)\s*;", f.read())
    assert len(found) == 1, f"{name}: {len(found)} plain integer definitions found. {WHY}"
    assert int(found[0]) == want, f"{source}: {name} = {found[0]}, the tests assume {want}. {WHY}"


def test_the_library_exports_the_same_values(hip_lib):
    assert hip_lib.wcn_seg_chunk_rows() == caps.SEG_CHUNK, WHY
    assert hip_lib.wcn_seg_max_grid() == caps.SEG_MAX_GRID, WHY


def test_the_length_sets_cross_what_they_are_meant_to_cross():
    t = caps.T
    assert {t - 1, t, t + 1, 3 * t + 7, 0, 1}.issubset(caps.MIXED)
    assert len(caps.MANY) > caps.SEG_CHUNK and set(caps.MANY) == {0, 1, 2, 3}
    assert -(-caps.LONG[0] // t) > caps.SEG_MERGE_SLICES and caps.LONG[0] % t != 0
    assert max(caps.PAST_CAPS) > caps.SEG_MAX_GRID * caps.SEG_CHUNK      # chunk workgroups and apply tiles: a second trip
    assert len(caps.PAST_CAPS) > caps.SEG_MAX_GRID                        # merge workgroups: a second trip
