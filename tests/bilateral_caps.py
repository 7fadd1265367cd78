"""Shapes at which the solver's and the kNN filter's capped, striding kernels of csrc/lattice.hip take a second trip, derived
from its constants (tests/test_bilateral_cap_constants.py fails when a constant changes without these being re-derived)."""
LT_THREADS = 256    # kRowThreads
LT_MAX_GRID = 4096  # kRowMaxGrid: also the slots of one scalar's partials

# matvec, update and direction kernels: min(64, pow2(pitch / 4)) lanes per row; 253 channels -> pitch 256 -> 64 lanes -> four
# rows per workgroup.  More vertices than this: every workgroup strides and every scalar has LT_MAX_GRID partials.
WIDE_CHANNELS = 253
WIDE_PITCH = 256
ROWS_PER_WORKGROUP = LT_THREADS // 64
VERTICES_SECOND_TRIP = LT_MAX_GRID * ROWS_PER_WORKGROUP + 1
# points on a SIDE x SIDE integer lattice in the plane: every point is its cell's lower corner and names the three other
# corners with weight zero -> (SIDE + 1)^2 vertices
LATTICE_SIDE = 130
LATTICE_VERTICES = (LATTICE_SIDE + 1) ** 2
# weights kernel: one thread per query, whatever k and the widths
QUERIES_SECOND_TRIP = LT_MAX_GRID * LT_THREADS + 1
