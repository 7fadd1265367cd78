"""Shapes at which the capped, striding kernels of csrc/grid.hip take a second trip, derived from its constants
(tests/test_grid_sample_cap_constants.py fails when a constant changes without these being re-derived)."""
GS_THREADS = 256    # kRowThreads
GS_MAX_GRID = 4096  # kRowMaxGrid
GS_CHUNK = 256      # kRowChunk: points of one chunk of a crowded cell = sorted positions of one tile of the chunk kernel
GS_PLANAR_CH = 8    # kGsPlanarCh: channels of one thread of the planar forward kernel

# keys: one thread per point
POINTS_SECOND_TRIP_KEYS = GS_MAX_GRID * GS_THREADS + 1
# forward, channel stride 1: min(64, pow2(C)) lanes per point; C = 1 -> one lane -> GS_THREADS points per workgroup
POINTS_SECOND_TRIP_ROWS = GS_MAX_GRID * GS_THREADS + 1
# forward, planar: one thread per (point, GS_PLANAR_CH channels); C = 1 -> one item per point
POINTS_SECOND_TRIP_PLANAR = GS_MAX_GRID * GS_THREADS + 1
# backward, chunk partials: one workgroup per GS_CHUNK sorted positions
POINTS_SECOND_TRIP_CHUNKS = GS_MAX_GRID * GS_CHUNK + 1
# backward, vertices: min(64, pow2(C)) lanes per vertex; C = 1 -> GS_THREADS vertices per workgroup
VERTICES_SECOND_TRIP = GS_MAX_GRID * GS_THREADS + 1
