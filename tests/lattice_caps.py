"""Shapes at which the capped, striding kernels of csrc/lattice.hip take a second trip, derived from its constants
(tests/test_lattice_cap_constants.py fails when a constant changes without these being re-derived)."""
LT_THREADS = 256    # kRowThreads
LT_PER = 8          # kRunPer: sorted entries per thread of a scan tile
LT_MAX_GRID = 4096  # kRowMaxGrid
LT_CHUNK = 256      # kRowChunk

# geometry, hash insert and hash search: one thread per point / key
POINTS_SECOND_TRIP = LT_MAX_GRID * LT_THREADS + 1
# run heads: one workgroup per tile of LT_THREADS * LT_PER sorted entries
ENTRIES_SECOND_TRIP = LT_MAX_GRID * LT_THREADS * LT_PER + 1
# splat / blur / slice: min(64, pow2(pitch / 4)) lanes per row; 253 channels -> pitch 256 -> 64 lanes -> 4 rows per workgroup
WIDE_CHANNELS = 253
WIDE_ROWS_SECOND_TRIP = LT_MAX_GRID * (LT_THREADS // 64) + 1
# longest row and chunk plan: one thread (one lane of a wave) per vertex row -> more vertices than this, one long row among the late ones
VERTICES_SECOND_TRIP = LT_MAX_GRID * LT_THREADS + 1
# chunk partials and their combination: one lane group per chunk item / per long row, four groups per workgroup at the wide
# pitch; a long row has at least LT_CHUNK + 1 entries, hence two chunks: this many long rows give the combine kernel its second
# trip and twice as many chunk items
LONG_ROWS_SECOND_TRIP = LT_MAX_GRID * (LT_THREADS // 64) + 1
