"""The constants of csrc/segmented.hip that the shapes of tests/test_gpu_segmented.py are derived from
(tests/test_segmented_cap_constants.py fails when one changes without these being re-derived)."""
SEG_THREADS = 256        # kSegThreads: threads of a workgroup
SEG_CHUNK = 256          # kSegChunk: rows of one chunk of a segment = rows of one tile of the apply pass (wcn_seg_chunk_rows)
SEG_MAX_GRID = 4096      # kRowMaxGrid: the cap of every grid (wcn_seg_max_grid)
SEG_MERGE_COLS = 32      # kSegMergeCols
SEG_MERGE_SLICES = 8     # kSegMergeSlices: runs of chunks of one segment in the merge

T = SEG_CHUNK

# lengths of the segments of a batch
MIXED = (0, 1, T - 1, T, T + 1, 3 * T + 7, 0, 2)
MANY = tuple(i % 4 for i in range(1500))  # more segments than a chunk has rows
LONG = (40 * T + 5,)                      # more chunks than the merge has slices, the last one short
# Past every cap at once (C = 1): the one long segment has more chunks than the chunk kernel has workgroups and more tiles
# than the apply kernel has, the one-row segments around it are more than the merge kernel has workgroups and more than one
# trip of the plan's scan.
PAST_CAPS = (1,) * (SEG_MAX_GRID // 2 + 1) + (SEG_MAX_GRID * SEG_CHUNK + 1,) + (1,) * (SEG_MAX_GRID // 2 + 1)
