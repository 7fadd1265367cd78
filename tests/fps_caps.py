"""The constants of csrc/fps.hip that the shapes of tests/test_gpu_fps.py are derived from
(tests/test_fps_cap_constants.py fails when one changes without these being re-derived)."""
FPS_THREADS = 1024           # kFpsThreads: threads of a workgroup, both tiers (wcn_fps_block_threads)
FPS_MAX_P = 16               # kFpsMaxP: points per thread of the largest resident instantiation
FPS_BLOCKS_PER_SEG = 64      # kFpsBlocksPerSeg: workgroups of one streamed segment (wcn_fps_blocks_per_segment)
FPS_MAX_GRID = 1024          # kFpsMaxGrid: segments of one grid (wcn_fps_max_grid)
FPS_INSTANTIATIONS = (1, 2, 4, 8, 16)  # the P the resident kernel is built for

T = FPS_THREADS
G = FPS_BLOCKS_PER_SEG
R = FPS_MAX_P * FPS_THREADS  # the resident cap (wcn_fps_resident_max_points)

# lengths of the segments of a batch
RESIDENT = (0, 1, 2, 63, 64, 65, T - 1, T, T + 1, R - 1, R)   # both sides of the wave, workgroup and cap edges
PER_INSTANTIATION = (T, T + 1, 2 * T, 2 * T + 1, 4 * T, 4 * T + 1, 8 * T, 8 * T + 1)  # each alone: its own P, both sides
SHORT = (1, 5, 7, 7)                                           # K = 7 (= N_b of the longest) and K = 10
MANY = tuple(i % 3 for i in range(FPS_MAX_GRID + 1))           # one segment more than a grid holds, empty ones in between
STREAMED = (1, 65, T + 1, G * T - 1, G * T + 1)                # the last one: a second trip of the stride
NATURAL = (R + 1,)                                             # the shortest segment that is streamed on its own
MIXED = (R + 1, 100, 0, R)                                     # both tiers in one call


def instantiation(length: int) -> int:
    """The P that a resident launch picks for its longest segment."""
    p = 1
    while p * T < length:
        p *= 2
    return p
