"""The constants of csrc/attn_varlen.hip that the shapes of tests/test_gpu_attention_shared.py are derived from
(tests/test_attention_shared_cap_constants.py fails when one changes without these being re-derived)."""
ATTN_MAX_GRID = 1 << 22      # kAttnMaxGrid: workgroups of one grid, every attention kernel
ATTN_BLOCK = 32              # kAttnBlock: rows of one wave (the MFMA edge)
ATTN_WAVES = 4               # kAttnWaves: waves of a shared-tile workgroup
ATTN_WG_ROWS = ATTN_WAVES * ATTN_BLOCK  # kAttnWgRows: rows of a shared-tile work item
SHARED_MIN_SWEEP = 512       # kAttnSharedMinSweep: the AUTO rule's swept-side length
