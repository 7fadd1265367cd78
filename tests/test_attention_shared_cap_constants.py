"""The constants that the shapes of tests/test_gpu_attention_shared.py are derived from (tests/attention_shared_cap_constants.py),
read from the source and from the library: a cap raised or a workgroup resized later would silently turn the case past the cap
into a plain one, and a changed AUTO rule must be a decision, not an accident."""
import os
import re

import pytest

from tests import attention_shared_cap_constants as caps

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "warpconvnet_amd", "csrc")
WHY = "tests/attention_shared_cap_constants.py feeds tests/test_gpu_attention_shared.py: re-derive its shapes with the new value"

CONSTANTS = [
    ("kAttnMaxGrid", r"constexpr\s+int64_t\s+kAttnMaxGrid\s*=\s*1\s*<<\s*([0-9]+)\s*;", caps.ATTN_MAX_GRID.bit_length() - 1),
    ("kAttnBlock", r"constexpr\s+int\s+kAttnBlock\s*=\s*([0-9]+)\s*;", caps.ATTN_BLOCK),
    ("kAttnWaves", r"constexpr\s+int\s+kAttnWaves\s*=\s*([0-9]+)\s*;", caps.ATTN_WAVES),
    ("kAttnSharedMinSweep", r"constexpr\s+int\s+kAttnSharedMinSweep\s*=\s*([0-9]+)\s*;", caps.SHARED_MIN_SWEEP),
]


@pytest.mark.parametrize("name,pattern,want", CONSTANTS, ids=[c[0] for c in CONSTANTS])
def test_constant_is_what_the_tests_assume(name, pattern, want):
    with open(os.path.join(CSRC, "attn_varlen.hip")) as f:
        text = f.read()
    found = re.findall(pattern, text)
    assert len(found) == 1, f"{name}: {len(found)} definitions found. {WHY}"
    assert int(found[0]) == want, f"attn_varlen.hip: {name} = {found[0]}, the tests assume {want}. {WHY}"
    assert "kAttnWgRows = kAttnWaves * kAttnBlock" in text, WHY


def test_the_auto_rule_is_the_stated_function(hip_lib):
    """SHARED exactly when the longest swept side has at least SHARED_MIN_SWEEP rows: the keys in the forward, the longer of
    the two sides in the backward (dQ sweeps the keys, dK/dV the queries)."""
    from warpconvnet_amd import _lib

    one, shared = _lib.WCN_ATTN_ONE_WAVE, _lib.WCN_ATTN_SHARED
    f = hip_lib.wcn_attn_varlen_variant
    n = caps.SHARED_MIN_SWEEP
    for direction in (0, 1):
        assert f(1, n, n, 1, direction) == shared and f(1, n - 1, n - 1, 1, direction) == one
        assert f(2, 8192, 8192, 12, direction) == shared
        assert f(4096, 128, 128, 8, direction) == one      # the patches and windows the one-wave kernels were built for
        assert f(0, 8192, 8192, 12, direction) == one and f(3, 0, 8192, 12, direction) == one  # nothing to launch
    # cross-attention, many queries over a short context: the forward sweeps the short side, the backward's dK/dV the long one
    assert f(1, 65536, n - 1, 12, 0) == one and f(1, 65536, n - 1, 12, 1) == shared
    assert f(1, 100, n, 12, 0) == shared
