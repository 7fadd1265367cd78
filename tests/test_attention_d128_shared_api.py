"""CPU: the variant-taking head-size-128 attention entry points (csrc/attn_varlen_d128.hip) - exports, the argument checks on
host pointers (nothing launches) and the AUTO rule as a pure function."""
import ctypes
import os

import pytest

NAMES = ("wcn_attn_d128_variant", "wcn_attn_d128_fwd_v", "wcn_attn_d128_bwd_v")
INVALID, UNSUPPORTED = -5, -4


def test_exported_and_declared(hip_lib):
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "wcn.h")).read()
    for name in NAMES:
        assert getattr(hip_lib, name) is not None and f" {name}(" in header, name
    assert hip_lib.wcn_abi_version() == 18


@pytest.mark.parametrize("direction", ["fwd", "bwd"])
def test_argument_checks(hip_lib, direction):
    from warpconvnet_amd import _lib

    buf = (ctypes.c_char * 8192)()
    p = (ctypes.addressof(buf) + 15) & ~15  # host memory: every call is refused, or is a no-op, before any launch
    base = dict(dout=p, q=p, qs=256, k=p, v=p, kvs=256, out=p, lse=p, cq=p, ck=p, s=2, tq=10, tk=10, h=2, d=128, mq=8, mk=8,
                dt=_lib.WCN_BF16, dq=p, dqs=256, dk=p, dv=p, dkvs=256, ws=p, wsb=8192, var=_lib.WCN_ATTN_SHARED)

    def call(**kw):
        a = dict(base, **kw)
        if direction == "fwd":
            return hip_lib.wcn_attn_d128_fwd_v(a["q"], a["qs"], a["k"], a["v"], a["kvs"], a["cq"], a["ck"], a["s"], a["tq"], a["tk"],
                                               a["h"], a["d"], a["mq"], a["mk"], 0.1, a["dt"], a["out"], a["lse"], 1, a["ws"],
                                               a["wsb"], a["var"], None)
        return hip_lib.wcn_attn_d128_bwd_v(a["dout"], a["q"], a["qs"], a["k"], a["v"], a["kvs"], a["out"], a["lse"], a["cq"], a["ck"],
                                           a["s"], a["tq"], a["tk"], a["h"], a["d"], a["mq"], a["mk"], 0.1, a["dt"], a["dq"], a["dqs"],
                                           a["dk"], a["dv"], a["dkvs"], 1, 1, a["ws"], a["wsb"], a["var"], None)

    for var in (-1, 3, 7):
        assert call(var=var) == INVALID, var
    empty = dict(s=0, tq=0, tk=0, q=None, k=None, v=None, cq=None, ck=None, out=None, lse=None, dout=None, dq=None, dk=None,
                 dv=None, ws=None, wsb=0)
    for var in (_lib.WCN_ATTN_AUTO, _lib.WCN_ATTN_ONE_WAVE, _lib.WCN_ATTN_SHARED):
        for d in (64, 96, 256):
            assert call(var=var, d=d, qs=2 * d, kvs=2 * d, dqs=2 * d, dkvs=2 * d) == UNSUPPORTED, (var, d)
        assert call(var=var, dt=_lib.WCN_F32) == UNSUPPORTED
        assert call(var=var, q=None) == INVALID and call(var=var, qs=255) == INVALID  # the existing checks, before any launch
        assert call(var=var, **empty) == 0


def test_auto_rule_is_a_pure_function(hip_lib):
    from warpconvnet_amd import _lib

    f = hip_lib.wcn_attn_d128_variant
    for direction in (0, 1):
        for seqs, mq, mk, h in ((0, 8192, 8192, 12), (2, 0, 64, 12), (2, 64, 0, 12), (2, 64, 64, 0)):
            assert f(seqs, mq, mk, h, direction) == _lib.WCN_ATTN_ONE_WAVE
        for n in (1, 128, 512, 2048, 16384, 1 << 20):
            got = [f(2, n, n, 12, direction) for _ in range(2)]
            assert got[0] == got[1] and got[0] in (_lib.WCN_ATTN_ONE_WAVE, _lib.WCN_ATTN_SHARED)
        assert f(4096, 128, 128, 12, direction) == _lib.WCN_ATTN_ONE_WAVE  # patches and windows stay on the pair kernels
