"""CPU: the head-size-128 attention entry points (csrc/attn_varlen_d128.hip) - exports, the predicate, the argument checks
on host pointers (nothing launches) and the functional's refusal of the shared-tile variant."""
import ctypes
import os

import pytest
import torch

NAMES = ("wcn_attn_d128_supported", "wcn_attn_d128_fwd", "wcn_attn_d128_bwd")
INVALID, UNSUPPORTED = -5, -4


def test_exported_and_declared(hip_lib):
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "wcn.h")).read()
    for name in NAMES:
        assert getattr(hip_lib, name) is not None and f" {name}(" in header, name


def test_predicates(hip_lib):
    from warpconvnet_amd import _lib

    for dt in (_lib.WCN_F16, _lib.WCN_BF16):
        assert hip_lib.wcn_attn_d128_supported(128, dt) == 1
        assert all(hip_lib.wcn_attn_d128_supported(d, dt) == 0 for d in (64, 96, 256))
        assert hip_lib.wcn_attn_varlen_supported(128, dt) == 0      # the narrower kernels' predicate is what it was
    assert hip_lib.wcn_attn_d128_supported(128, _lib.WCN_F32) == 0


def test_argument_checks(hip_lib):
    from warpconvnet_amd import _lib

    buf = (ctypes.c_char * 8192)()
    p = (ctypes.addressof(buf) + 15) & ~15  # host memory: every call is refused, or is a no-op, before any launch
    base = dict(dout=p, q=p, qs=256, k=p, v=p, kvs=256, out=p, lse=p, cq=p, ck=p, s=2, tq=10, tk=10, h=2, d=128, mq=8, mk=8,
                scale=0.1, dt=_lib.WCN_BF16, dq=p, dqs=256, dk=p, dv=p, dkvs=256, qsp=1, ksp=1, ws=p, wsb=8192)

    def fwd(**kw):
        a = dict(base, ws=None, wsb=0)
        a.update(kw)
        return hip_lib.wcn_attn_d128_fwd(a["q"], a["qs"], a["k"], a["v"], a["kvs"], a["cq"], a["ck"], a["s"], a["tq"], a["tk"],
                                         a["h"], a["d"], a["mq"], a["mk"], a["scale"], a["dt"], a["out"], a["lse"], a["ksp"],
                                         a["ws"], a["wsb"], None)

    def bwd(**kw):
        a = dict(base, **kw)
        return hip_lib.wcn_attn_d128_bwd(a["dout"], a["q"], a["qs"], a["k"], a["v"], a["kvs"], a["out"], a["lse"], a["cq"],
                                         a["ck"], a["s"], a["tq"], a["tk"], a["h"], a["d"], a["mq"], a["mk"], a["scale"], a["dt"],
                                         a["dq"], a["dqs"], a["dk"], a["dv"], a["dkvs"], a["qsp"], a["ksp"], a["ws"], a["wsb"], None)

    for call in (fwd, bwd):
        for d in (16, 64, 96, 256):
            assert call(d=d, qs=2 * d, kvs=2 * d, dqs=2 * d, dkvs=2 * d) == UNSUPPORTED, (call.__name__, d)
        assert call(dt=_lib.WCN_F32) == UNSUPPORTED
        for bad in (dict(q=None), dict(k=None), dict(v=None), dict(cq=None), dict(ck=None), dict(out=None), dict(lse=None),
                    dict(s=-1), dict(tq=-1), dict(tk=-1), dict(h=0), dict(mq=-1), dict(mk=-1), dict(scale=float("nan")),
                    dict(ksp=-1), dict(qs=255), dict(kvs=248), dict(q=p + 2)):
            assert call(**bad) == INVALID, (call.__name__, bad)
    assert fwd(ksp=2) == INVALID                                          # a split forward needs a workspace
    assert fwd(ksp=2, ws=p, wsb=2 * 10 * 2 * 130 * 4 - 1) == INVALID
    for bad in (dict(dout=None), dict(dq=None), dict(dk=None), dict(dv=None), dict(ws=None), dict(qsp=-1), dict(dqs=255),
                dict(wsb=10 * 2 * 4 - 1), dict(qsp=2, wsb=2 * 10 * 2 * 2 * 128 * 4 + 10 * 2 * 4 - 1)):
        assert bwd(**bad) == INVALID, bad
    # nothing to compute: valid, no launch
    empty = dict(s=0, tq=0, tk=0, q=None, k=None, v=None, cq=None, ck=None, out=None, lse=None)
    assert fwd(**empty) == 0
    assert bwd(dout=None, dq=None, dk=None, dv=None, ws=None, wsb=0, **empty) == 0


def test_shared_variant_is_refused(hip_lib):
    from warpconvnet_amd.nn.functional.attention import flash_attn_varlen_func, flash_attn_varlen_qkvpacked

    cu = torch.tensor([0, 4, 10], dtype=torch.int32)
    x = torch.randn(10, 3, 2, 128).bfloat16()
    with pytest.raises(NotImplementedError, match="head_dim 128"):
        flash_attn_varlen_qkvpacked(x, cu, 8, variant="shared")
    with pytest.raises(NotImplementedError, match="head_dim 128"):
        flash_attn_varlen_func(x[:, 0], x[:, 1], x[:, 2], cu, cu, 8, 8, variant="shared")
