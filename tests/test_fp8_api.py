"""CPU: the FP8 helpers, the ``hip_mfma_fp8`` algorithm name, its host-only probes and its refusals (no device work)."""
import inspect

import pytest
import torch


def test_fp8_utils_names_and_cpu_semantics():
    from warpconvnet_amd.nn.functional import fp8_utils as fu

    assert list(inspect.signature(fu.quantize_to_fp8).parameters) == ["tensor", "fp8_format"]
    assert inspect.signature(fu.quantize_to_fp8).parameters["fp8_format"].default == "e4m3"
    assert list(inspect.signature(fu.dequantize_from_fp8).parameters) == ["tensor", "scale_factor", "output_dtype"]
    assert inspect.signature(fu.dequantize_from_fp8).parameters["output_dtype"].default == torch.float16
    assert fu.is_fp8_dtype(torch.float8_e4m3fn) and fu.is_fp8_dtype(torch.float8_e5m2) and not fu.is_fp8_dtype(torch.float16)
    assert fu.get_fp8_format(torch.float8_e4m3fn) == "e4m3" and fu.get_fp8_format(torch.float8_e5m2) == "e5m2"
    with pytest.raises(ValueError):
        fu.get_fp8_format(torch.float16)
    with pytest.raises(ValueError):
        fu.quantize_to_fp8(torch.ones(2), "e3m4")

    x = torch.randn(257, 40, generator=torch.Generator().manual_seed(0)) * 3.0
    for dtype in (torch.float32, torch.float16, torch.bfloat16):
        t = x.to(dtype)
        q, s = fu.quantize_to_fp8(t)
        assert q.dtype == torch.float8_e4m3fn and q.shape == t.shape and s.dtype == torch.float32 and s.ndim == 0
        assert torch.equal(s, t.float().abs().max() / 448.0)
        back = fu.dequantize_from_fp8(q, s, torch.float32)
        # half an ulp of E4M3 (3 mantissa bits: 2^-4 relative), half the subnormal spacing 2^-9 below 2^-6; in units of s, and
        # 2^-22 relative for the two fp32 roundings (the division, the multiplication back)
        v = t.float().abs() / s
        half_ulp = torch.maximum(torch.exp2(torch.floor(torch.log2(v.clamp_min(2.0 ** -6))) - 4), torch.tensor(2.0 ** -10))
        assert bool(((back - t.float()).abs() <= s * (half_ulp + v * 2.0 ** -22)).all())
    q, s = fu.quantize_to_fp8(torch.zeros(5, 3))
    assert float(s) == 1.0 and not q.float().any()
    q, s = fu.quantize_to_fp8(x, "e5m2")
    assert q.dtype == torch.float8_e5m2 and torch.equal(s, x.abs().max() / 57344.0)


def test_name_is_a_forward_algorithm_only():
    from warpconvnet_amd.constants import VALID_ALGOS, _env_choice
    from warpconvnet_amd.nn.functional.sparse_conv.detail.backends import BACKWARD_BACKENDS, FORWARD_BACKENDS
    from warpconvnet_amd.nn.functional.sparse_conv.detail.unified import SPARSE_CONV_AB_ALGO_MODE

    assert "hip_mfma_fp8" in VALID_ALGOS and "hip_mfma_fp8" in FORWARD_BACKENDS and "hip_mfma_fp8" not in BACKWARD_BACKENDS
    assert SPARSE_CONV_AB_ALGO_MODE("hip_mfma_fp8") is SPARSE_CONV_AB_ALGO_MODE.HIP_MFMA_FP8
    assert _env_choice("WARPCONVNET_NO_SUCH_VARIABLE", "hip_mfma_fp8", VALID_ALGOS) == "hip_mfma_fp8"


def test_probes_and_refusals(hip_lib):
    from warpconvnet_amd import _lib

    L = hip_lib
    assert L.wcn_abi_version() == 18 and _lib.WCN_ALGO_MFMA_FP8 == 4
    ok = lambda cin, cout, K: L.wcn_conv_fp8_supported(cin, cout, K)
    assert ok(64, 128, 27) == 1 and ok(64, 32, 1) == 1 and ok(128, 160, 125) == 1 and ok(192, 96, 4096) == 1
    assert ok(32, 128, 27) == 0 and ok(96, 128, 27) == 0 and ok(64, 48, 27) == 0 and ok(64, 128, 0) == 0 and ok(64, 128, 4097) == 0
    assert L.wcn_fp8_packed_weight_bytes(27, 64, 128) == 27 * 64 * 128 and L.wcn_fp8_packed_weight_bytes(27, 60, 128) == 0
    assert L.wcn_fp8_amax_workspace() >= 8
    # refused before any launch: a shape outside the probe (-4), negative sizes and missing pointers (-5); nothing to do (0)
    gg = lambda n_out, cin, cout: L.wcn_conv_gather_gemm_fp8(None, None, None, None, None, None, None, None, None, 10, n_out, cin,
                                                             cout, 27, _lib.WCN_F16, None)
    assert gg(10, 96, 128) == -4 and gg(10, 64, 128) == -5 and gg(-1, 64, 128) == -5 and gg(0, 64, 128) == 0
    assert L.wcn_fp8_quantize_rows(None, 0, 40, _lib.WCN_F16, None, None, 64, None) == 0
    assert L.wcn_fp8_quantize_rows(None, 4, 40, _lib.WCN_F16, None, None, 64, None) == -5
    assert L.wcn_fp8_quantize_rows(None, 4, 40, _lib.WCN_F16, None, None, 24, None) == -5
    assert L.wcn_fp8_amax_scale(None, 4, _lib.WCN_F32, None, 0, None, None) == -5
    assert L.wcn_fp8_pack_weight(None, 27, 64, 128, _lib.WCN_F32, 64, 128, None, 0, None, None) == -5
    assert L.wcn_fp8_pack_weight(None, 27, 64, 128, _lib.WCN_F32, 96, 128, None, 0, None, None) == -4


def test_grad_and_cpu_tensors_raise(hip_lib):
    from warpconvnet_amd.geometry.coords.search.search_results import IntSearchResult
    from warpconvnet_amd.nn.functional.sparse_conv.detail import hip_gemm
    from warpconvnet_amd.geometry.types.voxels import Voxels
    from warpconvnet_amd.nn.modules.sparse_conv import SparseConv3d

    vox = Voxels([torch.tensor([[0, 0, 0], [0, 0, 1], [3, 1, 2]], dtype=torch.int32)], [torch.randn(3, 64)])
    with pytest.raises(RuntimeError, match="hip_mfma_fp8.*forward-only"):   # the layer's weight requires grad, grad mode is on
        SparseConv3d(64, 128, 3, fwd_algo="hip_mfma_fp8")(vox)
    z = torch.zeros(0, dtype=torch.int32)
    km = IntSearchResult(z, z, torch.zeros(28, dtype=torch.int32))
    x, w = torch.zeros(4, 64), torch.zeros(27, 64, 128)
    with pytest.raises(RuntimeError, match="hip_mfma_fp8.*GPU"):
        hip_gemm.hip_forward(x, w, km, 4, "hip_mfma_fp8")
    for xg, wg in ((x.clone().requires_grad_(True), w), (x, w.clone().requires_grad_(True))):
        with pytest.raises(RuntimeError, match="hip_mfma_fp8.*forward-only"):
            hip_gemm.hip_forward(xg, wg, km, 4, "hip_mfma_fp8")
    with pytest.raises(RuntimeError, match="hip_mfma_fp8"):
        hip_gemm._gather_plan("hip_mfma_fp8", 64, 128, 27, torch.float64, True)
    assert hip_gemm._gather_plan("hip_mfma_fp8", 13, 7, 27, torch.float16, True) == ("fp8", 4, 64, 32)
    assert hip_gemm._gather_plan("auto", 64, 128, 27, torch.float16, True)[1] == 2   # `auto` never picks FP8
