"""CPU: the ``hip_mfma_f32`` algorithm name, its host-only probes and its refusals (no device work)."""
import pytest
import torch


def test_name_is_accepted():
    from warpconvnet_amd.constants import VALID_ALGOS
    from warpconvnet_amd.nn.functional.sparse_conv.detail.backends import BACKWARD_BACKENDS, FORWARD_BACKENDS
    from warpconvnet_amd.nn.functional.sparse_conv.detail.unified import SPARSE_CONV_AB_ALGO_MODE, SPARSE_CONV_ATB_ALGO_MODE

    assert "hip_mfma_f32" in VALID_ALGOS and "hip_mfma_f32" in FORWARD_BACKENDS and "hip_mfma_f32" in BACKWARD_BACKENDS
    assert SPARSE_CONV_AB_ALGO_MODE("hip_mfma_f32") is SPARSE_CONV_AB_ALGO_MODE.HIP_MFMA_F32
    assert SPARSE_CONV_ATB_ALGO_MODE("hip_mfma_f32") is SPARSE_CONV_ATB_ALGO_MODE.HIP_MFMA_F32


def test_probes_and_refusals(hip_lib):
    from warpconvnet_amd import _lib

    L = hip_lib
    assert _lib.WCN_ALGO_MFMA_F32 == 3
    assert L.wcn_mfma_f32_gather_supported(64, 128, 27) == 1 and L.wcn_mfma_f32_gather_supported(16, 32, 125) == 1
    assert L.wcn_mfma_f32_gather_supported(7, 13, 27) == 0
    assert L.wcn_mfma_f32_wgrad_supported(64, 128) == 1 and L.wcn_mfma_f32_wgrad_supported(16, 32) == 1
    assert L.wcn_mfma_f32_wgrad_supported(7, 13) == 0
    assert L.wcn_conv_wgrad_workspace(27, 64, 128, 3) >= 27 * 64 * 128 * 4
    # refused before any launch: another dtype, a shape outside the probe (-4); missing pointers (-5)
    gg = lambda cin, cout, dtype: L.wcn_conv_gather_gemm(None, None, None, None, None, None, None, 10, 10, cin, cout, 27, dtype, 3,
                                                         0, 0, None)
    assert gg(64, 128, _lib.WCN_BF16) == -4 and gg(7, 13, _lib.WCN_F32) == -4 and gg(64, 128, _lib.WCN_F32) == -5


def test_cpu_tensors_and_other_dtypes_raise(hip_lib):
    from warpconvnet_amd.geometry.coords.search.search_results import IntSearchResult
    from warpconvnet_amd.nn.functional.sparse_conv.detail import hip_gemm

    z = torch.zeros(0, dtype=torch.int32)
    km = IntSearchResult(z, z, torch.zeros(28, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="GPU"):
        hip_gemm.hip_forward(torch.zeros(4, 64), torch.zeros(27, 64, 128), km, 4, "hip_mfma_f32")
    for plan in (lambda: hip_gemm._gather_plan("hip_mfma_f32", 64, 128, 27, torch.bfloat16, True),
                 lambda: hip_gemm._wgrad_plan("hip_mfma_f32", 64, 128, torch.float16, True)):
        with pytest.raises(RuntimeError, match="hip_mfma_f32"):
            plan()
