"""CPU: the torch definition of the packed attention mask and of masked attention against dense float64 expressions written
out here, the argument errors of ``attn_mask=``, and the C symbols of csrc/attn_varlen_masked.hip."""
import pytest
import torch

LQ, LK = (40, 33), (97, 70)
CU_Q, CU_K = torch.tensor([0, 40, 73]), torch.tensor([0, 97, 167])


def _dense_blocked(logits, release):
    """bool [Lq, Lk] per sequence straight from the rule: blocked <=> logit < 0, a fully blocked query released."""
    res = []
    for s in range(2):
        b = (logits[int(CU_K[s]):int(CU_K[s + 1]), :LQ[s]] < 0).t().clone()
        if release:
            b[b.all(1)] = False
        res.append(b)
    return res


@pytest.fixture(scope="module")
def logits():
    x = torch.randn(sum(LK), max(LQ), generator=torch.Generator().manual_seed(3))
    x[:, 5] = -1.0                      # query 5 of either sequence: every key blocked
    x[:, 6] = 0.0                       # at the threshold: not blocked
    return x


@pytest.mark.parametrize("release", [False, True])
def test_torch_pack_and_masked_attention_against_dense(logits, release):
    from warpconvnet_amd.nn.functional.attention import (flash_attn_varlen_func, masked_attention_reference, pack_attention_mask,
                                                         unpack_attention_mask)

    mask = pack_attention_mask(logits, CU_K, CU_Q, max(LQ), max(LK), release_full_rows=release, backend="torch")
    assert mask.q_words.shape == (73, 4) and mask.k_words.shape == (167, 2) and mask.q_words.dtype == torch.int32
    dense = _dense_blocked(logits, release)
    got = unpack_attention_mask(mask)
    g = torch.Generator().manual_seed(4)
    q, k, v = (torch.randn(n, 2, 16, dtype=torch.float64, generator=g) for n in (73, 167, 167))
    out, lse = masked_attention_reference(q, k, v, CU_Q, CU_K, max(LQ), max(LK), mask)
    assert torch.equal(flash_attn_varlen_func(q, k, v, CU_Q, CU_K, max(LQ), max(LK), attn_mask=mask), out)
    for s in range(2):
        rq, rk = slice(int(CU_Q[s]), int(CU_Q[s + 1])), slice(int(CU_K[s]), int(CU_K[s + 1]))
        assert torch.equal(got[rq, :LK[s]], dense[s]) and not bool(got[rq, LK[s]:].any())
        sc = torch.einsum("qhd,khd->hqk", q[rq], k[rk]) * 0.25
        sc = sc.masked_fill(dense[s][None], float("-inf"))
        want_lse = torch.logsumexp(sc, -1)                                              # -inf for the blocked query
        p = torch.nan_to_num(torch.exp(sc - want_lse[..., None]), nan=0.0)
        assert torch.allclose(out[rq], torch.einsum("hqk,khd->qhd", p, v[rk]), rtol=0, atol=1e-12)
        assert torch.allclose(lse[rq], want_lse.t(), rtol=0, atol=1e-12)
        assert bool((lse[int(CU_Q[s]) + 5] == float("-inf")).all()) != release


def test_attn_mask_argument_errors(logits):
    from warpconvnet_amd.nn.functional.attention import flash_attn_varlen_func, flash_attn_varlen_kvpacked_func, pack_attention_mask

    mask = pack_attention_mask(logits, CU_K, CU_Q, max(LQ), max(LK), backend="torch")
    q, k = torch.zeros(73, 2, 16, dtype=torch.bfloat16), torch.zeros(167, 2, 16, dtype=torch.bfloat16)
    args = (CU_Q, CU_K, max(LQ), max(LK))
    with pytest.raises(NotImplementedError, match="variant"):
        flash_attn_varlen_func(q, k, k, *args, variant="shared", attn_mask=mask)
    with pytest.raises(NotImplementedError, match="128"):
        flash_attn_varlen_func(torch.zeros(73, 2, 128), torch.zeros(167, 2, 128), torch.zeros(167, 2, 128), *args, attn_mask=mask)
    with pytest.raises(ValueError, match="built for"):
        flash_attn_varlen_func(q, k[:166], k[:166], CU_Q, torch.tensor([0, 97, 166]), max(LQ), max(LK), attn_mask=mask)
    with pytest.raises(ValueError, match="built for"):
        flash_attn_varlen_kvpacked_func(q, torch.stack([k, k], 1), CU_Q, CU_K, max(LQ), 128, attn_mask=mask)
    with pytest.raises(TypeError, match="PackedAttentionMask"):
        flash_attn_varlen_func(q, k, k, *args, attn_mask=torch.zeros(73, 167, dtype=torch.bool))


def test_masked_symbols_are_exported(hip_lib):
    from warpconvnet_amd import _lib

    for name in ("wcn_attn_mask_words", "wcn_attn_mask_pack", "wcn_attn_varlen_kv_fwd_m", "wcn_attn_varlen_kv_bwd_m"):
        assert name in _lib.SIGNATURES and getattr(hip_lib, name) is not None
    assert [hip_lib.wcn_attn_mask_words(n) for n in (0, 1, 32, 33, 100000)] == [0, 1, 1, 2, 3125]
    assert hip_lib.wcn_attn_mask_pack(None, 7, 0, 0, 0, 0.0, None, None, None, 0, 0, 0, 0, 0, 1, None, 0, None, 0, None) == -4
