"""GPU: wcn_attn_mask_pack (csrc/attn_varlen_masked.hip) against the torch definition of pack_attention_mask, word for word.

Lq = (40, 33), Lk = (97, 70): two query tiles and four key tiles with ragged tails.  Every source plants, per sequence, one
query whose keys are all blocked (cleared by the release, kept without it) and logits exactly at the threshold (not blocked).
With key_index the mask is over a permuted subset of the key rows."""
import pytest
import torch

pytestmark = pytest.mark.gpu

LQ, LK = (40, 33), (97, 70)
THRESHOLD = 0.25


def _cu(lens):
    return torch.tensor([0, lens[0], lens[0] + lens[1]])


def _source(kind, rows):
    """[rows, 40] logits (fp32 / bf16) or a bool tensor; column 7 blocked for every row, column 9 exactly at the threshold."""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(rows, max(LQ), generator=g) + THRESHOLD
    x[:, 7] = THRESHOLD - 1.0
    x[:, 9] = THRESHOLD
    if kind == "bool":
        return x < THRESHOLD
    return x.to(torch.bfloat16 if kind == "bf16" else torch.float32)


@pytest.mark.parametrize("release", [False, True])
@pytest.mark.parametrize("subset", [False, True])
@pytest.mark.parametrize("kind", ["fp32", "bf16", "bool"])
def test_pack_matches_torch_definition(hip_lib, kind, subset, release):
    from warpconvnet_amd.nn.functional.attention import _from_words, pack_attention_mask

    dev = torch.device("cuda:0")
    cu_q, cu_k = _cu(LQ), _cu(LK)
    key_index = None
    src = _source(kind, 400 if subset else sum(LK))
    if subset:  # 167 of 400 rows, permuted
        key_index = torch.randperm(400, generator=torch.Generator().manual_seed(6))[:sum(LK)].to(torch.int32)
    args = dict(threshold=THRESHOLD, release_full_rows=release)
    want = pack_attention_mask(src, cu_k, cu_q, max(LQ), max(LK), key_index=key_index, backend="torch", **args)
    got = pack_attention_mask(src.to(dev), cu_k.to(dev), cu_q.to(dev), max(LQ), max(LK), backend="hip", total_q=sum(LQ),
                              key_index=None if key_index is None else key_index.to(dev), **args)
    assert got.q_words.shape == (sum(LQ), 4) and got.k_words.shape == (sum(LK), 2)
    assert torch.equal(got.q_words.cpu(), want.q_words) and torch.equal(got.k_words.cpu(), want.k_words)
    qb, kb = _from_words(got.q_words.cpu()), _from_words(got.k_words.cpu())
    for s in range(2):  # tail bits, the planted query, the threshold column
        rq, rk = slice(int(cu_q[s]), int(cu_q[s + 1])), slice(int(cu_k[s]), int(cu_k[s + 1]))
        assert not bool(qb[rq, LK[s]:].any()) and not bool(kb[rk, LQ[s]:].any())
        assert bool(qb[int(cu_q[s]) + 7, :LK[s]].all()) != release and bool(kb[rk, 7].all()) != release
        assert not bool(qb[int(cu_q[s]) + 9].any()) and not bool(kb[rk, 9].any())
