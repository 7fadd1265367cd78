"""CPU: the split-key sweep of the attention forward and of dQ, tested without a GPU.  (1) The split rule
(``wcn_attn_varlen_k_splits``) and its workspace function are host-only: the library loads and answers here.  (2) A torch
model of the split-key kernels' roundings (tests/attention_split_bounds.py) stays under the bound the GPU test applies, on
the GPU test's own shapes: the combine's extra terms are proven here before a kernel is held to them."""
import pytest
import torch

from tests import attention_bounds as ab
from tests import attention_split_bounds as sb


def _lib():
    from warpconvnet_amd import _lib

    return _lib.lib()


# ---- 1. the rule ------------------------------------------------------------------------------------------------------------
def test_rule_is_one_for_degenerate_arguments():
    L = _lib()
    for direction in (0, 1):
        for args in ((0, 100, 100000, 8), (-1, 100, 100000, 8), (2, 0, 100000, 8), (2, 100, 0, 8), (2, 100, 100000, 0),
                     (2, -5, 100000, 8), (2, 100, -7, 8)):
            assert L.wcn_attn_varlen_k_splits(*args, direction) == 1, args


def _calls_of_the_existing_tests():
    """(num_seqs, max_q, max_k) of PACKED_LENS, SEPARATE_LENS and EDGE taken as single calls, and of each of their
    sequences alone."""
    calls = [(len(ab.PACKED_LENS), max(ab.PACKED_LENS), max(ab.PACKED_LENS))]
    calls += [(1, n, n) for n in ab.PACKED_LENS]
    for lens in (ab.SEPARATE_LENS, ab.EDGE):
        calls.append((len(lens), max(a for a, _ in lens), max(b for _, b in lens)))
        calls += [(1, a, b) for a, b in lens]
    return calls


def test_rule_leaves_the_existing_test_shapes_unsplit():
    L = _lib()
    for n, mq, mk in _calls_of_the_existing_tests():
        for heads in (1, 2, 3, 8):
            for direction in (0, 1):
                assert L.wcn_attn_varlen_k_splits(n, mq, mk, heads, direction) == 1, (n, mq, mk, heads)


def test_rule_is_monotone_and_capped():
    L = _lib()
    seen = set()
    for direction in (0, 1):
        for heads in (1, 8):
            for mk in (31, 1025, 2000, 20000, 100000, 3000000):
                cap = (mk + 31) // 32
                prev_n = None
                for n in (1, 2, 3, 8, 64, 1000, 100000):
                    prev_q = None
                    row = []
                    for mq in (1, 5, 100, 128, 129, 300, 513, 4096, 100000):
                        s = L.wcn_attn_varlen_k_splits(n, mq, mk, heads, direction)
                        assert 1 <= s <= cap, (n, mq, mk, heads, s)
                        assert prev_q is None or s <= prev_q, ("max_q", n, mq, mk, heads, s, prev_q)
                        prev_q = s
                        row.append(s)
                        seen.add(s)
                    if prev_n is not None:
                        assert all(x <= y for x, y in zip(row, prev_n)), ("num_seqs", n, mk, heads, row, prev_n)
                    prev_n = row
    assert max(seen) > 1, "the rule never splits"
    # the decoder's shape: 2 scenes, 100 queries, 8 heads, 100 000 points
    assert L.wcn_attn_varlen_k_splits(2, 100, 100000, 8, 0) > 1


def test_workspace_function():
    L = _lib()
    tq, tk, h, d = 205, 100000, 8, 32
    delta = 4 * tq * h
    assert L.wcn_attn_varlen_ksplit_workspace_bytes(tq, tk, h, d, 1, 1, 0) == 0
    assert L.wcn_attn_varlen_ksplit_workspace_bytes(tq, tk, h, d, 1, 1, 1) == delta == L.wcn_attn_varlen_kv_workspace_bytes(tq, tk, h, d, 1)
    for s in (2, 7, 64):
        assert L.wcn_attn_varlen_ksplit_workspace_bytes(tq, tk, h, d, 1, s, 0) == 4 * s * tq * h * (d + 2)
        assert L.wcn_attn_varlen_ksplit_workspace_bytes(tq, tk, h, d, 1, s, 1) == delta + 4 * s * tq * h * d
        assert (L.wcn_attn_varlen_ksplit_workspace_bytes(tq, tk, h, d, 3, s, 1)
                == L.wcn_attn_varlen_kv_workspace_bytes(tq, tk, h, d, 3) + 4 * s * tq * h * d)
    # what the rule asks for stays under its byte cap (256 MiB of partials at head_dim 64)
    for n, mq, mk, heads in ((2, 100, 100000, 8), (8, 300, 100000, 8), (1, 100000, 100000, 8), (64, 4096, 1 << 20, 16)):
        s = L.wcn_attn_varlen_k_splits(n, mq, mk, heads, 0)
        assert L.wcn_attn_varlen_ksplit_workspace_bytes(n * mq, n * mk, heads, 64, 1, s, 0) <= 256 << 20, (n, mq, mk, heads, s)
    assert L.wcn_attn_varlen_ksplit_workspace_bytes(-1, 5, 1, 16, 1, 2, 0) == 0
    assert L.wcn_abi_version() == 18


# ---- 2. the CPU model of the split sweep under the GPU test's bound ---------------------------------------------------------
def test_key_share_matches_the_definition():
    for lk in (0, 1, 31, 32, 33, 97, 257, 1025, 2100):
        for s in sb.K_SPLITS:
            nb = (lk + 31) // 32
            per = (nb + s - 1) // s if nb else 0
            shares = [sb.key_share(lk, s, j) for j in range(s)]
            assert shares[0][0] == 0 and shares[-1][1] == lk
            for j, (lo, hi) in enumerate(shares):
                assert lo == min(j * per * 32, lk) and hi == min((j + 1) * per * 32, lk)
                assert j == 0 or lo == shares[j - 1][1]
    # 97 keys in 3 splits: 4 blocks, 2 per split, the third share is empty
    assert [sb.key_share(97, 3, j) for j in range(3)] == [(0, 64), (64, 97), (97, 97)]


@pytest.mark.parametrize("dt,d,h", [("bf16", 16, 3), ("fp16", 16, 1), ("bf16", 32, 1), ("fp16", 32, 3), ("bf16", 64, 3),
                                    ("fp16", 64, 3)])
@pytest.mark.parametrize("kind", sb.KINDS, ids=lambda k: f"{k[0]}-{k[1]}")
def test_split_model_within_bound(kind, dt, d, h):
    args = sb.case_inputs(kind, dt, d, h)
    for s in sb.K_SPLITS:
        ref, bound = sb.reference_and_split_bounds(*args, s)
        got = sb.split_rounding_model(*args, s)
        r = ab.ratios(got, ref, bound)
        print(kind, dt, d, h, s, {n: round(x, 3) for n, x in r.items()})
        for n, x in r.items():
            assert x <= 1.0, (kind, dt, d, h, s, n, x)
        # the empty sides: sequence 1 has 5 queries and no key, sequence 2 five keys and no query
        assert not bool(got["out"][1:6].any()) and bool((got["lse"][1:6] == float("-inf")).all())


def test_split_bound_adds_nothing_at_one_split():
    args = sb.case_inputs(("random", 8), "bf16", 32, 3)
    _, b0 = ab.reference_and_bounds(*args)
    _, b1 = sb.reference_and_split_bounds(*args, 1)
    _, b5 = sb.reference_and_split_bounds(*args, 5)
    for n in ab.NAMES:
        assert torch.equal(b0[n], b1[n])
        assert bool((b5[n] >= b0[n]).all())
    assert bool((b5["out"] > b0["out"]).any()) and torch.equal(b5["dv"], b0["dv"])



# ---- 3. argument checks of the new entry points: refused before anything is launched, so they answer without a GPU ----------
def test_entry_points_refuse_bad_split_arguments():
    from warpconvnet_amd import _lib as lib

    L = lib.lib()
    INVALID = -5                      # WCN_ERROR_INVALID_PARAMETERS
    p = 0x10000                       # a 16-byte aligned address that is never dereferenced: every call below is refused
    tq, tk, h, d = 100, 5000, 2, 32
    fwd = (p, h * d, p, p, h * d, p, p, 1, tq, tk, h, d, tq, tk, 0.25, lib.WCN_BF16, p, p)
    need = L.wcn_attn_varlen_ksplit_workspace_bytes(tq, tk, h, d, 1, 4, 0)
    assert need == 4 * 4 * tq * h * (d + 2)
    assert L.wcn_attn_varlen_kv_fwd_s(*fwd, 0, -1, p, need, None) == INVALID          # k_splits < 0
    assert L.wcn_attn_varlen_kv_fwd_s(*fwd, 0, 4, p, need - 1, None) == INVALID       # one byte short
    assert L.wcn_attn_varlen_kv_fwd_s(*fwd, 0, 4, None, need, None) == INVALID        # null
    assert L.wcn_attn_varlen_kv_fwd_s(*fwd, 0, 4, p + 8, need, None) == INVALID       # misaligned
    assert L.wcn_attn_varlen_kv_fwd_s(*fwd, 3, 4, p, need, None) == INVALID           # an unknown variant
    bwd = (p, p, h * d, p, p, h * d, p, p, p, p, 1, tq, tk, h, d, tq, tk, 0.25, lib.WCN_BF16, p, h * d, p, p, h * d)
    need = L.wcn_attn_varlen_ksplit_workspace_bytes(tq, tk, h, d, 1, 4, 1)
    assert L.wcn_attn_varlen_kv_bwd_s(*bwd, 1, -1, p, need, 0, None) == INVALID
    assert L.wcn_attn_varlen_kv_bwd_s(*bwd, 1, 4, p, need - 1, 0, None) == INVALID
    assert L.wcn_attn_varlen_kv_bwd_s(*bwd, 1, 4, None, need, 0, None) == INVALID
    assert L.wcn_attn_varlen_kv_bwd_s(*bwd, 1, 4, p + 8, need, 0, None) == INVALID
    # the size k_splits = 1 needs (delta alone) is too small for four splits
    assert L.wcn_attn_varlen_kv_bwd_s(*bwd, 1, 4, p, L.wcn_attn_varlen_kv_workspace_bytes(tq, tk, h, d, 1), 0, None) == INVALID


def test_functional_refuses_a_bad_k_splits():
    from warpconvnet_amd.nn.functional.attention import flash_attn_varlen_func, flash_attn_varlen_kvpacked_func

    q, k = torch.zeros(4, 1, 16, dtype=torch.bfloat16), torch.zeros(8, 1, 16, dtype=torch.bfloat16)
    cu_q, cu_k = torch.tensor([0, 4]), torch.tensor([0, 8])
    for bad in (-1, 2.0, True):
        with pytest.raises(ValueError):
            flash_attn_varlen_func(q, k, k, cu_q, cu_k, 4, 8, k_splits=bad)
        with pytest.raises(ValueError):
            flash_attn_varlen_kvpacked_func(q, torch.stack([k, k], 1), cu_q, cu_k, 4, 8, k_splits=bad)
    with pytest.raises(RuntimeError):     # a valid count, CPU tensors: the existing "no CPU fallback" error
        flash_attn_varlen_func(q, k, k, cu_q, cu_k, 4, 8, k_splits=2)
