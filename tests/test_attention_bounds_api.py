"""CPU: the measure of tests/attention_bounds.py is tested before it tests a kernel.  (1) The fp32 model of the kernels'
roundings stays within the bound (ratio <= 1.0) on every case tests/test_gpu_attention_bounds.py runs, so the inputs are
fair: plain arithmetic with those roundings needs no more room than the bound gives.  (2) Four planted errors push a ratio
above 10 on layouts where the suite's older measure, rel_max_err < 2e-2 over a whole tensor, lets them pass.  (3) The
underflow floor and the empty-side conventions."""
import math

import pytest
import torch

from tests import attention_bounds as ab
from tests.util import rel_max_err

OLD_TOL = 2e-2     # TOL of tests/test_gpu_attention.py and tests/test_gpu_cross_attention.py


def _model_ratios(args, fault=None):
    q, k, v, dout, cu_q, cu_k, scale, dtype = args
    ref, bound = ab.reference_and_bounds(q, k, v, dout, cu_q, cu_k, scale, dtype)
    got = ab.rounding_model(q, k, v, dout, cu_q, cu_k, scale, dtype, fault=fault)
    return ab.ratios(got, ref, bound), got, ref, bound


def _assert_within(args, tag):
    r, got, ref, _ = _model_ratios(args)
    print(tag, {n: round(x, 3) for n, x in r.items()})
    for n, x in r.items():
        assert x <= 1.0, (tag, n, x)
        assert got[n].shape == ref[n].shape


# ---- 1. the model stays within the bound ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ab.grid_cases(), ids=lambda c: "-".join(map(str, c)))
def test_model_within_bound_grid(case):
    _assert_within(ab.grid_inputs(*case), case)


@pytest.mark.parametrize("case", ab.hard_cases(), ids=lambda c: "-".join(map(str, c)))
def test_model_within_bound_hard_logits(case):
    _assert_within(ab.hard_case_inputs(*case), case)


@pytest.mark.parametrize("case", ab.scale_cases(), ids=lambda c: "-".join(map(str, c)))
def test_model_within_bound_scales(case):
    args = ab.scale_inputs(*case)
    _assert_within(args, case)
    if case[2] == 0.0:   # uniform attention: lse = log(Lk), and no gradient reaches q or k
        ref, _ = ab.reference_and_bounds(*args)
        cq, ck = args[4].tolist(), args[5].tolist()
        for s in range(len(cq) - 1):
            if ck[s + 1] > ck[s]:
                assert bool(((ref["lse"][cq[s]:cq[s + 1]] - math.log(ck[s + 1] - ck[s])).abs() < 1e-12).all())
        assert not ref["dq"].any() and not ref["dk"].any()


@pytest.mark.parametrize("case", ab.split_cases(), ids=lambda c: "-".join(map(str, c)))
def test_model_within_bound_split_layout(case):
    _assert_within(ab.split_inputs(*case), case)


# ---- 2. planted errors ---------------------------------------------------------------------------------------------------
def _mixed(lens, q_gain, dout_gain, h, d, dtype, same_heads=(), seed=0):
    """randn inputs with a gain on q and on dout per sequence; the sequences of ``same_heads`` carry head 0's data in
    every head."""
    cu_q, cu_k = ab.boundaries(lens)
    q, k, v, dout = ab.random_inputs(cu_q, cu_k, h, d, torch.float32, 1.0, seed)
    for s in range(len(lens)):
        q[int(cu_q[s]):int(cu_q[s + 1])] *= q_gain[s]
        dout[int(cu_q[s]):int(cu_q[s + 1])] *= dout_gain[s]
    for s in same_heads:
        for t, cu in ((q, cu_q), (dout, cu_q), (k, cu_k), (v, cu_k)):
            t[int(cu[s]):int(cu[s + 1])] = t[int(cu[s]):int(cu[s + 1]), :1]
    return q.to(dtype), k.to(dtype), v.to(dtype), dout.to(dtype), cu_q, cu_k, d ** -0.5, dtype


def _planted(fault):
    """Inputs on which the old measure misses ``fault``, and the quantities it is taken over.  Every layout has 'anchor'
    sequences the fault leaves alone (they set max|ref|, as the 1-row sequences of the older tests' layouts do) and a long
    'victim' sequence at a non-zero offset whose values are small, because it averages many keys."""
    f16 = torch.float16
    if fault == "skip_alpha":          # soft logits: alpha stays near 1, as with every input of the older tests
        return _mixed([(5, 1), (16, 32), (33, 4097)], [1, 8, 0.3], [1, 1, 1], 2, 32, f16), ab.NAMES
    if fault == "zero_long_sequence":
        return _mixed([(5, 1), (16, 32), (300, 8193)], [1, 8, 0.3], [1, 1, 1], 2, 16, f16), ab.NAMES
    if fault == "delta_of_head0":      # the anchor's heads are copies of one another, so head 0's delta is right for it
        return _mixed([(16, 32), (300, 1025), (64, 513)], [8, 0.3, 0.3], [4, 1, 1], 3, 32, f16, same_heads=(0,)), ab.NAMES
    # padded_key: all logits about -30.  The anchor has 32 keys (no tail tile).  lse is left out of the old measure: a
    # padded key at logit 0 moves the lse of a row by about 30 - log(Lk), which no layout can hide.  (In this construction
    # the keys differ by their noise alone, so dq is what is left of a cancellation: its rel_max_err is about 1e-2 from
    # the roundings of a faultless run already.)
    cu_q, cu_k = ab.boundaries([(2, 32), (1, 200001)])
    q, k, v, dout = ab.hard_inputs("negative", cu_q, cu_k, 2, 16, f16)
    return (q, k, v, dout, cu_q, cu_k, 16 ** -0.5, f16), ("out", "dq", "dk", "dv")


@pytest.mark.parametrize("fault", ab.FAULTS)
def test_planted_error_is_caught_where_the_old_measure_misses_it(fault):
    args, old_names = _planted(fault)
    assert len(args[4]) > 2 and int(args[4][-2]) > 0      # several sequences, the victim at a non-zero offset
    r, got, ref, _ = _model_ratios(args, fault)
    finite = torch.isfinite(ref["lse"])
    old = {}
    for n in old_names:
        a, b = (got[n][finite], ref[n][finite]) if n == "lse" else (got[n], ref[n])
        old[n] = rel_max_err(a, b)
    print(fault, "ratio", {n: round(x, 1) for n, x in r.items()}, "rel_max_err", {n: round(x, 4) for n, x in old.items()})
    assert max(r.values()) > 10.0, r
    assert max(old.values()) < OLD_TOL, old


@pytest.mark.parametrize("fault", [f for f in ab.FAULTS if f != "padded_key"])
def test_planted_inputs_are_fair(fault):
    """The same inputs without the fault are within the bound (padded_key's inputs are the all-negative construction of
    test_model_within_bound_hard_logits at another layout; its 6251-tile model run is not repeated here)."""
    _assert_within(_planted(fault)[0], fault)


# ---- 3. underflow and empty sides ----------------------------------------------------------------------------------------
def test_underflow_floor_covers_a_never_attended_key():
    """fp16, gain 40: some key has p < 2**-25 for every query, so rd(p) = 0 and its dv is 0 where the reference has a
    tiny non-zero value.  With eta the model is within the bound; without it the ratio of dv or dk is above 10."""
    args = ab.grid_inputs("packed", "fp16", 32, 3, 40)
    q, k, v, dout, cu_q, cu_k, scale, dtype = args
    got = ab.rounding_model(*args)
    ref, bound = ab.reference_and_bounds(*args)
    ref0, bound0 = ab.reference_and_bounds(*args, floor=0.0)
    with_floor, without = ab.ratios(got, ref, bound), ab.ratios(got, ref0, bound0)
    print("with eta", {n: round(x, 3) for n, x in with_floor.items()}, "without", {n: round(x, 1) for n, x in without.items()})
    never = (got["dv"] == 0).all(-1) & (ref["dv"] != 0).any(-1)
    assert bool(never.any()), "no key of this layout is never attended"
    assert max(with_floor.values()) <= 1.0
    assert max(without["dv"], without["dk"]) > 10.0
    assert float((got["dv"].double() - ref["dv"])[never].abs().max()) < 1e-7      # not a fault: below 1e-7 in absolute terms


def test_empty_sides():
    cu_q, cu_k = ab.boundaries(ab.EDGE)
    for dtype in (torch.float16, torch.bfloat16):
        args = ab.random_inputs(cu_q, cu_k, 2, 16, dtype) + (cu_q, cu_k, 0.25, dtype)
        ref, bound = ab.reference_and_bounds(*args)
        got = ab.rounding_model(*args)
        for s, (lq, lk) in enumerate(ab.EDGE):
            a, b, c, e = int(cu_q[s]), int(cu_q[s + 1]), int(cu_k[s]), int(cu_k[s + 1])
            if lk == 0:
                assert bool(torch.isneginf(ref["lse"][a:b]).all()) and bool(torch.isneginf(got["lse"][a:b]).all())
                for n in ("out", "dq"):
                    assert not ref[n][a:b].any() and not got[n][a:b].any() and not bound[n][a:b].any()
                assert not bound["lse"][a:b].any()
            else:
                assert bool(torch.isfinite(ref["lse"][a:b]).all()) and bool((bound["out"][a:b] > 0).all())
            if lq == 0:
                for n in ("dk", "dv"):
                    assert not ref[n][c:e].any() and not got[n][c:e].any() and not bound[n][c:e].any()
        assert max(ab.ratios(got, ref, bound).values()) <= 1.0


def test_ratio_conventions():
    ref = torch.tensor([0.0, float("-inf"), 1.0, 2.0], dtype=torch.float64)
    bound = torch.tensor([0.0, 0.0, 0.5, 0.5], dtype=torch.float64)
    assert ab.ratio(torch.tensor([0.0, float("-inf"), 1.25, 2.0]), ref, bound) == 0.5
    assert ab.ratio(torch.tensor([1e-30, float("-inf"), 1.0, 2.0]), ref, bound) == float("inf")    # under a zero bound
    assert ab.ratio(torch.tensor([0.0, 0.0, 1.0, 2.0]), ref, bound) == float("inf")                 # finite against -inf
    assert ab.ratio(torch.tensor([0.0, float("-inf"), float("nan"), 2.0]), ref, bound) == float("inf")
    assert ab.ratio(torch.zeros(0), torch.zeros(0, dtype=torch.float64), torch.zeros(0, dtype=torch.float64)) == 0.0
