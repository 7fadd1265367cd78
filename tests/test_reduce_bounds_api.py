"""CPU: the bounds of tests/reduce_bounds.py hold for an fp32 model of every operation on every case (kernel order and back
to front, one rounding), every planted defect exceeds them or breaks exactness on a named case, and the CPU path of
`ops.reductions.row_reduction` stays inside them - the 70001-row fp16 segment included."""
import pytest
import torch

from tests import reduce_bounds as rb
from tests.conv_bounds import round_toward_zero
from tests.reduce_bounds import DTYPES, OPS, dtype_name, ratio

HALF = (torch.float16, torch.bfloat16)
IDS = dict(ids=dtype_name)


def _zeros(t):
    return torch.zeros(t.shape, dtype=torch.float64)


# ---- the fp32 model stays within 1 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, **IDS)
@pytest.mark.parametrize("c", rb.SEG_CHANNELS)
@pytest.mark.parametrize("variant", rb.VARIANTS)
@pytest.mark.parametrize("case", rb.SEG_CASES)
def test_model_segments_within_bounds(case, variant, c, dtype):
    d = rb.segment_case(case, variant, c, dtype)
    ref = rb.reference(d["x"], None, d["splits"])
    for op in ("sum", "mean"):
        want, bound = rb.want_and_bound(ref, op, dtype)
        for reverse in (False, True):
            for reciprocal in ((False, True) if op == "mean" else (False,)):
                r = ratio(rb.model_reduce(d["x"], None, d["splits"], op, dtype, reverse, reciprocal), want, bound)
                assert r <= 1.0, (op, reverse, reciprocal, r)
    for op in ("max", "min"):
        val, arg = rb.model_reduce(d["x"], None, d["splits"], op, dtype)
        assert ratio(val, ref[op], _zeros(val)) == 0.0 and torch.equal(arg, ref["arg" + op])
    # the gradient of the mean: the count as an fp32 number, one division, one rounding
    want, bound = rb.segment_grad_reference(d["dy"], ref, "mean", dtype, d["x"].shape[0])
    got = (d["dy"].float() / d["lengths"].clamp_min(1).float()[:, None]).to(dtype)
    assert ratio(torch.repeat_interleave(got, d["lengths"], dim=0), want, bound) <= 1.0


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
@pytest.mark.parametrize("c", rb.SEG_CHANNELS)
@pytest.mark.parametrize("variant", rb.VAR_VARIANTS)
@pytest.mark.parametrize("case", rb.SEG_CASES)
def test_model_var_std_within_bounds(case, variant, c, dtype):
    d = rb.segment_case(case, variant, c, dtype, var=True)
    for std in (False, True):
        want, bound = rb.var_reference(d["x"], d["lengths"], dtype, std)
        for reverse in (False, True):
            r = ratio(rb.model_var(d["x"], d["splits"], dtype, std, reverse=reverse), want, bound)
            assert r <= 1.0, (std, reverse, r)


def _pool_grad_models(dy, count, rev_i, rev_o, dtype, round_terms=False):
    """fp32 model of the mean's backward: terms dy[r] * (1 / count[r]); ``round_terms``: the planted defect 3."""
    terms = dy.float() * (1.0 / count.clamp_min(1).float())[:, None]
    if round_terms:
        terms = terms.to(dtype).float()
    return [rb.seq_sum(terms[rev_i], rev_o, reverse).to(dtype) for reverse in (False, True)]


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
@pytest.mark.parametrize("c", rb.POOL_CHANNELS)
@pytest.mark.parametrize("variant", rb.VARIANTS)
@pytest.mark.parametrize("K", rb.POOL_K)
def test_model_pool_tables_within_bounds(K, variant, c, dtype):
    d = rb.pool_case(K, c, dtype, variant)
    fi, fo = rb.table_csr(d["fwd"], K)
    ri, ro = rb.table_csr(d["rev"], K)
    ref = rb.reference(d["x"], fi, fo)
    assert ref["len"][0] == 0 and ref["len"][1] == 1 and ref["len"][2] == K
    for op in ("sum", "mean"):
        want, bound = rb.want_and_bound(ref, op, dtype)
        for reverse in (False, True):
            assert ratio(rb.model_reduce(d["x"], fi, fo, op, dtype, reverse, reciprocal=True), want, bound) <= 1.0
    for op in ("max", "min"):
        val, arg = rb.model_reduce(d["x"], fi, fo, op, dtype)
        assert ratio(val, ref[op], _zeros(val)) == 0.0 and torch.equal(arg, ref["arg" + op])
        assert (val[0] == 0).all() and (arg[0] == -1).all()
        want, bound = rb.pool_select_reference(d["dy"], ref["arg" + op], ri, ro, dtype)
        sel = ref["arg" + op][ri] == torch.repeat_interleave(torch.arange(len(ro) - 1), ro[1:] - ro[:-1])[:, None]
        terms = torch.where(sel, d["dy"][ri].float(), torch.zeros(()))
        for reverse in (False, True):
            assert ratio(rb.seq_sum(terms, ro, reverse).to(dtype), want, bound) <= 1.0
    want, bound = rb.pool_sum_grad_reference(d["dy"], ri, ro, dtype)
    for reverse in (False, True):
        assert ratio(rb.model_reduce(d["dy"], ri, ro, "sum", dtype, reverse), want, bound) <= 1.0
    want, bound = rb.pool_mean_grad_reference(d["dy"], ref["len"], ri, ro, dtype)
    for got in _pool_grad_models(d["dy"], ref["len"], ri, ro, dtype):
        assert ratio(got, want, bound) <= 1.0


@pytest.mark.parametrize("dtype", HALF, **IDS)
def test_model_scene_mean_gradient_within_bounds(dtype):
    """Kernel 3, stride 2: up to 8 overlapping windows per voxel.  Rounded once the model is inside the bound; rounded per
    term, as `sparse_pool.py` did, it is far outside (planted defect 3 on the real map)."""
    m = rb.scene_map(3, 2)
    dy = rb.upstream(m["num_out"], 16, dtype, 5)
    count = m["fwd"][1][1:] - m["fwd"][1][:-1]
    ri, ro = m["rev"]
    want, bound = rb.pool_mean_grad_reference(dy, count, ri, ro, dtype)
    for got in _pool_grad_models(dy, count, ri, ro, dtype):
        assert ratio(got, want, bound) <= 1.0
    worst = max(ratio(got, want, bound) for got in _pool_grad_models(dy, count, ri, ro, dtype, round_terms=True))
    print(f"mean gradient, terms rounded before the sum, {dtype_name(dtype)}: ratio {worst:.1f}")
    assert worst > 1.0


# ---- every planted defect is caught -----------------------------------------------------------------------------------------------
def _storage_sum(x, a, b):
    """Rows [a, b) of ``x`` summed in x's own type (planted defect: accumulation in the storage type)."""
    acc = torch.zeros(x.shape[1], dtype=x.dtype)
    for r in range(a, b):
        acc = acc + x[r]
    return acc


@pytest.mark.parametrize("dtype", HALF, **IDS)
def test_defect_storage_accumulation(dtype):
    """edges / random / C = 13, the 2049-row segment."""
    d = rb.segment_case("edges", "random", 13, dtype)
    ref = rb.reference(d["x"], None, d["splits"])
    i = rb.SEG_LENGTHS.index(2049)
    want, bound = rb.want_and_bound(ref, "sum", dtype)
    got = _storage_sum(d["x"], int(d["splits"][i]), int(d["splits"][i + 1]))
    assert ratio(got[None], want[i:i + 1], bound[i:i + 1]) > 1.0


def test_defect_count_in_storage_type():
    """Defect 1.  edges / fp16, the 70001-row segment: the count is inf in fp16, the mean and its gradient come out 0.  bf16 at
    257 rows (the count reads 256): the mean is off by 2**-8 of its value on top of its rounding (the gradient g / 256 of a bf16
    g is exact, so it sits a hair under the bound: 2**-8 |ref| against (3 f + 2**-8) |ref|)."""
    for dtype, length in ((torch.float16, 70001), (torch.bfloat16, 257)):
        d = rb.segment_case("edges", "random", 13, dtype)
        ref = rb.reference(d["x"], None, d["splits"])
        i = rb.SEG_LENGTHS.index(length)
        cnt = d["lengths"].clamp_min(1).to(dtype).float()[:, None]
        want, bound = rb.segment_grad_reference(d["dy"], ref, "mean", dtype, d["x"].shape[0])
        got = torch.repeat_interleave((d["dy"].float() / cnt).to(dtype), d["lengths"], dim=0)
        rows = slice(int(d["splits"][i]), int(d["splits"][i + 1]))
        r_grad = ratio(got[rows], want[rows], bound[rows])
        want, bound = rb.want_and_bound(ref, "mean", dtype)
        r_fwd = ratio((rb.seq_sum(d["x"], d["splits"]) / cnt).to(dtype)[i:i + 1], want[i:i + 1], bound[i:i + 1])
        print(f"count cast to {dtype_name(dtype)}, {length} rows: forward ratio {r_fwd:.3g}, gradient ratio {r_grad:.3g}")
        if dtype == torch.float16:
            assert r_grad > 1.0 and r_fwd > 1.0 and (got[rows] == 0).all()
        else:
            assert r_fwd > 1.0


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_defect_last_extremum(dtype):
    """ties: segments (short, C = 13) and the K = 27 table (C = 8)."""
    d = rb.segment_case("short", "ties", 13, dtype)
    ref = rb.reference(d["x"], None, d["splits"])
    p = rb.pool_case(27, 8, dtype, "ties")
    fi, fo = rb.table_csr(p["fwd"], 27)
    pref = rb.reference(p["x"], fi, fo)
    for op in ("max", "min"):
        val, arg = rb.model_extremum(d["x"], None, d["splits"], op, last=True)
        assert torch.equal(val.double(), ref[op]) and not torch.equal(arg, ref["arg" + op])
        val, arg = rb.model_extremum(p["x"][fi], fi, fo, op, last=True)
        assert torch.equal(val.double(), pref[op]) and not torch.equal(arg, pref["arg" + op])


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_defect_last_row_or_column_dropped(dtype):
    """Segments (edges / random / C = 13): every op notices a segment that stops one row early - the one-row segment reads 0.
    Tables (K = 8 and 27, C = 13): row 1 holds only column K - 1."""
    d = rb.segment_case("edges", "random", 13, dtype)
    ref = rb.reference(d["x"], None, d["splits"])
    keep = torch.ones(d["x"].shape[0], dtype=torch.bool)
    keep[(d["splits"][1:] - 1)[d["lengths"] > 0]] = False
    starts = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum((d["lengths"] - 1).clamp_min(0), 0)])
    for op in OPS:
        want, bound = rb.want_and_bound(ref, op, dtype)
        got = rb.model_reduce(d["x"][keep], None, starts, op, dtype)
        got = got[0] if isinstance(got, tuple) else got
        assert ratio(got, want, bound) > 1.0, op
    for K in (8, 27):
        p = rb.pool_case(K, 13, dtype, "random")
        fi, fo = rb.table_csr(p["fwd"], K)
        pref = rb.reference(p["x"], fi, fo)
        cut = p["fwd"].copy()
        cut[:, K - 1] = -1
        ci, co = rb.table_csr(cut, K)
        for op in OPS:
            want, bound = rb.want_and_bound(pref, op, dtype)
            got = rb.model_reduce(p["x"], ci, co, op, dtype)
            got = got[0] if isinstance(got, tuple) else got
            assert ratio(got[1:2], want[1:2], bound[1:2]) > 1.0, (K, op)


@pytest.mark.parametrize("dtype", HALF, **IDS)
def test_defect_mean_gradient_terms_rounded(dtype):
    """Defect 3 on the K = 27 table, C = 8."""
    p = rb.pool_case(27, 8, dtype, "random")
    fi, fo = rb.table_csr(p["fwd"], 27)
    ri, ro = rb.table_csr(p["rev"], 27)
    count = fo[1:] - fo[:-1]
    want, bound = rb.pool_mean_grad_reference(p["dy"], count, ri, ro, dtype)
    worst = max(ratio(g, want, bound) for g in _pool_grad_models(p["dy"], count, ri, ro, dtype, round_terms=True))
    print(f"K = 27 table, terms rounded before the sum, {dtype_name(dtype)}: ratio {worst:.1f}")
    assert worst > 1.0


def _one_pass_var(x, lengths, splits, std=False, eps=1e-6):
    """Defect 2, as `row_reduction` formed it: mean(x**2) - mean(x)**2 in the feature type (each mean an fp32 sum, rounded)."""
    cnt = lengths.clamp_min(1).float()[:, None]
    mean = (rb.seq_sum(x, splits) / cnt).to(x.dtype)
    var = (rb.seq_sum(x ** 2, splits) / cnt).to(x.dtype) - mean ** 2
    return torch.sqrt(var + eps) if std else var


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_defect_one_pass_variance(dtype):
    """edges / mean100 / C = 13: var at mean 100."""
    d = rb.segment_case("edges", "mean100", 13, dtype, var=True)
    for std in (False, True):
        want, bound = rb.var_reference(d["x"], d["lengths"], dtype, std)
        r = ratio(_one_pass_var(d["x"], d["lengths"], d["splits"], std), want, bound)
        print(f"one-pass {'std' if std else 'var'} at mean 100, {dtype_name(dtype)}: ratio {r:.3g}")
        assert r > 1.0


@pytest.mark.parametrize("dtype", HALF, **IDS)
def test_defect_round_toward_zero(dtype):
    """short / random / C = 13 (sum, mean) and the K = 8 table's mean gradient."""
    d = rb.segment_case("short", "random", 13, dtype)
    ref = rb.reference(d["x"], None, d["splits"])
    for op in ("sum", "mean"):
        want, bound = rb.want_and_bound(ref, op, dtype)
        acc = rb.seq_sum(d["x"], d["splits"])
        if op == "mean":
            acc = acc / d["lengths"].clamp_min(1).float()[:, None]
        assert ratio(round_toward_zero(acc, dtype), want, bound) > 1.0, op
    p = rb.pool_case(8, 13, dtype, "random")
    fo = rb.table_csr(p["fwd"], 8)[1]
    ri, ro = rb.table_csr(p["rev"], 8)
    count = fo[1:] - fo[:-1]
    want, bound = rb.pool_mean_grad_reference(p["dy"], count, ri, ro, dtype)
    terms = p["dy"].float() * (1.0 / count.clamp_min(1).float())[:, None]
    assert ratio(round_toward_zero(rb.seq_sum(terms[ri], ro), dtype), want, bound) > 1.0


# ---- the CPU path of row_reduction ------------------------------------------------------------------------------------------------
def _run(x, splits, op, dy):
    from warpconvnet_amd.ops.reductions import row_reduction

    xr = x.clone().requires_grad_(True)
    y = row_reduction(xr, splits, op)
    y.backward(dy)
    assert y.dtype == x.dtype and xr.grad.dtype == x.dtype
    return y.detach(), xr.grad


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
@pytest.mark.parametrize("variant", rb.VARIANTS)
@pytest.mark.parametrize("case", rb.SEG_CASES)
def test_row_reduction_cpu_within_bounds(case, variant, dtype):
    """C = 13.  edges holds the 70001-row segment: fp16 gave NaN in the forward and 0 in the backward of the mean."""
    d = rb.segment_case(case, variant, 13, dtype)
    ref = rb.reference(d["x"], None, d["splits"])
    for op in OPS:
        y, dx = _run(d["x"], d["splits"], op, d["dy"])
        want, bound = rb.want_and_bound(ref, op, dtype)
        assert ratio(y, want, bound) <= 1.0, op
        want, bound = rb.segment_grad_reference(d["dy"], ref, op, dtype, d["x"].shape[0])
        assert ratio(dx, want, bound) <= 1.0, (op, "gradient")
    if case == "edges" and dtype == torch.float16:
        i = rb.SEG_LENGTHS.index(70001)
        rows = slice(int(d["splits"][i]), int(d["splits"][i + 1]))
        _, dx = _run(d["x"], d["splits"], "mean", d["dy"])
        assert (dx[rows] != 0).all() and torch.isfinite(dx).all()


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
@pytest.mark.parametrize("variant", rb.VAR_VARIANTS)
@pytest.mark.parametrize("case", rb.SEG_CASES)
def test_row_reduction_cpu_var_std_within_bounds(case, variant, dtype):
    """C = 13; var at mean 100 is the case the one-pass form failed (negative variances, NaN std)."""
    d = rb.segment_case(case, variant, 13, dtype, var=True)
    for std in (False, True):
        y, dx = _run(d["x"], d["splits"], "std" if std else "var", d["dy"])
        want, bound = rb.var_reference(d["x"], d["lengths"], dtype, std)
        assert ratio(y, want, bound) <= 1.0, std
        gref, yard = rb.var_grad_reference(d["x"], d["dy"], d["lengths"], std)
        r = rb.grad_ratio(dx, gref, yard, dtype)
        assert r <= 1.0, (std, "gradient", r)


def test_pool_features_var_shares_the_two_passes():
    """`point_pool.pool_features` takes the same helper over a CSR map (CPU path): var at mean 100 in fp32."""
    from warpconvnet_amd.nn.functional.point_pool import pool_features
    from warpconvnet_amd.utils.unique import ToUnique

    d = rb.segment_case("edges", "mean100", 13, torch.float32, var=True)
    code = torch.repeat_interleave(torch.arange(len(d["lengths"])), d["lengths"])
    perm = torch.randperm(len(code), generator=torch.Generator().manual_seed(0))
    tu = ToUnique(return_to_unique_indices=True)
    uniq = tu.to_unique(code[perm])
    present = d["lengths"] > 0
    assert torch.equal(uniq, torch.arange(len(d["lengths"]))[present])
    for std in (False, True):
        want, bound = rb.var_reference(d["x"], d["lengths"], torch.float32, std)
        got = pool_features(d["x"][perm], tu, "std" if std else "var")
        assert ratio(got, want[present], bound[present]) <= 1.0


def test_pool_row_vec_checks_the_pointers(hip_lib):
    """Fix 4, host side (nothing is dereferenced): the 16-B row pieces need channels % (16 / element size) == 0 AND both
    feature pointers 16-B aligned; a contiguous view one element into its buffer takes the one-element path."""
    from warpconvnet_amd import _lib

    L = hip_lib
    base = 1 << 20
    for code, size in ((_lib.WCN_F32, 4), (_lib.WCN_F16, 2), (_lib.WCN_BF16, 2)):
        vec = 16 // size
        assert L.wcn_pool_row_vec(base, base + 4096, 9 * vec, code) == vec
        assert L.wcn_pool_row_vec(base, base + 4096, 9 * vec + 1, code) == 1
        assert L.wcn_pool_row_vec(base + size, base + 4096, 9 * vec, code) == 1  # the misaligned view as the source
        assert L.wcn_pool_row_vec(base, base + 4096 + size, 9 * vec, code) == 1  # ... as the destination
    assert L.wcn_pool_row_vec(base, base, 4, _lib.WCN_F32) == 4 and L.wcn_pool_row_vec(base, base, 4, _lib.WCN_BF16) == 1
    assert L.wcn_pool_row_vec(base, base, 8, 7) == 0 and L.wcn_pool_row_vec(base, base, 0, _lib.WCN_F32) == 0
    # a pointer that is not aligned to its element is refused before any launch
    assert L.wcn_pool_gather(base + 1, base, 4, 4, 8, 8, _lib.WCN_BF16, 0, base, None, None, None) == -5
    assert L.wcn_pool_select(base, base, base, 4, 4, 8, 8, _lib.WCN_BF16, base + 1, None) == -5
