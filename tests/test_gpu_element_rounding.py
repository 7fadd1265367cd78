"""What "a float stored as f16 / bf16" means in the kernels: round to nearest even, overflow to infinity, NaN stays NaN, on
the three routes a float takes to a 16-bit element - the cast of qk_prologue.hip, the piece store of segmented.hip, the
piece store of voxelize.hip.  The expected bits are torch's: the same fp32 arithmetic on the CPU, then ``.to(dtype)``.
No subnormal of either format is used: the denormal mode is not what this file is about."""
import pytest
import torch

from warpconvnet_amd.nn.functional.qk_prologue import qk_prologue
from warpconvnet_amd.nn.functional.segmented_arithmetics import segmented_add
from warpconvnet_amd.ops.csr_rows import csr_gather_reduce

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
DTYPES = (torch.float16, torch.bfloat16)
DT_IDS = ["float16", "bfloat16"]
FRAC = {torch.float16: 10, torch.bfloat16: 7}  # stored fraction bits


def _f32(v):
    return torch.tensor(v, dtype=torch.float32)


def _next(v, up):
    return torch.nextafter(v, _f32(float("inf") if up else float("-inf")))


def _top_gap(dtype):
    """Half an ulp of the format at its largest finite value (2 - ulp) 2^E."""
    return torch.finfo(dtype).max / (2.0 - 2.0 ** -FRAC[dtype]) * 2.0 ** -(FRAC[dtype] + 1)


def _values(dtype):
    """The fp32 values of the file, positive ones first, then their negatives."""
    half = 2.0 ** -(FRAC[dtype] + 1)  # half an ulp of the format at 1
    top = torch.finfo(dtype).max
    top, over = _f32(top), _f32(top + _top_gap(dtype))  # the largest finite value, the first that rounds to infinity
    t_down, t_up = _f32(1.0 + half), _f32(1.0 + 3.0 * half)  # ties: to 1 (even below), to 1 + 2 ulp (even above)
    pos = torch.stack([t_down, t_up, _next(t_down, False), _next(t_down, True), _next(t_up, False), _next(t_up, True), top,
                       over, _next(over, False), _f32(float("inf")), _f32(float("nan")), _f32(0.0)])
    if dtype == torch.float16:
        assert over.item() == 65520.0
    return torch.cat([pos, -pos])


def _same_bits(got, want):
    got, want = got.cpu(), want.cpu()
    assert got.dtype == want.dtype and got.shape == want.shape
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan)
    g, w = got.view(torch.int16), want.view(torch.int16)
    bad = (g != w) & ~nan
    assert not bad.any(), f"bits differ at {bad.nonzero().flatten().tolist()}: {g[bad].tolist()} != {w[bad].tolist()}"


def _padded(v, per):
    """``v`` in rows of ``per`` values, the last row filled up with ones."""
    rows = -(-v.numel() // per)
    return torch.cat([v, torch.ones(rows * per - v.numel())]).reshape(rows, per)


def test_values_are_what_they_claim():
    for dtype in DTYPES:
        v = _values(dtype)
        r = v.to(dtype).float()
        n = v.numel() // 2
        ulp = 2.0 ** -FRAC[dtype]
        assert r[:6].tolist() == [1.0, 1.0 + 2 * ulp, 1.0, 1.0 + ulp, 1.0 + ulp, 1.0 + 2 * ulp]
        assert r[6].item() == torch.finfo(dtype).max and torch.isinf(r[7]) and r[8].item() == torch.finfo(dtype).max
        assert torch.equal(r[n:n + 10], -r[:10])


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("d", [8, 2])
def test_cast_route_qk_prologue(d, dtype):
    # no table, no gammas: a pure cast of [T = 2, 3, H = 1, D] fp32; D = 8 takes 16-B pieces of floats, D = 2 single pairs
    per = 2 * 3 * d
    for chunk in _padded(_values(dtype), per):
        x = chunk.reshape(2, 3, 1, d)
        _same_bits(qk_prologue(x.to(DEV), out_dtype=dtype), x.to(dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("c", [8, 3])
def test_piece_route_segmented_add(c, dtype):
    # zeros in the 16-bit dtype plus an fp32 plane, one row per segment; C = 8 stores 16-B pieces, C = 3 single elements
    y = _padded(_values(dtype), c)
    n = y.shape[0]
    x = torch.zeros(n, c, dtype=dtype)
    got = segmented_add(x.to(DEV), y.to(DEV), torch.arange(n + 1), backend="hip")
    _same_bits(got, (x.float() + y).to(dtype))


def _addend_pairs(dtype):
    """Pairs of values of ``dtype`` whose exact sum is an fp32 value: the ties, the nearest sums either side of them that two
    addends of the format can make, the largest finite value, the first value that rounds to infinity and the nearest sum
    below it, infinities, NaN, zeros; then the negatives of all pairs."""
    half = 2.0 ** -(FRAC[dtype] + 1)
    eps = 2.0 ** -FRAC[dtype]
    top = torch.finfo(dtype).max
    gap = _top_gap(dtype)
    inf, nan = float("inf"), float("nan")
    pairs = [(1.0, half), (1.0, 3 * half), (1.0, half - half * eps / 2), (1.0, half + half * eps),
             (1.0, 3 * half - 2 * half * eps), (1.0, 3 * half + 2 * half * eps), (top, 0.0), (top, gap),
             (top, gap - gap * eps / 2), (inf, 1.0), (inf, -inf), (nan, 0.0), (0.0, 0.0)]
    a = torch.tensor([p[0] for p in pairs], dtype=torch.float32)
    b = torch.tensor([p[1] for p in pairs], dtype=torch.float32)
    for t in (a, b):  # every addend is a value of the format
        fin = torch.isfinite(t)
        assert torch.equal(t[fin].to(dtype).float(), t[fin])
    return torch.cat([a, -a]), torch.cat([b, -b])


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("c", [8, 3])
def test_pattern_route_csr_gather_reduce(c, dtype):
    # a sum over groups of two rows: C = 8 loads and stores 16-B pieces, C = 3 single elements
    a, b = _addend_pairs(dtype)
    a, b = _padded(a, c), _padded(b, c)
    m = a.shape[0]
    x = torch.stack([a, b], dim=1).reshape(2 * m, c).to(dtype)  # rows 2 i and 2 i + 1 are group i
    offsets = torch.arange(0, 2 * m + 1, 2, dtype=torch.int64)
    got = csr_gather_reduce(x.to(DEV), None, offsets.to(DEV), "sum", max_segment=2)
    xf = x.float()
    _same_bits(got, ((torch.zeros(m, c) + xf[0::2]) + xf[1::2]).to(dtype))  # the kernel adds the rows in order to a zero


def test_pattern_route_sums_hit_the_values():
    for dtype in DTYPES:
        a, b = _addend_pairs(dtype)
        s, v = a + b, _values(dtype)
        for i in (0, 1, 6, 7):  # the two ties, the largest finite value, the first that rounds to infinity
            assert s[i].item() == v[i].item()
        assert torch.isinf(s[9]) and torch.isnan(s[10]) and torch.isnan(s[11]) and s[12].item() == 0.0
