"""GPU: every BatchNorm pass of csrc/norm.hip against fp64 with the per-pass bounds of tests/bn_bounds.py (threshold: ratio <= 1),
through the pass-level C entries.

a. exact sums: integer planes whose partial sums are exact in fp32 in ANY order, at every layout of `norm_reduce_kernel`
   (second channel trip, lanes_c == 256, 256 % lanes_c != 0, second row trip, clamped rows in flight, 512 workgroups of more than
   128 rows, workgroups without rows, the widest layer) - `wcn_bn_stats` within a few roundings, `wcn_bn_backward_reduce[_masked]`
   EQUAL to the integer sums for all three mask sources.  tests/test_bn_bounds_api.py proves the layouts from `reduce_layout`.
b. the grid-stride apply kernels past their caps (2048 / 4096 workgroups), per element.
c. the whole chain, every pass on the fp32 vectors the previous pass produced, over types, sizes, modes and input families.
d. `hip_batch_norm` end to end on a layout with a second channel trip.

Largest ratio per pass and storage type over the whole file (`test_error_ratios_report` prints them; records, not thresholds -
the threshold is 1):

    pass                  fp32    fp16    bf16
    mean                  0.831   0.455   0.157
    var                   0.249   0.127   0.152
    mean (exact planes)   0.241   0.111   0.143
    var (exact planes)    0.326   0.239   0.323
    rstd                  0.601   0.620   0.587
    scale                 0.566   0.571   0.641
    shift                 0.768   0.770   0.768
    running_mean          0.673   0.688   0.647
    running_var           0.639   0.718   0.598
    y                     0.499   0.999   0.996
    z                     0.499   0.995   0.996
    sum_dy                0.247   0.003   0.002
    sum_dy_xhat           0.340   0.336   0.289
    dx                    0.393   0.998   0.996

(the sums of the exact planes are not in the table: they are equal, not close; sum_dy of 16-bit values is a sum of short
mantissas and all but exact.)
"""
import copy

import pytest
import torch
import torch.nn as nn

from tests import bn_bounds as bb
from tests.util import rel_max_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RATIOS = {}
_ID = lambda v: str(v).replace("torch.", "")


def _record(name, dtype, q):
    key = (name, _ID(dtype))
    RATIOS[key] = max(RATIOS.get(key, 0.0), q)


def _ratio_where_it_is(got, ref, bound):
    """`conv_bounds.ratio` without the trip to the CPU (the 33 M elements of the cap cases): equal elements count 0, a
    difference under a zero bound or a NaN counts inf."""
    diff = (got.double() - ref).abs()
    q = torch.where(got.double() == ref, torch.zeros_like(diff), diff / bound)
    return float(torch.where(torch.isnan(q), torch.full_like(q, float("inf")), q).max())


def _check(name, dtype, got, ref, bound):
    q = _ratio_where_it_is(got, ref, bound) if ref.is_cuda else bb.ratio(got, ref, bound)
    _record(name, dtype, q)
    print(f"{name} {_ID(dtype)}: ratio {q:.3g}")
    assert q <= 1.0, (name, bb.worst(got, ref.cpu(), bound.cpu()))


class HipBackend:
    """The pass entries of include/wcn.h behind the interface `bn_bounds.verify_chain` drives."""

    def __init__(self):
        from warpconvnet_amd import _lib

        self.lib, self.L, self.dev = _lib, _lib.lib(), torch.device(DEV)
        self.st = _lib.stream_handle(self.dev)

    def _f32(self, c, k):
        return [torch.empty(c, device=self.dev) for _ in range(k)]

    def _ws(self, c):
        return torch.empty(self.L.wcn_bn_workspace(c), dtype=torch.uint8, device=self.dev)

    def stats(self, x):
        p, (n, c) = self.lib.ptr, x.shape
        mean, var = self._f32(c, 2)
        ws = self._ws(c)
        self.lib.check(self.L.wcn_bn_stats(p(x), n, c, self.lib.dtype_code(x.dtype), p(mean), p(var), p(ws), ws.numel(), self.st),
                       "wcn_bn_stats")
        return mean, var

    def stats_fold(self, x, gamma, beta, rm, rv, momentum, eps):
        p, (n, c) = self.lib.ptr, x.shape
        mean, var, rstd, scale, shift = self._f32(c, 5)
        ws = self._ws(c)
        counter = torch.tensor(5, device=self.dev)
        self.lib.check(self.L.wcn_bn_stats_fold(p(x), n, c, self.lib.dtype_code(x.dtype), p(gamma), p(beta), p(rm), p(rv), momentum, eps,
                                                p(mean), p(var), p(rstd), p(scale), p(shift), p(counter), p(ws), ws.numel(), self.st),
                       "wcn_bn_stats_fold")
        assert int(counter) == 6
        m2, v2 = self.stats(x)                    # the statistics entry alone: the same two kernels
        assert torch.equal(m2, mean) and torch.equal(v2, var)
        return mean, var, rstd, scale, shift, rm, rv

    def fold(self, rm, rv, gamma, beta, eps):
        p, c = self.lib.ptr, rm.numel()
        mean, rstd, scale, shift = self._f32(c, 4)
        self.lib.check(self.L.wcn_bn_fold(p(rm), p(rv), p(gamma), p(beta), eps, c, p(mean), p(rstd), p(scale), p(shift), self.st),
                       "wcn_bn_fold")
        return mean, rstd, scale, shift

    def apply(self, x, scale, shift, relu, res):
        p, (n, c) = self.lib.ptr, x.shape
        y = torch.empty_like(x)
        code = self.lib.dtype_code(x.dtype)
        if res is None:
            self.lib.check(self.L.wcn_bn_apply(p(x), n, c, code, p(scale), p(shift), int(relu), p(y), self.st), "wcn_bn_apply")
        else:
            self.lib.check(self.L.wcn_bn_apply_residual(p(x), p(res), n, c, code, p(scale), p(shift), int(relu), p(y), self.st),
                           "wcn_bn_apply_residual")
        return y

    def _layer_backward(self, x, dy, mean, rstd, gamma, mask_kind, scale, shift, z, training, want_dx):
        """`wcn_bn_train_backward_ld`: dy is a column slice of a wider tensor, read in place."""
        p, (n, c) = self.lib.ptr, x.shape
        assert dy.stride(1) == 1 and dy.stride(0) > c
        stats = torch.stack([mean, rstd, scale, shift, torch.zeros_like(mean)]).contiguous()
        sums = torch.empty(2, c, device=self.dev)
        dx = torch.empty_like(x) if want_dx else None
        dres = torch.empty_like(x) if (want_dx and mask_kind == "z") else None
        ws = self._ws(c)
        self.lib.check(self.L.wcn_bn_train_backward_ld(p(dy), dy.stride(0), p(x), p(z) if mask_kind == "z" else None,
                                                       int(mask_kind is not None), n, c, self.lib.dtype_code(x.dtype), p(stats), p(gamma),
                                                       int(training), p(sums), p(dx), p(dres), p(ws), ws.numel(), self.st),
                       "wcn_bn_train_backward_ld")
        return sums, dx, dres

    def reduce(self, x, dy, mean, rstd, mask_kind, scale, shift, z):
        if not dy.is_contiguous():
            sums, _, _ = self._layer_backward(x, dy, mean, rstd, None, mask_kind, scale, shift, z, True, False)
            return sums[0].clone(), sums[1].clone()
        p, (n, c) = self.lib.ptr, x.shape
        s0, s1 = self._f32(c, 2)
        ws = self._ws(c)
        code = self.lib.dtype_code(x.dtype)
        if mask_kind == "z":
            self.lib.check(self.L.wcn_bn_backward_reduce_masked(p(dy), p(x), p(z), n, c, code, p(mean), p(rstd), p(s0), p(s1), p(ws),
                                                                ws.numel(), self.st), "wcn_bn_backward_reduce_masked")
        else:
            rsc, rsh = (scale, shift) if mask_kind == "recompute" else (None, None)
            self.lib.check(self.L.wcn_bn_backward_reduce(p(dy), p(x), p(rsc), p(rsh), n, c, code, p(mean), p(rstd), p(s0), p(s1), p(ws),
                                                         ws.numel(), self.st), "wcn_bn_backward_reduce")
        return s0, s1

    def bwd_apply(self, x, dy, mean, rstd, gamma, s0, s1, mask_kind, scale, shift, z, training):
        if not dy.is_contiguous():
            sums, dx, dres = self._layer_backward(x, dy, mean, rstd, gamma, mask_kind, scale, shift, z, training, True)
            if training:                          # the layer entry's own reduce: the same kernels, the same bits
                assert torch.equal(sums[0], s0) and torch.equal(sums[1], s1)
            return dx, dres
        p, (n, c) = self.lib.ptr, x.shape
        dx = torch.empty_like(x)
        code = self.lib.dtype_code(x.dtype)
        if mask_kind == "z":
            dres = torch.empty_like(x)
            self.lib.check(self.L.wcn_bn_backward_apply_masked(p(dy), p(x), p(z), n, c, code, p(mean), p(rstd), p(gamma), p(s0), p(s1),
                                                               p(dx), p(dres), self.st), "wcn_bn_backward_apply_masked")
            return dx, dres
        rsc, rsh = (scale, shift) if mask_kind == "recompute" else (None, None)
        self.lib.check(self.L.wcn_bn_backward_apply(p(dy), p(x), p(rsc), p(rsh), n, c, code, p(mean), p(rstd), p(gamma), p(s0), p(s1),
                                                    p(dx), self.st), "wcn_bn_backward_apply")
        return dx, None


# ---- a. exact sums at every reduce layout --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,c,n", bb.reduce_cases(), ids=_ID)
def test_exact_sums_at_every_reduce_layout(dtype, c, n):
    be = HipBackend()
    x_cpu, dy_cpu = bb.exact_planes(n, c, dtype)
    x, dy = x_cpu.to(DEV), dy_cpu.to(DEV)
    mean, var = be.stats(x)
    ref, bound = bb.stats_ref(x_cpu, few_roundings=True)
    if n == 1:                                   # legal for the pass entries: the pivot, and no variance
        assert torch.equal(mean.cpu(), x_cpu[0].float()) and not var.any()
    _check("mean (exact planes)", dtype, mean, ref["mean"], bound["mean"])
    _check("var (exact planes)", dtype, var, ref["var"], bound["var"])
    zero, one, half = torch.zeros(c, device=DEV), torch.ones(c, device=DEV), torch.full((c,), 0.5, device=DEV)
    g = torch.Generator().manual_seed(n + c)
    z_cpu = torch.randint(0, 3, (n, c), generator=g).to(dtype)            # a stored ReLU output: zeros and positive values
    for kind, mask, z in ((None, None, None), ("recompute", x_cpu > 0, None), ("z", z_cpu > 0, z_cpu.to(DEV))):
        s0, s1 = be.reduce(x, dy, zero, one, kind, one, half, z)          # x * 1 + 0.5 > 0 iff x > 0 (x is a non-zero integer)
        w0, w1 = bb.exact_sums(x_cpu, dy_cpu, mask)
        assert torch.equal(s0.cpu(), w0), (kind, "sum_dy", int((s0.cpu() != w0).sum()))
        assert torch.equal(s1.cpu(), w1), (kind, "sum_dy_xhat", int((s1.cpu() != w1).sum()))


# ---- b. the apply grids past their caps ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,c,n", bb.APPLY_CAP_CASES, ids=_ID)
def test_apply_kernels_past_their_grid_caps(dtype, c, n):
    """Planted per-channel vectors with mixed signs and one channel with scale == 0 and gamma == 0; the fp64 reference of these
    cases is evaluated on the device."""
    be = HipBackend()
    g = torch.Generator(device=DEV).manual_seed(c + n)
    rnd = lambda *shape: torch.randn(*shape, device=DEV, generator=g)
    x, dy, res = (rnd(n, c) * 2.0 + 0.7).to(dtype), rnd(n, c).to(dtype), rnd(n, c).to(dtype)
    scale, shift, mean, gamma = rnd(c), rnd(c) * 0.5, rnd(c) * 0.3, rnd(c)
    rstd = torch.rand(c, device=DEV, generator=g) + 0.5
    s0, s1 = rnd(c) * n ** 0.5, rnd(c) * n ** 0.5
    scale[3 % c] = 0.0
    gamma[3 % c] = 0.0
    shift[5 % c] = 0.0
    y = be.apply(x, scale, shift, True, None)
    _check("y", dtype, y, *bb.apply_ref(x, scale, shift, True))
    z = be.apply(x, scale, shift, True, res)
    _check("z", dtype, z, *bb.apply_ref(x, scale, shift, True, res))
    assert bool((y >= 0).all()) and bool((z >= 0).all()) and 0.1 < float((y > 0).float().mean()) < 0.9
    dx, _ = be.bwd_apply(x, dy, mean, rstd, gamma, s0, s1, "recompute", scale, shift, None, True)
    ref, bound, _ = bb.bwd_apply_ref(x, dy, y > 0, mean, rstd, gamma, s0, s1)
    _check("dx", dtype, dx, ref, bound)
    dx, dres = be.bwd_apply(x, dy, mean, rstd, gamma, s0, s1, "z", scale, shift, z, True)
    ref, bound, gm = bb.bwd_apply_ref(x, dy, z > 0, mean, rstd, gamma, s0, s1)
    _check("dx", dtype, dx, ref, bound)
    assert torch.equal(dres.double(), gm)


# ---- c. every pass against its bound -------------------------------------------------------------------------------------------------
MODES = [(training, relu, tail) for training in (True, False) for relu in (False, True) for tail in (False, True)]


def _chain(fam, dtype, crowd=False):
    be = HipBackend()
    for training, relu, tail in MODES:
        ratios, fails = bb.verify_chain(be, fam, training, relu, tail, crowd=crowd, dev=DEV)
        for k, v in ratios.items():
            _record(k, dtype, v)
        print(f"train={training} relu={relu} tail={tail}: " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
        assert not fails, (training, relu, tail, fails)


@pytest.mark.parametrize("c", [8, 13, 96])
@pytest.mark.parametrize("n", [2, 7, 130, 1024])
@pytest.mark.parametrize("dtype", bb.DTYPES, ids=_ID)
def test_every_pass_against_its_bound(dtype, n, c):
    _chain(bb.family("randn", n, c, dtype), dtype)


@pytest.mark.parametrize("name,dtype", [(f, d) for f in bb.FAMILIES[1:] for d in bb.family_dtypes(f)], ids=_ID)
def test_every_pass_against_its_bound_on_the_input_families(name, dtype):
    for n, c in ((7, 8), (130, 13), (130, 96), (1024, 8)):
        _chain(bb.family(name, n, c, dtype), dtype, crowd=name == "relu_crowded")


# ---- d. end to end through the Python path -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,c", [(torch.float32, 1028), (torch.bfloat16, 2056), (torch.float16, 2056)], ids=_ID)
def test_hip_batch_norm_reaches_the_wide_layouts(dtype, c):
    """`batch_norm_module_forward` against fp64 `nn.BatchNorm1d` at 1100 rows of a width with a second channel trip, with the
    tolerances of tests/test_gpu_batchnorm.py::test_training_forward_backward."""
    from warpconvnet_amd.nn.functional.normalizations import batch_norm_module_forward

    n = 1100
    assert bb.reduce_layout(n, c, dtype)["channel_trips"] == 2
    torch.manual_seed(c)
    bn = nn.BatchNorm1d(c).to(DEV)
    with torch.no_grad():
        bn.weight.normal_(1.0, 0.3)
        bn.bias.normal_(0.0, 0.3)
    x = (torch.randn(n, c, device=DEV) * 2.0 + 0.7).to(dtype).requires_grad_(True)
    g = torch.randn(n, c, device=DEV).to(dtype)
    ref = copy.deepcopy(bn).double().cpu()
    xr = x.detach().double().cpu().requires_grad_(True)
    y_ref = torch.relu(ref(xr))
    y_ref.backward(g.double().cpu())
    y = batch_norm_module_forward(bn, x, relu=True)
    y.backward(g)
    f32 = dtype == torch.float32
    assert y.dtype == dtype and rel_max_err(y.detach(), y_ref.detach()) < (1e-5 if f32 else 1.5e-2)
    assert rel_max_err(x.grad, xr.grad) < (1e-4 if f32 else 3e-2)
    assert rel_max_err(bn.weight.grad, ref.weight.grad) < (1e-4 if f32 else 2e-2)
    assert rel_max_err(bn.bias.grad, ref.bias.grad) < (1e-4 if f32 else 2e-2)
    assert rel_max_err(bn.running_mean, ref.running_mean) < 1e-4 and rel_max_err(bn.running_var, ref.running_var) < 1e-4
    assert int(bn.num_batches_tracked) == 1


def test_error_ratios_report():
    """Prints the largest ratio per pass and type of whatever ran before it in this process (for docs/OPTIMISATION_LOG.md)."""
    for (name, dtype), r in sorted(RATIOS.items()):
        print(f"ratio {name} {dtype}: {r:.3f}")
    assert all(r <= 1.0 for r in RATIOS.values())
