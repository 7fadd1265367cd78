"""GPU: `csrc/fps.hip` against the yardstick of tests/fps_helper.py - index-exact equality, plus the fp64 property that does
not depend on a rounding order.  Every case runs on two input classes: an integer lattice (exact distances, ties everywhere:
the tie rule) and ``randn`` (the rounding contract).  The shapes come from tests/fps_caps.py."""
import pytest
import torch

from tests import fps_caps as caps
from tests import fps_helper as H
from warpconvnet_amd.ops import sampling
from warpconvnet_amd.ops.sampling import farthest_point_sampling

pytestmark = pytest.mark.gpu

KINDS = ["lattice", "randn"]
DEV = "cuda:0"


def _run(lengths, kind, K, tier="auto", start=None, device_offsets=False):
    off = H.offsets_of(lengths)
    return farthest_point_sampling(H.cloud(lengths, kind).to(DEV), off.to(DEV) if device_offsets else off, K, start=start,
                                   backend="hip", _tier=tier)


def _check(lengths, kind, K, got, start=None):
    assert got.dtype == torch.int32 and got.is_cuda and got.shape == (len(lengths) * K,)
    got = got.cpu()
    want = H.expected(lengths, kind, K, start)
    wrong = torch.nonzero(got != want).reshape(-1)
    assert wrong.numel() == 0, (f"{wrong.numel()} of {got.numel()} indices differ, first at segment {int(wrong[0]) // K} "
                                f"sample {int(wrong[0]) % K}: {int(got[wrong[0]])} for {int(want[wrong[0]])}")
    H.check_property(H.cloud(lengths, kind), H.offsets_of(lengths), K, got, start)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("K", [1, 2, 17])
def test_resident_edges(kind, K):
    """Both sides of every wave, workgroup and cap edge in one ragged batch; one launch of the largest instantiation."""
    _check(caps.RESIDENT, kind, K, _run(caps.RESIDENT, kind, K))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("length", caps.PER_INSTANTIATION)
def test_every_resident_instantiation(kind, length):
    """A segment alone picks the instantiation of its own length: every P, full and with one row in its last slot."""
    _check((length,), kind, 5, _run((length,), kind, 5, tier="resident"))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("K", [7, 10])
@pytest.mark.parametrize("tier", ["resident", "streamed"])
def test_k_at_and_beyond_the_segment(kind, K, tier):
    _check(caps.SHORT, kind, K, _run(caps.SHORT, kind, K, tier=tier))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("tier", ["resident", "streamed"])
def test_more_segments_than_a_grid(kind, tier):
    """The stride over segments, with empty segments in between."""
    _check(caps.MANY, kind, 3, _run(caps.MANY, kind, 3, tier=tier))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("K", [2, 9])
def test_streamed_forced(kind, K):
    """One workgroup with rows, a second wave, a second workgroup, all workgroups, and the second trip of the stride."""
    _check(caps.STREAMED, kind, K, _run(caps.STREAMED, kind, K, tier="streamed"))


@pytest.mark.parametrize("kind", KINDS)
def test_streamed_natural(kind):
    _check(caps.NATURAL, kind, 33, _run(caps.NATURAL, kind, 33))


@pytest.mark.parametrize("kind", KINDS)
def test_both_tiers_in_one_call(kind):
    _check(caps.MIXED, kind, 5, _run(caps.MIXED, kind, 5))
    _check(caps.MIXED, kind, 5, _run(caps.MIXED, kind, 5, device_offsets=True))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("tier", ["resident", "streamed"])
def test_start(kind, tier):
    lengths = (0, 1, 65, caps.T + 1, 3 * caps.T)
    start = (0, 0, 64, caps.T, 2 * caps.T + 5)
    _check(lengths, kind, 6, _run(lengths, kind, 6, tier=tier, start=start), start)
    _check(lengths, kind, 6, _run(lengths, kind, 6, tier=tier, start=torch.tensor(start, device=DEV)), start)


@pytest.mark.parametrize("kind", KINDS)
def test_tiers_agree_and_calls_repeat(kind):
    a = _run(caps.RESIDENT, kind, 17, tier="resident")
    b = _run(caps.RESIDENT, kind, 17, tier="streamed")
    assert torch.equal(a, b)
    assert torch.equal(a, _run(caps.RESIDENT, kind, 17, tier="resident"))
    assert torch.equal(b, _run(caps.RESIDENT, kind, 17, tier="streamed"))


def test_forcing_the_resident_tier_above_its_cap_is_an_error():
    with pytest.raises(RuntimeError, match="Invalid parameters"):
        _run(caps.NATURAL, "lattice", 2, tier="resident")


def test_default_backend_and_the_composition_on_the_device():
    lengths = (0, 70, caps.T + 3)
    pts, off = H.cloud(lengths, "randn").to(DEV), H.offsets_of(lengths)
    want = H.expected(lengths, "randn", 12)
    assert torch.equal(farthest_point_sampling(pts, off, 12).cpu(), want)
    assert torch.equal(farthest_point_sampling(pts, off, 12, backend="torch").cpu(), want)
    assert torch.equal(farthest_point_sampling(pts.to(torch.bfloat16), off, 12).cpu(),
                       H.reference_fps(pts.to(torch.bfloat16).float(), off, 12))


def test_point_pool_fps_equals_its_torch_backend(monkeypatch):
    from warpconvnet_amd.geometry.types.points import Points
    from warpconvnet_amd.nn.functional.point_pool import point_pool

    g = torch.Generator().manual_seed(3)
    lengths = (700, 1500)
    pc = Points([torch.rand(n, 3, generator=g) for n in lengths], [torch.randn(n, 8, generator=g) for n in lengths], device=DEV)
    assert sampling.GPU_DEFAULT_BACKEND == "hip"
    a = point_pool(pc, "max", downsample_max_num_points=64, sample_method="fps")
    monkeypatch.setattr(sampling, "GPU_DEFAULT_BACKEND", "torch")
    b = point_pool(pc, "max", downsample_max_num_points=64, sample_method="fps")
    assert a.coordinate_tensor.is_cuda and a.offsets.tolist() == b.offsets.tolist() == [0, 64, 128]
    assert torch.equal(a.coordinate_tensor, b.coordinate_tensor) and torch.equal(a.feature_tensor, b.feature_tensor)
