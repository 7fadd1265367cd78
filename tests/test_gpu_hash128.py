"""GPU: PackedHashTable128 (csrc/lattice.hip) - round trips, misses, the key range, a full table, batched search, and the
second trip of the capped insert / search grids."""
import pytest
import torch

from tests.lattice_caps import POINTS_SECOND_TRIP

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _table():
    from warpconvnet_amd.geometry.coords.search.packed128_hashmap import PackedHashTable128

    return PackedHashTable128


def distinct_keys(n, key_dim, seed, low=-3000, high=3000):
    gen = torch.Generator().manual_seed(seed)
    keys = torch.unique(torch.randint(low, high, (int(n * 1.2) + 8, key_dim), generator=gen, dtype=torch.int32), dim=0)
    keys = keys[torch.randperm(keys.shape[0], generator=gen)][:n]
    assert keys.shape[0] == n
    return keys.to(DEV)


@pytest.mark.parametrize("key_dim", [2, 4, 7])
@pytest.mark.parametrize("n", [1000, 200_000])
def test_round_trip_and_misses(n, key_dim):
    T = _table()
    keys = distinct_keys(n, key_dim, seed=n + key_dim)
    assert bool((keys < 0).any()) and bool((keys > 0).any())
    table = T.from_keys(keys)
    assert table.key_dim == key_dim and table.num_entries == n and table.capacity >= 2 * n
    assert table.capacity & (table.capacity - 1) == 0
    found = table.search(keys)
    assert found.dtype == torch.int32 and torch.equal(found.long(), torch.arange(n, device=DEV))
    absent = keys.clone()
    absent[:, -1] += 10_000  # outside the drawn range, inside the key range
    assert bool((table.search(absent) == -1).all())


def test_bounds_of_the_key_range():
    T = _table()
    assert (T.DIM, T.COORD_BITS, T.COORD_MIN, T.COORD_MAX, T.MAX_BATCHED_K) == (7, 17, -65536, 65535, 32)
    edge = torch.tensor([[-65536, 65535, 0, 0, 0, 0, -65536], [65535, -65536, 1, 2, 3, 4, 65535], [0, 0, 0, 0, 0, 0, 0]],
                        dtype=torch.int32, device=DEV)
    table = T.from_keys(edge)
    assert table.search(edge).tolist() == [0, 1, 2]
    for bad in (65536, -65537):
        keys = edge.clone()
        keys[1, 3] = bad
        with pytest.raises(ValueError):
            T.from_keys(keys)
        assert table.search(keys).tolist() == [0, -1, 2]  # outside the range: a miss


def test_full_table_and_empty_input():
    T = _table()
    keys = distinct_keys(1000, 3, seed=5)
    with pytest.raises(RuntimeError):
        T.from_keys(keys, capacity=100)
    exact = T.from_keys(keys[:128], capacity=128)  # every slot taken: probes wrap around
    assert torch.equal(exact.search(keys[:128]).long(), torch.arange(128, device=DEV))
    assert bool((exact.search(keys[128:]) == -1).all())
    empty = T.from_keys(torch.zeros((0, 4), dtype=torch.int32, device=DEV))
    assert empty.num_entries == 0 and empty.capacity == 16
    assert empty.search(keys[:0].new_zeros((0, 4))).shape == (0,)
    assert empty.search(torch.ones((5, 4), dtype=torch.int32, device=DEV)).tolist() == [-1] * 5
    with pytest.raises(ValueError):
        T(16, DEV, key_dim=8)
    with pytest.raises(ValueError):
        T.from_keys(keys, key_dim=4)


@pytest.mark.parametrize("key_dim", [2, 7])
@pytest.mark.parametrize("k", [1, 14, 32])
def test_batched_search_equals_a_loop_of_searches(k, key_dim):
    T = _table()
    keys = distinct_keys(5000, key_dim, seed=k, low=-6, high=6) if key_dim == 7 else distinct_keys(5000, key_dim, seed=k, low=-100, high=100)
    table = T.from_keys(keys)
    gen = torch.Generator().manual_seed(k)
    offsets = torch.randint(-2, 3, (k, key_dim), generator=gen, dtype=torch.int32)
    offsets[0] = 0
    offsets = offsets.to(DEV)
    got = table.batched_search(keys, offsets)
    assert got.shape == (k, 5000) and got.dtype == torch.int32
    want = torch.stack([table.search(keys + o) for o in offsets])
    assert torch.equal(got, want) and bool((got >= 0).any()) and (k == 1 or bool((got < 0).any()))  # k = 1: the zero offset alone
    assert table.batched_search(keys[:0], offsets).shape == (k, 0)


def test_batched_search_rejects_more_than_32_offsets():
    T = _table()
    keys = distinct_keys(100, 3, seed=1)
    table = T.from_keys(keys)
    with pytest.raises(ValueError):
        table.batched_search(keys, torch.zeros((33, 3), dtype=torch.int32, device=DEV))


def test_second_trip_of_insert_and_search():
    """More keys than kRowMaxGrid * kRowThreads: the striding threads insert and look up a second key each."""
    T = _table()
    n = POINTS_SECOND_TRIP + 1000
    i = torch.arange(n, device=DEV)
    keys = torch.stack([i // 2048 - 300, i % 2048 - 1024], dim=1).to(torch.int32)
    table = T.from_keys(keys)
    assert torch.equal(table.search(keys).long(), i)
    both = table.batched_search(keys, torch.tensor([[0, 0], [0, 5000]], dtype=torch.int32, device=DEV))
    assert torch.equal(both[0].long(), i) and bool((both[1] == -1).all())
