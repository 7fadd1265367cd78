"""Cases and the yardstick of the flexible-dual-grid extractor.

`brute` is written against the definition alone: a Python dictionary from (batch, x, y, z) to the row for the neighbour
lookup, a loop over (row, axis) for the order, and numpy fp32 array operations - one numpy call per operation of the
definition, so every operation is rounded once and nothing is contracted - for the vertices and the split.  It shares no code
with `warpconvnet_amd.nn.functional.dual_grid`; the three tables are typed in again from the definition.
"""
import functools

import numpy as np
import torch

F32 = np.float32
DEFAULT_AABB = ((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5))

# the definition's tables, typed from DESIGN.md 4.28
AROUND = {
    0: ((0, 0, 0), (0, 0, 1), (0, 1, 1), (0, 1, 0)),
    1: ((0, 0, 0), (1, 0, 0), (1, 0, 1), (0, 0, 1)),
    2: ((0, 0, 0), (0, 1, 0), (1, 1, 0), (1, 0, 0)),
}
TRI_1 = ((0, 1, 2), (0, 2, 3))
TRI_2 = ((0, 1, 3), (3, 1, 2))


# ---- yardstick -------------------------------------------------------------------------------------------------------------
def _cross(u, v):
    return np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2],
                     u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], 1)


def _normal(a, b, c):
    return _cross(b - a, c - a)


def _align(m, n):
    return np.abs((m[:, 0] * n[:, 0] + m[:, 1] * n[:, 1]) + m[:, 2] * n[:, 2])


def brute(coords, offsets, flags, dual32, weight32, grid_size, aabb=DEFAULT_AABB):
    """dict(vertices fp32 [N, 3], quads int32 [L, 4] local, faces int32 [2L, 3] local, quad_offsets int32 [B + 1], split1 bool
    [L], flagged = number of set flags)."""
    coords = np.asarray(coords, np.int64).reshape(-1, 3)
    n, B = len(coords), len(offsets) - 1
    scene = np.zeros(n, np.int64)
    for b in range(B):
        scene[offsets[b]:offsets[b + 1]] = b
    voxel = F32((float(aabb[1][0]) - float(aabb[0][0])) / grid_size)
    low = np.asarray([F32(v) for v in aabb[0]], F32)
    verts = coords.astype(F32) + np.asarray(dual32, F32).reshape(-1, 3)
    verts = verts * voxel
    verts = verts + low
    assert verts.dtype == F32
    where = {}
    for r in range(n):
        where.setdefault((int(scene[r]), *map(int, coords[r])), r)
    quads, owner = [], []
    for r in range(n):
        for a in range(3):
            if not flags[r][a]:
                continue
            q = [r]
            for d in AROUND[a][1:]:
                q.append(where.get((int(scene[r]), int(coords[r][0]) + d[0], int(coords[r][1]) + d[1], int(coords[r][2]) + d[2]), -1))
            if min(q) >= 0:
                quads.append(q)
                owner.append(int(scene[r]))
    q = np.asarray(quads, np.int64).reshape(-1, 4)
    owner = np.asarray(owner, np.int64)
    if weight32 is not None:
        w = np.asarray(weight32, F32).reshape(-1)[q]
        split1 = w[:, 0] * w[:, 2] > w[:, 1] * w[:, 3]
    else:
        p = [verts[q[:, i]] for i in range(4)]
        split1 = _align(_normal(p[0], p[1], p[2]), _normal(p[0], p[2], p[3])) > _align(_normal(p[0], p[1], p[3]),
                                                                                     _normal(p[3], p[1], p[2]))
    local = q - np.asarray(offsets, np.int64)[owner][:, None]
    tri = np.where(split1[:, None], local[:, np.asarray(TRI_1).reshape(-1)], local[:, np.asarray(TRI_2).reshape(-1)])
    counts = np.bincount(owner, minlength=B)
    return {
        "vertices": verts, "quads": local.astype(np.int32), "faces": tri.reshape(-1, 3).astype(np.int32),
        "quad_offsets": np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), "split1": split1,
        "flagged": int(np.asarray(flags).sum()),
    }


def closed_surface(faces, num_quads):
    """Every mesh edge in exactly two faces and V - E + F = 2 over the referenced vertices."""
    edges = {}
    for f in np.asarray(faces).tolist():
        for i in range(3):
            e = (min(f[i], f[(i + 1) % 3]), max(f[i], f[(i + 1) % 3]))
            edges[e] = edges.get(e, 0) + 1
    assert len(faces) == 2 * num_quads
    assert set(edges.values()) == {2}, f"edge multiplicities {sorted(set(edges.values()))}"
    v = len(set(np.asarray(faces).reshape(-1).tolist()))
    assert v - len(edges) + len(faces) == 2, (v, len(edges), len(faces))


# ---- cases -----------------------------------------------------------------------------------------------------------------
def shell_coords():
    """8^3 grid, voxels with 2.0 <= |c + 0.5 - 4| < 3.5: 128 voxels."""
    g = np.stack(np.meshgrid(*[np.arange(8)] * 3, indexing="ij"), -1).reshape(-1, 3)
    r = np.linalg.norm(g + 0.5 - 4.0, axis=1)
    c = g[(r >= 2.0) & (r < 3.5)].astype(np.int32)
    assert len(c) == 128
    return c


def shell_flags(c):
    """Strict sign change of |p - 4| - 2.75 between the end points of the owned edge (c + 1 - e_a to c + 1)."""
    f = np.zeros((len(c), 3), bool)
    hi = np.linalg.norm(c + 1.0 - 4.0, axis=1) - 2.75
    for a in range(3):
        e = np.zeros(3)
        e[a] = 1.0
        lo = np.linalg.norm(c + 1.0 - e - 4.0, axis=1) - 2.75
        f[:, a] = lo * hi < 0
    return f


def _case(scenes, flags, dual=None, weight=None, dtype=torch.float32, grid_size=8, aabb=DEFAULT_AABB, seed=0, shuffle=True):
    """scenes: list of [N_b, 3] coordinate arrays; flags: "true" | "random" | "all" | "none"; dual: None (0.5) | "random";
    weight: None | "ties" | "random".  Rows of every scene are shuffled."""
    rng = np.random.default_rng(seed)
    scenes = [np.asarray(s, np.int32).reshape(-1, 3) for s in scenes]
    if shuffle:
        scenes = [s[rng.permutation(len(s))] for s in scenes]
    coords = np.concatenate(scenes, 0) if scenes else np.zeros((0, 3), np.int32)
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in scenes])]).astype(np.int32)
    n = len(coords)
    if flags == "true":
        fl = shell_flags(coords)
    elif flags == "random":
        fl = rng.random((n, 3)) < 0.5
    else:
        fl = np.full((n, 3), flags == "all")
    d = np.full((n, 3), 0.5) if dual is None else rng.uniform(-0.5, 1.5, (n, 3))
    d = torch.from_numpy(d).to(dtype)
    w = None
    if weight == "ties":
        w = torch.from_numpy(rng.choice([0.5, 1.0, 2.0], (n, 1))).to(dtype)
    elif weight == "random":
        w = torch.from_numpy(rng.uniform(0.25, 4.0, (n, 1))).to(dtype)
    return {"coords": torch.from_numpy(coords), "offsets": torch.from_numpy(offsets), "flags": torch.from_numpy(fl), "dual": d,
            "weight": w, "grid_size": grid_size, "aabb": aabb}


def _block(k, origin=(0, 0, 0)):
    return np.stack(np.meshgrid(*[np.arange(k)] * 3, indexing="ij"), -1).reshape(-1, 3) + np.asarray(origin)


def _rows(count, seed):
    """`count` voxels of a 7^3 block (343 >= 257)."""
    return _block(7)[np.random.default_rng(seed).permutation(343)[:count]]


def _holed():
    b = _block(4)
    return b[~(b == 2).all(1)]  # (2, 2, 2) is missing


def _wide(seed):
    """Voxel pairs, triples and 2^3 cells spread over a 1024^3 grid: coordinates up to 1023."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 1022, (60, 3))
    cells = np.concatenate([_block(2, o) for o in base] + [np.asarray([[1023, 1023, 1023], [1022, 1022, 1022]])])
    return np.unique(cells, axis=0)


CASES = {
    "shell": lambda: _case([shell_coords()], "true"),
    "shell_random_flags": lambda: _case([shell_coords()], "random", seed=1),
    "shell_negative": lambda: _case([shell_coords() - 37], "random", seed=2, dual="random"),
    "three_scenes_middle_empty": lambda: _case([shell_coords(), np.zeros((0, 3)), shell_coords() + 3], "random", seed=3),
    # scene 1 owns the voxel scene 0 lacks: a quad across the scenes would close the hole
    "hole_filled_by_other_scene": lambda: _case([_holed(), np.concatenate([[[2, 2, 2]], _block(2, (5, 5, 5))])], "all", seed=4),
    "rows_255": lambda: _case([_rows(255, 5)], "random", seed=5, dual="random"),
    "rows_256": lambda: _case([_rows(256, 6)], "random", seed=6, dual="random"),
    "rows_257": lambda: _case([_rows(257, 7)], "random", seed=7, dual="random"),
    "dense_40": lambda: _case([_block(40)], "all", seed=8, grid_size=64, shuffle=False),
    # 65 728 rows = 257 tiles: the tile scan takes a second trip, and a scene boundary falls inside a tile
    "dense_40_and_12": lambda: _case([_block(40), _block(12)], "all", seed=9, grid_size=64, shuffle=False),
    "no_flags": lambda: _case([shell_coords()], "none"),
    "empty": lambda: _case([np.zeros((0, 3))], "none"),
    "split_all_ties": lambda: _case([_block(5)], "all", seed=10),
    "split_geometric": lambda: _case([_block(6)], "random", seed=11, dual="random"),
    "split_weight_ties": lambda: _case([_block(6)], "random", seed=12, dual="random", weight="ties"),
    "split_weight_random": lambda: _case([_block(6)], "all", seed=13, weight="random"),
    "f16": lambda: _case([_block(6)], "random", seed=14, dual="random", weight="ties", dtype=torch.float16),
    "bf16": lambda: _case([_block(6)], "random", seed=15, dual="random", weight="ties", dtype=torch.bfloat16),
    "f16_geometric": lambda: _case([_block(6)], "random", seed=16, dual="random", dtype=torch.float16),
    "bf16_geometric": lambda: _case([_block(6)], "random", seed=17, dual="random", dtype=torch.bfloat16),
    # a voxel size that is no power of two and a box off the origin: a product fused into the sum behind it (FMA) changes bits
    "odd_box_geometric": lambda: _case([_block(6, (-2, 3, 40))], "random", seed=19, dual="random", grid_size=334,
                                       aabb=((-0.3, -0.7, 0.1), (0.7, 0.3, 1.1))),
    "odd_box_weights": lambda: _case([_block(6), _block(5, (7, 0, 1))], "random", seed=20, dual="random", weight="random",
                                     grid_size=97, aabb=((-0.3, -0.7, 0.1), (0.7, 0.3, 1.1))),
    "odd_box_bf16": lambda: _case([_block(6)], "random", seed=21, dual="random", dtype=torch.bfloat16, grid_size=334),
    "grid_1024": lambda: _case([_wide(18)], "all", seed=18, dual="random", grid_size=1024),
}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def expected(name):
    c = case(name)
    return brute(c["coords"].numpy(), c["offsets"].numpy(), c["flags"].numpy(), c["dual"].float().numpy(),
                 None if c["weight"] is None else c["weight"].float().numpy(), c["grid_size"], c["aabb"])


def check_bitwise(name, vertices, faces, face_offsets, quads=None, quad_offsets=None):
    """The outputs of an extraction of case `name` (torch tensors on any device) against the yardstick, bit for bit."""
    want = expected(name)
    got_v = vertices.detach().cpu().numpy()
    assert got_v.dtype == F32 and got_v.shape == want["vertices"].shape
    assert np.array_equal(got_v.view(np.uint32), want["vertices"].view(np.uint32)), "vertices differ"
    assert faces.dtype == torch.int32 and np.array_equal(faces.cpu().numpy().reshape(-1, 3), want["faces"]), "faces differ"
    assert np.array_equal(np.asarray(face_offsets.cpu()), 2 * want["quad_offsets"]), "face offsets differ"
    if quads is not None:
        assert quads.dtype == torch.int32 and np.array_equal(quads.cpu().numpy().reshape(-1, 4), want["quads"]), "quads differ"
        assert np.array_equal(np.asarray(quad_offsets.cpu()), want["quad_offsets"]), "quad offsets differ"
