"""Shared by the bilateral-solver tests: the golden file (tests/golden/make_bilateral_solver_golden.py) and its cases."""
import os

import numpy as np
import torch

from tests.conftest import GOLDEN
from tests.lattice_filter_helper import golden as lattice_golden
from tests.lattice_filter_helper import t

SOLVER_PARAMS = ((128.0, 1e-5, 25), (4.0, 0.0, 8), (1.0, 1e-3, 25))  # (lam, tol, max_iters), as the generator's
DENSE_DIMS = (2, 3, 5, 6)   # tag sd<d>: bistochastize=True
SPARSE_DIMS = (2, 3, 5, 6)  # tag ss<d>: bistochastize=False, the lattice golden's positions
SOLVER_TAGS = [f"sd{d}" for d in DENSE_DIMS] + [f"ss{d}" for d in SPARSE_DIMS]
KNN_SIGMAS = ((0.05, 20.0), (0.2, 60.0), (0.02, 5.0))
KNN_K = 16
LABEL_SIGMAS = (0.1, 60.0)
_CACHE = {}


def golden():
    """tests/golden/bilateral_solver.npz, loaded once and left unchanged."""
    if "g" not in _CACHE:
        with np.load(os.path.join(GOLDEN, "bilateral_solver.npz")) as z:
            _CACHE["g"] = {k: z[k] for k in z.files}
    return _CACHE["g"]


def solver_inputs(tag, device="cpu", dtype=torch.float32):
    """(positions, target, confidence, bistochastize) of a solver case."""
    g = golden()
    pos = g[f"{tag}_pos"] if tag.startswith("sd") else lattice_golden()[f"d{tag[2:]}_pos"]
    return (t(pos, device).to(dtype), t(g[f"{tag}_target"], device).to(dtype), t(g[f"{tag}_conf"], device).to(dtype),
            tag.startswith("sd"))


def knn_inputs(name, device="cpu", dtype=torch.float32):
    """(src_xyz, src_feat, src_value, query_xyz, query_feat, g) of the self-filter or the query case."""
    g = golden()
    src = [t(g[k], device).to(dtype) for k in ("knn_xyz", "knn_rgb", "knn_val")]
    query = [None, None] if name == "self" else [t(g[k], device).to(dtype) for k in ("knn_qxyz", "knn_qrgb")]
    return (*src, *query, t(g[f"knn_g_{name}"], device).to(dtype))
