"""Generator of tests/golden/bilateral_solver.npz: the reference's fast bilateral solver, kNN bilateral filter and label
propagation run on the CPU.

    python -O tests/golden/make_bilateral_solver_golden.py

Needs the reference tree on the authoring machine (see make_golden.py: import_reference) and tests/golden/lattice_filter.npz
(the sparse solver cases reuse its positions); the tests read only the .npz files.  ``-O`` switches off the reference's
``is_cuda`` assertions; its ``PackedHashTable128`` is replaced by the dictionary of make_lattice_filter_golden.py and its CUDA
kNN by ``cdist`` + ``topk``.  Only arrays are written, with fixed zip time stamps: a second run gives the same bytes.

Inputs are fp32 values.  Every result is the reference's float64 run on them (``y64``); beside it ``err32 = max|y32 - y64|``
of the reference's own float32 run, the yardstick of an fp32 implementation.  Asserted for every case written: the fp32 and
the fp64 grid have the same ``unique_keys`` and ``inverse``, and ``err32 <= 1e-4 max|y64|`` (a badly conditioned case cannot
slip in: sparse cells with bistochastization are such cases and are left out on purpose - there the reference's two precisions
disagree by O(1) at d = 2 and the fp32 run is NaN at d = 6).  In the dense cases at d <= 3 the Sinkhorn vectors drift to
m ~ 1e7 .. 1e12 and n ~ 1e-8 .. 1e-14; that is the reference's behaviour and is recorded as it is.
"""
import io
import os
import sys
import types
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference  # noqa: E402
from make_lattice_filter_golden import DictTable  # noqa: E402

SOLVER_PARAMS = ((128.0, 1e-5, 25), (4.0, 0.0, 8), (1.0, 1e-3, 25))  # (lam, tol, max_iters)
DENSE = ((2, 600, 1.0), (3, 1200, 0.8), (5, 1500, 0.45), (6, 1500, 0.4))  # (d, N, s): positions uniform in [0, 4 s)^d
SPARSE_DIMS = (2, 3, 5, 6)  # the lattice golden's positions: N = 300, standard normal * 2
CHANNELS = 3
KNN_SIGMAS = ((0.05, 20.0), (0.2, 60.0), (0.02, 5.0))
KNN_N, KNN_QUERIES, KNN_VALUES, KNN_K = 500, 64, 5, 16
LABEL_SRC, LABEL_DST, LABEL_CLASSES, LABEL_SIGMAS = 200, 100, 4, (0.1, 60.0)
RELATIVE_ERR32 = 1e-4


def knn_cdist(ref_positions, query_positions, k, search_method="chunk", chunk_size=32768):
    return torch.topk(torch.cdist(query_positions, ref_positions), k, dim=1, largest=False).indices


def solver_cases(out, ref_grid):
    sparse = np.load(os.path.join(HERE, "lattice_filter.npz"))
    cases = [(f"sd{d}", d, n, True, None, s) for d, n, s in DENSE] + [(f"ss{d}", d, 300, False, sparse[f"d{d}_pos"], 0) for d in SPARSE_DIMS]
    for tag, d, n, bisto, pos, s in cases:
        rng = np.random.default_rng(100 + d + (50 if bisto else 0))
        if pos is None:
            pos = rng.uniform(0.0, 4.0 * s, size=(n, d)).astype(np.float32)
            out[f"{tag}_pos"] = pos
        target = rng.standard_normal((n, CHANNELS)).astype(np.float32)
        conf = rng.uniform(0.1, 1.0, size=n).astype(np.float32)
        out[f"{tag}_target"], out[f"{tag}_conf"] = target, conf
        p32 = torch.from_numpy(pos)
        g32, g64 = ref_grid.BilateralGrid.build(p32), ref_grid.BilateralGrid.build(p32.double())
        assert torch.equal(g32.unique_keys, g64.unique_keys) and torch.equal(g32.inverse, g64.inverse), tag
        t32, c32 = torch.from_numpy(target), torch.from_numpy(conf)
        for j, (lam, tol, iters) in enumerate(SOLVER_PARAMS):
            kw = dict(lam=lam, tol=tol, max_iters=iters, bistochastize=bisto)
            y64 = ref_grid.bilateral_solver(g64, t32.double(), c32.double(), **kw)
            y32 = ref_grid.bilateral_solver(g32, t32, c32, **kw)
            err32 = float((y32.double() - y64).abs().max())
            scale = float(y64.abs().max())
            assert np.isfinite(err32) and err32 <= RELATIVE_ERR32 * scale, (tag, j, err32, scale)
            out[f"{tag}_y64_{j}"] = y64.numpy()
            out[f"{tag}_err32_{j}"] = np.float64(err32)
            print(f"{tag} V={g32.num_vertices} lam={lam} tol={tol} iters={iters}: err32 {err32:.2e}, max|y64| {scale:.2e}")


def knn_cases(out, ref_bilateral):
    rng = np.random.default_rng(7)
    xyz = rng.uniform(0, 1, size=(KNN_N, 3)).astype(np.float32)
    rgb = rng.uniform(0, 255, size=(KNN_N, 3)).astype(np.float32)
    val = rng.standard_normal((KNN_N, KNN_VALUES)).astype(np.float32)
    qxyz = rng.uniform(0, 1, size=(KNN_QUERIES, 3)).astype(np.float32)
    qrgb = rng.uniform(0, 255, size=(KNN_QUERIES, 3)).astype(np.float32)
    g_self = rng.integers(-3, 4, size=(KNN_N, KNN_VALUES)).astype(np.float32)
    g_query = rng.integers(-3, 4, size=(KNN_QUERIES, KNN_VALUES)).astype(np.float32)
    out.update(knn_xyz=xyz, knn_rgb=rgb, knn_val=val, knn_qxyz=qxyz, knn_qrgb=qrgb, knn_g_self=g_self, knn_g_query=g_query)
    t = torch.from_numpy
    for name, q, qf, g in (("self", None, None, g_self), ("query", qxyz, qrgb, g_query)):
        nbr = knn_cdist(t(xyz).double(), t(xyz if q is None else q).double(), KNN_K)
        assert torch.equal(nbr.sort(1).values, knn_cdist(t(xyz), t(xyz if q is None else q), KNN_K).sort(1).values), name
        out[f"knn_{name}_nbr"] = nbr.sort(1).values.numpy().astype(np.int16)
        for j, (sx, sf) in enumerate(KNN_SIGMAS):
            def run(dtype, grad):
                v = t(val).to(dtype).requires_grad_(grad)
                args = [t(xyz).to(dtype), t(rgb).to(dtype), v] + ([] if q is None else [t(q).to(dtype), t(qf).to(dtype)])
                return v, ref_bilateral.bilateral_filter(*args, sigma_xyz=sx, sigma_feat=sf, k=KNN_K)
            v64, y64 = run(torch.float64, True)
            (y64 * t(g).double()).sum().backward()
            _, y32 = run(torch.float32, False)
            err32 = float((y32.double() - y64.detach()).abs().max())
            assert err32 <= RELATIVE_ERR32 * float(y64.abs().max()), (name, j, err32)
            out[f"knn_{name}_y64_{j}"] = y64.detach().numpy()
            out[f"knn_{name}_grad64_{j}"] = v64.grad.numpy()
            out[f"knn_{name}_err32_{j}"] = np.float64(err32)
            print(f"knn {name} sigma=({sx}, {sf}): err32 {err32:.2e}")


def label_case(out, ref_bilateral):
    rng = np.random.default_rng(11)
    xyz = rng.uniform(0, 1, size=(LABEL_SRC, 3)).astype(np.float32)
    rgb = rng.uniform(0, 255, size=(LABEL_SRC, 3)).astype(np.float32)
    labels = rng.integers(-1, LABEL_CLASSES, size=LABEL_SRC).astype(np.int64)  # -1: background
    dxyz = rng.uniform(0, 1, size=(LABEL_DST, 3)).astype(np.float32)
    drgb = rng.uniform(0, 255, size=(LABEL_DST, 3)).astype(np.float32)
    assert (labels == -1).any() and labels.max() == LABEL_CLASSES - 1
    t = torch.from_numpy
    sx, sf = LABEL_SIGMAS
    kw = dict(sigma_xyz=sx, sigma_feat=sf, k=KNN_K)
    got = ref_bilateral.bilateral_label_propagate(t(xyz).double(), t(rgb).double(), t(labels), t(dxyz).double(), t(drgb).double(), **kw)
    got32 = ref_bilateral.bilateral_label_propagate(t(xyz), t(rgb), t(labels), t(dxyz), t(drgb), **kw)
    assert torch.equal(got, got32)
    # the vote is decided by a margin no fp32 rounding can bridge
    onehot = torch.zeros(LABEL_SRC, LABEL_CLASSES, dtype=torch.float64)
    onehot[t(labels) >= 0, t(labels)[t(labels) >= 0]] = 1.0
    soft = ref_bilateral.bilateral_filter(t(xyz).double(), t(rgb).double(), onehot, t(dxyz).double(), t(drgb).double(), **kw)
    top = soft.topk(2, dim=1).values
    assert float((top[:, 0] - top[:, 1]).min()) > 1e-3 and float(top[:, 0].min()) > 1e-3
    out.update(label_xyz=xyz, label_rgb=rgb, label_src=labels.astype(np.int8), label_dxyz=dxyz, label_drgb=drgb,
               label_out=got.numpy().astype(np.int64))
    print("labels:", np.bincount(got.numpy() + 1, minlength=LABEL_CLASSES + 1))


def save(path, arrays):
    """np.savez_compressed with fixed time stamps."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def main():
    if __debug__:
        sys.exit("run with python -O: the reference asserts CUDA tensors")
    import_reference()
    knn = types.ModuleType("warpconvnet.geometry.coords.search.knn")
    knn.knn_search = knn_cdist
    sys.modules["warpconvnet.geometry.coords.search.knn"] = knn
    from warpconvnet.nn.functional import bilateral as ref_bilateral
    from warpconvnet.nn.functional import bilateral_grid as ref_grid

    ref_grid.PackedHashTable128 = DictTable
    torch.manual_seed(0)
    out = {}
    solver_cases(out, ref_grid)
    knn_cases(out, ref_bilateral)
    label_case(out, ref_bilateral)
    path = os.path.join(HERE, "bilateral_solver.npz")
    save(path, out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
