"""Generator of tests/golden/pad_layouts.npz: the reference's padded / patch layouts, ``bmm``, whole-scene attention and
PointNet run on the CPU.

    python tests/golden/make_pad_layouts_golden.py

Needs the reference tree on the authoring machine (see make_golden.py: import_reference); the tests read only the npz file.
Everything is the reference's code.  ``torch_scatter.segment_csr`` (a third-party package absent from this image, behind
PointNet's global max pool) is a plain per-segment reduction here, as in make_golden.py; the other stand-in is a placeholder
for the ``flash_attn`` package where a constructor merely checks that it was imported (state-dict layouts of
``enable_flash=True``) - no flash attention is run here.  Recorded, inputs from tests/pad_layouts_helper.py:

* offsets [0, 5, 5, 12, 13], rows [13, 3] in float32 / int64 / bool: ``cat_to_pad_tensor`` for pad_multiple None and 8 and the
  way back, ``CatPatchFeatures.from_cat`` (patch 4) with its offsets and ``to_cat``, ``clear_padding(-1)`` of both (float),
  ``PadFeatures.replace(pad_multiple=8)`` and ``list_to_pad_tensor``;
* ``bmm`` on the same offsets, in fp32 and fp64;
* ``Attention`` (flash disabled) on the padded batch of 0 / 17 / 70 points, dim 64, 2 and 4 heads, and
  ``SpatialFeatureAttention`` (flash disabled) with and without the coordinate encoding, parameters re-drawn by
  ``volt_helper.redraw``, each in fp32 and fp64;
* the state-dict keys and shapes of ``Attention`` (both ``use_batched_qkv``), ``SpatialFeatureAttention`` (``use_encoding``
  on / off) and ``PointNet`` (the four transform combinations);
* PointNet on 40 / 1 / 25 points in training and eval mode, in fp64 and in fp32 with 1, 4 and 16 CPU threads, and the largest
  fp32-to-fp64 difference over the three (the reference's fp32 result depends on the summation order of its GEMMs).
Arrays and names only - no reference source.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import import_reference  # noqa: E402
import pad_layouts_helper as H  # noqa: E402


def _segment_csr(src, indptr, out=None, reduce="sum"):
    rows = []
    for a, b in zip(indptr[:-1].tolist(), indptr[1:].tolist()):
        seg = src[a:b]
        rows.append({"sum": lambda t: t.sum(0), "mean": lambda t: t.mean(0), "max": lambda t: t.max(0).values,
                     "min": lambda t: t.min(0).values}[reduce](seg))
    return torch.stack(rows)


def main():
    import_reference()
    import torch_scatter
    import warpconvnet.ops.reductions as R

    torch_scatter.segment_csr = R.segment_csr = _segment_csr
    import warpconvnet.nn.modules.attention as ref_attn
    from warpconvnet.geometry.features.cat import CatFeatures
    from warpconvnet.geometry.features.ops.convert import cat_to_pad_tensor, pad_to_cat_tensor
    from warpconvnet.geometry.features.pad import PadFeatures
    from warpconvnet.geometry.features.patch import CatPatchFeatures
    from warpconvnet.geometry.types.points import Points
    from warpconvnet.geometry.utils.list_to_batch import list_to_pad_tensor
    from warpconvnet.models.pointnet import PointNet
    from warpconvnet.nn.functional.bmm import bmm

    out = {}
    offsets = torch.tensor(H.OFFSETS, dtype=torch.int32)
    out["offsets"] = offsets.numpy()

    # ---- layouts
    for kind in H.ROW_DTYPES:
        x = H.rows_of(kind)
        for pm in H.PAD_MULTIPLES:
            padded = cat_to_pad_tensor(x, offsets, pm)
            out[f"pad_{kind}_{pm}"] = padded.numpy()
            assert torch.equal(pad_to_cat_tensor(padded, offsets), x)
        patch = CatPatchFeatures.from_cat(CatFeatures(x, offsets), H.PATCH_SIZE)
        out[f"patch_{kind}"] = patch.batched_tensor.numpy()
        out["patch_offsets"] = patch.patch_offsets.numpy()
        assert torch.equal(patch.to_cat().batched_tensor, x)
    x = H.rows_of("float")
    pf = PadFeatures(cat_to_pad_tensor(x, offsets, 8) + 100.0, offsets, 8)
    out["pad_cleared"] = pf.clear_padding(-1.0).batched_tensor.numpy()
    patch = CatPatchFeatures.from_cat(CatFeatures(x, offsets), H.PATCH_SIZE)
    patch.batched_tensor += 100.0
    out["patch_cleared"] = patch.clear_padding(-1.0).batched_tensor.numpy()
    out["pad_replaced"] = PadFeatures(cat_to_pad_tensor(x, offsets), offsets).replace(pad_multiple=8).batched_tensor.numpy()
    lp, lo, _ = list_to_pad_tensor([x[H.OFFSETS[i]:H.OFFSETS[i + 1]] for i in range(len(H.OFFSETS) - 1)], 8)
    out["list_pad"], out["list_offsets"] = lp.numpy(), lo.numpy()

    # ---- bmm
    for name, dtype in (("f32", torch.float32), ("f64", torch.float64)):
        xb, wb = H.bmm_operands(dtype)
        pc = Points(torch.zeros(H.OFFSETS[-1], 3), xb, offsets=offsets)
        out[f"bmm_{name}"] = bmm(pc, wb).feature_tensor.numpy()

    # ---- attention (flash disabled: the reference's masked softmax)
    coords, feats, aoff = H.attention_inputs()
    sums = {}
    for heads in H.ATTN_HEADS:
        for name, dtype in (("f32", torch.float32), ("f64", torch.float64)):
            att = ref_attn.Attention(H.ATTN_DIM, heads, qkv_bias=True, enable_flash=False).to(dtype).eval()
            sums[f"attn{heads}"] = H.redraw(att)
            pc = Points(coords.to(dtype), feats.to(dtype), offsets=aoff)
            with torch.no_grad():
                padded = cat_to_pad_tensor(pc.feature_tensor, aoff)
                mask = ref_attn.offset_to_mask(padded, aoff, padded.shape[1])
                out[f"attn{heads}_{name}"] = att(padded, None, mask, aoff.diff()).numpy()
                if name == "f32" and heads == H.ATTN_HEADS[0]:
                    out["attn_mask"] = mask.numpy()
                    out["attn_zeroed"] = ref_attn.zero_out_points(padded.clone() + 1.0, aoff.diff()).numpy()
                for enc in (False, True):
                    sfa = ref_attn.SpatialFeatureAttention(H.ATTN_DIM, heads, use_encoding=enc, num_encoding_channels=8,
                                                           encoding_range=1.0, enable_flash=False).to(dtype).eval()
                    sums[f"sfa{heads}_{int(enc)}"] = H.redraw(sfa)
                    out[f"sfa{heads}_{int(enc)}_{name}"] = sfa(pc).feature_tensor.numpy()

    # ---- state-dict layouts
    layouts = {}
    ref_attn.flash_attn = object()  # the constructor only asserts that the package was imported
    for batched in (True, False):
        for flash in (True, False):
            layouts[f"attention_batched{int(batched)}_flash{int(flash)}"] = H.layout_of(
                ref_attn.Attention(H.ATTN_DIM, 4, qkv_bias=True, enable_flash=flash, use_batched_qkv=batched))
    for enc in (True, False):
        layouts[f"sfa_encoding{int(enc)}"] = H.layout_of(
            ref_attn.SpatialFeatureAttention(H.ATTN_DIM, 4, use_encoding=enc, num_encoding_channels=8, encoding_range=1.0))
    for it, ft in H.TRANSFORMS:
        layouts[f"pointnet_{int(it)}{int(ft)}"] = H.layout_of(PointNet(**H.POINTNET, input_transform=it, feature_transform=ft))
    out["state_layouts"] = np.asarray(json.dumps(layouts))

    # ---- PointNet
    # the fp32 result depends on the summation order of the CPU GEMMs, i.e. on the thread count (pad_layouts_helper.py:
    # pointnet_inputs); the recorded gap is the largest the reference shows over POINTNET_THREADS
    pcoords, pfeats = H.pointnet_inputs()
    threads = torch.get_num_threads()
    for mode in ("train", "eval"):
        def run(dtype):
            model = PointNet(**H.POINTNET).to(dtype)
            sums["pointnet"] = H.redraw(model)
            model.train(mode == "train")
            pc = Points([c.to(dtype) for c in pcoords], [f.to(dtype) for f in pfeats])
            with torch.no_grad():
                return model(pc).double()

        f64 = run(torch.float64)
        gaps = []
        for t in H.POINTNET_THREADS:
            torch.set_num_threads(t)
            f32 = run(torch.float32)
            gaps.append(float((f32 - f64).abs().max()))
        torch.set_num_threads(threads)
        out[f"pointnet_{mode}_f32"], out[f"pointnet_{mode}_f64"] = f32.float().numpy(), f64.numpy()
        out[f"pointnet_{mode}_gaps"] = np.asarray(gaps)
        out[f"pointnet_{mode}_gap"] = np.asarray(max(gaps))
    out["param_sums"] = np.asarray(json.dumps({k: sorted(v.items()) for k, v in sums.items()}))

    path = os.path.join(HERE, "pad_layouts.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; pointnet gaps", float(out["pointnet_train_gap"]), float(out["pointnet_eval_gap"]),
          "max |out|", float(np.abs(out["pointnet_train_f64"]).max()))


if __name__ == "__main__":
    main()
