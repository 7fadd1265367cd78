"""Generate tests/golden/dgcnn.json by IMPORTING THE REFERENCE (authoring container only):

    python tests/golden/make_dgcnn_golden.py

The reference's DGCNN(3, 10, knn_ks=4, emb_dims=32) is built on the CPU with the stubs of make_golden.py.  Recorded: the
names and shapes of its state dict, and - with the closed-form parameters and the input of tests/dgcnn_helper.py - its
eval-mode and train-mode logits (dropout 0, so that train mode is a function of the input alone) in fp32, and how far
the fp32 logits are from the same model run in fp64.  Only data is written - no reference source."""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from make_golden import import_reference  # noqa: E402
from dgcnn_helper import CONFIG, cloud_input, fill_closed_form  # noqa: E402


def main():
    import_reference()
    import torch_scatter

    def segment_csr(src, indptr, reduce="sum"):
        rows = []
        for i in range(indptr.numel() - 1):
            seg = src[int(indptr[i]): int(indptr[i + 1])]
            rows.append({"sum": lambda t: t.sum(0), "mean": lambda t: t.mean(0), "max": lambda t: t.max(0).values,
                         "min": lambda t: t.min(0).values}[reduce](seg))
        return torch.stack(rows)

    torch_scatter.segment_csr = segment_csr
    import warpconvnet.ops.reductions as R

    R.segment_csr = segment_csr
    from warpconvnet.geometry.types.points import Points
    from warpconvnet.models.dgcnn import DGCNN

    out = {"config": CONFIG}
    model = DGCNN(**CONFIG)
    out["state_dict"] = {k: list(v.shape) for k, v in model.state_dict().items()}

    def run(dtype, train):
        m = DGCNN(**CONFIG, dropout=0.0).to(dtype)
        fill_closed_form(m)
        m.train(train)
        coords, offsets = cloud_input(dtype)
        with torch.no_grad():
            return m(Points(coords, coords.clone(), offsets=offsets)).double()

    for mode, train in (("eval", False), ("train", True)):
        y32, y64 = run(torch.float32, train), run(torch.float64, train)
        out[f"{mode}_logits"] = y32.tolist()
        out[f"{mode}_logits_fp64"] = y64.tolist()
        out[f"{mode}_fp32_vs_fp64"] = float((y32 - y64).abs().max())
        print(mode, "max |logit|", float(y64.abs().max()), "fp32 vs fp64", out[f"{mode}_fp32_vs_fp64"])
    with open(os.path.join(HERE, "dgcnn.json"), "w") as f:
        json.dump(out, f, indent=1)
    print("dgcnn.json", len(out["state_dict"]), "entries")


if __name__ == "__main__":
    main()
