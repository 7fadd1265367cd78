"""Generate tests/golden/maskformer.json by IMPORTING THE REFERENCE (authoring container only):

    python tests/golden/make_maskformer_golden.py

The reference's MaskTransformer(hidden_dim=32, num_queries=5, num_heads=2, num_layers=2, dim_feedforward=64) and a MaskFormer
around a one-Linear backbone are built on the CPU with the stubs of make_golden.py.  Recorded: the names and shapes of their
state dicts, and - with the closed-form parameters and the input of tests/maskformer_helper.py, dropout 0 - the reference's
logits and masks in fp32 and in fp64 for point scenes of 3, 40 and 0 points, and ``max |fp32 - fp64|`` of both.  If the
reference fails on the empty scene that is recorded (``empty_scene_error``) and the scene dropped.  Only data is written - no
reference source."""
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
from maskformer_helper import IN_CHANNELS, MODEL_CONFIG, SCENES, TRANSFORMER_CONFIG, fill_closed_form, scene_input  # noqa: E402


def main():
    import_reference()
    from warpconvnet.geometry.types.points import Points
    from warpconvnet.models.maskformer import MaskFormer, MaskTransformer
    from warpconvnet.nn.modules.mlp import Linear

    out = {"transformer_config": TRANSFORMER_CONFIG, "model_config": MODEL_CONFIG, "in_channels": IN_CHANNELS}
    out["transformer_state_dict"] = {k: list(v.shape) for k, v in MaskTransformer(**TRANSFORMER_CONFIG).state_dict().items()}
    backbone = lambda: Linear(IN_CHANNELS, MODEL_CONFIG["hidden_dim"])
    out["model_state_dict"] = {k: list(v.shape) for k, v in MaskFormer(backbone(), **MODEL_CONFIG).state_dict().items()}

    def run(dtype, scenes):
        torch.manual_seed(0)
        m = MaskFormer(backbone(), **MODEL_CONFIG).to(dtype).eval()
        fill_closed_form(m)
        coords, feats, offsets = scene_input(dtype, scenes)
        with torch.no_grad():
            logits, masks = m(Points(coords, feats, offsets=offsets))
        return logits.double(), [x.double() for x in masks]

    scenes = SCENES
    try:
        run(torch.float32, scenes)
    except Exception as e:  # the reference's own behaviour on a scene without points
        out["empty_scene_error"] = f"{type(e).__name__}: {e}"[:300]
        scenes = tuple(s for s in SCENES if s > 0)
        print("the reference fails on the empty scene:", out["empty_scene_error"])
    out["scenes"] = list(scenes)
    (l32, m32), (l64, m64) = run(torch.float32, scenes), run(torch.float64, scenes)
    out["logits"], out["logits_fp64"] = l32.tolist(), l64.tolist()
    out["masks"], out["masks_fp64"] = [x.tolist() for x in m32], [x.tolist() for x in m64]
    out["logits_fp32_vs_fp64"] = float((l32 - l64).abs().max())
    out["masks_fp32_vs_fp64"] = max(float((a - b).abs().max()) if a.numel() else 0.0 for a, b in zip(m32, m64))
    print("max |logit|", float(l64.abs().max()), "fp32 vs fp64", out["logits_fp32_vs_fp64"], "masks", out["masks_fp32_vs_fp64"])
    with open(os.path.join(HERE, "maskformer.json"), "w") as f:
        json.dump(out, f, indent=1)
    print("maskformer.json", len(out["model_state_dict"]), "entries")


if __name__ == "__main__":
    main()
