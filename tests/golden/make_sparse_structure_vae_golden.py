"""Generator of tests/golden/sparse_structure_vae_state.json: state-dict names and shapes of the reference's
``SparseStructureEncoder`` / ``SparseStructureDecoder`` over a few constructor settings, and the modules its
``convert_to_fp16`` converts (names of the parameters that come out fp16).

    python tests/golden/make_sparse_structure_vae_golden.py

Needs the reference tree on the authoring machine (see make_golden.py: import_reference); the tests read only the file."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import import_reference  # noqa: E402

CONFIGS = [
    ("SparseStructureEncoder", dict(in_channels=1, latent_channels=8, num_res_blocks=2, channels=[32, 128, 512])),
    ("SparseStructureDecoder", dict(out_channels=1, latent_channels=8, num_res_blocks=2, channels=[512, 128, 32])),
    ("SparseStructureEncoder", dict(in_channels=2, latent_channels=4, num_res_blocks=1, channels=[32, 64], num_res_blocks_middle=1,
                                    norm_type="group")),
    ("SparseStructureDecoder", dict(out_channels=3, latent_channels=4, num_res_blocks=1, channels=[64, 32], num_res_blocks_middle=1,
                                    norm_type="group", use_fp16=True)),
]

if __name__ == "__main__":
    import_reference()
    import types

    tv = types.ModuleType("torchvision")  # (the package's __init__ pulls in the image conditioner; nothing here uses it)
    tv.transforms = types.ModuleType("torchvision.transforms")
    sys.modules["torchvision"], sys.modules["torchvision.transforms"] = tv, tv.transforms
    from warpconvnet.models.trellis2 import sparse_structure_vae as ref

    out = []
    for name, kw in CONFIGS:
        m = getattr(ref, name)(**kw)
        layout = [[k, list(v.shape)] for k, v in m.state_dict().items()]
        m.convert_to_fp16()
        half = [k for k, v in m.state_dict().items() if v.dtype == torch.float16]
        out.append([name, kw, layout, half])
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sparse_structure_vae_state.json")
    with open(path, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(entry) for entry in out) + "\n]\n")  # one configuration per line
    print(path, [len(o[2]) for o in out])
