"""Closed-form parameters and the small input of the MaskFormer fixture (tests/golden/maskformer.json): shared by the
generator tests/golden/make_maskformer_golden.py, which writes them into the reference's model, and by the tests, which write
them into this package's.  A helper, not a test."""
import math

import torch

TRANSFORMER_CONFIG = dict(hidden_dim=32, num_queries=5, num_heads=2, num_layers=2, dim_feedforward=64)
MODEL_CONFIG = dict(hidden_dim=32, num_queries=5, num_heads=2, num_decoders=2, dim_feedforward=64, dropout=0.0, num_classes=4)
IN_CHANNELS = 3
SCENES = (3, 40, 0)          # 3 points < 5 queries: the trailing query rows are zeroed; 0: a scene without points


def fill_closed_form(model: torch.nn.Module) -> None:
    """Every floating-point entry of the state dict from the sine of its flat index: matrices scaled by 1 / sqrt(fan_in)
    (the stacked [2, in, out] kv weight by its ``in``), LayerNorm weights around 1, everything else small.  The frequencies
    of the positional encoding keep their values."""
    with torch.no_grad():
        for n, (key, t) in enumerate(model.state_dict().items()):
            if not t.is_floating_point() or key.endswith("freqs"):
                continue
            idx = torch.arange(t.numel(), dtype=torch.float64)
            wave = torch.sin(0.37 * idx + 0.61 * n + 0.2)
            if t.ndim == 1 and key.endswith("norm.weight"):
                v = 1.0 + 0.3 * wave
            elif t.ndim == 2:
                v = wave / math.sqrt(t.shape[1])
            elif t.ndim == 3:
                v = wave / math.sqrt(t.shape[1])
            else:
                v = 0.1 * wave
            t.copy_(v.reshape(t.shape).to(t.dtype))


def scene_input(dtype=torch.float32, scenes=SCENES):
    """(coordinates [N, 3] in [0, 1), features [N, 3], offsets): points on a sine lattice, no two alike."""
    n = sum(scenes)
    i = torch.arange(n, dtype=torch.float64).unsqueeze(1)
    coords = 0.5 + 0.45 * torch.sin(0.73 * i * torch.tensor([[1.0, 1.7, 2.3]], dtype=torch.float64)
                                    + torch.tensor([[0.0, 1.3, 2.1]], dtype=torch.float64))
    feats = torch.cos(0.41 * i * torch.tensor([[1.0, 2.1, 3.3]], dtype=torch.float64) + 0.3)
    offsets = [0]
    for s in scenes:
        offsets.append(offsets[-1] + s)
    return coords.to(dtype), feats.to(dtype), torch.tensor(offsets)


def exact_chain(params, x, feats, sin, G, offsets, heads):
    """The stages of ``SpatialFeatureCrossAttention`` - the formulas tests/test_gpu_maskformer.py applies stage by stage to
    recorded tensors - composed end to end in the dtype of the arguments (fp64): ``params`` = the module's named parameters,
    ``x`` [B, Q, C] queries, ``feats`` [N, C], ``sin`` [N, E] the sinusoidal features of the coordinates, ``G`` [B, Q, C] the
    gradient of the output.  Returns ``y`` [B, Q, C] and the gradients of x, feats and the six parameters by their names."""
    from warpconvnet_amd.nn.functional.attention import cross_attention_reference

    Wq, Wkv, Wp, bp = params["q.weight"], params["kv.weight"], params["proj.weight"], params["proj.bias"]
    We, be = params["to_attn.encoding.1.weight"], params["to_attn.encoding.1.bias"]
    nb, nq, dim = x.shape
    n, hd = feats.shape[0], dim // heads
    offsets = torch.as_tensor(offsets).to(torch.int64)
    x2 = x.reshape(nb * nq, dim)
    pos = sin @ We.t() + be
    q = (x2 @ Wq.t()).reshape(nb * nq, heads, hd).detach().requires_grad_(True)
    kv = torch.stack([feats @ Wkv[0], feats @ Wkv[1]], dim=1)
    kv[:, 0] += pos.repeat(1, heads)
    kv = kv.reshape(n, 2, heads, hd).detach().requires_grad_(True)
    cu_q = torch.arange(nb + 1) * nq
    out = cross_attention_reference(q, kv[:, 0], kv[:, 1], cu_q, offsets, hd ** -0.5, dtype=x.dtype)[0]
    valid = (torch.arange(nq)[None, :] < (offsets[1:] - offsets[:-1])[:, None]).reshape(nb * nq, 1).to(x.dtype)
    o2 = out.reshape(nb * nq, dim)
    y = (o2 @ Wp.t() + bp) * valid
    g = G.reshape(nb * nq, dim) * valid
    dq, dkv = torch.autograd.grad(out, (q, kv), (g @ Wp).reshape(nb * nq, heads, hd))
    dq, dkv, o2 = dq.reshape(nb * nq, dim), dkv.reshape(n, 2, dim), o2.detach()
    dpos = dkv[:, 0].reshape(n, heads, hd).sum(1)
    grads = {
        "proj.weight": g.t() @ o2, "proj.bias": g.sum(0), "q.weight": dq.t() @ x2, "x": (dq @ Wq).reshape(nb, nq, dim),
        "kv.weight": torch.stack([feats.t() @ dkv[:, 0], feats.t() @ dkv[:, 1]]),
        "feats": dkv[:, 0] @ Wkv[0].t() + dkv[:, 1] @ Wkv[1].t(),
        "to_attn.encoding.1.weight": dpos.t() @ sin, "to_attn.encoding.1.bias": dpos.sum(0),
    }
    return y.detach().reshape(nb, nq, dim), grads
