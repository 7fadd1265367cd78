"""Feature transforms that accept a geometry or a plain tensor (module path and names of the reference's
`warpconvnet/nn/functional/transforms.py`): an activation or normalisation from ``torch.nn.functional`` acts on the feature
tensor and the geometry keeps its coordinates, offsets and caches; ``cat`` joins the features of several geometries that
share their offsets."""
from typing import Callable, Sequence, Union

import torch
import torch.nn.functional as F
from torch import Tensor

from warpconvnet_amd.geometry.base.geometry import Geometry

__all__ = ["apply_feature_transform", "create_activation_function", "create_norm_function", "cat", "relu", "gelu", "silu",
           "tanh", "sigmoid", "leaky_relu", "elu", "softmax", "log_softmax", "layer_norm", "batch_norm", "instance_norm",
           "group_norm"]


def apply_feature_transform(input: Union[Geometry, Tensor], transform: Callable):
    """``transform`` of the feature tensor: a geometry comes back with the new features, a tensor as a tensor."""
    if isinstance(input, Geometry):
        return input.replace(batched_features=transform(input.feature_tensor))
    assert isinstance(input, Tensor), f"Expected Tensor, got {type(input)}"
    return transform(input)


def create_activation_function(torch_func: Callable) -> Callable:
    """A one-argument activation that takes geometries as well as tensors."""

    def wrapper(input):
        return apply_feature_transform(input, torch_func)

    wrapper.__name__ = getattr(torch_func, "__name__", "activation")
    return wrapper


def create_norm_function(torch_norm_func: Callable) -> Callable:
    """A normalisation whose further arguments are those of ``torch_norm_func``."""

    def wrapper(input, *args, **kwargs):
        return apply_feature_transform(input, lambda x: torch_norm_func(x, *args, **kwargs))

    wrapper.__name__ = getattr(torch_norm_func, "__name__", "norm")
    return wrapper


relu = create_activation_function(F.relu)
gelu = create_activation_function(F.gelu)
silu = create_activation_function(F.silu)
tanh = create_activation_function(F.tanh)
sigmoid = create_activation_function(F.sigmoid)
leaky_relu = create_activation_function(F.leaky_relu)
elu = create_activation_function(F.elu)
softmax = create_activation_function(F.softmax)
log_softmax = create_activation_function(F.log_softmax)

layer_norm = create_norm_function(F.layer_norm)        # (input, normalized_shape, weight=None, bias=None, eps=1e-5)
batch_norm = create_norm_function(F.batch_norm)        # (input, running_mean, running_var, weight=None, bias=None, ...)
instance_norm = create_norm_function(F.instance_norm)  # (input, running_mean=None, running_var=None, weight=None, ...)
group_norm = create_norm_function(F.group_norm)        # (input, num_groups, weight=None, bias=None, eps=1e-5)


def cat(*inputs: Geometry, dim: int = -1):
    """The first geometry with the features of all of them joined along ``dim``; one sequence argument is unpacked.  The
    geometries must share their offsets (the integer type may differ)."""
    if len(inputs) == 1 and isinstance(inputs[0], Sequence):
        inputs = tuple(inputs[0])
    assert all(isinstance(x, Geometry) for x in inputs), f"Expected geometries, got {[type(x) for x in inputs]}"
    first = inputs[0].offsets.long()
    assert all(x.offsets.shape == first.shape and torch.equal(x.offsets.long(), first) for x in inputs), (
        "All inputs must have the same offsets")
    return inputs[0].replace(batched_features=torch.cat([x.feature_tensor for x in inputs], dim=dim))
