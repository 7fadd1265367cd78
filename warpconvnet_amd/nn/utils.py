"""Small helpers for building modules and for the mixed-precision convention of the diffusion / VAE model ports: matmul-like
layers hold their parameters in a low precision, normalisations stay fp32 (reference `nn/utils.py`)."""
from typing import Tuple, Type

import torch
import torch.nn as nn

__all__ = ["DEFAULT_MIXED_PRECISION_MODULES", "convert_module_parameters_to", "convert_module_to_f16", "convert_module_to_f32",
           "manual_cast", "str_to_dtype", "zero_module"]

# the layer families whose parameters follow a model's ``use_fp16`` switch
DEFAULT_MIXED_PRECISION_MODULES: Tuple[Type[nn.Module], ...] = (
    nn.Conv1d, nn.Conv2d, nn.Conv3d, nn.ConvTranspose1d, nn.ConvTranspose2d, nn.ConvTranspose3d, nn.Linear,
)

_DTYPE_NAMES = {
    torch.float16: ("f16", "fp16", "float16"),
    torch.bfloat16: ("bf16", "bfloat16"),
    torch.float32: ("f32", "fp32", "float32"),
}


def zero_module(module: nn.Module) -> nn.Module:
    """Set every parameter of ``module`` to zero in place and hand the module back: a residual branch that ends in such a
    module starts as the identity."""
    with torch.no_grad():
        for p in module.parameters():
            p.zero_()
    return module


def manual_cast(tensor: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """``tensor`` in ``dtype``, unless autocast is active: then autocast decides and the tensor comes back untouched."""
    return tensor if torch.is_autocast_enabled() else tensor.to(dtype)


def str_to_dtype(s: str) -> torch.dtype:
    """The dtype a configuration file spells ``"fp16"``, ``"bf16"``, ``"float32"``, ...; an unknown spelling is a ``KeyError``."""
    for dtype, names in _DTYPE_NAMES.items():
        if s in names:
            return dtype
    raise KeyError(s)


def convert_module_parameters_to(module: nn.Module, dtype: torch.dtype,
                                 module_types: Tuple[Type[nn.Module], ...] = DEFAULT_MIXED_PRECISION_MODULES) -> None:
    """Cast the parameters of ``module`` in place if it is one of ``module_types``; made for ``model.apply``, which visits
    every submodule, so that normalisations in between keep their fp32 parameters."""
    if not isinstance(module, module_types):
        return
    for p in module.parameters():
        p.data = p.data.to(dtype)


def convert_module_to_f16(module: nn.Module,
                          module_types: Tuple[Type[nn.Module], ...] = DEFAULT_MIXED_PRECISION_MODULES) -> None:
    convert_module_parameters_to(module, torch.float16, module_types=module_types)


def convert_module_to_f32(module: nn.Module,
                          module_types: Tuple[Type[nn.Module], ...] = DEFAULT_MIXED_PRECISION_MODULES) -> None:
    convert_module_parameters_to(module, torch.float32, module_types=module_types)
