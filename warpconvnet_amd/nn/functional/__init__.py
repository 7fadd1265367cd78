"""Functional layer.  The segmented operations and the ragged ``segment_bmm`` are exported here by name; they are resolved on
first use, so importing a submodule of this package stays as cheap as it was."""
import importlib

_EXPORTS = {
    "segmented_add": "segmented_arithmetics",
    "segmented_subtract": "segmented_arithmetics",
    "segmented_multiply": "segmented_arithmetics",
    "segmented_divide": "segmented_arithmetics",
    "segmented_norm": "normalizations",
    "segmented_layer_norm": "normalizations",
    "segmented_range_norm": "normalizations",
    "segment_bmm": "bmm",  # (bmm the function shares its name with that submodule: import it from there)
    "edge_conv_supported": "edge_conv",  # (edge_conv the function shares its name with that submodule: import it from there)
    "transposed_lists": "edge_conv",
    "apply_feature_transform": "transforms",
    "create_activation_function": "transforms",
    "create_norm_function": "transforms",
    "cat": "transforms",
    "global_scale": "global_pool",  # (global_pool the function shares its name with that submodule: import it from there)
}

__all__ = sorted(_EXPORTS)


def __getattr__(name):
    if name in _EXPORTS:
        value = getattr(importlib.import_module(f"{__name__}.{_EXPORTS[name]}"), name)
        globals()[name] = value
        return value
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
