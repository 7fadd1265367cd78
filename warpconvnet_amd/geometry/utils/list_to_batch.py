"""List -> concatenated or padded tensor + CPU offsets (reference `geometry/utils/list_to_batch.py:11-52`)."""
from typing import List, Optional, Tuple

import torch
from torch import Tensor


def list_to_cat_tensor(tensor_list: List[Tensor]) -> Tuple[Tensor, Tensor, int]:
    """Returns ``(cat, offsets[B+1] int32 on CPU, B)``."""
    sizes = torch.tensor([0] + [int(t.shape[0]) for t in tensor_list], dtype=torch.int64)
    offsets = sizes.cumsum(0).to(torch.int32)
    return torch.cat(list(tensor_list), dim=0), offsets, len(tensor_list)


def list_to_pad_tensor(tensor_list: List[Tensor], pad_to_multiple: Optional[int] = None) -> Tuple[Tensor, Tensor, int]:
    """Returns ``(padded [B, M, C], offsets[B+1] int32 on CPU, B)``; M = the longest element, rounded up to ``pad_to_multiple``."""
    from torch.nn.utils.rnn import pad_sequence

    assert len(tensor_list) > 0, "an empty list has no channel count"
    sizes = torch.tensor([0] + [int(t.shape[0]) for t in tensor_list], dtype=torch.int64)
    offsets = sizes.cumsum(0).to(torch.int32)
    padded = pad_sequence(list(tensor_list), batch_first=True)
    m = padded.shape[1]
    if pad_to_multiple is not None:
        m = (m + pad_to_multiple - 1) // pad_to_multiple * pad_to_multiple
        if m > padded.shape[1]:
            padded = torch.nn.functional.pad(padded, (0, 0, 0, m - padded.shape[1]))
    return padded, offsets, len(tensor_list)
