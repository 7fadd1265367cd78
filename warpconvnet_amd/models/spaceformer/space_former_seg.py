"""SpaCeFormerInstSeg: a Mask2Former-style decoder of learned queries over a point backbone such as ``SpaCeFormer`` (reference
`warpconvnet/models/spaceformer/space_former_seg.py`).  One pass gives, per learned query, an objectness logit, a per-point
mask and an embedding: ``{"logit": [B, Q, 2], "mask": [[N_b, Q]], "clip_feat": [B, Q, clip_dim]}`` (``pred_iou`` with an IoU
head, ``backbone_pc`` in eval).  Constructor arguments and ``state_dict`` keys are the reference's - the attention layers keep
``nn.MultiheadAttention``'s ``in_proj_weight`` / ``in_proj_bias`` / ``out_proj.*`` - so its released checkpoint loads.

Every decoder iteration is masked attention: query i attends only to the points its current mask prediction marks
foreground (``point_feat @ mask_embed.T < 0`` is blocked); a query that blocks every point attends to all of them.
``decoder_iteration`` takes that mask as an argument, so the discontinuous step (the threshold) is apart from the smooth one.

Backends (``backend="hip" | "torch" | None``, None = hip for GPU features with a head size of 16 / 32 / 64).  The torch side is
the reference's composition: a padded [B, N, C] batch through ``nn.MultiheadAttention`` with a bool mask repeated over the heads.
The hip side builds no padded batch and no bool mask: the keys are the scene's concatenated rows with ``cu_k = offsets`` (in
training with more points than ``max_sample_size``, the subsampled rows through ``key_index``), the mask logits of the existing
``segment_bmm`` are bit-packed on the device by ``pack_attention_mask`` (with the release rule; the reference's pad mask goes
with the padding), Q is the first third of ``in_proj`` and K, V one projection of the RoPE'd key rows (``memory`` is key and value
here), and the core is ``flash_attn_varlen_kvpacked_func(.., k_splits=0, attn_mask=..)`` on the masked split-key kernels.  The
self-attention among the queries is the packed varlen call.  fp32 features run the cores in fp16 (``MaskFormer``'s policy).
Whole-model outputs of the two backends may differ where a mask logit lies near zero: a flipped bit is a legitimate difference."""
from contextlib import nullcontext
from typing import Any, List, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch import Tensor

from warpconvnet_amd.geometry.types.points import Points
from warpconvnet_amd.nn.functional.attention import (flash_attn_varlen_kvpacked_func, flash_attn_varlen_qkvpacked,
                                                     pack_attention_mask)
from warpconvnet_amd.nn.functional.bmm import segment_bmm
from warpconvnet_amd.nn.modules.sparse_pool import PointToVoxel

__all__ = ["SpaCeFormerInstSeg", "build_backbone", "build_spaceformer", "load_spaceformer_checkpoint", "SelfAttentionLayer",
           "CrossAttentionLayer", "FFNLayer", "FlatRotaryPositionalEmbeddings"]

_KERNEL_HEAD_DIMS = (16, 32, 64)


class FlatRotaryPositionalEmbeddings(nn.Module):
    """3-D RoPE of flat features ``x`` [N, C] by coordinates [N, 3] (the reference decoder's variant; `nn/modules/rope.py`
    rotates a packed qkv tensor and is another function).  Per head the largest multiple of 6 channels is rotated, a third per
    axis, by ``(coord - min coord + 1) * theta``; the rest passes through."""

    def __init__(self, dim: int, num_heads: int, base: int = 10_000, learnable_theta: bool = False) -> None:
        super().__init__()
        assert dim % num_heads == 0, f"dim {dim} must be divisible by num_heads {num_heads}"
        self.dim, self.num_heads, self.head_dim = dim, num_heads, dim // num_heads
        self.rope_dim = (self.head_dim // 6) * 6
        if self.rope_dim == 0:
            self.theta = None
        else:
            third = self.rope_dim // 3
            theta = 1.0 / (base ** (torch.arange(0, third, 2).float() / third))
            if learnable_theta:
                self.theta = nn.Parameter(theta)
            else:
                self.register_buffer("theta", theta, persistent=False)

    def forward(self, x: Tensor, coords: Tensor, **kwargs: Any) -> Tensor:
        n, c = x.shape
        if c != self.dim:
            raise ValueError(f"feature dim {c} != num_heads * head_dim {self.dim}")
        if self.rope_dim == 0 or n == 0:
            return x
        xh = x.view(n, self.num_heads, self.head_dim)
        pos = coords.float() - coords.min(dim=0).values.float() + 1.0                       # [N, 3]
        freqs = (pos[:, :, None] * self.theta.float()).reshape(n, 1, -1)                    # x, y, z thirds in turn
        cos, sin = torch.cos(freqs), torch.sin(freqs)
        pair = xh[..., :self.rope_dim].float().reshape(n, self.num_heads, self.rope_dim // 2, 2)
        rot = torch.stack([pair[..., 0] * cos - pair[..., 1] * sin, pair[..., 0] * sin + pair[..., 1] * cos], dim=-1)
        out = torch.cat([rot.reshape(n, self.num_heads, self.rope_dim), xh[..., self.rope_dim:].float()], dim=-1)
        return out.reshape(n, c).to(x.dtype)


def _activation_fn(activation: str):
    if activation not in ("relu", "gelu"):
        raise RuntimeError(f"activation should be relu/gelu, not {activation}.")
    return F.relu if activation == "relu" else F.gelu


class _DecoderLayer(nn.Module):
    """What the three decoder layers share: the (unused) activation and pre/post-norm switch, xavier weights."""

    def __init__(self, d_model: int, dropout: float, activation: str, normalize_before: bool):
        super().__init__()
        self.norm = nn.LayerNorm(d_model)
        self.dropout = nn.Dropout(dropout)
        self.activation = _activation_fn(activation)
        self.normalize_before = normalize_before

    def _reset_parameters(self):
        for p in self.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)

    def _residual(self, tgt: Tensor, branch) -> Tensor:
        if self.normalize_before:
            return tgt + self.dropout(branch(self.norm(tgt)))
        return self.norm(tgt + self.dropout(branch(tgt)))


def _heads(mha: nn.MultiheadAttention, x: Tensor, lo: int, hi: int) -> Tensor:
    """Slots ``lo .. hi - 1`` of the in-projection of ``x`` [T, C] -> [T, hi - lo, H, D] (0 = Q, 1 = K, 2 = V)."""
    c = mha.embed_dim
    y = F.linear(x, mha.in_proj_weight[lo * c:hi * c], mha.in_proj_bias[lo * c:hi * c])
    return y.view(x.shape[0], hi - lo, mha.num_heads, c // mha.num_heads)


def _core_dtype(t: Tensor) -> torch.dtype:
    return t.dtype if t.dtype in (torch.float16, torch.bfloat16) else torch.float16


class SelfAttentionLayer(_DecoderLayer):
    """Self-attention among the queries, sequence-first [Q, B, C] as the reference; ``forward_rows`` is the same layer on the
    rows [B * Q, C] through the packed varlen HIP attention."""

    def __init__(self, d_model, nhead, dropout=0.0, activation="relu", normalize_before=False):
        super().__init__(d_model, dropout, activation, normalize_before)
        self.self_attn = nn.MultiheadAttention(d_model, nhead, dropout=dropout)
        self._reset_parameters()

    def forward(self, tgt, tgt_mask=None, tgt_key_padding_mask=None, query_pos=None):
        def branch(x):
            qk = x if query_pos is None else x + query_pos
            return self.self_attn(qk, qk, value=x, attn_mask=tgt_mask, key_padding_mask=tgt_key_padding_mask)[0]
        return self._residual(tgt, branch)

    def forward_rows(self, tgt: Tensor, batch_size: int) -> Tensor:
        def branch(x):
            nq = x.shape[0] // batch_size
            qkv = _heads(self.self_attn, x, 0, 3).to(_core_dtype(x))
            cu = torch.arange(batch_size + 1, dtype=torch.int32) * nq
            out = flash_attn_varlen_qkvpacked(qkv, cu, nq)
            return self.self_attn.out_proj(out.reshape(x.shape).to(x.dtype))
        return self._residual(tgt, branch)


class CrossAttentionLayer(_DecoderLayer):
    """Queries over ``memory``, which is key and value alike.  ``forward`` is the reference's padded call; ``forward_rows`` runs
    the queries [B * Q, C] over the key rows [Tk, C] of ``cu_k`` under a ``PackedAttentionMask`` on the masked HIP kernels."""

    def __init__(self, d_model, nhead, dropout=0.0, activation="relu", normalize_before=False):
        super().__init__(d_model, dropout, activation, normalize_before)
        self.multihead_attn = nn.MultiheadAttention(d_model, nhead, dropout=dropout)
        self._reset_parameters()

    def forward(self, tgt, memory, memory_mask=None, memory_key_padding_mask=None, pos=None, query_pos=None):
        def branch(x):
            return self.multihead_attn(query=x if query_pos is None else x + query_pos,
                                       key=memory if pos is None else memory + pos, value=memory, attn_mask=memory_mask,
                                       key_padding_mask=memory_key_padding_mask)[0]
        return self._residual(tgt, branch)

    def forward_rows(self, tgt: Tensor, memory: Tensor, batch_size: int, cu_k: Tensor, max_k: int, mask) -> Tensor:
        def branch(x):
            nq = x.shape[0] // batch_size
            core = _core_dtype(x)
            q = _heads(self.multihead_attn, x, 0, 1)[:, 0].to(core)
            kv = _heads(self.multihead_attn, memory, 1, 3).to(core)
            cu_q = torch.arange(batch_size + 1, dtype=torch.int32) * nq
            out = flash_attn_varlen_kvpacked_func(q, kv, cu_q, cu_k, nq, max_k, k_splits=0, attn_mask=mask)
            return self.multihead_attn.out_proj(out.reshape(x.shape).to(x.dtype))
        return self._residual(tgt, branch)


class FFNLayer(_DecoderLayer):
    def __init__(self, d_model, dim_feedforward=2048, dropout=0.0, activation="relu", normalize_before=False):
        super().__init__(d_model, dropout, activation, normalize_before)
        self.linear1 = nn.Linear(d_model, dim_feedforward)
        self.linear2 = nn.Linear(dim_feedforward, d_model)
        self._reset_parameters()

    def forward(self, tgt):
        return self._residual(tgt, lambda x: self.linear2(self.dropout(self.activation(self.linear1(x)))))


class _QueryMLP(nn.Module):
    """Linear-ReLU-Linear-ReLU under ``layers`` (the checkpoint's ``query_proj.layers.0/2``)."""

    def __init__(self, dim: int):
        super().__init__()
        self.layers = nn.Sequential(nn.Linear(dim, dim), nn.ReLU(), nn.Linear(dim, dim), nn.ReLU())

    def forward(self, x):
        return self.layers(x)


class _PosEncBuffer(nn.Module):
    """The ``gauss_B`` buffer of the released checkpoint; the learned-query decoder never reads it."""

    def __init__(self, d_pos: int, d_in: int = 3):
        super().__init__()
        self.register_buffer("gauss_B", torch.zeros(d_in, d_pos // 2))


class SpaCeFormerInstSeg(nn.Module):
    """``backbone`` (voxels in, voxels out; wrapped in ``PointToVoxel`` at ``voxel_size``), a decoder of ``num_queries``
    learned queries run ``decoder_iterations`` times with shared weights, and the class / mask / embedding heads.
    ``max_sample_size`` caps the attention keys per scene in training."""

    def __init__(self, backbone: nn.Module, hidden_dim: int, feedforward_dim: int, clip_dim: int, num_queries: int, num_heads: int,
                 decoder_iterations: int, max_sample_size: int = 51200, voxel_size: float = 0.02, concat_unpooled_pc: bool = False,
                 freeze_backbone: bool = False, rope_base: int = 2000, rope_learnable_theta: bool = False,
                 use_iou_head: bool = False, backend: Optional[str] = None):
        super().__init__()
        if backend not in (None, "torch", "hip"):
            raise ValueError(f"backend must be 'torch', 'hip' or None, got {backend!r}")
        self.backend = backend
        self.backbone = PointToVoxel(backbone, voxel_size=voxel_size, concat_unpooled_pc=concat_unpooled_pc)
        self.hidden_dim, self.clip_dim, self.num_queries, self.num_heads = hidden_dim, clip_dim, num_queries, num_heads
        self.decoder_iterations, self.max_sample_size = decoder_iterations, max_sample_size
        backbone_out_dim = getattr(backbone, "out_channels", clip_dim)
        self.decoder_proj = nn.Linear(backbone_out_dim, hidden_dim)
        self.query_proj = _QueryMLP(hidden_dim)
        self.pos_enc = _PosEncBuffer(hidden_dim)
        self.decoder_norm = nn.LayerNorm(hidden_dim)
        self.linear = nn.Linear(backbone_out_dim, hidden_dim)
        self.cross_attention = CrossAttentionLayer(d_model=hidden_dim, nhead=num_heads)
        self.self_attention = SelfAttentionLayer(d_model=hidden_dim, nhead=num_heads)
        self.ffn = FFNLayer(d_model=hidden_dim, dim_feedforward=feedforward_dim)
        self.class_head = nn.Linear(hidden_dim, 2)
        self.mask_head = nn.Sequential(nn.Linear(hidden_dim, hidden_dim), nn.ReLU(), nn.Linear(hidden_dim, hidden_dim))
        self.clip_head = nn.Linear(hidden_dim, clip_dim)
        self.iou_head = None
        if use_iou_head:
            self.iou_head = nn.Sequential(nn.Linear(hidden_dim, hidden_dim), nn.GELU(), nn.Linear(hidden_dim, hidden_dim), nn.GELU(),
                                          nn.Linear(hidden_dim, 1))
        self.learned_content = nn.Embedding(num_queries, hidden_dim)
        self.learned_pos = nn.Embedding(num_queries, hidden_dim)
        self.rope_cross = FlatRotaryPositionalEmbeddings(hidden_dim, num_heads, base=rope_base, learnable_theta=rope_learnable_theta)
        self.rope_self = FlatRotaryPositionalEmbeddings(hidden_dim, num_heads, base=rope_base, learnable_theta=rope_learnable_theta)
        self.backbone_frozen = bool(freeze_backbone)
        if freeze_backbone:
            for p in self.backbone.parameters():
                p.requires_grad = False

    # ---- pieces ------------------------------------------------------------------------------------------------------------
    def _use_hip(self, feats: Tensor) -> bool:
        ok = feats.is_cuda and feats.dtype in (torch.float32, torch.float16, torch.bfloat16) and \
            self.hidden_dim // self.num_heads in _KERNEL_HEAD_DIMS
        if self.backend == "hip" and not ok:
            raise RuntimeError(f"backend='hip' needs GPU features in fp32 / fp16 / bf16 and a head size of 16 / 32 / 64, got "
                               f"{feats.device}, {feats.dtype}, {self.hidden_dim // self.num_heads}; there is no CPU fallback")
        return ok and self.backend != "torch"

    def _extract_backbone_features(self, data_dict: dict) -> Tuple[Points, Tensor, Tensor, Tensor]:
        pc = data_dict["pc"] if "pc" in data_dict else Points(batched_coordinates=data_dict["coord"],
                                                              batched_features=data_dict["feat"], offsets=data_dict.get("offset"))
        with torch.no_grad() if self.backbone_frozen else nullcontext():
            if self.backbone_frozen and self.backbone.training:
                self.backbone.eval()
            out_pc = self.backbone(pc)
        offsets = torch.as_tensor(out_pc.offsets).to(device="cpu", dtype=torch.int64)
        return out_pc, out_pc.feature_tensor, out_pc.coordinate_tensor, offsets

    def _sample_key_indices(self, offsets: Tensor, device: torch.device) -> Tuple[Tensor, Tensor, int]:
        """Per scene ``sample_size`` key rows in random order (all of them in eval; at most ``max_sample_size`` in training):
        ``global_idx`` [B, S] and ``pad_mask`` [B, S], True where a scene has fewer points (the slot then names its row 0)."""
        counts = (offsets[1:] - offsets[:-1]).to(device)
        if int(counts.min()) == 1:
            raise RuntimeError("only a single point gives nans in cross-attention")
        max_count = int(counts.max())
        sample_size = min(max_count, self.max_sample_size) if self.training else max_count
        valid = torch.arange(max_count, device=device)[None, :] < counts[:, None]
        scores = torch.rand(counts.numel(), max_count, device=device).masked_fill(~valid, float("-inf"))
        local = torch.topk(scores, k=sample_size, dim=1).indices
        pad_mask = local >= counts[:, None]
        local = local.masked_fill(pad_mask, 0)
        return local + offsets[:-1].to(device)[:, None], pad_mask, sample_size

    def _mask_embeds(self, queries: Tensor) -> Tensor:
        return self.mask_head(self.decoder_norm(queries))                                  # [B, Q, C]

    def mask_logits(self, queries: Tensor, feats_proj: Tensor, offsets: Tensor) -> Tensor:
        """``point_feat @ mask_embed.T`` of every scene as one [N, Q] tensor (``segment_bmm``)."""
        return segment_bmm(feats_proj, self._mask_embeds(queries).transpose(1, 2).contiguous(), offsets)

    def decoder_iteration(self, queries: Tensor, blocked: Tensor, point_features: Tensor, point_coords: Tensor,
                          offsets: Tensor) -> Tensor:
        """One decoder iteration on ``queries`` [B, Q, C]: masked cross-attention over the scene's points, self-attention
        among the queries, FFN.  ``blocked`` [N, Q] says which (point, query) pairs may not attend: a bool tensor, or mask
        logits (blocked where < 0); a query that blocks every sampled point of its scene is released."""
        B, Q, C = queries.shape
        dev = queries.device
        zeros = torch.zeros(B * Q, 3, device=dev, dtype=point_coords.dtype)                # learned queries have no location
        if self._use_hip(point_features):
            counts = offsets[1:] - offsets[:-1]
            if int(counts.min()) == 1:
                raise RuntimeError("only a single point gives nans in cross-attention")
            key_index, cu_k = None, offsets
            if self.training and int(counts.max()) > self.max_sample_size:                # the training-time key subsample
                global_idx, pad_mask, _ = self._sample_key_indices(offsets, dev)
                key_index = global_idx[~pad_mask]
                cu_k = F.pad(torch.cumsum((~pad_mask).sum(1).cpu(), 0), (1, 0))
            max_k = int((cu_k[1:] - cu_k[:-1]).max())
            mask = pack_attention_mask(blocked.detach(), cu_k, torch.arange(B + 1) * Q, Q, max_k, threshold=0.0,
                                       key_index=key_index, release_full_rows=True, backend="hip", total_q=B * Q)
            keys, coords = (point_features, point_coords) if key_index is None else (point_features[key_index],
                                                                                      point_coords[key_index])
            k_rope = self.rope_cross(self.linear(keys), coords)
            q_rope = self.rope_cross(queries.reshape(B * Q, C), zeros)
            x = self.cross_attention.forward_rows(q_rope, k_rope, B, cu_k, max_k, mask)
            x = self.self_attention.forward_rows(self.rope_self(x, zeros), B)
            return self.ffn(x).reshape(B, Q, C)
        # the reference's composition: a padded batch and a bool mask repeated over the heads
        blocked = blocked if blocked.dtype == torch.bool else blocked < 0
        global_idx, pad_mask, S = self._sample_key_indices(offsets, dev)
        flat = global_idx.reshape(-1)
        attn = blocked[flat].reshape(B, S, Q).clone()
        attn.permute(0, 2, 1)[attn.sum(1) == S] = False                                    # the release rule
        attn = attn | pad_mask[..., None]
        k_rope = self.rope_cross(self.linear(point_features[flat]), point_coords[flat]).reshape(B, S, C).transpose(0, 1)
        q_rope = self.rope_cross(queries.reshape(B * Q, C), zeros).reshape(B, Q, C).transpose(0, 1)
        memory_mask = attn.permute(0, 2, 1).repeat_interleave(self.num_heads, dim=0)       # [(B H), Q, S]
        x = self.cross_attention(q_rope, k_rope, memory_mask=memory_mask)                  # [Q, B, C]
        xs = self.rope_self(x.transpose(0, 1).reshape(B * Q, C), zeros).reshape(B, Q, C).transpose(0, 1)
        return self.ffn(self.self_attention(xs)).transpose(0, 1)

    def mask_module(self, queries: Tensor, feats_proj: Tensor, offsets: Tensor) -> Tuple[Tensor, List[Tensor], Tensor]:
        normed = self.decoder_norm(queries)
        logits = self.mask_logits(queries, feats_proj, offsets)
        off = offsets.tolist()
        return self.class_head(normed), [logits[off[b]:off[b + 1]] for b in range(len(off) - 1)], self.clip_head(normed)

    def forward(self, data_dict: dict) -> dict:
        out_pc, point_features, point_coords, offsets = self._extract_backbone_features(data_dict)
        B = offsets.numel() - 1
        feats_proj = self.decoder_proj(point_features)
        num_queries = int(data_dict.get("num_queries", self.num_queries))
        ids = torch.arange(num_queries, device=point_features.device) % self.num_queries   # eval may ask for more queries
        queries = (self.learned_content(ids) + self.query_proj(self.learned_pos(ids))).unsqueeze(0).expand(B, -1, -1)
        queries = queries.to(point_features.dtype)
        for _ in range(self.decoder_iterations):
            blocked = self.mask_logits(queries, feats_proj, offsets).detach()
            queries = self.decoder_iteration(queries, blocked, point_features, point_coords, offsets)
        logit, masks, clip_feat = self.mask_module(queries, feats_proj, offsets)
        result = dict(logit=logit, mask=masks, clip_feat=clip_feat)
        if self.iou_head is not None:
            result["pred_iou"] = self.iou_head(self.decoder_norm(queries)).squeeze(-1)
        if not self.training:
            result["backbone_pc"] = out_pc                                                 # eval only, as the reference
        return result


# ---- the released open-vocabulary architecture ------------------------------------------------------------------------------
GRID_SIZE = 0.02
CLIP_TEXT_DIM = 1152
NUM_QUERIES = 200
HIDDEN_DIM = 512


def build_backbone(out_channels: int = CLIP_TEXT_DIM) -> nn.Module:
    """The ``SpaCeFormer`` backbone of the released checkpoint."""
    from .space_former import SpaCeFormer

    return SpaCeFormer(
        in_channels=3, out_channels=out_channels, block_type="stream_norm", enc_channels=[32, 64, 128, 256, 512],
        enc_num_head=[2, 4, 8, 16, 32], enc_patch_size=[64, 48, 1024, 1024, 1024], enc_depths=[2, 2, 2, 6, 2], enc_attn_types="ssccc",
        dec_channels=[512, 384, 256, 256], dec_num_head=[8, 8, 8, 16], dec_patch_size=[64, 48, 1024, 1024], dec_depths=[2, 2, 2, 2],
        dec_attn_types="sscc", kernel_size=3, voxel_offsets=["zero", "xy", "xz", "yz", "xyz"],
        patch_orders=["random", "morton_xyz", "morton_xzy", "morton_yxz", "morton_yzx", "morton_zxy", "morton_zyx"], mlp_ratio=2.0,
        attn_drop=0.0, proj_drop=0.0, drop_path=0.2, shuffle_orders=True, use_rope=True, rope_base=2000,
        enc_rope_bases=[250, 250, 250, 250, 250], dec_rope_bases=[250, 250, 250, 250])


def build_spaceformer(use_iou_head: bool = False, device: Optional[torch.device] = None,
                      backend: Optional[str] = None) -> SpaCeFormerInstSeg:
    """The released SpaCeFormerInstSeg: 200 learned queries, hidden 512, 8 heads (head size 64), three decoder iterations."""
    net = SpaCeFormerInstSeg(backbone=build_backbone(), hidden_dim=HIDDEN_DIM, feedforward_dim=1024, clip_dim=CLIP_TEXT_DIM,
                             num_queries=NUM_QUERIES, num_heads=8, decoder_iterations=3, max_sample_size=51200, voxel_size=GRID_SIZE,
                             concat_unpooled_pc=False, freeze_backbone=False, rope_base=2000, rope_learnable_theta=False,
                             use_iou_head=use_iou_head, backend=backend)
    net.eval()
    return net if device is None else net.to(device)


def load_spaceformer_checkpoint(net: nn.Module, ckpt_path: str, strict: bool = False) -> Tuple[list, list]:
    """Loads a released weights-only checkpoint (a Lightning ``state_dict`` whose keys carry a ``net.`` prefix) ->
    ``(missing_keys, unexpected_keys)``."""
    ckpt = torch.load(ckpt_path, map_location="cpu", weights_only=True)
    state = ckpt.get("state_dict", ckpt)
    missing, unexpected = net.load_state_dict({k[4:]: v for k, v in state.items() if k.startswith("net.")}, strict=strict)
    return list(missing), list(unexpected)
