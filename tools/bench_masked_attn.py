"""Masked cross-attention of a query decoder: B = 2 scenes, Q = 200 queries per scene, H = 8 heads of D = 64, bf16, against
20 000 and 100 000 keys per scene, forward and forward + backward, at about 5 %, 50 % and 100 % allowed pairs.  GPU box only.

    python tools/bench_masked_attn.py [--repeats 10] [--warmup 3] [--burn-in 20] [--json PATH] [--quick]

Masks.  100 %: nothing blocked.  5 % and 50 %: spatially coherent - the keys are random points in the unit cube and a query
allows the points of a ball around a random centre whose radius is the quantile of its distances that gives the fraction (what a
decoder's mask predictions look like: tiles of 32 keys are mostly all-blocked or all-allowed after the points are sorted along
a Morton-like key, here x-major cells).
Settings, alternating call by call inside one process (medians, min and (max - min) / median over the repeats):
  masked    flash_attn_varlen_func(.., k_splits=0, attn_mask=packed)        the masked HIP kernels
  unmasked  flash_attn_varlen_func(.., k_splits=0)                          the split-key kernels at the same shape, no mask
  composed  nn.MultiheadAttention on the padded [N, B, C] batch with the bool mask repeated over the heads (the reference's
            composition; its mask alone is B H Q N bytes)
  pack      pack_attention_mask from bf16 logits [B N, Q] with the release rule (forward rows only)
The figure is the whole call on the device's clock: allocations, autograd bookkeeping and launches included."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from warpconvnet_amd.nn.functional.attention import flash_attn_varlen_func, pack_attention_mask  # noqa: E402

B, Q, H, D = 2, 200, 8, 64
SETTINGS = ("masked", "unmasked", "composed", "pack")


def ball_logits(nk, frac, g, dev):
    """[B nk, Q] logits, >= 0 (allowed) inside a ball per query that holds ``frac`` of the scene's points, < 0 outside."""
    out = []
    for _ in range(B):
        pts = torch.rand(nk, 3, generator=g)
        pts = pts[torch.argsort((pts * 16).floor() @ torch.tensor([256.0, 16.0, 1.0]))].to(dev)   # cell order: coherent tiles
        dist = torch.cdist(pts, torch.rand(Q, 3, generator=g).to(dev))                            # [nk, Q]
        out.append(torch.quantile(dist[::max(nk // 4096, 1)], frac, dim=0)[None, :] - dist if frac < 1.0 else torch.ones_like(dist))
    return torch.cat(out).to(torch.bfloat16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--burn-in", type=int, default=20)
    ap.add_argument("--json", default=None)
    ap.add_argument("--quick", action="store_true", help="20 000 keys only")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_masked_attn.py measures on the GPU; there is no CPU timing"
    dev = torch.device("cuda:0")
    mha = torch.nn.MultiheadAttention(H * D, H).to(dev, torch.bfloat16)
    rows, first = [], True
    for nk in (20000,) if args.quick else (20000, 100000):
        g = torch.Generator().manual_seed(nk)
        q, k, v = (torch.randn(n, H, D, generator=g).to(dev, torch.bfloat16).requires_grad_(True) for n in (B * Q, B * nk, B * nk))
        dout = torch.randn(B * Q, H, D, generator=g).to(dev, torch.bfloat16)
        cu_q, cu_k = (torch.arange(B + 1) * Q).to(dev, torch.int32), (torch.arange(B + 1) * nk).to(dev, torch.int32)
        qp, kp = q.detach().reshape(B, Q, H * D).transpose(0, 1), k.detach().reshape(B, nk, H * D).transpose(0, 1)
        for frac in (0.05, 0.5, 1.0):
            logits = ball_logits(nk, frac, g, dev)
            pack = lambda: pack_attention_mask(logits, cu_k, cu_q, Q, nk, backend="hip", total_q=B * Q)
            mask = pack()
            allowed = 1.0 - float((logits < 0).float().mean())
            dense = (logits < 0).reshape(B, nk, Q).permute(0, 2, 1).repeat_interleave(H, dim=0)      # [(B H), Q, N] bool

            def call(setting, backward):
                q.grad = k.grad = v.grad = None
                with torch.enable_grad() if backward else torch.no_grad():
                    if setting == "pack":
                        return pack()
                    if setting == "composed":
                        x, y = (qp.clone().requires_grad_(True), kp.clone().requires_grad_(True)) if backward else (qp, kp)
                        out = mha(x, y, y, attn_mask=dense, need_weights=False)[0]
                        return out.backward(dout.reshape(B, Q, H * D).transpose(0, 1)) if backward else out
                    out = flash_attn_varlen_func(q, k, v, cu_q, cu_k, Q, nk, k_splits=0, attn_mask=mask if setting == "masked" else None)
                    return out.backward(dout) if backward else out

            if first:
                for i in range(args.burn_in):
                    call(SETTINGS[i % 2], True)
                torch.cuda.synchronize()
                first = False
            for backward in (False, True):
                todo = [s for s in SETTINGS if not (backward and s == "pack")]
                times = {s: [] for s in todo}
                for _ in range(args.warmup):
                    for s in todo:
                        call(s, backward)
                torch.cuda.synchronize()
                for _ in range(args.repeats):
                    for s in todo:
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        call(s, backward)
                        e1.record()
                        e1.synchronize()
                        times[s].append(e0.elapsed_time(e1))
                row = dict(keys=nk, allowed=round(allowed, 3), mode="fwdbwd" if backward else "fwd")
                for s in todo:
                    med = statistics.median(times[s])
                    row[f"ms_{s}"] = round(med, 4)
                    row[f"min_{s}"] = round(min(times[s]), 4)
                    row[f"spread_{s}"] = round((max(times[s]) - min(times[s])) / med, 3)
                rows.append(row)
                print(json.dumps(row), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
