"""Times the DINOv2 UNet decoder (B = 24, 518 px, 768 -> 2 classes, bf16) with HIP events, median of 20 after 5 warm-up runs:
the HIP decoder forward (train mode) and backward, and as a yardstick the same decoder as eager PyTorch-ROCm modules (MIOpen convs, torch BatchNorm,
F.interpolate) in bf16 autocast-free NCHW form.  Prints one JSON line.

    python tools/time_dino_seg.py [--batch 24]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "nextgen-uia_amd")]


def median_ms(fn, steps=20, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return sorted(times)[len(times) // 2]


class EagerBlock(nn.Module):
    def __init__(self, cin, cout, embed):
        super().__init__()
        self.upconv = nn.ConvTranspose2d(cin, cout, 2, 2)
        self.conv = nn.Sequential(nn.Conv2d(2 * cout, cout, 3, padding=1), nn.BatchNorm2d(cout), nn.ReLU())
        self.skip_conv = nn.Sequential(nn.Conv2d(embed, cout, 3, padding=1), nn.BatchNorm2d(cout), nn.ReLU())

    def forward(self, x, s):
        a = self.upconv(x)
        s = F.interpolate(self.skip_conv(s), scale_factor=a.shape[2] / s.shape[2], mode="bilinear", align_corners=True)
        return self.conv(torch.cat([a, s], 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=24)
    args = ap.parse_args()
    from src.third_party.dino.dinov2 import UNetDecoder
    from uia_hip import functional as UF
    B, D, nc = args.batch, 768, 2
    UF.set_compute_dtype(torch.bfloat16)
    maps = [torch.randn(B, 1369, D, device="cuda", dtype=torch.bfloat16) for _ in range(5)]
    dec = UNetDecoder(D, nc, image_size=518, resize_image=True, patch_size=14).cuda().train()
    g = torch.randn(B, nc, 518, 518, device="cuda")
    res = {"batch": B}
    res["hip_fwd_ms"] = median_ms(lambda: dec(maps))

    def hip_step():
        dec.zero_grad(set_to_none=True)
        dec(maps).backward(g)
    res["hip_fwd_bwd_ms"] = median_ms(hip_step)
    res["hip_bwd_ms"] = res["hip_fwd_bwd_ms"] - res["hip_fwd_ms"]

    blocks = nn.ModuleList([EagerBlock(D, D // 2, D), EagerBlock(D // 2, D // 4, D), EagerBlock(D // 4, D // 8, D), EagerBlock(D // 8, nc, D)])
    blocks = blocks.cuda().to(torch.bfloat16).train()
    nchw = [m.reshape(B, 37, 37, D).permute(0, 3, 1, 2).contiguous() for m in maps]

    def eager_fwd():
        x = nchw[4]
        for blk, s in zip(blocks, (nchw[3], nchw[2], nchw[1], nchw[0])):
            x = blk(x, s)
        return F.interpolate(x.float(), size=(518, 518), mode="bicubic", align_corners=False, antialias=True)
    res["eager_fwd_ms"] = median_ms(eager_fwd)

    def eager_step():
        blocks.zero_grad(set_to_none=True)
        eager_fwd().backward(g)
    res["eager_fwd_bwd_ms"] = median_ms(eager_step)
    res["eager_bwd_ms"] = res["eager_fwd_bwd_ms"] - res["eager_fwd_ms"]
    print(json.dumps({k: round(v, 3) if isinstance(v, float) else v for k, v in res.items()}))


if __name__ == "__main__":
    main()
